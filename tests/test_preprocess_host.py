"""Host-side checks of lavt_hip.preprocess (no GPU): the fixed-point resample tables and the nearest index tables against the PIL results stored in
tests/golden/preprocess_cases.npz and, where PIL imports, against a live `Image.resize`; table invariants; the refusals without a GPU."""
import numpy as np
import pytest
import torch

from lavt_hip import preprocess as P

CASES = "abcdefgh"
# (source H, W) -> (output H, W): the pairs the recipe was established on
LIVE_PAIRS = [((720, 1280), (480, 480)), ((360, 640), (480, 480)), ((37, 53), (32, 32)), ((17, 96), (32, 32)), ((32, 45), (32, 32)), ((500, 375), (480, 480)),
              ((480, 480), (480, 480)), ((427, 640), (96, 96)), ((5, 7), (32, 32)), ((1, 1), (8, 8)), ((333, 500), (224, 224))]
# the strong downscales tests/test_gpu_preprocess.py uses for the lower tile heights (its reference there is apply_tables_numpy), and load_frames' sizes
LIVE_PAIRS += [((700, 8), (24, 8)), ((640, 70), (12, 66)), ((700, 8), (10, 5)), ((1200, 12), (8, 9)), ((150, 200), (224, 224)), ((50, 90), (64, 64))]


def _nearest(m, ho, wo):
    return m[P.nearest_table(m.shape[0], ho)][:, P.nearest_table(m.shape[1], wo)]


@pytest.mark.parametrize("case", CASES)
def test_tables_reproduce_the_pil_fixtures(golden, case):
    g = golden("preprocess_cases")
    src, pil, msrc, mpil = (g[f"{case}_{k}"] for k in ("src", "pil", "msrc", "mpil"))
    ho, wo = pil.shape[1:3]
    for f in range(src.shape[0]):
        assert np.array_equal(P.apply_tables_numpy(src[f], ho, wo), pil[f]), f"case {case} frame {f}: bilinear tables differ from PIL"
        assert np.array_equal(_nearest(msrc[f], ho, wo), mpil[f]), f"case {case} frame {f}: nearest table differs from PIL"


@pytest.mark.parametrize("pair", LIVE_PAIRS, ids=lambda p: f"{p[0][0]}x{p[0][1]}-{p[1][0]}x{p[1][1]}")
def test_tables_equal_live_pil(pair):
    Image = pytest.importorskip("PIL.Image")
    (hs, ws), (ho, wo) = pair
    rng = np.random.default_rng(hs * 10007 + ws)
    img = rng.integers(0, 256, (hs, ws, 3), dtype=np.uint8)
    ref = np.asarray(Image.fromarray(img, "RGB").resize((wo, ho), Image.BILINEAR))
    assert np.array_equal(P.apply_tables_numpy(img, ho, wo), ref)
    mask = rng.integers(0, 3, (hs, ws), dtype=np.uint8)
    mref = np.asarray(Image.fromarray(mask, "L").resize((wo, ho), Image.NEAREST))
    assert np.array_equal(_nearest(mask, ho, wo), mref)


@pytest.mark.parametrize("sizes", [(1280, 480), (720, 480), (53, 32), (96, 32), (17, 32), (134, 20), (7, 32), (1, 8), (200, 130), (50, 33), (40000, 1), (3, 1000)])
def test_table_invariants(sizes):
    n_in, n_out = sizes
    coef, bounds = P.resample_tables(n_in, n_out)
    ksize = int(np.ceil(max(n_in / n_out, 1.0))) * 2 + 1
    assert coef.dtype == np.int32 and bounds.dtype == np.int32 and coef.shape == (n_out, ksize) and bounds.shape == (n_out, 2)
    assert (coef >= 0).all()
    assert (np.abs(coef.astype(np.int64).sum(1) - (1 << 22)) <= ksize).all(), "every row sums to 2^22 within one rounding per tap"
    xmin, n = bounds[:, 0].astype(np.int64), bounds[:, 1].astype(np.int64)
    assert (xmin >= 0).all() and (n >= 1).all() and (n <= ksize).all() and (xmin + n <= n_in).all()
    assert (np.diff(xmin) >= 0).all() and (np.diff(xmin + n) >= 0).all(), "the tile rule reads the first and last row of a tile only"
    for xx in range(0, n_out, max(n_out // 7, 1)):
        assert (coef[xx, n[xx]:] == 0).all()
    idx = P.nearest_table(n_in, n_out)
    assert idx.dtype == np.int32 and idx.shape == (n_out,) and idx.min() >= 0 and idx.max() <= n_in - 1 and (np.diff(idx) >= 0).all()
    assert P.resample_tables(n_in, n_out)[0] is coef, "tables are cached per (in, out)"


@pytest.mark.parametrize("n", [1, 8, 480])
def test_identity_tables(n):
    coef, bounds = P.resample_tables(n, n)
    assert coef.shape == (n, 3)
    assert (coef == np.array([1 << 22, 0, 0], dtype=np.int32)).all()
    assert (bounds[:, 0] == np.arange(n)).all(), "the one nonzero tap sits on the pixel itself (a second tap of weight 0 may be in range)"
    assert (P.nearest_table(n, n) == np.arange(n)).all()


def test_bad_sizes_raise():
    for fn in (P.resample_tables, P.nearest_table):
        with pytest.raises(ValueError):
            fn(0, 8)
        with pytest.raises(ValueError):
            fn(8, 0)
    with pytest.raises(ValueError):
        P.FramePreprocessor(32, std=(0.2, 0.0, 0.2))


def test_c_entry_refuses_a_span_beyond_lds_without_launching():
    """400 -> 1 rows: the single output row reads 400 source rows x 192 bytes > 64 KB.  The argument check returns LAVT_ERR_INVALID before anything is
    launched (this test has no GPU: the pointers are host memory that a launch could not use)."""
    from lavt_hip import _capi as K
    hs, ws = 400, 4
    cx, bx = P.resample_tables(ws, 1)
    cy, by = P.resample_tables(hs, 1)
    src, out = np.zeros((hs, ws, 3), np.uint8), np.zeros((3, 1, 1), np.float32)
    rc = K.lib.lavt_resize_norm_u8(src.ctypes.data, src.size, 1, hs, ws, cx.ctypes.data, bx.ctypes.data, cx.shape[1], cy.ctypes.data, by.ctypes.data, cy.shape[1],
                                   by.ctypes.data, out.ctypes.data, 1, 1, 0.5, 0.5, 0.5, 0.25, 0.25, 0.25, None)
    assert rc == -22 and b"LDS" in K.lib.lavt_last_error()
    bad = by.copy()
    bad[0, 1] = hs + 1          # a row range outside the source
    rc = K.lib.lavt_resize_norm_u8(src.ctypes.data, src.size, 1, hs, ws, cx.ctypes.data, bx.ctypes.data, cx.shape[1], cy.ctypes.data, by.ctypes.data, cy.shape[1],
                                   bad.ctypes.data, out.ctypes.data, 1, 1, 0.5, 0.5, 0.5, 0.25, 0.25, 0.25, None)
    assert rc == -22 and b"bounds_y_host" in K.lib.lavt_last_error()
    rc = K.lib.lavt_resize_norm_u8(src.ctypes.data, src.size - 1, 1, hs, ws, cx.ctypes.data, bx.ctypes.data, cx.shape[1], cy.ctypes.data, by.ctypes.data, cy.shape[1],
                                   by.ctypes.data, out.ctypes.data, 1, 1, 0.5, 0.5, 0.5, 0.25, 0.25, 0.25, None)
    assert rc == -22 and b"frame_stride" in K.lib.lavt_last_error()


def test_no_cpu_fallback():
    """CPU tensors are refused with the project's message; host input needs a GPU to be uploaded to: neither path computes anything on the CPU"""
    pp = P.FramePreprocessor(32)
    with pytest.raises(RuntimeError, match="GPU memory only.*no CPU fallback"):
        pp.images(torch.zeros(1, 40, 50, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="GPU memory only.*no CPU fallback"):
        pp.targets(torch.zeros(1, 40, 50, dtype=torch.uint8))
    from lavt_hip import ops
    with pytest.raises(RuntimeError, match="GPU memory only.*no CPU fallback"):
        ops.resize_normalize_u8(torch.zeros(1, 40, 50, 3, dtype=torch.uint8), torch.zeros(1, 3, 32, 32), P.MEAN, P.STD)
    with pytest.raises(RuntimeError, match="GPU memory only.*no CPU fallback"):
        ops.resize_nearest_u8(torch.zeros(1, 40, 50, dtype=torch.uint8), torch.zeros(1, 32, 32, dtype=torch.int64))
    if not torch.cuda.is_available():
        import transforms
        t = transforms.get_device_transform(32)
        with pytest.raises(RuntimeError, match="GPU memory only.*no CPU fallback"):
            t(np.zeros((40, 50, 3), np.uint8), np.zeros((40, 50), np.uint8))
        with pytest.raises(RuntimeError, match="GPU memory only.*no CPU fallback"):
            pp.images(np.zeros((1, 40, 50, 3), np.uint8))
        with pytest.raises(RuntimeError, match="GPU memory only.*no CPU fallback"):
            pp.images([np.zeros((40, 50, 3), np.uint8)])


def test_load_frames_is_part_of_the_predictor():
    from lavt_hip.engine import Predictor
    import inspect
    ps = inspect.signature(Predictor.load_frames).parameters
    assert list(ps) == ["self", "frames_u8", "targets_u8"] and ps["targets_u8"].default is None
