"""GPU checks of the device-side frame preprocessing (csrc/preprocess.hip, lavt_hip.preprocess, Predictor.load_frames) against what PIL gives
(tests/golden/preprocess_cases.npz: sources and PIL's uint8 results; generator beside it) finished with the reference's three fp32 operations.

Bounds: the integer stage is exact (PIL's uint8 on every pixel).  The fp32 result lies in [-2.12, 2.64], where fp32 spacing is at most 2.4e-7; the
operations are the reference's own, so equality is expected, and 1e-6 allows a differently rounded division and nothing larger."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from lavt_hip import preprocess as P
from lavt_hip.detweights import det_inputs, fill_state_dict_

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = "abcdefgh"
MEAN_T, STD_T = torch.tensor(P.MEAN, dtype=torch.float32).view(-1, 1, 1), torch.tensor(P.STD, dtype=torch.float32).view(-1, 1, 1)
TOL = 1e-6


def _expected(pil_u8):
    """ToTensor + Normalize of the reference (transforms.py:83-87, 106-113) on PIL's uint8 (N, H, W, 3), on the CPU"""
    t = torch.from_numpy(np.ascontiguousarray(pil_u8)).permute(0, 3, 1, 2).to(torch.float32).div(255)
    return (t - MEAN_T) / STD_T


def _check_images(out, pil_u8, what):
    out = out.cpu()
    assert not torch.isnan(out).any(), f"{what}: NaN survived (pixels not written)"
    err = float((out - _expected(pil_u8)).abs().max())
    back = torch.round((out.double() * STD_T.double() + MEAN_T.double()) * 255).to(torch.int64).permute(0, 2, 3, 1)
    wrong = int((back != torch.from_numpy(pil_u8.astype(np.int64))).sum())
    print(f"\n[{what}] max |out - expected| = {err:.3e}, pixels whose integer stage differs from PIL: {wrong}")
    assert wrong == 0
    assert err <= TOL


# ================================================================================================ kernels against the fixtures
@pytest.mark.parametrize("case", CASES)
def test_resize_normalize_fixture(golden, case):
    from lavt_hip import ops
    g = golden("preprocess_cases")
    src, pil = g[f"{case}_src"], g[f"{case}_pil"]
    n, hs, ws, _ = src.shape
    ho, wo = pil.shape[1:3]
    if case == "h":
        # the frames are cut from a larger upload: 517 bytes of 255 after every frame, which no pixel of the expected result contains
        frame = hs * ws * 3
        big = torch.full((n, frame + 517), 255, dtype=torch.uint8)
        big[:, :frame] = torch.from_numpy(src).view(n, frame)
        dsrc = big.to(DEV)[:, :frame].view(n, hs, ws, 3)
        assert not dsrc.is_contiguous() and dsrc.stride(0) == frame + 517
    else:
        dsrc = torch.from_numpy(src).to(DEV)
    out = torch.full((n, 3, ho, wo), float("nan"), device=DEV)
    ops.resize_normalize_u8(dsrc, out, P.MEAN, P.STD)
    torch.cuda.synchronize()
    _check_images(out, pil, f"case {case} {hs}x{ws}->{ho}x{wo}")


@pytest.mark.parametrize("case", CASES)
def test_resize_nearest_fixture(golden, case):
    from lavt_hip import ops
    g = golden("preprocess_cases")
    msrc, mpil = g[f"{case}_msrc"], g[f"{case}_mpil"]
    n, hs, ws = msrc.shape
    if case == "h":
        big = torch.full((n, hs * ws + 33), 7, dtype=torch.uint8)
        big[:, :hs * ws] = torch.from_numpy(msrc).view(n, -1)
        dsrc = big.to(DEV)[:, :hs * ws].view(n, hs, ws)
    else:
        dsrc = torch.from_numpy(msrc).to(DEV)
    out = torch.full(mpil.shape, -1, dtype=torch.int64, device=DEV)
    ops.resize_nearest_u8(dsrc, out)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.from_numpy(mpil.astype(np.int64)))


@pytest.mark.parametrize("sizes,th", [(((700, 8), (24, 8)), 8), (((640, 70), (12, 66)), 4), (((700, 8), (10, 5)), 2), (((1200, 12), (8, 9)), 1)])
def test_tile_heights_below_16(sizes, th):
    """Strong vertical downscales, where the source-row span of a 16-row tile exceeds 64 KB of LDS and the entry takes a lower tile (the expected TH is
    recomputed here from the rule: largest of 16, 8, 4, 2, 1 with span * 192 <= 65536).  Reference: the tables applied in numpy, which
    tests/test_preprocess_host.py holds equal to PIL (fixtures and live)."""
    from lavt_hip import ops
    (hs, ws), (ho, wo) = sizes
    _, by = P.resample_tables(hs, ho)
    fits = [t for t in (16, 8, 4, 2, 1)
            if max(int(by[min(r + t, ho) - 1].sum()) - int(by[r, 0]) for r in range(0, ho, t)) * 192 <= 65536]
    assert fits and fits[0] == th, (fits, th)
    src = np.random.default_rng(hs + ws).integers(0, 256, (2, hs, ws, 3), dtype=np.uint8)
    ref = np.stack([P.apply_tables_numpy(f, ho, wo) for f in src])
    out = torch.full((2, 3, ho, wo), float("nan"), device=DEV)
    ops.resize_normalize_u8(torch.from_numpy(src).to(DEV), out, P.MEAN, P.STD)
    torch.cuda.synchronize()
    _check_images(out, ref, f"TH={th} {hs}x{ws}->{ho}x{wo}")


# ================================================================================================ FramePreprocessor / get_device_transform
def test_frame_preprocessor_inputs(golden):
    """CUDA tensor, numpy array, list of arrays, with and without the pinned staging buffer, and `out=`: all the same bytes"""
    g = golden("preprocess_cases")
    src, pil, msrc, mpil = g["h_src"], g["h_pil"], g["h_msrc"], g["h_mpil"]
    pp = P.FramePreprocessor((16, 16))
    a = pp.images(torch.from_numpy(src).to(DEV))
    b = pp.images(src)
    c = pp.images([f for f in src])
    pp.reserve_staging(src.shape)
    d = pp.images(src)
    e = pp.images(src[::-1].copy())          # the staging buffer is reused: waits for the previous copy out of it
    buf = torch.full((3, 1, 3, 16, 16), float("nan"), device=DEV)
    assert pp.images(src, out=buf) is buf
    torch.cuda.synchronize()
    _check_images(a, pil, "FramePreprocessor.images")
    for other in (b, c, d, buf.view(3, 3, 16, 16), e.flip(0)):
        assert torch.equal(a, other)
    one = pp.images(src[1])
    assert tuple(one.shape) == (1, 3, 16, 16) and torch.equal(one[0], a[1])
    t = pp.targets(msrc)
    t1 = pp.targets(torch.from_numpy(msrc[2]).to(DEV))
    torch.cuda.synchronize()
    assert t.dtype == torch.int64 and torch.equal(t.cpu(), torch.from_numpy(mpil.astype(np.int64))) and torch.equal(t1[0], t[2])
    with pytest.raises(ValueError):
        pp.images(src, out=torch.empty(3, 3, 16, 17, device=DEV))
    with pytest.raises(TypeError):
        pp.images(src.astype(np.float32))


def test_device_transform_equals_get_transform():
    """transforms.get_device_transform against the untouched CPU pipeline transforms.get_transform on the same PIL image and target"""
    from PIL import Image
    import transforms
    rng = np.random.default_rng(3)
    img = Image.fromarray(rng.integers(0, 256, (45, 70, 3), dtype=np.uint8), "RGB")
    tgt = Image.fromarray(rng.integers(0, 2, (45, 70), dtype=np.uint8), "L")
    ref_i, ref_t = transforms.get_transform(32)(img, tgt)
    dev_t = transforms.get_device_transform(32)
    got_i, got_t = dev_t(img, tgt)
    only_i, none_t = dev_t(img, None)
    torch.cuda.synchronize()
    assert got_i.is_cuda and got_i.dtype == ref_i.dtype and got_i.shape == ref_i.shape and got_t.dtype == ref_t.dtype and got_t.shape == ref_t.shape
    assert float((got_i.cpu() - ref_i).abs().max()) <= TOL
    assert torch.equal(got_t.cpu(), ref_t) and none_t is None and torch.equal(only_i, got_i)


# ================================================================================================ Predictor.load_frames
def _cpu_pipeline(frames, size, masks=None):
    """the parent's path: transforms.get_transform on PIL images, one frame at a time"""
    from PIL import Image
    import transforms
    tf = transforms.get_transform(size)
    pairs = [tf(Image.fromarray(f, "RGB"), None if masks is None else Image.fromarray(masks[i], "L")) for i, f in enumerate(frames)]
    return torch.stack([p[0] for p in pairs]), (None if masks is None else torch.stack([p[1] for p in pairs]))


@pytest.fixture(scope="module")
def swin_t():
    import lavt_hip
    from lib._utils import LAVT
    from lib.backbone import MultiModalSwinTransformer
    from lib.mask_predictor import SimpleDecoding
    args = SimpleNamespace(swin_type="tiny")
    bb = MultiModalSwinTransformer(embed_dim=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24], window_size=7, drop_path_rate=0.3, args=args)
    model = LAVT(bb, SimpleDecoding(768, args))
    fill_state_dict_(model)
    lavt_hip.set_compute_dtype(torch.float32)
    return model.to(DEV).eval()


@pytest.mark.parametrize("use_graph", [False, True])
def test_predictor_load_frames(swin_t, use_graph):
    """Swin-T 224^2 (the model of test_gpu_infer.py), source frames 150x200: the image buffer equals the CPU pipeline's tensor within 1e-6, the mask after
    load_frames equals, byte for byte, the mask after copying the CPU pipeline's tensor in; other frames change the mask without a re-capture."""
    import lavt_hip
    from lavt_hip import ops
    from lavt_hip.engine import Predictor
    lavt_hip.set_compute_dtype(torch.float32)
    rng = np.random.default_rng(11)
    # smooth content (a random 10 x 13 grid enlarged) so that the masks of the two frames are not noise
    coarse = rng.integers(0, 256, (2, 10, 13, 3), dtype=np.uint8)
    frames = np.stack([np.kron(c, np.ones((15, 16, 1), dtype=np.uint8))[:150, :200] for c in coarse])
    masks = rng.integers(0, 2, (2, 150, 200), dtype=np.uint8)
    ref_x, ref_t = _cpu_pipeline(frames, 224, masks)
    _, l, m, _ = det_inputs(1, 224, 20, seed=1234)
    x = torch.zeros(1, 3, 224, 224, device=DEV)
    tgt = torch.zeros(1, 224, 224, dtype=torch.int64, device=DEV)
    p = Predictor(swin_t, x, l.to(DEV), m.to(DEV), target=tgt, use_graph=use_graph, context=ops.StepContext())
    p.warmup_and_capture()
    assert p.captured == use_graph
    graph = p.graph

    p.load_frames(torch.from_numpy(frames[:1]).to(DEV), torch.from_numpy(masks[:1]).to(DEV))
    mask_dev = p.step().clone()
    iu_dev = p.iu.clone()
    torch.cuda.synchronize()
    err = float((p.x.cpu() - ref_x[:1]).abs().max())
    print(f"\n[load_frames use_graph={use_graph}] max |image buffer - CPU pipeline| = {err:.3e}, elements that differ: {int((p.x.cpu() != ref_x[:1]).sum())}")
    assert err <= TOL
    assert torch.equal(p.t.cpu(), ref_t[:1])

    p.x.copy_(ref_x[:1].to(DEV))
    mask_cpu = p.step().clone()
    torch.cuda.synchronize()
    assert torch.equal(mask_dev, mask_cpu), f"{int((mask_dev != mask_cpu).sum())} mask pixels differ between load_frames and the CPU pipeline's tensor"
    assert torch.equal(iu_dev, p.iu)

    p.load_frames(frames[1:2])          # host input, no target: the target buffer keeps the first frame's
    mask_other = p.step().clone()
    p.x.copy_(ref_x[1:2].to(DEV))
    mask_other_cpu = p.step().clone()
    torch.cuda.synchronize()
    assert p.graph is graph, "no re-capture"
    assert torch.equal(mask_other, mask_other_cpu)
    print(f"[load_frames] share of mask pixels the second frame moves: {float((mask_other != mask_dev).float().mean()):.4f}")
    assert not torch.equal(mask_other, mask_dev), "other frames must change the mask"
    assert torch.equal(p.t.cpu(), ref_t[:1])

    # errors: frame count, CPU tensor, target count
    with pytest.raises(ValueError, match="frames"):
        p.load_frames(torch.from_numpy(frames).to(DEV))
    with pytest.raises(RuntimeError, match="GPU memory only.*no CPU fallback"):
        p.load_frames(torch.from_numpy(frames[:1]))
    with pytest.raises(ValueError, match="target masks"):
        p.load_frames(frames[:1], masks)
    assert torch.equal(p.x.cpu(), ref_x[1:2]), "a refused call must not touch the buffers"


def test_load_frames_refuses_targets_of_another_size(swin_t):
    """the via_size flow of test_ytvos.py keeps targets at the original frame size: load_frames does not resize into such a buffer"""
    from lavt_hip.engine import Predictor
    _, l, m, _ = det_inputs(1, 224, 20, seed=1234)
    x = torch.zeros(1, 3, 224, 224, device=DEV)
    frames, masks = np.zeros((1, 150, 200, 3), np.uint8), np.zeros((1, 150, 200), np.uint8)
    p = Predictor(swin_t, x, l.to(DEV), m.to(DEV), target=torch.zeros(1, 150, 200, dtype=torch.int64, device=DEV), out_size=(150, 200), via_size=(224, 224))
    with pytest.raises(ValueError, match="network input size"):
        p.load_frames(frames, masks)
    p.load_frames(frames)
    q = Predictor(swin_t, x, l.to(DEV), m.to(DEV))
    with pytest.raises(ValueError, match="without a target"):
        q.load_frames(frames, masks)


def test_load_frames_video_layout():
    """LAVTVideo's image buffer (B, T, 3, H, W) is written as (B*T, 3, H, W): frame b*T + t of the input lands at [b, t].  Micro video model, T = 2."""
    from lavt_hip.engine import Predictor
    from lib._utils import LAVTVideo
    from lib.mask_predictor import SimpleDecoding
    from lib.video_swin_transformer import MultiModalSwinTransformer3D
    a = SimpleNamespace()
    bb = MultiModalSwinTransformer3D(patch_size=(1, 4, 4), embed_dim=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8], window_size=(8, 7, 7),
                                     drop_path_rate=0.0, patch_norm=True, out_indices=(0, 1, 2, 3), use_checkpoint=False,
                                     num_heads_fusion=[1, 1, 1, 1], fusion_drop=0.0, args=a)
    model = LAVTVideo.__new__(LAVTVideo)
    torch.nn.Module.__init__(model)
    model.backbone, model.classifier, model.text_encoder = bb, SimpleDecoding(256, a), torch.nn.Identity()
    model.lazy_pred, model.seg_last = False, False
    model.to(DEV).eval()
    B, T, S = 2, 2, 64
    x = torch.full((B, T, 3, S, S), float("nan"), device=DEV)
    tgt = torch.full((B * T, S, S), -1, dtype=torch.int64, device=DEV)
    p = Predictor(model, x, torch.zeros(B, 22, dtype=torch.long, device=DEV), torch.ones(B, 22, device=DEV), target=tgt)
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, (B * T, 50, 90, 3), dtype=np.uint8)
    masks = rng.integers(0, 2, (B * T, 50, 90), dtype=np.uint8)
    p.load_frames(frames, masks)
    torch.cuda.synchronize()
    ref_x, ref_t = _cpu_pipeline(frames, S, masks)
    assert p.x is x and float((x.cpu().view(B * T, 3, S, S) - ref_x).abs().max()) <= TOL
    for b in range(B):
        for t in range(T):
            assert float((x[b, t].cpu() - ref_x[b * T + t]).abs().max()) <= TOL
    assert torch.equal(tgt.cpu(), ref_t)
    with pytest.raises(ValueError, match="frames"):
        p.load_frames(frames[:B])


# ================================================================================================ errors of the C entry
def test_span_beyond_lds_is_refused_by_the_argument_check():
    """One output pixel from a 400 x 400 source: the single output row reads 400 source rows x 192 bytes > 64 KB of LDS, also at TH = 1.  The C entry
    returns LAVT_ERR_INVALID from its argument check: nothing is launched, the NaN-filled output is untouched.  Through the wrapper: RuntimeError."""
    from lavt_hip import _capi as K
    from lavt_hip import ops
    hs = ws = 400
    src = torch.zeros(1, hs, ws, 3, dtype=torch.uint8, device=DEV)
    out = torch.full((1, 3, 1, 1), float("nan"), device=DEV)
    cx, bx = P.device_resample_tables(ws, 1, src.device)
    cy, by = P.device_resample_tables(hs, 1, src.device)
    by_host = P.resample_tables(hs, 1)[1]
    rc = K.lib.lavt_resize_norm_u8(K.ptr(src), hs * ws * 3, 1, hs, ws, K.ptr(cx), K.ptr(bx), cx.shape[1], K.ptr(cy), K.ptr(by), cy.shape[1], by_host.ctypes.data,
                                   K.ptr(out), 1, 1, *P.MEAN, *P.STD, K.stream())
    assert rc == -22 and b"LDS" in K.lib.lavt_last_error()          # LAVT_ERR_INVALID
    with pytest.raises(RuntimeError, match="rc=-22.*LDS"):
        ops.resize_normalize_u8(src, out, P.MEAN, P.STD)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    # the same width against a source of few rows is fine: the width does not enter the LDS request
    out2 = torch.full((1, 3, 1, 1), float("nan"), device=DEV)
    ops.resize_normalize_u8(src[:, :3], out2, P.MEAN, P.STD)
    torch.cuda.synchronize()
    assert float((out2.cpu() - _expected(np.zeros((1, 1, 1, 3), np.uint8))).abs().max()) <= TOL
