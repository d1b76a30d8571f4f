"""GPU checks of the J&F measure on the device: lavt_boundary_counts (csrc/jf_measure.hip) against the yardstick tests/jf_ref.py -- integers, so every
comparison is exact --, lavt_jf_meter_append (csrc/meters.hip) against the host form of its block byte for byte, both inside one captured graph,
and Predictor(jf_meter=) on the micro video model of tests/test_gpu_infer.py.

The boundary pass works on tiles of 64 rows x 256 columns (one 64-bit word of a row per thread, 4 words per tile row) with a halo of bound_pix
rows and one word; the pack pass on runs of 64 words.  So the frames below include 65 x 257 (tile + 1 in each direction, more than one workgroup
both ways), 65 x 129 and 130 x 67 (a partial last word, two and three tile rows), 64 x 64 (exactly one word, one tile) and 1 x 1 / 5 x 7 (smaller
than any halo)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import jf_ref
from lavt_hip import metrics as M
from lavt_hip.detweights import det_inputs, fill_state_dict_

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FRAMES = [(1, 1), (5, 7), (37, 53), (64, 64), (65, 129), (130, 67), (65, 257)]
RADII = [1, 2, 3, 5, 12, M.BOUNDARY_MAX_RADIUS]


def _shift(m, dy, dx):
    """m moved by (dy, dx), zero fill"""
    H, W = m.shape
    out = np.zeros_like(m)
    if dy < H and dx < W:
        out[dy:, dx:] = m[:H - dy, :W - dx]
    return out


def _blobs(rng, H, W, density):
    coarse = rng.random(((H + 2) // 3, (W + 2) // 3)) < density
    return np.kron(coarse, np.ones((3, 3), dtype=bool))[:H, :W]


def _pairs(H, W, r):
    """the mask pairs of the case table for one frame size and radius -> (P, G) uint8 (n, H, W); deterministic"""
    rng = np.random.default_rng(1000 * H + W)
    z, o = np.zeros((H, W), bool), np.ones((H, W), bool)
    pairs = [(z, z), (o, o), (z, o), (o, z)]
    pix = []
    for y, x in [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H - 1, W // 2), (H // 2, W - 1)]:
        m = z.copy()
        m[y, x] = True
        pix.append(m)
    for k, m in enumerate(pix):
        pairs += [(m, m), (m, pix[(k + 1) % len(pix)])]
    pairs.append((pix[0], z))
    yy, xx = np.mgrid[0:H, 0:W]
    checker = (yy + xx) % 2 == 0
    pairs += [(checker, checker), (checker, ~checker)]
    for d in (0.05, 0.5, 0.95):
        pairs.append((_blobs(rng, H, W, d), _blobs(rng, H, W, d)))
    pairs.append((rng.random((H, W)) < 0.5, rng.random((H, W)) < 0.05))          # (pixel noise: every word of the row differs)
    sq = z.copy()
    sq[H // 4:H // 2 + 1, W // 4:W // 2 + 1] = True
    # exactly r and r + 1 along x, along y; the diagonals on a Pythagorean disk edge: (3, 4) inside and (4, 4) outside at r = 5, (24, 32) and (25, 32) at r = 40
    for dy, dx in [(0, r), (0, r + 1), (r, 0), (r + 1, 0), (3, 4), (4, 4), (24, 32), (25, 32)]:
        pairs.append((sq, _shift(sq, dy, dx)))
    one = z.copy()
    one[H // 4, W // 4] = True
    for dy, dx in [(0, r), (0, r + 1), (r, 0), (r + 1, 0), (3, 4), (4, 4), (24, 32), (25, 32)]:
        pairs.append((one, _shift(one, dy, dx)))
    P = np.stack([p for p, _ in pairs]).astype(np.uint8)
    G = np.stack([g for _, g in pairs]).astype(np.uint8)
    return P, G


_REF = {}


def _case(H, W, r):
    """(P, G, reference counts int64 (n, 6)) of a frame size and radius: computed once, shared, never modified"""
    key = (H, W, r)
    if key not in _REF:
        P, G = _pairs(H, W, r)
        ref = jf_ref.counts_batch(P, G, r)
        for a in (P, G, ref):
            a.setflags(write=False)
        _REF[key] = (P, G, ref)
    return _REF[key]


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _counts(P, G, r, **kw):
    from lavt_hip import ops
    out = ops.boundary_counts(P, G, r, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("H,W", FRAMES)
def test_case_table(H, W, r):
    """all six integers of every frame equal the yardstick; columns 6 and 7 are zero"""
    P, G, ref = _case(H, W, r)
    got = _counts(_dev(P), _dev(G, torch.int64), r)
    assert got.dtype == np.int32 and got.shape == (P.shape[0], 8)
    bad = np.nonzero((got[:, :6] != ref).any(axis=1))[0]
    assert bad.size == 0, f"{H}x{W} r={r}: pairs {bad.tolist()[:8]} differ, first: got {got[bad[0]].tolist()} want {ref[bad[0]].tolist()}"
    assert not got[:, 6:].any()


def test_davis_radius_is_the_default():
    P, G, ref = _case(37, 53, 1)          # ceil(0.008 * sqrt(37^2 + 53^2)) = 1
    from lavt_hip import ops
    got = ops.boundary_counts(_dev(P), _dev(G, torch.int64)).cpu().numpy()
    assert M.davis_bound_pix(37, 53) == 1 and np.array_equal(got[:, :6], ref)


@pytest.mark.parametrize("H,W,r", [(37, 53, 12), (65, 129, 5), (5, 7, 40)])
def test_frames_do_not_leak_into_each_other(H, W, r):
    """five different frames in one call equal five calls of one frame: a halo never reaches the frame next in memory"""
    rng = np.random.default_rng(7)
    P = (rng.random((5, H, W)) < 0.5).astype(np.uint8)
    G = (rng.random((5, H, W)) < 0.3).astype(np.uint8)
    P[1], G[3] = 1, 0          # a full frame between two noisy ones, an empty one
    ref = jf_ref.counts_batch(P, G, r)
    dP, dG = _dev(P), _dev(G, torch.int64)
    together = _counts(dP, dG, r)
    alone = np.concatenate([_counts(dP[k:k + 1], dG[k:k + 1], r) for k in range(5)])
    assert np.array_equal(together, alone) and np.array_equal(together[:, :6], ref)


def test_target_types_and_foreground_values():
    """uint8 and int64 targets; 255, 7 and 1 << 32 are foreground"""
    H, W, r = 37, 53, 3
    rng = np.random.default_rng(9)
    P = (rng.random((3, H, W)) < 0.4).astype(np.uint8) * 255
    G = rng.random((3, H, W)) < 0.4
    ref = jf_ref.counts_batch(P, G, r)
    for value in (1, 7, 255):
        assert np.array_equal(_counts(_dev(P), _dev(G.astype(np.uint8) * value), r)[:, :6], ref)
        assert np.array_equal(_counts(_dev(P), _dev(G.astype(np.int64) * value), r)[:, :6], ref)
    assert np.array_equal(_counts(_dev(P), _dev(G.astype(np.int64) << 32), r)[:, :6], ref)
    mixed = G.astype(np.int64) * rng.choice([1, 7, 255, 1 << 32, -1], size=G.shape)
    assert np.array_equal(_counts(_dev(P), _dev(mixed), r)[:, :6], ref)


def test_every_row_is_overwritten():
    P, G, ref = _case(65, 129, 5)
    dP, dG = _dev(P), _dev(G, torch.int64)
    out = torch.full((P.shape[0], 8), 0x7f7f7f7f, dtype=torch.int32, device=DEV)
    first = _counts(dP, dG, 5, out=out).copy()
    assert np.array_equal(first[:, :6], ref) and not first[:, 6:].any()
    second = _counts(dP, dG, 5, out=out)
    assert np.array_equal(first, second)


def test_bad_arguments_leave_counts_alone():
    from lavt_hip import _capi as K
    n, H, W = 2, 9, 70
    pred = torch.ones(n, H, W, dtype=torch.uint8, device=DEV)
    t8 = torch.ones(n, H, W, dtype=torch.uint8, device=DEV)
    t64 = torch.ones(n, H, W, dtype=torch.int64, device=DEV)
    words = int(K.lib.lavt_boundary_counts_ws(n, H, W))
    assert words == 2 * n * H * 2
    ws = torch.empty(words, dtype=torch.int64, device=DEV)
    counts = torch.full((n, 8), 0x5a5a5a5a, dtype=torch.int32, device=DEV)
    p, a, b, w, c, st = K.ptr(pred), K.ptr(t8), K.ptr(t64), K.ptr(ws), K.ptr(counts), K.stream()
    bad = [
        (None, None, b, n, H, W, 1, w, words, c),          # null pred
        (p, a, b, n, H, W, 1, w, words, c),                # both targets
        (p, None, None, n, H, W, 1, w, words, c),          # neither
        (p, None, b, 0, H, W, 1, w, words, c),
        (p, None, b, n, 0, W, 1, w, words, c),
        (p, None, b, n, H, -1, 1, w, words, c),
        (p, None, b, n, H, W, 0, w, words, c),
        (p, None, b, n, H, W, M.BOUNDARY_MAX_RADIUS + 1, w, words, c),
        (p, None, b, n, H, W, 1, None, words, c),          # no scratch
        (p, None, b, n, H, W, 1, w, words - 1, c),         # scratch below the query
    ]
    for args in bad:
        assert K.lib.lavt_boundary_counts(*args, st) == -22, args
    assert K.lib.lavt_boundary_counts(p, None, b, n, H, W, 1, w, words, None, st) == -22          # null counts
    torch.cuda.synchronize()
    assert (counts == 0x5a5a5a5a).all()
    assert K.lib.lavt_boundary_counts(p, None, b, n, H, W, 1, w, words, c, st) == 0
    torch.cuda.synchronize()
    assert counts[:, :6].cpu().tolist() == [[H * W, H * W, 0, 0, 0, 0]] * n
    meter = M.DeviceJFMeter(capacity=4)
    before = meter.read()
    assert K.lib.lavt_jf_meter_append(c, None, 3, 2, K.ptr(meter.block), 4, st) == -22             # 3 frames are not sequences of 2
    assert K.lib.lavt_jf_meter_append(None, None, 2, 2, K.ptr(meter.block), 4, st) == -22
    assert K.lib.lavt_jf_meter_append(c, None, 2, 0, K.ptr(meter.block), 4, st) == -22
    after = meter.read()
    assert before.header.tobytes() == after.header.tobytes() and before.ring.tobytes() == after.ring.tobytes()


def _rows(rng, n):
    """count rows with every edge of the F rules: U == 0, an empty boundary on one side, on both, p + r == 0"""
    rows = np.zeros((n, 8), dtype=np.int32)
    rows[:, 1] = rng.integers(1, 5000, n)
    rows[:, 0] = (rows[:, 1] * rng.random(n)).astype(np.int32)
    rows[:, 2], rows[:, 3] = rng.integers(1, 300, n), rng.integers(1, 300, n)
    rows[:, 4], rows[:, 5] = (rows[:, 2] * rng.random(n)).astype(np.int32), (rows[:, 3] * rng.random(n)).astype(np.int32)
    rows[0::7, :2] = 0
    rows[1::7, 2], rows[1::7, 4] = 0, 0
    rows[2::7, 3], rows[2::7, 5] = 0, 0
    rows[3::7, 2:6] = 0
    rows[4::7, 4:6] = 0
    return rows


def _same_block(snap, ref):
    assert snap.header.tobytes() == ref.header.tobytes(), (snap.header.tolist(), ref.header.tolist())
    assert snap.ring.tobytes() == ref.ring.tobytes()


def test_meter_block_matches_the_host_form():
    """three appends, then with live, with hold set, and across a ring wrap: header and ring byte for byte"""
    rng = np.random.default_rng(5)
    cap = 5
    meter = M.DeviceJFMeter(capacity=cap)
    ref = None
    for k, (n, T) in enumerate([(6, 3), (140, 70), (8, 1)]):          # (140: more than one chunk of 64 frames, a sequence across the chunk edge)
        rows = _rows(rng, n)
        meter.append(_dev(rows), T)
        ref = M.reference_jf_block(rows, T, cap, block=ref)
        _same_block(meter.read(), ref)
    assert ref.n == 2 + 2 + 8 and ref.n > cap          # the ring has wrapped
    rows = _rows(rng, 12)
    live = np.array([1, 0, 1, 0, 0, 0, 1, 1, 1, 0, 0, 1], dtype=np.int32)          # the second sequence of 3 has no live frame
    meter.append(_dev(rows), 3, live=_dev(live))
    ref = M.reference_jf_block(rows, 3, cap, live=live, block=ref)
    snap = meter.read()
    _same_block(snap, ref)
    assert snap.n == 12 + 3
    meter.pause()
    meter.append(_dev(rows), 3)
    meter.resume()
    _same_block(meter.read(), ref)
    # reset keeps the running number; a state dict comes back bit for bit
    state = meter.state_dict()
    meter.reset()
    snap = meter.read()
    assert snap.n == 15 and snap.sequences == 0 and snap.frames == 0
    meter.load_state_dict(state)
    _same_block(meter.read(), ref)
    s, want = meter.read().summary(), ref.summary()
    assert s == want and s["J&F"] == (s["J"] + s["F"]) / 2.0


def test_counts_and_append_in_one_graph():
    """boundary_counts + append captured once; three replays with new masks in the static buffers; the block equals the host reference"""
    from lavt_hip import ops
    n, H, W, r, T, cap = 4, 37, 53, 3, 2, 4
    rng = np.random.default_rng(21)
    P = torch.zeros(n, H, W, dtype=torch.uint8, device=DEV)
    G = torch.zeros(n, H, W, dtype=torch.int64, device=DEV)
    counts = torch.full((n, 8), -1, dtype=torch.int32, device=DEV)
    meter = M.DeviceJFMeter(capacity=cap)
    meter.pause()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.boundary_counts(P, G, r, out=counts)
        meter.append(counts, T)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.boundary_counts(P, G, r, out=counts)
        meter.append(counts, T)
    meter.resume()
    assert meter.read().n == 0          # warm-up and capture stored nothing
    ref = None
    for _ in range(3):
        p, t = (rng.random((n, H, W)) < 0.4).astype(np.uint8), (rng.random((n, H, W)) < 0.4).astype(np.int64) * 255
        P.copy_(_dev(p))
        G.copy_(_dev(t))
        g.replay()
        want = jf_ref.counts_batch(p, t, r)
        torch.cuda.synchronize()
        assert np.array_equal(counts.cpu().numpy()[:, :6], want)
        ref = M.reference_jf_block(want, T, cap, block=ref)
    _same_block(meter.read(), ref)
    assert ref.n == 6


# ---------------------------------------------------------------------------------------------- Predictor (the micro video model of test_gpu_infer.py)
def _video_model(golden):
    from lib._utils import LAVTVideo
    from lib.mask_predictor import SimpleDecoding
    from lib.video_swin_transformer import MultiModalSwinTransformer3D
    g = golden("video_forward_feats")
    a = SimpleNamespace()
    bb = MultiModalSwinTransformer3D(patch_size=(1, 4, 4), embed_dim=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8], window_size=(8, 7, 7),
                                     drop_path_rate=0.0, patch_norm=True, out_indices=(0, 1, 2, 3), use_checkpoint=False,
                                     num_heads_fusion=[1, 1, 1, 1], fusion_drop=0.0, args=a)
    parts = torch.nn.ModuleDict({"backbone": bb, "classifier": SimpleDecoding(256, a)})
    fill_state_dict_(parts)
    parts.to(DEV)
    frames, l, m, _ = det_inputs(2, 64, 22, seed=int(g["seed"]), frames=4)
    frames, l, m = frames.to(DEV), l.to(DEV), m.to(DEV)

    class _Text(torch.nn.Module):
        def forward(self, ids, attention_mask=None):
            return (l.permute(0, 2, 1),)

    model = LAVTVideo.__new__(LAVTVideo)
    torch.nn.Module.__init__(model)
    model.backbone, model.classifier, model.text_encoder = parts["backbone"], parts["classifier"], _Text()
    model.lazy_pred, model.seg_last = False, False
    model.eval()
    ids, am = torch.zeros(2, 22, dtype=torch.long, device=DEV), m.squeeze(-1).contiguous()
    return model, frames, ids, am


@pytest.fixture(autouse=True)
def _fp32():
    import lavt_hip
    lavt_hip.set_compute_dtype(torch.float32)
    yield
    lavt_hip.set_compute_dtype(torch.float32)


OUT = (96, 160)          # the "original frame size": bound_pix = ceil(0.008 * sqrt(96^2 + 160^2)) = 2


def _targets(seed):
    rng = np.random.default_rng(seed)
    t = np.stack([_blobs(rng, OUT[0], OUT[1], 0.4) for _ in range(8)]).astype(np.int64)
    t[3] = 0          # a frame without ground truth
    return t


@pytest.mark.parametrize("use_graph", [True, False], ids=["captured", "eager"])
def test_predictor_jf_meter(golden, use_graph):
    from lavt_hip.engine import Predictor
    from lavt_hip.metrics import DeviceEvalMeter, DeviceJFMeter, reference_block
    model, frames, ids, am = _video_model(golden)
    assert M.davis_bound_pix(*OUT) == 2
    tgt = torch.zeros(8, *OUT, dtype=torch.int64, device=DEV)
    plain = Predictor(model, frames, ids, am, target=tgt, out_size=OUT, use_graph=use_graph)
    plain.warmup_and_capture()
    p = Predictor(model, frames, ids, am, target=tgt, out_size=OUT, use_graph=use_graph, meter=DeviceEvalMeter(capacity=64))
    jf = p.make_jf_meter(capacity=8)
    assert p.jf_meter is jf
    p.warmup_and_capture()
    assert p.captured == plain.captured == use_graph
    assert jf.read().n == 0 and p.meter.read().n == 0          # both meters were paused
    ref_jf, iu_rows, host = None, [], M.JFMeter()
    for step in range(2):
        t = _targets(step)
        tgt.copy_(_dev(t))
        m0 = plain.step().clone()
        iu0 = plain.iu.clone()
        m1 = p.step()
        torch.cuda.synchronize()
        assert torch.equal(m0, m1) and torch.equal(iu0, p.iu)          # bit-identical to the predictor without the J&F meter
        assert plain.jf is None and tuple(p.jf.shape) == (8, 8)
        want = jf_ref.counts_batch(m1.cpu().numpy(), t, 2)
        got = p.jf.cpu().numpy()
        assert np.array_equal(got[:, :6], want) and not got[:, 6:].any()
        assert torch.equal(p.jf[:, :2], p.iu)
        ref_jf = M.reference_jf_block(want, 4, 8, block=ref_jf)          # (B, T, 3, H, W): sequences of T = 4 frames
        host.update(p.jf, [2 * step + k // 4 for k in range(8)])         # the host meter, same grouping
        iu_rows += p.iu.cpu().tolist()
    _same_block(jf.read(), ref_jf)
    assert ref_jf.n == 4 and ref_jf.frames == 16
    ev, ev_ref = p.meter.read(), reference_block(iu_rows, 64)
    assert ev.header.tobytes() == ev_ref.header.tobytes() and ev.ring.tobytes() == ev_ref.ring.tobytes()
    s = jf.read().summary()
    assert s == host.summary() and s["sequences"] == 4 and s["frames"] == 16 and 0.0 <= s["J&F"] <= 100.0


def test_predictor_jf_sequence_length_and_refusals(golden):
    from lavt_hip.engine import Predictor
    from lavt_hip.metrics import DeviceJFMeter
    model, frames, ids, am = _video_model(golden)
    tgt = torch.zeros(8, *OUT, dtype=torch.int64, device=DEV)
    meter = DeviceJFMeter(capacity=4)
    with pytest.raises(ValueError):          # 1. no target
        Predictor(model, frames, ids, am, out_size=OUT, jf_meter=meter)
    with pytest.raises(ValueError):          # 2. valid_indices
        Predictor(model, frames, ids, am, target=tgt[:2], out_size=OUT, jf_meter=meter, valid_indices=torch.tensor([1, 5], dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):          # 3. image_of
        Predictor(model, frames, ids, am, target=tgt, out_size=OUT, jf_meter=meter, image_of=torch.zeros(2, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):          # 4. expressions_per_image > 1
        Predictor(model, frames, ids.repeat(2, 1), am.repeat(2, 1), target=tgt, out_size=OUT, jf_meter=meter, expressions_per_image=2)
    with pytest.raises(ValueError):          # 8 frames are not sequences of 3
        Predictor(model, frames, ids, am, target=tgt, out_size=OUT, jf_meter=meter, jf_frames_per_sequence=3)
    p = Predictor(model, frames, ids, am, target=tgt, out_size=OUT, use_graph=False, jf_meter=meter, jf_frames_per_sequence=8)
    with pytest.raises(RuntimeError):
        p.attach_jf_meter(DeviceJFMeter(capacity=4))
    p.warmup_and_capture(eager_iters=1)
    p.step()
    snap = meter.read()
    assert snap.n == 1 and int(snap.ring[0]["frames"]) == 8
    late = Predictor(model, frames, ids, am, target=tgt, out_size=OUT, use_graph=False)
    late.warmup_and_capture(eager_iters=1)
    with pytest.raises(RuntimeError):          # the launch sequence is frozen
        late.make_jf_meter()
