"""GPU checks of the batched input stage: lavt_resize_norm_u8_batch / lavt_resize_nearest_u8_batch (csrc/preprocess.hip) through
lavt_hip.preprocess.BatchPreprocessor, TrainStep.load_batch / stage_batch / commit_batch and Predictor.load_batch.

References: PIL's results for batches of mixed-size sources (tests/golden/preprocess_batch_cases.npz, and cases a, b, c, e of preprocess_cases.npz as a
fourth batch) finished with the reference's three fp32 operations on the CPU, and the unchanged per-image route FramePreprocessor.images / .targets.
Every comparison is torch.equal: the integer stage is PIL's on every pixel and the three fp32 operations are IEEE operations in the reference's order,
so there is nothing to tolerate.  Sources of random content other than the fixtures take their expectation from apply_tables_numpy, which
tests/test_preprocess_host.py holds equal to PIL.

The train-step checks run the micro LAVT model of the suite's train-step tests at 64 x 64, the size those tests run it at."""
import numpy as np
import pytest
import torch

from lavt_hip import preprocess as P
from lavt_hip.detweights import det_inputs
from test_preprocess_batch_host import BATCHES, expected_images, expected_targets, load_batch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _neg(*shape):
    return torch.full(shape, -1, dtype=torch.int64, device=DEV)


def _per_image(images, masks, out):
    """the per-image route of the parent: one FramePreprocessor call per source"""
    pp = P.FramePreprocessor(out)
    x = torch.cat([pp.images(np.ascontiguousarray(a)) for a in images])
    t = torch.cat([pp.targets(np.ascontiguousarray(m)) for m in masks]) if masks is not None else None
    return x, t


def _random_batch(seed, sizes, out):
    """-> (images, masks, expected fp32 images, expected int64 targets) for sources of the given (H, W), by the host tables"""
    rng = np.random.default_rng(seed)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    masks = [rng.integers(0, 3, (h, w), dtype=np.uint8) for h, w in sizes]
    ex = expected_images([P.apply_tables_numpy(a, *out) for a in images])
    et = expected_targets([m[P.nearest_table(m.shape[0], out[0])][:, P.nearest_table(m.shape[1], out[1])] for m in masks])
    return images, masks, ex, et


# ================================================================================================ kernels against the fixtures
@pytest.mark.parametrize("name", BATCHES)
def test_batch_equals_pil_and_the_per_image_route(golden, name):
    src, pil, msrc, mpil, out = load_batch(golden, name)
    pp = P.BatchPreprocessor(out)
    x, t = pp.batch(src, msrc, out_images=_nan(len(src), 3, *out), out_targets=_neg(len(src), *out))
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), expected_images(pil)), f"batch {name}: {int((x.cpu() != expected_images(pil)).sum())} image values differ from PIL's"
    assert torch.equal(t.cpu(), expected_targets(mpil)), f"batch {name}: masks differ from PIL's"
    rx, rt = _per_image(src, msrc, out)
    for i in range(len(src)):
        assert torch.equal(x[i], rx[i]) and torch.equal(t[i], rt[i]), f"batch {name} item {i} differs from FramePreprocessor"
    # without targets, into fresh outputs
    x2, none = pp.batch(src)
    assert none is None and torch.equal(x2, x)


def test_repeat_and_maps(golden):
    src, pil, msrc, mpil, out = load_batch(golden, "v")
    pp = P.BatchPreprocessor(out)
    x, t = pp.batch(src, msrc, repeat=3)
    ex, et = expected_images(pil), expected_targets(mpil)
    assert tuple(x.shape) == (6, 3, *out) and torch.equal(x.cpu(), ex.repeat_interleave(3, 0)) and torch.equal(t.cpu(), et.repeat_interleave(3, 0))
    src, pil, msrc, mpil, out = load_batch(golden, "n")
    fm, tm = [3, 0, 4, 0, 2, 1], [1, 1, 0]
    x, t = P.BatchPreprocessor(out).batch(src, msrc[:2], frame_map=fm, target_map=tm)
    assert torch.equal(x.cpu(), expected_images(pil)[fm]) and torch.equal(t.cpu(), expected_targets(mpil)[tm])


def test_one_by_one_source():
    images, masks = [np.array([[[7, 130, 255]]], dtype=np.uint8)], [np.array([[2]], dtype=np.uint8)]
    x, t = P.BatchPreprocessor((5, 70)).batch(images, masks, out_images=_nan(1, 3, 5, 70), out_targets=_neg(1, 5, 70))
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), expected_images([np.broadcast_to(images[0], (5, 70, 3))])) and bool((t == 2).all())


def test_many_taps_and_tall_downscale():
    """one launch whose items ask for different tile heights: 700 -> 24 rows alone takes TH = 8 (tests/test_gpu_preprocess.py), so the launch does; the
    other items run with a tile lower than they would alone"""
    out = (24, 8)
    images, masks, ex, et = _random_batch(77, [(700, 8), (24, 8), (90, 134), (5, 3)], out)
    x, t = P.BatchPreprocessor(out).batch(images, masks, out_images=_nan(4, 3, *out), out_targets=_neg(4, *out))
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), ex) and torch.equal(t.cpu(), et)


# ================================================================================================ slots and events
def test_slot_reuse_keeps_every_batch_its_own():
    """five batches through the two slots, the next one staged before the current one's kernels have run (a matrix product queued in front of them keeps
    the stream busy), growing sizes so that both slots are re-allocated on the way: every committed result is its own batch's"""
    out = (32, 32)
    sizes = [[(20, 31), (33, 17)], [(48, 64), (64, 48), (30, 30)], [(150, 200)], [(200, 170), (1, 5)], [(9, 40), (41, 9)]]
    batches = [_random_batch(100 + i, s, out) for i, s in enumerate(sizes)]
    pp = P.BatchPreprocessor(out)
    busy = torch.randn(2048, 2048, device=DEV)
    xbuf, tbuf = _nan(3, 3, *out), _neg(3, *out)          # ONE output pair for all batches, as a train step's static buffers are
    got = []
    pp.stage(batches[0][0], batches[0][1])
    for i, (images, masks, _, _) in enumerate(batches):
        n = len(images)
        busy @ busy
        pp.commit(xbuf[:n], tbuf[:n])
        if i + 1 < len(batches):
            pp.stage(batches[i + 1][0], batches[i + 1][1])          # while batch i's kernels are still queued behind the product
        got.append((xbuf[:n].clone(), tbuf[:n].clone()))
    torch.cuda.synchronize()
    for i, ((x, t), (_, _, ex, et)) in enumerate(zip(got, batches)):
        assert torch.equal(x.cpu(), ex) and torch.equal(t.cpu(), et), f"batch {i} is not its own"
    assert pp._host[0].numel() >= 150 * 200 * 3 > 1 << 16 and pp._host[1].numel() >= 200 * 170 * 3, "both slots grew on the way"
    # a batch staged and never committed is dropped; commit without a staged batch is refused
    pp.stage(batches[1][0])
    pp.stage(batches[3][0], batches[3][1])
    x, t = pp.commit(_nan(2, 3, *out), _neg(2, *out))
    assert torch.equal(x.cpu(), batches[3][2]) and torch.equal(t.cpu(), batches[3][3])
    with pytest.raises(RuntimeError, match="no staged batch"):
        pp.commit(xbuf[:2], tbuf[:2])


# ================================================================================================ TrainStep / Predictor
def test_train_step_load_batch(monkeypatch):
    import lavt_hip
    from lavt_hip import ops
    from lavt_hip.engine import TrainStep
    from test_gpu_deterministic import _micro2d
    S = (64, 64)
    _, l, m, _ = det_inputs(2, 64, 20, seed=5)
    rng = np.random.default_rng(21)

    def smooth(h, w):          # smooth content (a coarse random grid enlarged), so that the loss is not that of noise
        return np.kron(rng.integers(0, 256, (h // 8 + 1, w // 8 + 1, 3), dtype=np.uint8), np.ones((8, 8, 1), dtype=np.uint8))[:h, :w]
    batch1 = ([smooth(50, 90), smooth(77, 41)], [rng.integers(0, 2, (50, 90), dtype=np.uint8), rng.integers(0, 2, (77, 41), dtype=np.uint8)])
    batch2 = ([smooth(64, 64), smooth(30, 100)], [rng.integers(0, 2, (64, 64), dtype=np.uint8), rng.integers(0, 2, (30, 100), dtype=np.uint8)])
    with lavt_hip.use_dtype(torch.float32):
        x, t = torch.zeros(2, 3, *S, device=DEV), torch.zeros(2, *S, dtype=torch.int64, device=DEV)
        step = TrainStep(_micro2d(), x, l.to(DEV), m.to(DEV), t, context=ops.StepContext(), deterministic=True)
        step.warmup_and_capture()
        assert step.captured
        graph = step.graph
        ref1, ref2 = _per_image(*batch1, S), _per_image(*batch2, S)

        step.load_batch(*batch1)
        assert step.x is x and step.t is t and torch.equal(x, ref1[0]) and torch.equal(t, ref1[1]), "load_batch differs from the per-image route"
        loss_batch = step.step().clone()
        x.zero_()
        t.zero_()
        x.copy_(ref1[0])
        t.copy_(ref1[1])
        loss_hand = step.step().clone()
        assert torch.equal(loss_batch, loss_hand), (float(loss_batch), float(loss_hand))

        # stage while the replay is running, commit behind it
        step.step()
        step.stage_batch(*batch2)
        assert torch.equal(x, ref1[0]), "stage_batch writes neither x nor t"
        step.commit_batch()
        assert torch.equal(x, ref2[0]) and torch.equal(t, ref2[1])
        loss_staged = step.step().clone()
        step.load_batch(*batch1)
        step.load_batch(*batch2)
        loss_loaded = step.step().clone()
        torch.cuda.synchronize()
        assert torch.equal(loss_staged, loss_loaded) and not torch.equal(loss_staged, loss_batch), (float(loss_staged), float(loss_loaded), float(loss_batch))
        assert step.graph is graph, "nothing re-captures"

        # refusals: nothing is written
        keep_x, keep_t = x.clone(), t.clone()
        with pytest.raises(ValueError, match="frames"):
            step.load_batch(batch1[0] + batch2[0], batch1[1])
        with pytest.raises(ValueError, match="target masks"):
            step.load_batch(batch1[0], batch1[1][:1])
        with pytest.raises(TypeError, match=r"FramePreprocessor\.images"):
            step.load_batch([torch.from_numpy(a).to(DEV) for a in batch1[0]], batch1[1])
        with pytest.raises(RuntimeError, match="no staged batch"):
            step.commit_batch()
        monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        for call in (lambda: step.load_batch(*batch1), lambda: step.stage_batch(*batch1), step.commit_batch):
            with pytest.raises(RuntimeError, match="outside the graph capture"):
                call()
        monkeypatch.undo()
        torch.cuda.synchronize()
        assert torch.equal(x, keep_x) and torch.equal(t, keep_t)


def test_predictor_load_batch_equals_load_frames():
    from lavt_hip import ops
    from lavt_hip.engine import Predictor
    from test_gpu_deterministic import _micro2d
    model = _micro2d().eval()
    S = (64, 64)
    _, l, m, _ = det_inputs(3, 64, 20, seed=5)
    l, m = l.to(DEV), m.to(DEV)
    images, masks, _, _ = _random_batch(31, [(50, 90), (77, 41), (64, 64)], S)
    x, t = _nan(3, 3, *S), _neg(3, *S)
    Predictor(model, x, l, m, target=t, context=ops.StepContext()).load_batch(images, masks)
    rx, rt = _nan(3, 3, *S), _neg(3, *S)
    for i in range(3):
        Predictor(model, rx[i:i + 1], l[i:i + 1], m[i:i + 1], target=rt[i:i + 1], context=ops.StepContext()).load_frames(images[i][None], masks[i][None])
    torch.cuda.synchronize()
    assert torch.equal(x, rx) and torch.equal(t, rt)
    # images only: the target buffer keeps what it holds; a predictor without a target buffer refuses targets
    p = Predictor(model, x, l, m, context=ops.StepContext())
    p.load_batch(images[::-1])
    assert torch.equal(x, rx.flip(0)) and torch.equal(t, rt)
    with pytest.raises(ValueError, match="no target buffer"):
        p.load_batch(images, masks)
    q = Predictor(model, x, l, m, target=torch.zeros(3, 50, 90, dtype=torch.int64, device=DEV), out_size=(50, 90), context=ops.StepContext())
    with pytest.raises(ValueError, match="network input size"):
        q.load_batch(images, masks)


def test_clip_layout_with_repeat_and_valid_indices():
    """a clip buffer (B, T, 3, H, W) filled from B still images with repeat=T; with valid_indices the target buffer holds one mask per clip"""
    from lavt_hip import ops
    from lavt_hip.engine import TrainStep
    from test_gpu_deterministic import _video
    model, frames, ids, am, tgt = _video("pwam")
    B, T = frames.shape[:2]
    S = tuple(frames.shape[-2:])
    images, masks, _, _ = _random_batch(41, [(50, 90), (77, 41)], S)
    rx, rt = _per_image(images, masks, S)
    x, t = torch.full_like(frames, float("nan")), _neg(B, *S)
    step = TrainStep(model, x, ids, am, t, context=ops.StepContext(), valid_indices=torch.zeros(B, dtype=torch.int32, device=DEV))
    step.load_batch(images, masks, repeat=T)
    torch.cuda.synchronize()
    for b in range(B):
        for f in range(T):
            assert torch.equal(x[b, f], rx[b])
    assert torch.equal(t, rt)
    # without valid_indices the target buffer holds B*T masks: B masks are repeated like the images
    x2, t2 = torch.full_like(frames, float("nan")), _neg(B * T, *S)
    step2 = TrainStep(_video("pwam")[0], x2, ids, am, t2, context=ops.StepContext())
    step2.load_batch(images, masks, repeat=T)
    assert torch.equal(x2, x) and torch.equal(t2, rt.repeat_interleave(T, 0))
    with pytest.raises(ValueError, match="frames"):
        step2.load_batch(images, masks)
    assert torch.equal(x2, x)


# ================================================================================================ refusals: nothing is written
def test_refusals_write_nothing(golden):
    from lavt_hip import _capi as K
    from lavt_hip import ops
    src, _, msrc, _, out = load_batch(golden, "v")
    x, t = _nan(2, 3, *out), _neg(2, *out)

    # a descriptor offset past the blob, for either kernel
    blob, L = P.pack_batch(src, msrc, out_size=out)
    for section, field, past, call in ((L.items_off, "src_off", L.pixel_bytes - 5, lambda d, h: ops.resize_normalize_u8_batch(d, h, L, x, P.MEAN, P.STD)),
                                       (L.titems_off, "mask_off", L.mask_bytes - 5, lambda d, h: ops.resize_nearest_u8_batch(d, h, L, t))):
        bad = blob.copy()
        bad[section:section + 128].view(P.ITEM_DTYPE)[field][1] = past
        with pytest.raises(RuntimeError, match="rc=-22.*outside"):
            call(torch.from_numpy(bad).to(DEV), bad)
    # a span beyond LDS: one output row of a 400-row source reads 400 x 192 bytes
    pp = P.BatchPreprocessor((1, 1))
    x1 = _nan(2, 3, 1, 1)
    with pytest.raises(RuntimeError, match="rc=-22.*item 1.*LDS"):
        pp.batch([np.zeros((3, 400, 3), np.uint8), np.zeros((400, 400, 3), np.uint8)], out_images=x1)
    assert K.lib.lavt_last_error().startswith(b"lavt_resize_norm_u8_batch")
    torch.cuda.synchronize()
    assert torch.isnan(x1).all()
    pp.batch([np.zeros((3, 400, 3), np.uint8), np.zeros((3, 3, 3), np.uint8)], out_images=x1)          # (the width does not enter the LDS request; the preprocessor works on)
    assert not torch.isnan(x1).any()
    # wrong frame counts, CUDA input
    pp = P.BatchPreprocessor(out)
    pp.stage(src, msrc)
    with pytest.raises(ValueError, match="out_images"):
        pp.commit(_nan(3, 3, *out)[:, :, :, :], t)
    with pytest.raises(ValueError, match="out_targets"):
        pp.batch(src, msrc, out_images=x, out_targets=_neg(3, *out))
    with pytest.raises(ValueError, match="out_targets is missing"):
        pp.stage(src, msrc) and pp.commit(x)
    with pytest.raises(TypeError, match=r"FramePreprocessor\.images"):
        pp.batch(torch.from_numpy(np.stack([src[0], src[0]])).to(DEV), out_images=x)
    with pytest.raises(TypeError, match=r"FramePreprocessor\.images"):
        pp.batch(src, [torch.from_numpy(m).to(DEV) for m in msrc], out_images=x, out_targets=t)
    torch.cuda.synchronize()
    assert torch.isnan(x).all() and bool((t == -1).all())
