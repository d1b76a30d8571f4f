"""GPU checks of pair-list evaluation batches (Predictor(image_of=)) and the device-side evaluation meter (lavt_hip.metrics.DeviceEvalMeter).

The two kernels through the C ABI: lavt_upsample_mask_pairs against lavt_upsample_mask on the same rows (bit for bit on live slots, zero on empty
ones), lavt_eval_meter_append against EvalMeter on the host (integers exact, the fp64 sum within the summation bound).  Then the Predictor on the micro
2-D geometry (embed_dim 32, depths 2-2-2-2, heads 1-2-4-8, window 7, 64 x 64 images, 20 tokens): image_of against expressions_per_image, the gather
against swapped images, empty slots, replays that follow the buffer, the meter at the end of the body, and the default predictor against what the
parent commit launched and stored (tests/golden/eval_pairs_parent.json, written on the parent commit's tree).  Comparisons between two runs of this
code are bit for bit; no tolerance below is taken from what the code gives."""
import ctypes as C
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from lavt_hip.detweights import det_inputs, fill_state_dict_

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16]
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_pairs_parent.json")
IMAGE_SEED = 5          # det_inputs(2, 64, 20, seed): with _model()'s balanced classes its two images give masks that differ on ~46 % of the pixels for one
                        # expression (measured with plain forward passes before this test was written; test 4 asserts > 5 %)


def randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator("cpu").manual_seed(seed))


@pytest.fixture(autouse=True)
def _fp32():
    import lavt_hip
    lavt_hip.set_compute_dtype(torch.float32)
    yield
    lavt_hip.set_compute_dtype(torch.float32)


def _sync():
    torch.cuda.synchronize()


def _i32(values):
    return torch.tensor(list(values), dtype=torch.int32, device=DEV)


# ================================================================================================ 1. the mask kernel through the C ABI
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("geom", [((3, 4), (5, 7), None), ((7, 7), (23, 23), (13, 11))])
def test_mask_kernel_pairs_equals_the_plain_kernel_on_live_slots(geom, dtype):
    """4 slots, image_of = [1, -1, 7, 0] with 2 images: slots 1 and 2 are empty and their logit rows are NaN.  (3, 4) -> (5, 7): 35 pixels per
    sample, so the 4-pixel words and the one wave straddle every sample boundary; (7, 7) -> (23, 23) through (13, 11): 529 pixels per sample, waves
    inside one sample and waves across two, two interpolations."""
    from lavt_hip import _capi as K
    (Hi, Wi), (Ho, Wo), via = geom
    Hm, Wm = via if via is not None else (0, 0)
    n, pairs, n_images = 4, [1, -1, 7, 0], 2
    live = [0 <= v < n_images for v in pairs]
    rows = (randn(31, n, Hi * Wi, 2) * 2)
    for s in range(n):
        if not live[s]:
            rows[s] = float("nan")
    rows = rows.reshape(n * Hi * Wi, 2).to(dtype).to(DEV).contiguous()
    tgt = torch.randint(0, 3, (n, Ho, Wo), generator=torch.Generator("cpu").manual_seed(32)).to(DEV)
    image_of = _i32(pairs)

    def plain():
        mask, iu = torch.full((n, Ho, Wo), 255, dtype=torch.uint8, device=DEV), torch.zeros(n, 2, dtype=torch.int32, device=DEV)
        K.check(K.lib.lavt_upsample_mask(K.dt(dtype), K.ptr(rows), n, Hi, Wi, Hm, Wm, Ho, Wo, K.ptr(mask), K.ptr(tgt), K.ptr(iu), K.stream()))
        return mask, iu

    def paired(with_target=True):
        mask, iu = torch.full((n, Ho, Wo), 255, dtype=torch.uint8, device=DEV), torch.zeros(n, 2, dtype=torch.int32, device=DEV)
        K.check(K.lib.lavt_upsample_mask_pairs(K.dt(dtype), K.ptr(rows), n, Hi, Wi, Hm, Wm, Ho, Wo, K.ptr(mask), K.ptr(tgt) if with_target else None,
                                               K.ptr(iu) if with_target else None, K.ptr(image_of), n_images, K.stream()))
        return mask, iu
    want_mask, want_iu = plain()
    mask, iu = paired()
    mask2, iu2 = paired()
    mask3, _ = paired(with_target=False)
    _sync()
    assert set(mask.unique().tolist()) <= {0, 1}
    for s in range(n):
        if live[s]:
            assert torch.equal(mask[s], want_mask[s]) and torch.equal(iu[s], want_iu[s]), s
            assert int(iu[s, 1]) > 0
        else:
            assert not mask[s].any() and iu[s].tolist() == [0, 0], (s, iu[s].tolist())
    assert torch.equal(iu2, iu) and torch.equal(mask2, mask), "a second launch on a zeroed iu gives the same counts"
    assert torch.equal(mask3, mask), "without a target the mask bytes are the same"
    # every slot live: the plain kernel's bytes for the whole batch (on finite rows)
    finite = torch.nan_to_num(rows.float(), nan=0.25).to(dtype).contiguous()
    rows = finite
    want_mask, want_iu = plain()
    image_of = _i32([0, 1, 1, 0])
    mask, iu = paired()
    _sync()
    assert torch.equal(mask, want_mask) and torch.equal(iu, want_iu)


# ================================================================================================ 2. the meter kernel through the C ABI
BIG = 2 ** 31 - 1
IU12 = [(0, 0), (0, 9), (5, 5), (1, 2), (3, 5), (7, 10), (4, 5), (9, 10), (16777217, 33554433), (BIG - 1, BIG), (2 ** 30, BIG), (BIG, BIG)]


def _fresh_block(capacity):
    from lavt_hip import metrics as M
    words = torch.zeros(M.eval_meter_bytes(capacity) // 8, dtype=torch.float64)
    words[M.E_CAPACITY] = float(capacity)
    return words.to(DEV)


@pytest.mark.parametrize("capacity", [32, 5])
def test_meter_kernel_equals_eval_meter(capacity):
    """one append of 12 rows with 3 empty slots, then one of the same 12 rows with image_of = NULL: 21 samples.  count, the five precision counters and
    the cumulative I / U (past 2^32) equal EvalMeter's exactly; the sum of IoU is within n * 2^-53 * sum(iou) of numpy's (the device adds the n
    terms one after the other in fp64, numpy pairwise: each has at most n - 1 roundings of relative size 2^-53 on partial sums <= the total; the
    bound is computed from n here); the ring holds the live rows in slot order.  capacity 5: the ring wraps.  With hold set nothing changes."""
    from lavt_hip import _capi as K
    from lavt_hip import metrics as M
    pairs, n_images = [0, -1, 2, 1, 0, 2, 3, 1, 0, 2, -1, 1], 3          # slots 1, 6 (3 >= n_images) and 10 are empty
    live = [0 <= v < n_images for v in pairs]
    assert live.count(False) == 3
    iu = torch.tensor(IU12, dtype=torch.int32, device=DEV)
    image_of = _i32(pairs)
    block = _fresh_block(capacity)
    assert int(K.lib.lavt_eval_meter_bytes(capacity)) == block.numel() * 8
    K.check(K.lib.lavt_eval_meter_append(K.ptr(iu), K.ptr(image_of), n_images, 12, K.ptr(block), capacity, K.stream()))
    first = M.EvalSnapshot(block.cpu().view(torch.uint8).numpy(), capacity)
    K.check(K.lib.lavt_eval_meter_append(K.ptr(iu), None, 0, 12, K.ptr(block), capacity, K.stream()))
    _sync()
    snap = M.EvalSnapshot(block.cpu().view(torch.uint8).numpy(), capacity)
    kept = [r for r, f in zip(IU12, live) if f]
    host = M.EvalMeter()
    host.update(kept)
    assert (first.count, first.n, first.cum_I, first.cum_U, first.correct) == (9, 9, host.cum_I, host.cum_U, [int(c) for c in host.correct])
    host.update(IU12)
    seen = kept + IU12
    n = len(seen)
    assert (snap.count, snap.n, snap.cum_I, snap.cum_U, snap.correct) == (n, n, host.cum_I, host.cum_U, [int(c) for c in host.correct])
    assert snap.cum_U > 2 ** 32 and n == 21
    total = float(np.sum(np.array(host.ious)))
    bound = n * 2.0 ** -53 * total
    err = abs(float(snap.header[M.E_IOU_SUM]) - total)
    print(f"\n[eval meter, capacity {capacity}] sum of iou {float(snap.header[M.E_IOU_SUM])!r} vs numpy {total!r}: |diff| {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    got, want = snap.summary(), host.summary()
    assert abs(got["mean_iou"] - want["mean_iou"]) <= bound * 100.0 / n
    for k in want:
        if k != "mean_iou":
            assert got[k] == want[k], k
    tail = seen[-min(capacity, n):]
    recs = snap.records()
    assert [(int(r["I"]), int(r["U"])) for r in recs] == tail, "the ring holds the live rows in slot order, empty slots absent"
    assert [int(r["sample"]) for r in recs] == list(range(n - len(tail), n))
    # hold: the block's bytes do not change
    block[M.E_HOLD] = 1.0
    before = block.clone()
    K.check(K.lib.lavt_eval_meter_append(K.ptr(iu), K.ptr(image_of), n_images, 12, K.ptr(block), capacity, K.stream()))
    K.check(K.lib.lavt_eval_meter_append(K.ptr(iu), None, 0, 12, K.ptr(block), capacity, K.stream()))
    _sync()
    assert torch.equal(block.view(torch.uint8), before.view(torch.uint8))


# ================================================================================================ the Predictor on the micro geometry
ARGS = SimpleNamespace(swin_type="tiny")


def _model(balance=True):
    """balance: the deterministic weights alone leave ~1.5 % of the pixels foreground (the median of logit 1 - logit 0 is -1.2 on these inputs), too few
    for two masks to differ by much; 1.2 on the class-1 bias of the last layer puts the median margin at 0, so about half of every mask is
    foreground and masks of different images or expressions differ on 40 % of the pixels"""
    from lib._utils import LAVT
    from lib.backbone import MultiModalSwinTransformer
    from lib.mask_predictor import SimpleDecoding
    bb = MultiModalSwinTransformer(embed_dim=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8], window_size=7, drop_path_rate=0.0, args=ARGS)
    model = LAVT(bb, SimpleDecoding(256, ARGS))
    fill_state_dict_(model)
    if balance:
        with torch.no_grad():
            model.classifier.conv1_1.bias[1] += 1.2
    return model.to(DEV).eval()


def _images():
    return det_inputs(2, 64, 20, seed=IMAGE_SEED)[0].to(DEV)


def _expressions(n, seed=77):
    """n expressions with ragged valid lengths, and n target masks"""
    _, l, m, tgt = det_inputs(n, 64, 20, seed=seed)
    return l.to(DEV), m.to(DEV), tgt.to(DEV)


def _predictor(model, x, l, m, tgt, **kw):
    from lavt_hip import ops
    from lavt_hip.engine import Predictor
    p = Predictor(model, x, l, m, target=tgt, context=ops.StepContext(), **kw)
    p.warmup_and_capture()
    assert p.captured == kw.get("use_graph", True)
    return p


def _run(p):
    mask = p.step().clone()
    _sync()
    return mask, p.iu.clone()


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_image_of_equals_expressions_per_image(dtype, use_graph):
    """2 images, image_of = [0, 0, 0, 1, 1, 1] against expressions_per_image=3 on the same buffers: the gather copies the rows the expand copies, so
    mask and iu are equal bit for bit, eagerly and replayed; stage 0's blocks saw batch 2, stage 1's batch 6"""
    import lavt_hip
    with lavt_hip.use_dtype(dtype):
        model, x = _model(), _images()
        l, m, tgt = _expressions(6)
        want_mask, want_iu = _run(_predictor(model, x, l, m, tgt, expressions_per_image=3, use_graph=use_graph))
        seen = {0: [], 1: []}
        hooks = [model.backbone.layers[i].blocks[0].register_forward_hook(lambda mod, inp, out, i=i: seen[i].append(int(inp[0].shape[0]))) for i in (0, 1)]
        p = _predictor(model, x, l, m, tgt, image_of=_i32([0, 0, 0, 1, 1, 1]), use_graph=use_graph)
        for h in hooks:
            h.remove()
        assert seen[0] and set(seen[0]) == {2}, f"stage 0's blocks run once per image, saw batches {seen[0]}"
        assert seen[1] and set(seen[1]) == {6}, f"stage 1 runs per pair, saw batches {seen[1]}"
        mask, iu = _run(p)
        assert tuple(mask.shape) == (6, 64, 64) and tuple(iu.shape) == (6, 2) and mask.dtype == torch.uint8
        assert torch.equal(mask, want_mask) and torch.equal(iu, want_iu)
        assert len({tuple(r) for r in iu.tolist()}) > 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_gather_names_the_right_image(dtype):
    """pairs [1, 0, 1, 0, 0] on images (a, b) against [0, 1, 0, 1, 1] on images (b, a): equal slot by slot, bit for bit.  Slots 0 and 1 hold the same
    expression, so they differ by the image alone -- on more than 5 % of the pixels, else an index that named the wrong image would pass"""
    import lavt_hip
    with lavt_hip.use_dtype(dtype):
        model, x = _model(), _images()
        l, m, tgt = _expressions(5)
        l[1], m[1] = l[0], m[0]
        one = _run(_predictor(model, x, l, m, tgt, image_of=_i32([1, 0, 1, 0, 0])))
        share = float((one[0][0] != one[0][1]).float().mean())
        print(f"\n[{dtype}] the two images' masks for one expression differ on {share:.4f} of the pixels")
        assert share > 0.05
        other = _run(_predictor(model, x.flip(0).contiguous(), l, m, tgt, image_of=_i32([0, 1, 0, 1, 1])))
        for s in range(5):
            assert torch.equal(one[0][s], other[0][s]) and torch.equal(one[1][s], other[1][s]), s


@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_slots_do_not_leak(dtype):
    """[1, -1, 0, 0] against [1, 0, 0, 0]: slots 0, 2, 3 bit-equal (no live slot's mask or iu changed), slot 1 zero with iu (0, 0).  The empty slot's
    language features are NaN on top of its zero image rows: whatever the network makes of them is not read"""
    import lavt_hip
    with lavt_hip.use_dtype(dtype):
        model, x = _model(), _images()
        l, m, tgt = _expressions(4)
        full = _run(_predictor(model, x, l, m, tgt, image_of=_i32([1, 0, 0, 0])))
        l_nan = l.clone()
        l_nan[1] = float("nan")
        part = _run(_predictor(model, x, l_nan, m, tgt, image_of=_i32([1, -1, 0, 0])))
        for s in (0, 2, 3):
            assert torch.equal(part[0][s], full[0][s]) and torch.equal(part[1][s], full[1][s]), s
        assert set(part[0].unique().tolist()) <= {0, 1}
        assert not part[0][1].any() and part[1][1].tolist() == [0, 0]
        assert full[0][1].any() or int(full[1][1, 1]) > 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_replays_follow_the_buffer_and_refusals(dtype):
    """capture with one pair list, set_image_of another, step(): the bits of a fresh predictor captured on the second list"""
    import lavt_hip
    from lavt_hip.engine import Predictor
    with lavt_hip.use_dtype(dtype):
        model, x = _model(), _images()
        l, m, tgt = _expressions(5)
        first, second = [0, 1, 1, 0, 1], [1, 1, -1, 0, 0]
        p = _predictor(model, x, l, m, tgt, image_of=_i32(first))
        a = _run(p)
        p.set_image_of(second)
        b = _run(p)
        assert p.image_of.tolist() == second
        fresh = _run(_predictor(model, x, l, m, tgt, image_of=_i32(second)))
        assert torch.equal(b[0], fresh[0]) and torch.equal(b[1], fresh[1])
        assert not torch.equal(a[0], b[0])
        p.set_image_of(first)
        again = _run(p)
        assert torch.equal(again[0], a[0]) and torch.equal(again[1], a[1])
        for bad in ([0, 1, 1, 0], [0, 1, 1, 0, 1, 0], [0, 1, 2, 0, 1], [0, -2, 1, 0, 1]):
            with pytest.raises(ValueError):
                p.set_image_of(bad)
        assert p.image_of.tolist() == first, "a refused list is not written"
        with pytest.raises(ValueError):
            _predictor(model, x, l, m, tgt).set_image_of([0, 1])          # built without the buffer
        with pytest.raises(ValueError, match="expressions_per_image"):
            Predictor(model, x, l[:4].contiguous(), m[:4].contiguous(), expressions_per_image=2, image_of=_i32([0, 0, 1, 1]))
        with pytest.raises(ValueError, match="valid_indices"):
            Predictor(model, x, l[:2].contiguous(), m[:2].contiguous(), valid_indices=_i32([1]), image_of=_i32([0, 1]))
        with pytest.raises(ValueError):
            Predictor(model, x, l, m, image_of=_i32([0, 1, 1]))                                  # one entry per expression
        with pytest.raises(ValueError):
            Predictor(model, x, l, m, image_of=torch.zeros(5, dtype=torch.int64, device=DEV))
        with pytest.raises(RuntimeError, match="GPU memory only"):
            Predictor(model, x, l, m, image_of=torch.zeros(5, dtype=torch.int32))


def test_image_of_refuses_the_video_model():
    """built as test_gpu_infer.py builds it: the video backbone shares no stage 0"""
    from lavt_hip.engine import Predictor
    from lib._utils import LAVTVideo
    from lib.mask_predictor import SimpleDecoding
    from lib.video_swin_transformer import MultiModalSwinTransformer3D
    a = SimpleNamespace()
    bb = MultiModalSwinTransformer3D(patch_size=(1, 4, 4), embed_dim=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8], window_size=(8, 7, 7),
                                     drop_path_rate=0.0, patch_norm=True, out_indices=(0, 1, 2, 3), use_checkpoint=False,
                                     num_heads_fusion=[1, 1, 1, 1], fusion_drop=0.0, args=a)
    parts = torch.nn.ModuleDict({"backbone": bb, "classifier": SimpleDecoding(256, a)})
    fill_state_dict_(parts)
    parts.to(DEV)
    frames, l, m, _ = det_inputs(2, 64, 22, seed=3, frames=4)
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
    with pytest.raises(NotImplementedError, match="image_of"):
        Predictor(model, frames, ids, am, image_of=_i32([0, 1]))
    with pytest.raises(NotImplementedError, match="image_of"):
        model.forward_lowres(frames, ids, am, folded=True, image_of=_i32([0, 1]))


def _same_counts(snap, host):
    assert (snap.count, snap.cum_I, snap.cum_U, snap.correct) == (host.count, host.cum_I, host.cum_U, [int(c) for c in host.correct])
    got, want = snap.summary(), host.summary()
    n = host.count
    bound = n * 2.0 ** -53 * float(np.sum(np.array(host.ious)))          # the summation bound of test_meter_kernel_equals_eval_meter
    assert abs(got["mean_iou"] - want["mean_iou"]) <= bound * 100.0 / n
    for k in want:
        if k != "mean_iou":
            assert got[k] == want[k], k
    assert str(snap).splitlines()[0] == "Final results:"


@pytest.mark.parametrize("dtype", DTYPES)
def test_meter_on_the_pair_list_predictor(dtype):
    """warmup_and_capture leaves the count at 0; three replays over different pair lists (one with empty slots): read() equals EvalMeter fed
    pred.iu[live] after each; poll() never hands out a snapshot newer than the replays issued; reset() zeroes the accumulators"""
    import lavt_hip
    from lavt_hip.metrics import DeviceEvalMeter, EvalMeter
    with lavt_hip.use_dtype(dtype):
        model, x = _model(), _images()
        l, m, tgt = _expressions(4)
        from lavt_hip import ops
        from lavt_hip.engine import Predictor
        p = Predictor(model, x, l, m, target=tgt, image_of=_i32([0, 1, 1, 0]), context=ops.StepContext())
        meter = p.make_meter(capacity=8)
        assert isinstance(meter, DeviceEvalMeter) and p.meter is meter
        with pytest.raises(RuntimeError, match="already"):
            p.attach_meter(DeviceEvalMeter(capacity=4))
        p.warmup_and_capture()
        assert p.captured
        with pytest.raises(RuntimeError, match="before warmup_and_capture"):
            p.make_meter()
        snap = meter.read()
        assert (snap.count, snap.n) == (0, 0) and not snap.ring.view(np.uint8).any() and float(snap.header[1]) == 0.0
        host, issued = EvalMeter(), 0
        for pairs in ([0, 1, 1, 0], [1, -1, 0, -1], [0, 0, 0, 1]):
            p.set_image_of(pairs)
            p.step()
            issued += sum(v >= 0 for v in pairs)
            polled = meter.poll()
            assert polled is None or polled.n <= issued          # never a snapshot newer than the replays issued
            _sync()
            live = torch.tensor([v >= 0 for v in pairs], device=DEV)
            host.update(p.iu[live])
            snap = meter.read()
            _same_counts(snap, host)
            assert snap.n == issued
        assert host.count == 10 and host.cum_U > 0
        recs = meter.read().records()
        assert len(recs) == 8 and [int(r["sample"]) for r in recs] == list(range(2, 10))          # capacity 8 < 10 samples
        assert [(int(r["I"]), int(r["U"])) for r in recs[-4:]] == [tuple(r) for r in p.iu.tolist()]
        meter.poll()
        _sync()
        polled = meter.poll()          # the copy enqueued above has arrived: handed out without waiting
        assert polled is not None and polled.n == 10
        sd = meter.state_dict()
        meter.reset()
        snap = meter.read()
        assert (snap.count, snap.cum_I, snap.cum_U, snap.correct, float(snap.header[4])) == (0, 0, 0, [0] * 5, 0.0) and snap.n == 10
        with pytest.raises(RuntimeError, match="no samples"):
            snap.summary()
        meter.load_state_dict(sd)
        _same_counts(meter.read(), host)
        p.step()
        _sync()
        host.update(p.iu)
        _same_counts(meter.read(), host)


@pytest.mark.parametrize("kind", ["plain", "valid_indices", "expressions"])
def test_meter_on_the_other_predictors(kind):
    """the append passes NULL for image_of: every row of iu counts.  One step each, bf16"""
    import lavt_hip
    from lavt_hip import ops
    from lavt_hip.engine import Predictor
    from lavt_hip.metrics import DeviceEvalMeter, EvalMeter
    with lavt_hip.use_dtype(torch.bfloat16):
        model, x = _model(), _images()
        l, m, tgt = _expressions(4)
        if kind == "plain":
            p = Predictor(model, x, l[:2].contiguous(), m[:2].contiguous(), target=tgt[:2].contiguous(), meter=DeviceEvalMeter(capacity=4), context=ops.StepContext())
        elif kind == "valid_indices":
            p = Predictor(model, x, l[:2].contiguous(), m[:2].contiguous(), target=tgt[[1]].contiguous(), valid_indices=_i32([1]), context=ops.StepContext())
            p.attach_meter(DeviceEvalMeter(capacity=4))
        else:
            p = Predictor(model, x, l, m, target=tgt, expressions_per_image=2, context=ops.StepContext())
            p.make_meter(capacity=4)
        p.warmup_and_capture()
        assert p.captured and p.meter.read().count == 0
        p.step()
        _sync()
        host = EvalMeter()
        host.update(p.iu)
        _same_counts(p.meter.read(), host)
        assert host.count == {"plain": 2, "valid_indices": 1, "expressions": 4}[kind]
        with pytest.raises(ValueError, match="target"):
            Predictor(model, x, l[:2].contiguous(), m[:2].contiguous(), meter=DeviceEvalMeter(capacity=4))


# ================================================================================================ 8. the default predictor is the parent's
def _rows(recs):
    from lavt_hip import _capi as K
    out = []
    for name, scope, note, _ in recs:
        args = K._PROTOTYPES.get(name)
        if args and args[-1] is C.c_void_p:
            out.append([name, scope, note["shape"] if note else None])
    return out


@pytest.mark.parametrize("name,dtype", [("fp32", torch.float32), ("bf16", torch.bfloat16)])
def test_the_default_predictor_is_unchanged(name, dtype):
    """A Predictor built without image_of and meter: the launch rows of one eager step (recorded as tests/test_gpu_launch_records.py records them)
    and the mask bytes and counts are those the fixture holds, written on the parent commit's tree with the same model and inputs"""
    import lavt_hip
    from lavt_hip import _capi as K
    from lavt_hip import ops
    from lavt_hip.engine import Predictor
    want = json.load(open(FIXTURE))[name]
    with lavt_hip.use_dtype(dtype):
        model = _model(balance=False)
        x, l, m, tgt = (t.to(DEV) for t in det_inputs(2, 64, 20, seed=5))
        p = Predictor(model, x, l, m, target=tgt, use_graph=False, context=ops.StepContext())
        assert p.image_of is None and p.meter is None
        p.warmup_and_capture(eager_iters=2)
        K.prof.start()
        try:
            p.step()
        finally:
            recs = K.prof.stop()
        got = _rows(recs)
        _sync()
        assert len(want["rows"]) > 0
        assert [r[:2] for r in got] == [r[:2] for r in want["rows"]], next(((i, a, b) for i, (a, b) in enumerate(zip(got, want["rows"])) if a[:2] != b[:2]),
                                                                          (len(got), len(want["rows"])))
        bad = [(i, a, b) for i, (a, b) in enumerate(zip(got, want["rows"])) if b[2] is not None and a[2] != b[2]]
        assert not bad, bad[:4]
        assert "lavt_upsample_mask_pairs" not in [r[0] for r in got] and "lavt_eval_meter_append" not in [r[0] for r in got]
        assert np.packbits(p.mask.cpu().numpy().reshape(-1)).tobytes().hex() == want["mask"]
        assert p.iu.cpu().tolist() == want["iu"]
