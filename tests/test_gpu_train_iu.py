"""The hard-mask I / U pass of the training meters (DESIGN.md "Training meters"; include/lavt_hip.h: lavt_upsample_iu / _sel) and TrainStep.meter_stats.

Reference: tests/train_iu_ref.py, the literal fp64 restatement of train.py:64-76 on the CPU.  Every count is compared EXACTLY: the exact cases are exact
in fp32 in any evaluation order (multiples of 1/8 through dyadic weights), the margin cases keep |up1 - up0| >= 1e-4 in fp64 (asserted first) against
an fp32 interpolation error of about 1e-6, so a mismatch is a coordinate or tie bug, never rounding.  All counts are below 2^24 (exact in the fp32 row).

The harness tests (7, 8) fail on a tree without TrainStep.meter_stats: there the meters of a Dice criterion log slots 2, 3 of the criterion's `stats`."""
import collections

import numpy as np
import pytest
import torch

import train_iu_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN_BITS = 0x7FC12345          # a quiet NaN with a payload: a copy through float arithmetic could lose it


@pytest.fixture(autouse=True)
def _fp32():
    import lavt_hip
    lavt_hip.set_compute_dtype(torch.float32)
    yield
    lavt_hip.set_compute_dtype(torch.float32)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _nan_row():
    return torch.full((4,), float("nan"), dtype=torch.float32, device=DEV)


def _iu(x, target, dims, sel=None, loss_src=None, row=None, ws_words=None, nsel=None, null_row=False):
    """lavt_upsample_iu / _sel through the C ABI on device tensors -> (rc, row).  x: NHWC rows (fp32 | bf16), sel: device int32 or None"""
    from lavt_hip import _capi as K
    B, Hi, Wi, Ho, Wo = dims
    ns = B if sel is None else (sel.numel() if nsel is None else nsel)
    need = K.lib.lavt_upsample_iu_ws(ns, Ho, Wo)
    words = need if ws_words is None else ws_words
    ws = torch.empty(max(int(words), 1), dtype=torch.int32, device=DEV)
    row = _nan_row() if row is None else row
    rp = None if null_row else K.ptr(row)
    if sel is None:
        rc = K.lib.lavt_upsample_iu(K.dt(x.dtype), K.ptr(x), K.ptr(target), K.ptr(loss_src), K.ptr(ws), int(words), rp, B, Hi, Wi, Ho, Wo, K.stream())
    else:
        rc = K.lib.lavt_upsample_iu_sel(K.dt(x.dtype), K.ptr(x), K.ptr(sel), ns, K.ptr(target), K.ptr(loss_src), K.ptr(ws), int(words), rp, B, Hi, Wi, Ho, Wo,
                                        K.stream())
    torch.cuda.synchronize()
    return rc, row


def _ce(x, target, dims, sel=None):
    """out4 of lavt_upsample_ce_fwd / _sel_fwd on the same buffers"""
    from lavt_hip import _capi as K
    B, Hi, Wi, Ho, Wo = dims
    ws = torch.empty(4 * 2048, dtype=torch.float32, device=DEV)
    out4 = _nan_row()
    if sel is None:
        K.check(K.lib.lavt_upsample_ce_fwd(K.dt(x.dtype), K.ptr(x), K.ptr(target), 0.9, 1.1, K.ptr(ws), ws.numel(), K.ptr(out4), B, Hi, Wi, Ho, Wo, K.stream()))
    else:
        K.check(K.lib.lavt_upsample_ce_sel_fwd(K.dt(x.dtype), K.ptr(x), K.ptr(sel), sel.numel(), K.ptr(target), 0.9, 1.1, K.ptr(ws), ws.numel(), K.ptr(out4), B, Hi, Wi,
                                               Ho, Wo, K.stream()))
    torch.cuda.synchronize()
    return out4


def _dims(logits, target):
    return (logits.shape[0], logits.shape[2], logits.shape[3], target.shape[-2], target.shape[-1])


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------------------------------------ 1. exact cases
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", sorted(R.EXACT_GEOMETRIES))
def test_exact_cases(name, dtype):
    logits, target = R.exact_case(name)
    want = R.train_iu(logits, target)
    assert want == R.train_iu(logits, target, dtype=torch.float32)
    rc, row = _iu(R.nhwc_rows(logits, dtype).to(DEV), target.to(DEV), _dims(logits, target))
    got = row.tolist()
    print(f"[{name} {dtype}] I, U = {got[2]}, {got[3]}; restatement {want}; ties {R.ties(logits, *target.shape[-2:])}")
    assert rc == 0 and got == [0.0, 0.0, float(want[0]), float(want[1])]


# ------------------------------------------------------------------------------------------------ 2. non-dyadic geometry
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", sorted(R.MARGIN_GEOMETRIES))
def test_margin_cases(name, dtype):
    logits, target = R.margin_case(name)
    m = R.margin(logits, *target.shape[-2:])
    print(f"[{name}] smallest fp64 |up1 - up0| = {m:.3e}")
    assert m >= R.MIN_MARGIN, "precondition on the inputs"
    want = R.train_iu(logits, target)
    rc, row = _iu(R.nhwc_rows(logits, dtype).to(DEV), target.to(DEV), _dims(logits, target))
    got = row.tolist()
    print(f"[{name} {dtype}] I, U = {got[2]}, {got[3]}; restatement {want}")
    assert rc == 0 and got == [0.0, 0.0, float(want[0]), float(want[1])]


# ------------------------------------------------------------------------------------------------ 3. equality with the cross-entropy pair
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", sorted(R.EXACT_GEOMETRIES) + sorted(R.MARGIN_GEOMETRIES))
def test_counts_equal_the_cross_entropy_kernels(name, dtype):
    logits, target = R.exact_case(name) if name in R.EXACT_GEOMETRIES else R.margin_case(name)
    dims = _dims(logits, target)
    x, t = R.nhwc_rows(logits, dtype).to(DEV), target.to(DEV)
    rc, row = _iu(x, t, dims)
    out4 = _ce(x, t, dims)
    assert rc == 0 and float(out4[3]) < 2 ** 24 and torch.equal(row[2:4], out4[2:4]), (row.tolist(), out4.tolist())
    # _sel_: the last frame scored against target 0, frame 0 against target 1
    B = dims[0]
    sel = _i32([B - 1, 0])
    t2 = t[:2].contiguous()
    rc, row = _iu(x, t2, dims, sel=sel)
    out4 = _ce(x, t2, dims, sel=sel)
    want = R.train_iu(logits, target[:2], sel=[B - 1, 0])
    assert rc == 0 and torch.equal(row[2:4], out4[2:4]) and row[2:4].tolist() == [float(want[0]), float(want[1])], (row.tolist(), out4.tolist(), want)


# ------------------------------------------------------------------------------------------------ 4. frame selection
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_frame_selection_follows_the_device_buffer(dtype):
    g = torch.Generator().manual_seed(77)
    B, Hi, Wi, Ho, Wo = 4, 5, 9, 17, 33
    logits = torch.randint(-16, 17, (B, 2, Hi, Wi), generator=g).float() / 8
    target = torch.randint(0, 2, (2, Ho, Wo), generator=g, dtype=torch.int64)
    x, t = R.nhwc_rows(logits, dtype).to(DEV), target.to(DEV)
    sel = _i32([3, 1])
    seen = []
    for entries in ([3, 1], [0, 2], [2, 9], [-1, 4]):
        sel.copy_(torch.tensor(entries, dtype=torch.int32))          # the SAME device buffer
        rc, row = _iu(x, t, (B, Hi, Wi, Ho, Wo), sel=sel)
        want = R.train_iu(logits, target, sel=entries)
        seen.append(want)
        assert rc == 0 and row.tolist() == [0.0, 0.0, float(want[0]), float(want[1])], (entries, row.tolist(), want)
    assert seen[2] == R.train_iu(logits[2:3], target[:1]) and seen[3] == (0, 0)
    assert len(set(seen)) == 4, "the selections must give different counts for the test to see the buffer being followed"


# ------------------------------------------------------------------------------------------------ 5. loss_src
def test_loss_src_is_copied_bit_for_bit():
    logits, target = R.exact_case("q_2x4x3_13x9")
    dims = _dims(logits, target)
    x, t = R.nhwc_rows(logits).to(DEV), target.to(DEV)
    want = R.train_iu(logits, target)
    for bits_ in (np.float32(0.734619140625).view(np.int32).item(), NAN_BITS, np.float32(-0.0).view(np.int32).item()):
        src = torch.tensor([bits_, 0x40400000, 0x40800000], dtype=torch.int32, device=DEV).view(torch.float32)          # {value, 3.0, 4.0}: only [0] is read
        rc, row = _iu(x, t, dims, loss_src=src)
        assert rc == 0 and int(_bits(row)[0]) == bits_ and _bits(row)[1:].tolist() == _bits(torch.tensor([0.0, want[0], want[1]], dtype=torch.float32)).tolist()
        rc, row = _iu(x, t[:1].contiguous(), dims, sel=_i32([1]), loss_src=src)
        assert rc == 0 and int(_bits(row)[0]) == bits_ and float(row[1]) == 0.0
    rc, row = _iu(x, t, dims, loss_src=None)
    assert rc == 0 and _bits(row)[:2].tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------ 6. reproducibility and refusal
def test_two_runs_are_bit_identical_and_bad_arguments_are_refused():
    from lavt_hip import _capi as K
    logits, target = R.margin_case("m_2x30x30_120x120")          # 113 workgroups
    dims = _dims(logits, target)
    x, t = R.nhwc_rows(logits, torch.bfloat16).to(DEV), target.to(DEV)
    rows = [_iu(x, t, dims)[1] for _ in range(2)]
    assert torch.equal(_bits(rows[0]), _bits(rows[1])) and float(rows[0][3]) > 0
    need = K.lib.lavt_upsample_iu_ws(dims[0], dims[3], dims[4])
    assert need == 2 * 113
    nan = _bits(_nan_row())
    sel3 = _i32([0, 1, 0])
    for what, kw in (("scratch one word too small", dict(ws_words=need - 1)),
                     ("nsel = B + 1", dict(sel=sel3, nsel=dims[0] + 1)),
                     ("nsel = 0", dict(sel=sel3, nsel=0)),
                     ("a null row", dict(null_row=True))):
        rc, row = _iu(x, t, dims, **kw)
        assert rc != 0 and torch.equal(_bits(row), nan), what
        assert K.lib.lavt_last_error().decode().startswith("lavt_upsample_iu"), what
    row = _nan_row()          # (K.dt refuses other dtypes on the host: the C check is reached with a raw dtype code)
    ws = torch.empty(need, dtype=torch.int32, device=DEV)
    rc = K.lib.lavt_upsample_iu(2, K.ptr(x), K.ptr(t), None, K.ptr(ws), need, K.ptr(row), *dims, K.stream())          # dtype 2 = fp8
    torch.cuda.synchronize()
    assert rc != 0 and torch.equal(_bits(row), nan)
    for bad in ((0,) + dims[1:], dims[:1] + (0,) + dims[2:], dims[:4] + (-1,)):
        rc = K.lib.lavt_upsample_iu(K.dt(x.dtype), K.ptr(x), K.ptr(t), None, K.ptr(ws), need, K.ptr(row), *bad, K.stream())
        torch.cuda.synchronize()
        assert rc != 0 and torch.equal(_bits(row), nan), bad
    rc = K.lib.lavt_upsample_iu(K.dt(x.dtype), None, K.ptr(t), None, K.ptr(ws), need, K.ptr(row), *dims, K.stream())
    assert rc != 0 and torch.equal(_bits(row), nan)


def test_the_python_op():
    """ops.upsample_iu / lib._utils.fused_iu: the row of the C ABI from the (B, 2, h, w)-shaped output, no autograd node, loss[0] in row[0]"""
    from lavt_hip import ops
    from lib._utils import fused_iu, fused_loss
    logits, target = R.margin_case("m_2x7x5_23x18")
    want = R.train_iu(logits, target)
    y = logits.to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2).requires_grad_(True)          # NCHW-shaped view of NHWC memory, as forward_lowres gives
    t = target.to(DEV)
    stats = torch.tensor([1.5, 7.0, 8.0, 9.0, 10.0], device=DEV)
    row = fused_iu(y, t, loss=stats)
    assert not row.requires_grad and row.dtype == torch.float32 and row.tolist() == [1.5, 0.0, float(want[0]), float(want[1])]
    assert fused_iu(y, t).tolist() == [0.0, 0.0, float(want[0]), float(want[1])]
    _, ce = fused_loss(y, t)
    assert torch.equal(row[2:4], ce[2:4])
    w1 = R.train_iu(logits, target[:1], sel=[1])
    assert fused_iu(y, t[:1].contiguous(), valid_indices=_i32([1])).tolist() == [0.0, 0.0, float(w1[0]), float(w1[1])]
    with pytest.raises(RuntimeError, match="GPU memory only"):
        ops.upsample_iu(R.nhwc_rows(logits).to(DEV), t, *_dims(logits, target), loss=torch.zeros(4))
    with pytest.raises(ValueError):
        ops.upsample_iu(R.nhwc_rows(logits).to(DEV), t, *_dims(logits, target), loss=torch.zeros(4, dtype=torch.float64, device=DEV))


# ------------------------------------------------------------------------------------------------ 7. the harness
@pytest.fixture(scope="module")
def batches():
    """the micro-batches of tests/test_gpu_meters.py: made once, never written"""
    from lavt_hip.detweights import det_inputs
    return [tuple(v.to(DEV) for v in det_inputs(2, 64, 20, seed=17 + i)) for i in range(3)]


def _step(batches, loss, meters, **kw):
    """the harness of tests/test_gpu_meters.py without an optimizer: the weights stay put, every replay sees the same forward.
    -> (step, static input buffers, meters or None), before warmup_and_capture()"""
    from lavt_hip import ops
    from lavt_hip.engine import TrainStep
    from test_gpu_meters import _micro
    static = tuple(v.clone() for v in batches[0])
    step = TrainStep(_micro(), *static, world=1, context=ops.StepContext(), deterministic=True, loss=loss, **kw)
    return step, static, (step.make_meters(capacity=8, window_size=4) if meters else None)


@pytest.fixture(scope="module")
def ce_counts(batches):
    """stats[2:4] of a captured TrainStep(loss="ce") from the same seed on each of the three batches -- the forward does not depend on the criterion"""
    import lavt_hip
    with lavt_hip.use_dtype(torch.bfloat16):
        step, static, _ = _step(batches, "ce", False)
        step.warmup_and_capture()
        assert step.captured
        out = []
        for b in batches:
            for dst, src in zip(static, b):
                dst.copy_(src)
            step.step()
            torch.cuda.synchronize()
            out.append(tuple(step.stats[2:4].tolist()))
    lavt_hip.set_compute_dtype(torch.float32)
    assert all(0 < i < u for i, u in out) and len(set(out)) == 3, out
    return out


@pytest.mark.parametrize("loss", ["mc_dice", "dice_boundary"])
def test_metered_dice_step_logs_the_hard_mask_counts(batches, ce_counts, loss):
    import lavt_hip
    n = batches[0][3].shape[0]
    with lavt_hip.use_dtype(torch.bfloat16):
        step, static, meters = _step(batches, loss, True)
        step.warmup_and_capture()
        assert step.captured and meters.read().n == 0
        losses = []
        for b in batches:
            for dst, src in zip(static, b):
                dst.copy_(src)
            step.step()
            torch.cuda.synchronize()
            losses.append(int(_bits(step.stats)[0]))
            assert step.stats.numel() == (2 + 6 * n if loss == "mc_dice" else 3 + 14 * n)
        snap = meters.read()
        recs = snap.records()
        assert snap.n == 3 and len(recs) == 3
        for rec, (I, U), lbits in zip(recs, ce_counts, losses):
            print(f"[{loss}] record it={int(rec['it'])}: I, U = {float(rec['I'])}, {float(rec['U'])} (ce twin {I}, {U}); loss {float(rec['loss']):.6f}; iou {float(rec['iou']):.6f}")
            assert (float(rec["I"]), float(rec["U"])) == (I, U)
            assert int(np.float32(rec["loss"]).view(np.int32)) == lbits
            assert float(rec["iou"]) == float(np.float64(I) / np.float64(U))
        s = meters.epoch_summary()
        sI, sU = sum(np.float64(i) for i, _ in ce_counts), sum(np.float64(u) for _, u in ce_counts)
        assert s["iterations"] == 3 and s["overall_iou"] == float(sI * 100. / sU)
        # the row the last replay logged
        assert step.meter_stats is not step.stats and step.meter_stats.shape == (4,)
        assert int(_bits(step.meter_stats)[0]) == losses[-1] and step.meter_stats[1:].tolist() == [0.0, *ce_counts[-1]]


def test_metered_dice_boundary_video_step_follows_the_index_buffer():
    """the micro Video-Swin of tests/test_gpu_dice_boundary.py, valid_indices = [2, 5], then the buffer refilled to [0, 7] between two replays"""
    import lavt_hip
    from lavt_hip import ops
    from lavt_hip.engine import TrainStep
    from test_gpu_dice_boundary import _video_model

    def build(loss, metered):
        model, frames, ids, am, tgt = _video_model()
        vi = torch.tensor([2, 5], dtype=torch.int32, device=DEV)
        step = TrainStep(model.train(), frames, ids, am, tgt[[2, 5]].to(DEV), context=ops.StepContext(), deterministic=True, loss=loss, valid_indices=vi)
        meters = step.make_meters(capacity=8, window_size=4) if metered else None
        step.warmup_and_capture(eager_iters=1)
        assert step.captured
        return step, meters

    with lavt_hip.use_dtype(torch.bfloat16):
        twin, _ = build("ce", False)
        step, meters = build("dice_boundary", True)
        want, lbits = [], []
        for per_clip in ([2, 1], [0, 3]):
            for s in (twin, step):
                s.set_valid_indices(per_clip, 4)
                s.step()
            torch.cuda.synchronize()
            want.append(tuple(twin.stats[2:4].tolist()))
            lbits.append(int(_bits(step.stats)[0]))
            assert step.stats.numel() == 3 + 14 * 2
        assert step.valid_indices.tolist() == [0, 7]
        recs = meters.read().records()
    print(f"[video dice_boundary] ce twin counts {want}; ring {[(float(r['I']), float(r['U'])) for r in recs]}")
    assert want[0] != want[1] and all(u > 0 for _, u in want)
    assert [(float(r["I"]), float(r["U"])) for r in recs] == want
    assert [int(np.float32(r["loss"]).view(np.int32)) for r in recs] == lbits
    assert [float(r["iou"]) for r in recs] == [float(np.float64(i) / np.float64(u)) if i else 0.0 for i, u in want]
    assert step.meter_stats[1:].tolist() == [0.0, *want[-1]] and twin.meter_stats is twin.stats


# ------------------------------------------------------------------------------------------------ 8. launch accounting
def _eager(batches, loss, metered, **kw):
    """an uncaptured step after two eager iterations: -> (step, the launches of one more _body(), its loss, its parameter gradients)"""
    from lavt_hip import _capi as K
    step, _, meters = _step(batches, loss, metered, use_graph=False, **kw)
    step.warmup_and_capture(eager_iters=2)
    K.prof.start()
    try:
        out = step._body().clone()
    finally:
        launches = collections.Counter(r[0] for r in K.prof.stop())
    grads = [p.grad.detach().clone() for p in step.model.parameters() if p.grad is not None]
    return step, launches, out, grads


IU = ("lavt_upsample_iu", "lavt_upsample_iu_sel")


def test_launch_accounting(batches):
    import lavt_hip
    with lavt_hip.use_dtype(torch.bfloat16):
        # mc_dice: one lavt_upsample_iu (and the append) more, loss and gradients untouched
        m_step, m_l, m_loss, m_grads = _eager(batches, "mc_dice", True)
        u_step, u_l, u_loss, u_grads = _eager(batches, "mc_dice", False)
        assert m_l - u_l == collections.Counter({"lavt_upsample_iu": 1, "lavt_meter_append": 1}) and not u_l - m_l, (m_l - u_l, u_l - m_l)
        assert u_step.meter_stats is None and not any(k in u_l for k in IU)
        assert m_step.meter_stats is not None and m_step.meter_stats is not m_step.stats
        assert torch.equal(_bits(m_loss), _bits(u_loss)) and torch.equal(_bits(m_step.stats), _bits(u_step.stats))
        assert len(m_grads) == len(u_grads) > 0 and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(m_grads, u_grads))
        # dice_boundary with valid_indices: the _sel form
        t1 = tuple(b[:3] + (b[3][[1]].contiguous(),) for b in batches)
        m_step, m_l, _, _ = _eager(t1, "dice_boundary", True, valid_indices=torch.tensor([1], dtype=torch.int32, device=DEV))
        u_step, u_l, _, _ = _eager(t1, "dice_boundary", False, valid_indices=torch.tensor([1], dtype=torch.int32, device=DEV))
        assert m_l - u_l == collections.Counter({"lavt_upsample_iu_sel": 1, "lavt_meter_append": 1}) and not u_l - m_l, (m_l - u_l, u_l - m_l)
        assert u_step.meter_stats is None and not any(k in u_l for k in IU) and m_step.stats.numel() == 3 + 14
        # ce: never
        m_step, m_l, _, _ = _eager(batches, "ce", True)
        u_step, u_l, _, _ = _eager(batches, "ce", False)
        assert m_l - u_l == collections.Counter({"lavt_meter_append": 1}) and not u_l - m_l, (m_l - u_l, u_l - m_l)
        assert not any(k in m_l for k in IU) and not any(k in u_l for k in IU)
        assert m_step.meter_stats is m_step.stats and u_step.meter_stats is u_step.stats
