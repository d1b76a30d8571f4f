"""Training meters on the device (DESIGN.md "Training meters"): lavt_meter_append and lavt_grad_norm_tensors through the C ABI, TrainMeters in a captured
TrainStep, FusedAdamW(tensor_norms=True), and the trip through a checkpoint.

What the device block must hold is computed by lavt_hip.meters.reference_log, the host restatement that tests/test_meters_host.py checks bit for bit
against the reference's own SmoothedValue / MetricLogger / IoU (tests/golden/train_meter_cases.npz).  Bounds: the ring and the accumulators are compared
exactly; the logged lr within 1e-6 relative of the fp64 formula (a powf result and one fp32 multiply: a few ulp of 6e-8); per-tensor norms within 2e-6
relative of fp64 torch, the bound tests/test_gpu_train_iteration.py uses for the global norm.

The non-finite inputs used here are ordinary floating-point values (NaN / Inf) in a gradient or an input image."""
import collections
import math

import numpy as np
import pytest
import torch

from meter_cases import PROPS, bits, cases, same_block

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OKW = dict(lr=3e-4, weight_decay=1e-2, max_grad_norm=1.0, skip_nonfinite=True, total_steps=40, power=0.9)


@pytest.fixture(autouse=True)
def _fp32():
    import lavt_hip
    lavt_hip.set_compute_dtype(torch.float32)
    yield
    lavt_hip.set_compute_dtype(torch.float32)


def _bits(t):
    t = t.detach().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _eq(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _lr64(base, k, total, power):
    return base * max(1.0 - k / total, 0.0) ** power if total > 0 else base


# ------------------------------------------------------------------------------------------------ 1. lavt_meter_append through the C ABI
def test_append_ring_and_accumulators_equal_the_fixture():
    """capacity 8, the fixture's 19 (loss, I, U): two wrap-arounds plus 3.  Hand-written stats / ctl / step / hyper; NULL ctl / step at 3 and 11, accumulating
    micro-steps at 4 and 12, a skipped update at 13; a held append (the block's own word, then ctl[4]) after 6 leaves every bit where it was."""
    from lavt_hip import meters as M
    c = cases()["run19"]
    n, window, base_lr, total, power = len(c["losses"]), int(c["window"]), 5e-5, 40.0, 0.9
    meters = M.TrainMeters(capacity=8, window_size=window, device=DEV)
    stats = torch.zeros(4, device=DEV)
    ctl = torch.tensor([0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], device=DEV)
    cnt = torch.zeros(1, device=DEV)
    hyper = torch.tensor([base_lr, 1e-2, 0.9, 0.999, 1e-8], device=DEV)
    null, accumulating, skipped = {3, 11}, {4, 12}, {13}
    lrs, norms, flags = [], [], []
    for i in range(n):
        stats.copy_(torch.tensor([float(c["losses"][i]), 7.0, float(c["I"][i]), float(c["U"][i])]))
        gn = 0.5 + 0.125 * i
        ctl.copy_(torch.tensor([gn, 1.0, 1.0 if i in skipped else 0.0, 0.0, 0.0, 1.0 if i in accumulating else 0.0, 0.0, 0.0]))
        cnt.fill_(float(i + 1))
        if i in null:
            meters.append(stats)
            lr64, want_flags, gn = 0.0, 0, None          # (no control block: 0 in the ring, no norm counted)
        else:
            meters.append(stats, ctl, cnt, hyper, total, power)
            lr64 = _lr64(base_lr, i + 1, total, power)
            want_flags = M.ACCUMULATING if i in accumulating else M.SKIPPED if i in skipped else M.APPLIED
        snap = meters.read()
        got_lr = float(snap.records(1)[0]["lr"])
        print(f"[append {i}] lr {got_lr!r} vs fp64 {lr64!r}: relative {abs(got_lr - lr64) / lr64 if lr64 else 0.0:.3e}")
        assert abs(got_lr - lr64) <= 1e-6 * lr64
        lrs.append(got_lr), norms.append(gn), flags.append(want_flags)
        want = M.reference_log(c["losses"][:i + 1], c["I"][:i + 1], c["U"][:i + 1], 8, window, lrs=lrs, grad_norms=norms, flags=flags)
        diff = same_block(snap, want)
        assert not diff, (i, diff)
        # the reference's own numbers, from the fixture
        assert bits(np.float64(snap.records(1)[0]["iou"])) == bits(c["iou"][i])
        assert [int(v) for v in snap.header[M.H_SEG0:M.H_SEG0 + 5]] == c["seg_correct"][i].tolist()
        assert (int(snap.header[M.H_CUM_I]), int(snap.header[M.H_CUM_U])) == (int(c["cum_I"][i]), int(c["cum_U"][i]))
        for meter, ref in ((snap.loss, c["loss_props"][i]), (snap.iou, c["iou_props"][i])):
            assert np.array_equal(bits(np.array([getattr(meter, p) for p in PROPS])), bits(ref)), i
        assert str(snap).split("  ")[1:] == c["strings"][i].split("  ")[1:]          # (loss and iou; the lr is compared above, within its bound)
        if i == 6:          # held: no record, nothing moves
            before = meters.block.clone()
            meters.pause()
            paused = meters.block.clone()
            meters.append(stats, ctl, cnt, hyper, total, power)
            assert _eq(meters.block, paused) and float(paused[M.H_HOLD]) == 1.0
            meters.resume()
            ctl[4:5].fill_(1.0)
            meters.append(stats, ctl, cnt, hyper, total, power)
            torch.cuda.synchronize()
            assert _eq(meters.block, before)
    s = snap.summary()
    assert bits(np.float64(s["mean_iou"])) == bits(c["mean_iou"]) and np.float32(s["overall_iou"]) == np.float32(c["overall_iou"])
    assert (s["iterations"], s["applied"], s["skipped"], s["nonfinite_losses"]) == (19, 19 - 2 - 2 - 1, 1, 0)
    assert snap.n == 19 and sorted(snap.ring["it"].tolist()) == list(range(11, 19))


def test_append_refuses_bad_arguments():
    from lavt_hip import _capi as K
    stats = torch.zeros(4, device=DEV)
    block = torch.zeros(32 + 5 * 8, dtype=torch.float64, device=DEV)
    for args in ((None, None, None, None, 0.0, 0.0, K.ptr(block), 8), (K.ptr(stats), None, None, None, 0.0, 0.0, None, 8),
                 (K.ptr(stats), None, None, None, 0.0, 0.0, K.ptr(block), 0), (K.ptr(stats), None, None, None, 0.0, 0.0, K.ptr(block) + 4, 8)):
        assert K.lib.lavt_meter_append(*args, K.stream()) != 0
    torch.cuda.synchronize()
    assert not bool(block.any())


# ------------------------------------------------------------------------------------------------ 2. lavt_grad_norm_tensors
SIZES = [1, 31, 8192, 8193, 20000]          # a lone element, a partial chunk, exactly one chunk, two chunks with a tail of 1, three with a tail


def _five(seed, **kw):
    from lavt_hip.optim import FusedAdamW
    g = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter(torch.zeros(n, device=DEV)) for n in SIZES]
    for p in ps:
        p.grad = (torch.randn(p.numel(), generator=g) * 3.0).to(DEV)
    return ps, FusedAdamW(ps, lr=0.0, weight_decay=0.0, skip_nonfinite=True, tensor_norms=True, **kw)


def test_tensor_norms_against_fp64_and_the_non_finite_report():
    ps, opt = _five(3)
    assert opt.guard is not None and opt.last_nonfinite() is None
    opt.step()
    assert opt._tn[0].tolist() == [0, 1, 2, 3, 5, 8]
    got = opt.grad_norms()
    assert list(got) == [0, 1, 2, 3, 4]          # (no owning step: the keys are table indices)
    for i, p in enumerate(ps):
        want = float(torch.linalg.vector_norm(p.grad.double()))
        print(f"[tensor {i}, {p.numel()} elements] {got[i]!r} vs fp64 {want!r}: relative {abs(got[i] - want) / want:.3e}")
        assert abs(got[i] - want) <= 2e-6 * want
    total = math.sqrt(sum(v * v for v in got.values()))
    assert abs(total - opt.last_grad_norm()) <= 2e-6 * total
    assert opt._tn_bad.tolist()[:3] == [-1, 0, -1]
    clean = ps[3].grad.clone()
    ps[3].grad[8192] = math.inf          # the tail chunk of tensor 3 only
    opt.step()
    assert opt._tn_bad.tolist()[:3] == [3, 1, 3] and opt.last_nonfinite() == 3 and opt.skipped_steps() == 1
    norms = opt.grad_norms()
    assert math.isinf(norms[3]) and all(math.isfinite(norms[i]) for i in (0, 1, 2, 4))
    ps[3].grad.copy_(clean)
    opt.step()
    assert opt._tn_bad.tolist()[:3] == [-1, 0, 3] and opt.last_nonfinite() == 3 and math.isfinite(opt.grad_norms()[3])
    # hold / accumulating: returns before any store
    out, bad = opt._tn[1].clone(), opt._tn_bad.clone()
    ps[1].grad.fill_(math.nan)
    for word in (4, 5):
        opt.guard[word:word + 1].fill_(1.0)
        opt.step()
        torch.cuda.synchronize()
        assert _eq(opt._tn[1], out) and _eq(opt._tn_bad, bad)
        opt.guard[word:word + 1].fill_(0.0)


def test_tensor_norms_are_bit_reproducible():
    outs = []
    for _ in range(2):
        _, opt = _five(11)
        opt.step()
        torch.cuda.synchronize()
        outs.append(opt._tn[1].clone())
    assert bool((outs[0] > 0).all()) and _eq(outs[0], outs[1])


# ------------------------------------------------------------------------------------------------ 3 - 6. the harness
def _micro(dpr=0.0):
    from test_gpu_modules import _build          # the micro model of tests/test_gpu_train_iteration.py
    return _build(32, [2, 2, 2, 2], [1, 2, 4, 8], 7, dpr=dpr).train()


@pytest.fixture(scope="module")
def batches():
    """the micro-batches every harness test loads into its static buffers: made once, never written"""
    from lavt_hip.detweights import det_inputs
    return [tuple(v.to(DEV) for v in det_inputs(2, 64, 20, seed=17 + i)) for i in range(3)]


def _load(static, batch):
    for dst, src in zip(static, batch):
        dst.copy_(src)


def _harness(batches, meters=True, **step_kw):
    """-> (step, opt, parameters, static input buffers, meters) in a private context, deterministic, before warmup_and_capture()"""
    from lavt_hip import ops
    from lavt_hip.engine import TrainStep
    static = tuple(v.clone() for v in batches[0])
    model = _micro()
    step = TrainStep(model, *static, world=1, use_graph=True, context=ops.StepContext(), deterministic=True, **step_kw)
    ps = [p for p in model.parameters()]
    opt = step.make_optimizer(ps, tensor_norms=bool(meters), **OKW)
    m = step.make_meters(capacity=8, window_size=4) if meters else None
    return step, opt, ps, static, m


def test_captured_step_logs_every_replay(batches):
    """13 replays into a ring of 8: after every replay a synchronous read of step.stats, opt.guard and the step counter gives the record the ring must hold"""
    import lavt_hip
    from lavt_hip import meters as M
    with lavt_hip.use_dtype(torch.bfloat16):
        step, opt, ps, static, meters = _harness(batches)
        step.warmup_and_capture()
        assert step.captured
        snap = meters.read()
        assert snap.n == 0 and snap.iterations == 0 and not snap.ring.view(np.uint8).any() and float(snap.header[M.H_HOLD]) == 0.0
        assert opt.steps_taken() == 0
        losses, Is, Us, lrs, norms, flags = [], [], [], [], [], []
        for i in range(13):
            _load(static, batches[i % 3])
            step.step()
            polled = meters.poll()
            assert polled is None or polled.n <= i + 1          # never a snapshot newer than the replays issued
            torch.cuda.synchronize()
            st, guard, k = step.stats.tolist(), opt.guard.tolist(), opt.steps_taken()
            assert k == i + 1 and guard[2] == 0.0
            snap = meters.read()
            rec = snap.records(1)[0]
            lr64 = _lr64(OKW["lr"], k, OKW["total_steps"], OKW["power"])
            assert abs(float(rec["lr"]) - lr64) <= 1e-6 * lr64, (float(rec["lr"]), lr64)
            losses.append(st[0]), Is.append(st[2]), Us.append(st[3]), lrs.append(float(rec["lr"])), norms.append(guard[0]), flags.append(M.APPLIED)
            want = M.reference_log(losses, Is, Us, 8, 4, lrs=lrs, grad_norms=norms, flags=flags)
            diff = same_block(snap, want)
            assert not diff, (i, diff)
        assert Us[-1] > 0 and len(set(losses)) > 3
        assert snap.header[M.H_LOSS_SUM] == sum(float(np.float32(v)) for v in losses)          # Python's double sum of the fp32 losses, in order
        last = meters.read()
        assert last.n == 13 and last.loss.value == float(np.float32(losses[-1])) and last.grad_norm.value == float(np.float32(norms[-1]))
        assert last.loss.global_avg == sum(float(np.float32(v)) for v in losses) / 13
        polled = meters.poll() or meters.poll()
        assert polled is not None and polled.n <= 13
        got = opt.grad_norms()
        names = {id(p): n for n, p in step.model.named_parameters()}
        assert set(got) == set(names.values())
        worst = 0.0
        for p in ps:
            want_n = float(torch.linalg.vector_norm(p.grad.double()))
            assert abs(got[names[id(p)]] - want_n) <= 2e-6 * want_n, (names[id(p)], got[names[id(p)]], want_n)
            worst = max(worst, abs(got[names[id(p)]] - want_n) / want_n if want_n else 0.0)
        print(f"[tensor norms] {len(ps)} tensors, worst relative error {worst:.3e}")
        assert opt.last_nonfinite() is None
        s = meters.epoch_summary()
        assert (s["iterations"], s["applied"], s["skipped"], s["nonfinite_losses"]) == (13, 13, 0, 0)


def test_meters_change_nothing_and_cost_two_launches(batches):
    """two steps from one state, one with meters and tensor norms, one without: after 3 replays parameters, moments and loss are bit-identical; an eager
    iteration of the metered step issues exactly one lavt_meter_append and one lavt_grad_norm_tensors more"""
    import lavt_hip
    from lavt_hip import _capi as K
    sides, launches = [], []
    with lavt_hip.use_dtype(torch.bfloat16):
        for with_meters in (True, False):
            step, opt, ps, static, meters = _harness(batches, meters=with_meters)
            step.warmup_and_capture()
            assert step.captured
            out = []
            for i in range(3):
                _load(static, batches[i])
                out.append(step.step().clone())
            torch.cuda.synchronize()
            assert opt.steps_taken() == 3
            sides.append([p.detach().clone() for p in ps] + [opt.state[p][k].clone() for k in ("exp_avg", "exp_avg_sq") for p in ps] + [torch.stack(out)])
            K.prof.start()
            try:
                step._body()
            finally:
                launches.append(collections.Counter(r[0] for r in K.prof.stop()))
    assert len(sides[0]) == len(sides[1]) and all(_eq(a, b) for a, b in zip(sides[0], sides[1]))
    more = launches[0] - launches[1]
    assert more == collections.Counter({"lavt_meter_append": 1, "lavt_grad_norm_tensors": 1}) and not launches[1] - launches[0], (more, launches[1] - launches[0])


def test_accumulation_and_a_skipped_cycle(batches):
    """accumulate=2; the first micro-batch of the second cycle is a NaN image: that cycle reads accumulating, then skipped, exactly once"""
    import lavt_hip
    from lavt_hip import meters as M
    with lavt_hip.use_dtype(torch.bfloat16):
        step, opt, ps, static, meters = _harness(batches, accumulate=2)
        step.warmup_and_capture()
        assert step.captured and meters.read().n == 0
        for i in range(6):
            _load(static, batches[i % 2])
            if i == 2:
                static[0].fill_(math.nan)
            step.step()
            if i == 3:
                bad = opt.last_nonfinite()
                assert bad is not None and opt.skipped_steps() == 1
        snap = meters.read()
        recs = snap.records()
        assert recs["it"].tolist() == list(range(6))
        assert [int(f) & 7 for f in recs["flags"]] == [M.ACCUMULATING, M.APPLIED, M.ACCUMULATING, M.SKIPPED, M.ACCUMULATING, M.APPLIED]
        # (whether the criterion's loss of the NaN image is itself NaN is the criterion's business: the flag must say what the ring's raw value is)
        nonfinite = [not math.isfinite(float(v)) for v in recs["loss"]]
        assert [bool(int(f) & M.LOSS_NONFINITE) for f in recs["flags"]] == nonfinite and not any(nonfinite[:2] + nonfinite[3:])
        print(f"[skipped cycle] losses {recs['loss'].tolist()}, norms {recs['grad_norm'].tolist()}")
        assert not math.isfinite(float(recs["grad_norm"][3])) and math.isfinite(float(recs["grad_norm"][5]))
        assert opt.last_nonfinite() == bad and isinstance(bad, str)          # sticky over the clean cycle
        s = meters.epoch_summary()
        assert (s["iterations"], s["applied"], s["skipped"], s["nonfinite_losses"]) == (6, 2, 1, sum(nonfinite)) and math.isfinite(s["mean_loss"])
        assert int(snap.header[M.H_ACCUMULATING]) == 3 and int(snap.header[M.H_NORM_COUNT]) == 2
        meters.reset_epoch()
        for i in range(2):
            _load(static, batches[i])
            step.step()
        snap = meters.read()
        assert snap.n == 8 and snap.iterations == 2 and int(snap.header[M.H_EPOCH_START]) == 6
        assert snap.records()["it"].tolist() == [6, 7] and len(snap.loss.window) == 2
        s = snap.summary()
        assert (s["iterations"], s["applied"], s["skipped"], s["nonfinite_losses"]) == (2, 1, 0, 0)
        assert snap.loss.global_avg == sum(float(v) for v in snap.records()["loss"]) / 2


def test_wiring(batches):
    import lavt_hip
    from lavt_hip import ops
    from lavt_hip.engine import TrainStep
    from lavt_hip.meters import TrainMeters
    with lavt_hip.use_dtype(torch.bfloat16):
        with pytest.raises(ValueError, match="fused criterion"):
            TrainStep(_micro(), *batches[0], context=ops.StepContext(), fused_loss=False, meters=TrainMeters(capacity=4, window_size=2, device=DEV))
        with pytest.raises(ValueError, match="window_size"):
            TrainMeters(capacity=4, window_size=5, device=DEV)
        step = TrainStep(_micro(), *batches[0], context=ops.StepContext())          # no optimizer: NULL ctl / step / hyper
        meters = step.make_meters(capacity=4, window_size=2)
        with pytest.raises(RuntimeError, match="already attached"):
            step.make_meters()
        step.warmup_and_capture()
        with pytest.raises(RuntimeError, match="before warmup_and_capture"):
            step.attach_meters(meters)
        assert meters.read().n == 0
        step.step()
        snap = meters.read()
        rec = snap.records()[0]
        assert snap.n == 1 and int(rec["flags"]) == 0 and float(rec["lr"]) == 0.0 and float(rec["grad_norm"]) == 0.0
        assert float(rec["loss"]) == float(step.stats[0]) and float(rec["U"]) == float(step.stats[3])


def test_save_and_load_round_trip(tmp_path):
    """6 steps without interruption against 3 steps, a file, a new process-like rebuild, 3 more: the resumed block equals the uninterrupted one bit for bit"""
    import lavt_hip
    from lavt_hip.checkpoint import load_train_state, save_train_state
    from lavt_hip.meters import TrainMeters
    from test_gpu_train_state import _batches2d, _micro2d, _start, _steps
    data = _batches2d(6)
    path = str(tmp_path / "run.pt")

    def start(salt, seed):
        meters = TrainMeters(capacity=4, window_size=3, device=DEV)
        step, static = _start(_micro2d, salt, seed, {}, meters=meters)
        return step, static, meters

    with lavt_hip.use_dtype(torch.bfloat16):
        step, static, meters = start(0, 1234)
        _steps(step, static, data, 0, 6)
        whole = meters.read()
        del step
        step, static, meters = start(0, 1234)
        _steps(step, static, data, 0, 3)
        save_train_state(path, step, meters=meters.state_dict(), epoch=0)
        del step
        step, static, meters = start(7, 99)
        extra = load_train_state(path, step)
        assert set(extra) == {"meters", "epoch"}
        meters.load_state_dict(extra["meters"])
        assert meters.read().n == 3
        _steps(step, static, data, 3, 6)
        resumed = meters.read()
    diff = same_block(resumed, whole)
    assert not diff, diff
    assert resumed.n == 6 and resumed.loss.global_avg == whole.loss.global_avg and resumed.summary() == whole.summary() and str(resumed) == str(whole)
