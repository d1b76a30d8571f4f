"""Gradient accumulation over micro-batches: lavt_grad_accumulate through the C ABI (select / fold, the float4 and the element-wise path, the phase in
the control block, hold), and TrainStep(accumulate=k) -- one captured graph serves every micro-step of a cycle, replay k applies one AdamW update from
the mean of the k gradients.

The non-finite inputs used here are ordinary floating-point values (NaN / Inf) in an accumulation buffer or an input image."""
import math

import pytest
import torch

from lavt_hip.detweights import det_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OKW = dict(lr=3e-4, weight_decay=1e-2, max_grad_norm=1.0, skip_nonfinite=True)


@pytest.fixture(autouse=True)
def _fp32():
    import lavt_hip
    lavt_hip.set_compute_dtype(torch.float32)
    yield
    lavt_hip.set_compute_dtype(torch.float32)


def _bits(t):
    return t.detach().contiguous().view(torch.uint8 if t.element_size() == 1 else torch.int16 if t.element_size() == 2 else torch.int32)


def _eq(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ 1. the kernel through the C ABI
SIZES = [1, 3, 1023, 4096, 262151]
# (the issue's sizes never reach the cap of 2048 workgroups; this one does on both paths: float4 with 8 M + 4099 elements, element-wise from 512 K on)
BIG = 2048 * 256 * 4 * 4 + 4099
OFFSETS = [(0, 0), (0, 1), (1, 0), (1, 1)]          # float offsets of g and acc from an aligned allocation: only (0, 0) takes the float4 path


class _Cycle:
    """The launch sequence of one micro-step, as the harness issues it, on buffers of the test's own: lavt_grad_accumulate, then a guarded update -- a
    one-tensor FusedAdamW with lr 0 whose control block is the `ctl` of the fold and whose tick is what advances the micro index (the write of m comes
    after everything of the step that reads the phase, include/lavt_hip.h)."""

    def __init__(self):
        from lavt_hip.optim import FusedAdamW
        self.p = torch.nn.Parameter(torch.zeros(8, device=DEV))
        self.p.grad = torch.zeros_like(self.p)
        self.opt = FusedAdamW([self.p], lr=0.0, weight_decay=0.0)
        self.opt.hold(False)                          # creates the control block: the guarded launches
        self.ctl = self.opt.guard
        assert self.ctl.tolist() == [0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]

    def fold(self, g, acc, k):
        from lavt_hip import _capi as K
        K.check(K.lib.lavt_grad_accumulate(K.ptr(g), K.ptr(acc), g.numel(), k, K.ptr(self.ctl), K.stream()))

    def tick(self):
        self.opt.step()


def _views(n, og, oa, seed):
    gen = torch.Generator().manual_seed(seed)
    gbuf, abuf = torch.zeros(n + 8, device=DEV), torch.zeros(n + 8, device=DEV)
    g, acc = gbuf[og:og + n], abuf[oa:oa + n]
    assert gbuf.data_ptr() % 16 == 0 and abuf.data_ptr() % 16 == 0
    acc.copy_(torch.randn(n, generator=gen))          # what an earlier cycle left: the first fold must not look at it
    return gbuf, abuf, g, acc, gen


@pytest.mark.parametrize("k,n", [(k, n) for k in (2, 4) for n in SIZES] + [(2, BIG)])
def test_fold_is_bitwise_the_torch_expression_and_the_phase_follows(k, n):
    """s = 1/k is a power of two: s * g is exact and fmaf equals multiply-then-add, so after every call acc is BITWISE s * g (m == 0) or acc + s * g in
    torch's fp32.  Two whole cycles per alignment: after the fold ctl[5] = (m != k - 1) with m still in ctl[6], after the step's tick ctl[6] = (m + 1) % k
    (the wrap included); the words around both views are untouched."""
    cyc = _Cycle()
    s, applied = 1.0 / k, 0
    for og, oa in OFFSETS:
        gbuf, abuf, g, acc, gen = _views(n, og, oa, seed=100 * k + 10 * og + oa)
        for call in range(2 * k):
            m = call % k
            g.copy_(torch.randn(n, generator=gen) * (1.0 + call))
            want = s * g if m == 0 else acc + s * g
            cyc.fold(g, acc, k)
            torch.cuda.synchronize()
            assert _eq(acc, want), (n, k, og, oa, call)
            assert cyc.ctl[5:7].tolist() == [float(m != k - 1), float(m)], (call, cyc.ctl.tolist())
            cyc.tick()
            assert cyc.ctl[5:7].tolist() == [float(m != k - 1), float((m + 1) % k)], (call, cyc.ctl.tolist())
            applied += m == k - 1
            assert cyc.opt.steps_taken() == applied                                           # the update ran on the k-th micro-step only
        assert not bool(abuf[:oa].any()) and not bool(abuf[oa + n:].any()) and not bool(gbuf[:og].any()) and not bool(gbuf[og + n:].any())
    assert cyc.ctl[[0, 2, 3, 4]].tolist() == [0.0, 0.0, 0.0, 0.0] and float(cyc.ctl[1]) == 1.0


@pytest.mark.parametrize("n", SIZES)
def test_fold_k3_within_the_derived_bound(n):
    """k = 3: s = fp32(1/3).  Element-wise |acc - fp64 reference| <= k * 2^-23 * sum_i |s * g_i|: k roundings (one product, k - 1 fused multiply-adds) of at
    most one ulp of a running sum that never exceeds sum_i |s * g_i|; the rounding of s itself (2^-24 relative) fits in the same allowance."""
    k = 3
    cyc = _Cycle()
    for og, oa in OFFSETS:
        _, _, g, acc, gen = _views(n, og, oa, seed=7 + 10 * og + oa)
        ref, mag = torch.zeros(n, dtype=torch.float64, device=DEV), torch.zeros(n, dtype=torch.float64, device=DEV)
        for m in range(k):
            g.copy_(torch.randn(n, generator=gen) * (1.0 + m))
            ref += g.double() / 3.0
            mag += (g.double() / 3.0).abs()
            cyc.fold(g, acc, k)
            cyc.tick()
        torch.cuda.synchronize()
        err = (acc.double() - ref).abs()
        bound = k * 2.0 ** -23 * mag
        worst = int((err - bound).argmax())
        print(f"\n[k=3 n={n} offsets=({og},{oa})] max err {float(err.max()):.3e}, err/bound max {float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= bound).all()), (n, og, oa, float(err[worst]), float(bound[worst]))
        assert cyc.ctl[5:7].tolist() == [0.0, 0.0]


@pytest.mark.parametrize("n", SIZES)
def test_first_micro_step_selects_nan_and_inf_do_not_survive(n):
    """m == 0 never reads acc: whatever an earlier cycle left there -- NaN, +Inf, -Inf -- the result is exactly s * g"""
    cyc = _Cycle()
    for og, oa in OFFSETS:
        _, _, g, acc, gen = _views(n, og, oa, seed=31 + 10 * og + oa)
        poison = torch.tensor([math.nan, math.inf, -math.inf], device=DEV)
        acc.copy_(poison[torch.arange(n, device=DEV) % 3])
        g.copy_(torch.randn(n, generator=gen))
        cyc.fold(g, acc, 2)
        torch.cuda.synchronize()
        assert _eq(acc, 0.5 * g) and bool(torch.isfinite(acc).all())
        cyc.tick()
        cyc.fold(g, acc, 2)                            # ends the cycle, so that the next alignment starts at m == 0 again
        cyc.tick()
        assert cyc.ctl[5:7].tolist() == [0.0, 0.0]


@pytest.mark.parametrize("n", SIZES)
def test_hold_stops_the_fold(n):
    """ctl[4] = 1: nothing is read or written -- acc and the whole control block keep their bits, at m == 0 and in the middle of a cycle"""
    cyc = _Cycle()
    for og, oa in OFFSETS:
        _, _, g, acc, gen = _views(n, og, oa, seed=53 + 10 * og + oa)
        g.copy_(torch.randn(n, generator=gen))
        for mid in (False, True):
            if mid:
                cyc.fold(g, acc, 3)
                cyc.tick()
                assert cyc.ctl[5:7].tolist() == [1.0, 1.0]
            cyc.opt.hold(True)
            acc0, ctl0 = acc.clone(), cyc.ctl.clone()
            cyc.fold(g, acc, 3)
            cyc.tick()                                 # a held step does not advance m either
            torch.cuda.synchronize()
            assert _eq(acc, acc0) and _eq(cyc.ctl, ctl0)
            cyc.opt.hold(False)
        for _ in range(2):                             # end the open cycle of three
            cyc.fold(g, acc, 3)
            cyc.tick()
        assert cyc.ctl[5:7].tolist() == [0.0, 0.0]


def test_fold_refuses_bad_arguments():
    from lavt_hip import _capi as K
    ctl = torch.tensor([0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]).to(DEV)
    buf = torch.zeros(64, device=DEV)
    for g, acc, n, k in ((buf[:32], buf[32:], 32, 0), (buf[:32], buf[16:48], 32, 2), (buf[:32], buf[32:], 0, 2)):
        with pytest.raises(RuntimeError, match="lavt_grad_accumulate"):
            K.check(K.lib.lavt_grad_accumulate(K.ptr(g), K.ptr(acc), n, k, K.ptr(ctl), K.stream()))
    torch.cuda.synchronize()
    assert not bool(buf.any()) and ctl.tolist() == [0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]


# ------------------------------------------------------------------------------------------------ 2-7. the harness
def _micro():
    from test_gpu_modules import _build          # the micro model of tests/test_gpu_train_iteration.py
    return _build(32, [2, 2, 2, 2], [1, 2, 4, 8], 7, dpr=0.0).train()


def _batch(seed):
    return tuple(v.to(DEV) for v in det_inputs(2, 64, 20, seed=seed))


@pytest.fixture(scope="module")
def batches():
    """the two micro-batches every harness test loads into its static buffers: made once, never written"""
    return _batch(17), _batch(18)


def _load(static, batch):
    for dst, src in zip(static, batch):
        dst.copy_(src)


def _harness(batches, accumulate=2, use_graph=True, optimizer=True, **step_kw):
    """-> (step, opt, parameters, static input buffers) in a private context, bf16, before warmup_and_capture()"""
    from lavt_hip import ops
    from lavt_hip.engine import TrainStep
    static = tuple(v.clone() for v in batches[0])
    model = _micro()
    step = TrainStep(model, *static, world=1, use_graph=use_graph, context=ops.StepContext(), accumulate=accumulate, **step_kw)
    ps = [p for p in model.parameters()]
    opt = step.make_optimizer(ps, **OKW) if optimizer else None
    return step, opt, ps, static


def _state(opt, ps):
    """bitwise snapshot of what an update may write: parameters, both moments, the bf16 compute copies, the step counter"""
    from lavt_hip import ops
    torch.cuda.synchronize()
    out = [p.detach().clone() for p in ps]
    out += [opt.state[p][key].clone() for key in ("exp_avg", "exp_avg_sq") for p in ps]
    with ops.use_context(opt.context):
        out += [ops.weights.store[(id(p), torch.bfloat16, "lin")][1].clone() for p in ps if (id(p), torch.bfloat16, "lin") in ops.weights.store]
    out.append(opt._step.clone())
    return out


def _same(a, b):
    return len(a) == len(b) and all(_eq(x, y) for x, y in zip(a, b))


def test_one_cycle_in_the_captured_harness(batches):
    """accumulate=2, bf16, deterministic, captured: replay 1 leaves parameters, moments, compute copies and the step counter bit for bit alone; replay 2
    applies ONE update from acc = 0.5 * g1 + 0.5 * g2 -- the bits of a twin FusedAdamW stepped once, eagerly, on the initial parameters with that acc as
    its gradients -- and the norm it reports is acc's."""
    import lavt_hip
    from lavt_hip import ops
    from lavt_hip.optim import FusedAdamW
    with lavt_hip.use_dtype(torch.bfloat16):
        step, opt, ps, static = _harness(batches, deterministic=True)
        init = [p.detach().clone() for p in ps]
        step.warmup_and_capture()
        assert step.captured and step.acc is not None and step.acc.shape == step.buckets.flat.shape
        before = _state(opt, ps)
        assert len(before) > 3 * len(ps) + 1, "the micro model has bf16 compute copies in the parameter's layout"

        _load(static, batches[0])
        loss1 = float(step.step())
        assert _same(_state(opt, ps), before)
        assert opt.steps_taken() == 0 and step.micro_step() == 1 and opt.guard[5:7].tolist() == [1.0, 1.0]
        g1 = step.buckets.flat.clone()

        _load(static, batches[1])
        loss2 = float(step.step())
        torch.cuda.synchronize()
        g2 = step.buckets.flat.clone()
        assert math.isfinite(loss1) and math.isfinite(loss2) and loss1 != loss2          # each call returns its own micro-batch's loss
        assert bool(g1.any()) and not torch.equal(g1, g2)
        assert opt.steps_taken() == 1 and opt.skipped_steps() == 0 and step.micro_step() == 0 and opt.guard[5:7].tolist() == [0.0, 0.0]
        assert _eq(step.acc, 0.5 * g1 + 0.5 * g2)
        norm = float(torch.linalg.vector_norm(step.acc.double()))
        print(f"\n[one cycle] last_grad_norm {opt.last_grad_norm():.9g} vs fp64 {norm:.9g}: relative {abs(opt.last_grad_norm() - norm) / norm:.3e}")
        assert abs(opt.last_grad_norm() - norm) <= 1e-6 * norm

        qs = [torch.nn.Parameter(v.clone()) for v in init]
        for q, p in zip(qs, ps):
            o = step.buckets.offset_of[id(p)]
            q.grad = step.acc[o:o + p.numel()].view_as(p)
        twin = FusedAdamW(qs, **OKW)
        twin.step()
        torch.cuda.synchronize()
        assert twin.steps_taken() == 1 and twin.skipped_steps() == 0
        bad = [i for i, (p, q) in enumerate(zip(ps, qs)) if not (_eq(p, q) and _eq(opt.state[p]["exp_avg"], twin.state[q]["exp_avg"])
                                                                 and _eq(opt.state[p]["exp_avg_sq"], twin.state[q]["exp_avg_sq"]))]
        assert not bad, f"{len(bad)} of {len(ps)} tensors differ from the twin's, e.g. {bad[:6]}"
        assert any(not _eq(p, v) for p, v in zip(ps, init))
        with ops.use_context(step.context):
            lin = [e for key, e in ops.weights.store.items() if key[1] == torch.bfloat16 and key[2] == "lin" and e[2]() is not None]
            assert lin and all(torch.equal(e[1].view(-1), e[2]().detach().to(torch.bfloat16).view(-1)) for e in lin)


def test_warm_up_leaves_the_accumulation_alone(batches):
    """the optimizer is on hold for the eager iterations and the validation replays, and hold stops the fold: parameters, the micro index and every bit
    of acc (a sentinel) leave warmup_and_capture() as they entered it"""
    import lavt_hip
    with lavt_hip.use_dtype(torch.bfloat16):
        step, opt, ps, _ = _harness(batches)
        step.acc.fill_(123.25)
        init = [p.detach().clone() for p in ps]
        step.warmup_and_capture()
        torch.cuda.synchronize()
        assert step.captured
        assert all(_eq(p, v) for p, v in zip(ps, init))
        assert step.micro_step() == 0 and opt.guard[4:7].tolist() == [0.0, 0.0, 0.0] and opt.steps_taken() == 0 and opt.skipped_steps() == 0
        assert _eq(step.acc, torch.full_like(step.acc, 123.25))


def test_a_non_finite_micro_batch_skips_its_cycle_once(batches):
    """The FIRST micro-batch of a cycle is a NaN image, through a replay: the NaN has to survive the second fold, the cycle's update is skipped and counted
    once (not once per micro-step); the next, clean cycle selects over the NaN in acc and applies."""
    import lavt_hip
    with lavt_hip.use_dtype(torch.bfloat16):
        step, opt, ps, static = _harness(batches)
        step.warmup_and_capture()
        assert step.captured
        before = _state(opt, ps)
        _load(static, batches[0])
        static[0].fill_(math.nan)
        step.step()
        _load(static, batches[1])
        step.step()
        torch.cuda.synchronize()
        assert bool(torch.isnan(step.acc).any())
        assert _same(_state(opt, ps), before)
        assert opt.steps_taken() == 0 and opt.skipped_steps() == 1 and step.micro_step() == 0
        assert not math.isfinite(opt.last_grad_norm())
        for b in batches:
            _load(static, b)
            step.step()
        torch.cuda.synchronize()
        assert opt.steps_taken() == 1 and opt.skipped_steps() == 1 and step.micro_step() == 0
        assert bool(torch.isfinite(step.acc).all()) and math.isfinite(opt.last_grad_norm())
        assert all(bool(torch.isfinite(p).all()) for p in ps) and any(not _eq(p, v) for p, v in zip(ps, before))


def test_graph_equals_eager_over_two_cycles(batches):
    """deterministic=True, two cycles of accumulate=2 from identical state on identical batches: replayed and eagerly launched steps leave the same bits in
    parameters, moments and acc (DropPath is off and BatchNorm normalises with batch statistics, so the extra validation replays of a capture do not
    enter)"""
    import lavt_hip
    sides = []
    with lavt_hip.use_dtype(torch.bfloat16):
        for use_graph in (True, False):
            step, opt, ps, static = _harness(batches, use_graph=use_graph, deterministic=True)
            step.warmup_and_capture()
            assert step.captured == use_graph
            losses = []
            for it in range(4):
                _load(static, batches[it % 2])
                losses.append(step.step().clone())
            torch.cuda.synchronize()
            assert opt.steps_taken() == 2 and opt.skipped_steps() == 0 and step.micro_step() == 0
            sides.append((_state(opt, ps) + [step.acc.clone()], torch.stack(losses)))
    assert _same(sides[0][0], sides[1][0])
    assert _eq(sides[0][1], sides[1][1])


def test_replays_see_the_language_inputs_of_the_next_batch(batches):
    """What accumulation over micro-batches rests on: a replay computes on what the static buffers hold NOW, the language features and mask included (the
    per-forward language context -- transposed features, mask rows -- is rebuilt inside the capture, not left in the graph as constants of the warm-up
    batch).  accumulate=1, deterministic: after one update on batch 17, the replayed and the eagerly launched step give the same loss bits on batch 18."""
    import lavt_hip
    losses = []
    with lavt_hip.use_dtype(torch.bfloat16):
        for use_graph in (True, False):
            step, opt, _, static = _harness(batches, accumulate=1, use_graph=use_graph, deterministic=True)
            step.warmup_and_capture()
            assert step.captured == use_graph and step.acc is None
            out = []
            for b in batches:
                _load(static, b)
                out.append(step.step().clone())
            torch.cuda.synchronize()
            assert opt.steps_taken() == 2
            losses.append(torch.stack(out))
    assert not _eq(batches[0][1], batches[1][1]), "the two batches must differ in their language features"
    assert _eq(losses[0], losses[1]), (losses[0].tolist(), losses[1].tolist())


def test_accumulate_one_is_the_harness_as_it_was(batches):
    """no second buffer and, without guard options, no control block"""
    import lavt_hip
    from lavt_hip import ops
    from lavt_hip.engine import TrainStep
    with lavt_hip.use_dtype(torch.bfloat16):
        for kw in ({}, {"accumulate": 1}):
            step = TrainStep(_micro(), *batches[0], world=1, use_graph=True, context=ops.StepContext(), **kw)
            opt = step.make_optimizer(lr=3e-4)
            assert step.accumulate == 1 and step.acc is None and opt.guard is None and opt._grad_source is None
            assert step.micro_step() == 0
            step.reset_accumulation()                  # nothing to reset: no control block appears
            assert opt.guard is None


def test_wiring_and_reset(batches):
    """accumulate > 1 without an owned optimizer is refused where the launch sequence is fixed; reset_accumulation() restarts an open cycle"""
    import lavt_hip
    with lavt_hip.use_dtype(torch.bfloat16):
        step, _, _, _ = _harness(batches, optimizer=False)
        with pytest.raises(RuntimeError, match="make_optimizer"):
            step.warmup_and_capture()
        step, opt, ps, static = _harness(batches, use_graph=False)
        with pytest.raises(RuntimeError, match="warmup_and_capture"):
            step.step()
        step.warmup_and_capture(eager_iters=1)
        step.step()
        assert step.micro_step() == 1 and opt.guard[5:7].tolist() == [1.0, 1.0]
        step.reset_accumulation()
        assert step.micro_step() == 0 and opt.guard[5:7].tolist() == [0.0, 0.0]
        step.acc.fill_(math.nan)                       # (as after loading a checkpoint: acc holds nothing of value)
        step.step()
        assert step.micro_step() == 1 and opt.steps_taken() == 0
        step.step()
        torch.cuda.synchronize()
        assert step.micro_step() == 0 and opt.steps_taken() == 1 and opt.skipped_steps() == 0 and bool(torch.isfinite(step.acc).all())
