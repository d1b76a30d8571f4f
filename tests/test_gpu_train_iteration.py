"""The captured train iteration: global gradient norm (lavt_grad_norm), the guarded AdamW update (clip by global norm, skip-if-non-finite, hold) and
the step harness owning its optimizer (TrainStep.make_optimizer / attach_optimizer: one hipGraph replay = one whole training iteration).

The non-finite inputs used here are ordinary floating-point values (Inf / NaN) in gradient buffers."""
import json
import math
import os

import numpy as np
import pytest
import torch

from lavt_hip.detweights import det_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _fp32():
    import lavt_hip
    lavt_hip.set_compute_dtype(torch.float32)
    yield
    lavt_hip.set_compute_dtype(torch.float32)


def _problem(steps=6):
    """the data of test_gpu_ops._adamw_problem (own copy) plus one tensor of several whole chunks and a partial one"""
    g = torch.Generator().manual_seed(11)
    shapes = [(33, 17), (128,), (5, 3, 3, 3), (1000, 64), (7,)]
    params = [torch.randn(*s, generator=g) for s in shapes]
    grads = [[torch.randn(*s, generator=g) * (0.1 + k) for s in shapes] for k in range(steps)]
    return params, grads


def _groups(ps):
    return [{"params": ps[:2], "weight_decay": 0.0}, {"params": ps[2:4]}, {"params": ps[4:], "lr": 3e-3}]


def _gate(q, p):
    """the project's own gate (test_fused_adamw_matches_torch)"""
    err = float((q.detach().cpu() - p.detach()).abs().max())
    return err, 2e-6 * max(1.0, float(p.abs().max()))


def _state(opt, ps):
    """bitwise snapshot of everything an update may write: parameters, both moments, the bf16 compute copies, step counter"""
    from lavt_hip import ops
    torch.cuda.synchronize()
    out = [p.detach().clone() for p in ps]
    out += [opt.state[p]["exp_avg"].clone() for p in ps if "exp_avg" in opt.state[p]]
    out += [opt.state[p]["exp_avg_sq"].clone() for p in ps if "exp_avg_sq" in opt.state[p]]
    with ops.use_context(opt.context):
        out += [ops.weights.store[(id(p), torch.bfloat16, "lin")][1].clone() for p in ps if (id(p), torch.bfloat16, "lin") in ops.weights.store]
    out.append(opt._step.clone() if opt._step is not None else torch.zeros(1, device=DEV))
    return out


def _same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(x.view(torch.uint8 if x.element_size() == 1 else torch.int16 if x.element_size() == 2 else torch.int32),
                                                                        y.view(torch.uint8 if y.element_size() == 1 else torch.int16 if y.element_size() == 2 else torch.int32))
                                    for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ 1. the norm
def test_grad_norm_matches_fp64_and_is_reproducible():
    """lavt_grad_norm over a ragged tensor list (sizes around the chunk size, a 1 M-element tensor, a view 4 bytes off 16-byte alignment) vs the fp64 norm
    of the same values on the CPU.  Gate: relative error <= 2e-6 -- per chunk 32 sequential adds per thread and an 8-level tree in fp32 put the sum of
    squares off by at most ~41 * 2^-24 ~ 2.5e-6, the square root halves that, and the final reduction is fp64.  Two runs give identical bits."""
    from lavt_hip import _capi as K
    ce = int(K.lib.lavt_adamw_chunk_elems())
    assert ce == 8192
    gen = torch.Generator().manual_seed(5)
    sizes = [1, 3, 8191, 8192, 8193, 1 << 20]
    host = [torch.randn(n, generator=gen) * (0.5 + i) for i, n in enumerate(sizes)]
    mis_host = torch.randn(20001, generator=gen)
    tensors = [h.to(DEV) for h in host]
    mis_buf = mis_host.to(DEV)
    mis = mis_buf[1:]                                    # 20000 elements starting 4 bytes past a 16-byte boundary
    assert mis.data_ptr() % 16 == 4
    tensors.append(mis)
    host.append(mis_host[1:])
    desc, chunks = [], []
    for t in tensors:
        for c in range(-(-t.numel() // ce)):
            chunks.append([len(desc), c])
        desc.append([0, t.data_ptr(), 0, 0, t.numel(), 0])
    desc_d, chunks_d = torch.tensor(desc, dtype=torch.int64).to(DEV), torch.tensor(chunks, dtype=torch.int32).to(DEV)
    n = len(chunks)
    ref = math.sqrt(sum(float((h.double() ** 2).sum()) for h in host))
    runs = []
    for _ in range(2):
        ws = torch.full((int(K.lib.lavt_grad_norm_ws(n)),), float("nan"), device=DEV)
        ctl = torch.tensor([0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]).to(DEV)
        K.check(K.lib.lavt_grad_norm(K.ptr(desc_d), K.ptr(chunks_d), n, K.ptr(ws), K.ptr(ctl), 0.0, 1, K.stream()))
        torch.cuda.synchronize()
        runs.append((ctl.cpu(), ws.cpu()))
    ctl = runs[0][0]
    rel = abs(float(ctl[0]) - ref) / ref
    print(f"\n[grad norm] device {float(ctl[0]):.9g} vs fp64 {ref:.9g}: relative error {rel:.3e} (gate 2e-6)")
    assert rel <= 2e-6, rel
    assert ctl[1:].tolist() == [1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]                     # no clipping asked for, finite, nothing else touched
    assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32)) and torch.equal(runs[0][1].view(torch.int32), runs[1][1].view(torch.int32))
    # the clip coefficient: torch.nn.utils.clip_grad_norm_'s formula, in fp32
    ctl2 = torch.tensor([0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]).to(DEV)
    K.check(K.lib.lavt_grad_norm(K.ptr(desc_d), K.ptr(chunks_d), n, K.ptr(ws), K.ptr(ctl2), 3.0, 0, K.stream()))
    want = float(torch.clamp(torch.tensor(3.0) / (ctl[0] + 1e-6), max=1.0))
    assert abs(float(ctl2[1]) - want) <= 2e-7 * want and float(ctl2[2]) == 0.0


# ------------------------------------------------------------------------------------------------ 2. clipped update vs torch
def test_clipped_update_matches_torch():
    """6 steps with max_grad_norm between the smallest and the largest gradient norm of the sequence (some steps clip, some do not) vs
    torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW + LambdaLR on the CPU.  Gate: 2e-6 * max(1, |p|max) -- the coefficient's ~1e-6 relative
    rounding perturbs an update of size ~lr by ~lr * 1e-6, far below it."""
    from lavt_hip.optim import FusedAdamW
    params, grads = _problem()
    T, max_norm = 10, 100.0
    ref_p = [torch.nn.Parameter(p.clone()) for p in params]
    ref = torch.optim.AdamW(_groups(ref_p), lr=1e-2, weight_decay=0.05)
    sched = torch.optim.lr_scheduler.LambdaLR(ref, lambda x: (1 - x / T) ** 0.9)
    our_p = [torch.nn.Parameter(p.clone().to(DEV)) for p in params]
    ours = FusedAdamW(_groups(our_p), lr=1e-2, weight_decay=0.05, total_steps=T, power=0.9, max_grad_norm=max_norm)
    coefs = []
    for k in range(6):
        for p, q, gr in zip(ref_p, our_p, grads[k]):
            p.grad = gr.clone()
            q.grad = gr.clone().to(DEV)
        total = math.sqrt(sum(float((gr.double() ** 2).sum()) for gr in grads[k]))          # fp64 norm of the unclipped gradients
        torch.nn.utils.clip_grad_norm_(ref_p, max_norm)
        ref.step()
        sched.step()
        ours.step()
        coefs.append(float(ours.guard[1]))
        assert abs(ours.last_grad_norm() - float(total)) <= 2e-6 * float(total)
        for p, q in zip(ref_p, our_p):
            err, gate = _gate(q, p)
            assert err <= gate, (k, err, gate)
    print("\n[clip coefficients]", coefs)
    assert any(c == 1.0 for c in coefs) and any(c < 1.0 for c in coefs), coefs
    assert ours.steps_taken() == 6 and ours.skipped_steps() == 0


# ------------------------------------------------------------------------------------------------ 3. bitwise identity
def test_guarded_entry_equals_unguarded_bitwise():
    """coefficient 1, skip 0, hold 0: lavt_adamw_step_chunks_guarded vs lavt_adamw_step_chunks on cloned state (one shared update body)"""
    from lavt_hip import ops
    from lavt_hip.optim import FusedAdamW
    params, grads = _problem(3)
    g = torch.Generator().manual_seed(3)
    params.append(torch.randn(20000, 64, generator=g) * 0.3)          # whole chunks + a partial one, with a bf16 copy
    for gr in grads:
        gr.append(torch.randn(20000, 64, generator=g))
    sides = []
    for guarded in (False, True):
        ps = [torch.nn.Parameter(p.clone().to(DEV)) for p in params]
        for p in (ps[0], ps[3], ps[5]):
            ops.weights.get(p, torch.bfloat16, "lin")
        opt = FusedAdamW(ps + [], lr=1e-2, weight_decay=0.05, total_steps=10)
        if guarded:
            opt.hold(False)                                            # creates the control block: step() goes through the guarded entry, no norm launch
            assert opt.guard is not None and opt.guard.tolist() == [0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
        else:
            assert opt.guard is None
        for k in range(3):
            for q, gr in zip(ps, grads[k]):
                q.grad = gr.clone().to(DEV)
            opt.step()
        assert len(opt._tables[6]) == 3
        sides.append(_state(opt, ps))
    assert len(sides[0]) == 6 * 3 + 3 + 1
    assert _same(sides[0], sides[1])


# ------------------------------------------------------------------------------------------------ 4. non-finite skip
@pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_nonfinite_step_is_skipped(bad):
    from lavt_hip import ops
    from lavt_hip.optim import FusedAdamW
    params, grads = _problem(3)
    T = 10
    ref_p = [torch.nn.Parameter(p.clone()) for p in params]
    ref = torch.optim.AdamW(_groups(ref_p), lr=1e-2, weight_decay=0.05)
    sched = torch.optim.lr_scheduler.LambdaLR(ref, lambda x: (1 - x / T) ** 0.9)
    our_p = [torch.nn.Parameter(p.clone().to(DEV)) for p in params]
    copies = [ops.weights.get(our_p[i], torch.bfloat16, "lin") for i in (0, 3)]
    ours = FusedAdamW(_groups(our_p), lr=1e-2, weight_decay=0.05, total_steps=T, power=0.9, skip_nonfinite=True)

    def set_grads(k, poison=None):
        for i, (q, gr) in enumerate(zip(our_p, grads[k])):
            gr = gr.clone()
            if poison is not None and i == 3:
                gr.view(-1)[12345] = poison
            q.grad = gr.to(DEV)
    set_grads(0)
    ours.step()
    before = _state(ours, our_p)
    set_grads(1, poison=bad)
    ours.step()
    assert _same(_state(ours, our_p), before)
    assert ours.steps_taken() == 1 and ours.skipped_steps() == 1 and float(ours.guard[2]) == 1.0
    assert not math.isfinite(ours.last_grad_norm())
    assert all(torch.equal(ops.weights.get(our_p[i], torch.bfloat16, "lin"), c) and torch.equal(c, our_p[i].detach().to(torch.bfloat16)) for i, c in zip((0, 3), copies))
    assert ours.state_dict()["lavt_schedule"]["skipped_steps"] == 1
    set_grads(2)
    ours.step()
    assert ours.steps_taken() == 2 and ours.skipped_steps() == 1 and float(ours.guard[2]) == 0.0
    for k in (0, 2):                                   # the torch run simply omits the bad step
        for p, gr in zip(ref_p, grads[k]):
            p.grad = gr.clone()
        ref.step()
        sched.step()
    for p, q in zip(ref_p, our_p):
        err, gate = _gate(q, p)
        assert err <= gate, (err, gate)
    # without skip_nonfinite the same input is NOT skipped (the parent's behaviour: the bad value goes into the update)
    plain_p = [torch.nn.Parameter(p.clone().to(DEV)) for p in params]
    plain = FusedAdamW(_groups(plain_p), lr=1e-2, weight_decay=0.05, total_steps=T, power=0.9, max_grad_norm=1e9, skip_nonfinite=False)
    for k, poison in ((0, None), (1, bad)):
        for i, (q, gr) in enumerate(zip(plain_p, grads[k])):
            gr = gr.clone()
            if poison is not None and i == 3:
                gr.view(-1)[12345] = poison
            q.grad = gr.to(DEV)
        snap = [q.detach().clone() for q in plain_p]
        plain.step()
    assert plain.steps_taken() == 2 and plain.skipped_steps() == 0 and plain.guard[1:3].tolist() == [1.0, 0.0]
    assert not torch.equal(plain_p[0].detach(), snap[0])


# ------------------------------------------------------------------------------------------------ 5. hold
def test_hold_freezes_the_update_and_is_not_a_skip():
    from lavt_hip import ops
    from lavt_hip.optim import FusedAdamW
    params, grads = _problem(3)
    for skip in (False, True):
        ps = [torch.nn.Parameter(p.clone().to(DEV)) for p in params]
        ops.weights.get(ps[3], torch.bfloat16, "lin")
        opt = FusedAdamW(_groups(ps), lr=1e-2, weight_decay=0.05, total_steps=10, skip_nonfinite=skip)
        twin_p = [torch.nn.Parameter(p.clone().to(DEV)) for p in params]
        ops.weights.get(twin_p[3], torch.bfloat16, "lin")
        twin = FusedAdamW(_groups(twin_p), lr=1e-2, weight_decay=0.05, total_steps=10, skip_nonfinite=skip)

        def set_grads(qs, k, poison=None):
            for i, (q, gr) in enumerate(zip(qs, grads[k])):
                gr = gr.clone()
                if poison is not None and i == 0:
                    gr.view(-1)[5] = poison
                q.grad = gr.to(DEV)
        set_grads(ps, 0), set_grads(twin_p, 0)
        opt.step(), twin.step()
        before = _state(opt, ps)
        opt.hold(True)
        set_grads(ps, 1)
        opt.step()
        set_grads(ps, 1, poison=float("nan"))          # held: not even a non-finite gradient is counted
        opt.step()
        assert _same(_state(opt, ps), before) and opt.steps_taken() == 1 and opt.skipped_steps() == 0
        opt.hold(False)
        set_grads(ps, 2), set_grads(twin_p, 2)
        opt.step(), twin.step()
        assert opt.steps_taken() == 2 and opt.skipped_steps() == 0
        assert _same(_state(opt, ps), _state(twin, twin_p))          # resumed exactly where a never-held twin is


# ------------------------------------------------------------------------------------------------ 6. the guard inside a hipGraph
def test_guard_in_hip_graph_follows_the_eager_sequence():
    """step(check_tables=False) with clip + skip captured into a graph; replays with finite, non-finite, finite gradients written into the same buffers"""
    from lavt_hip.optim import FusedAdamW
    params, grads = _problem(4)
    seq = [(1, None), (2, float("inf")), (3, None)]
    sides = []
    for captured in (False, True):
        ps = [torch.nn.Parameter(p.clone().to(DEV)) for p in params]
        for q, gr in zip(ps, grads[0]):
            q.grad = gr.clone().to(DEV)
        opt = FusedAdamW(_groups(ps), lr=1e-2, weight_decay=0.05, total_steps=10, max_grad_norm=300.0, skip_nonfinite=True)
        opt.step()                                       # builds the tables outside the capture
        torch.cuda.synchronize()
        graph = None
        if captured:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                opt.step(check_tables=False)
        norms = []
        for k, poison in seq:
            for i, (q, gr) in enumerate(zip(ps, grads[k])):
                gr = gr.clone()
                if poison is not None and i == 2:
                    gr.view(-1)[7] = poison
                q.grad.copy_(gr.to(DEV))
            if captured:
                graph.replay()
            else:
                opt.step()
            norms.append(opt.last_grad_norm())
        assert opt.steps_taken() == 3 and opt.skipped_steps() == 1
        sides.append((_state(opt, ps), norms, opt.guard.clone()))
    assert _same(sides[0][0], sides[1][0])
    assert sides[0][1][0] == sides[1][1][0] and sides[0][1][2] == sides[1][1][2] and math.isinf(sides[1][1][1])
    assert torch.equal(sides[0][2], sides[1][2])


# ------------------------------------------------------------------------------------------------ 7-9. the harness
def _micro():
    from test_gpu_modules import _build          # the micro model of test_captured_step_with_fused_adamw_overfits_one_batch
    return _build(32, [2, 2, 2, 2], [1, 2, 4, 8], 7, dpr=0.0).train()


def _batch(seed=17):
    x, l, m, t = det_inputs(2, 64, 20, seed=seed)
    return x.to(DEV), l.to(DEV), m.to(DEV), t.to(DEV)


def test_harness_owns_its_optimizer():
    """make_optimizer + warmup_and_capture: captured; parameters, moments, counters bitwise as before the warm-up (the optimizer is on hold for the eager
    iterations and the NaN-poisoned validation replays); afterwards K calls of step() alone are K optimizer steps."""
    import lavt_hip
    from lavt_hip import ops
    from lavt_hip.engine import TrainStep
    x, l, m, t = _batch()
    ctx = ops.StepContext()
    with lavt_hip.use_dtype(torch.bfloat16):
        model = _micro()
        step = TrainStep(model, x, l, m, t, world=1, use_graph=True, context=ctx)
        opt = step.make_optimizer([p for p in model.parameters()], lr=3e-4, weight_decay=1e-2, max_grad_norm=1.0, skip_nonfinite=True)
        assert step.opt is opt and opt.context is ctx
        ps = [p for p in model.parameters()]
        before = [p.detach().clone() for p in ps]
        step.warmup_and_capture()
        torch.cuda.synchronize()
        assert step.captured
        assert all(torch.equal(p.detach().view(torch.int32), b.view(torch.int32)) for p, b in zip(ps, before))
        assert opt.steps_taken() == 0 and opt.skipped_steps() == 0 and float(opt.guard[4]) == 0.0
        moments = [opt.state[p][k] for p in ps for k in ("exp_avg", "exp_avg_sq") if k in opt.state[p]]
        assert len(moments) == 2 * len(ps) and all(not bool(mo.any()) for mo in moments)          # created by the warm-up, still all zero
        with ops.use_context(ctx):
            lin = [(k, e) for k, e in ops.weights.store.items() if k[1] == torch.bfloat16 and k[2] == "lin" and e[2]() is not None]
            assert lin and all(torch.equal(e[1].view(-1), e[2]().detach().to(torch.bfloat16).view(-1)) for _, e in lin)
        K_ = 5
        losses = [float(step.step()) for _ in range(K_)]
        torch.cuda.synchronize()
        assert all(np.isfinite(losses)), losses
        assert opt.steps_taken() == K_ and opt.skipped_steps() == 0
        assert any(not torch.equal(p.detach(), b) for p, b in zip(ps, before))
        assert 0.0 < opt.last_grad_norm() < float("inf")
        with ops.use_context(ctx):                       # the replays keep the compute copies current: the weights the next forward reads
            assert all(torch.equal(e[1].view(-1), e[2]().detach().to(torch.bfloat16).view(-1)) for _, e in lin)


def _run_route(owned, steps, lr):
    """one training run on the fixed batch in a private context -> per-iteration losses"""
    import lavt_hip
    from lavt_hip import ops
    from lavt_hip.engine import TrainStep
    from lavt_hip.optim import FusedAdamW
    x, l, m, t = _batch()
    ctx = ops.StepContext()
    with lavt_hip.use_dtype(torch.bfloat16):
        model = _micro()
        step = TrainStep(model, x, l, m, t, world=1, use_graph=True, context=ctx)
        if owned:
            opt = step.make_optimizer([p for p in model.parameters()], lr=lr, weight_decay=1e-2)
        step.warmup_and_capture()
        assert step.captured
        if not owned:
            opt = FusedAdamW([p for p in model.parameters()], lr=lr, weight_decay=1e-2, context=ctx)
        losses = []
        for _ in range(steps):
            losses.append(float(step.step()))
            if not owned:
                opt.step()
        torch.cuda.synchronize()
        assert opt.steps_taken() == steps
    return losses


def test_owned_optimizer_trains_like_the_parent_route():
    """40 iterations on one fixed batch, DropPath 0: the owned optimizer (one replay per iteration) vs the parent route (captured step, then opt.step()
    from Python).  Backward uses float atomics, so the curves are not bitwise equal: the parent route runs twice, its own run-to-run spread of the
    per-iteration loss is the unit (floor 1e-6 where the two runs coincide), and the owned route must stay within 4 x that spread of the parent's mean
    curve at every iteration.  The measured figures go to profiles/train_iter_parity.json.  Also the existing overfit criterion: final < 0.6 x first."""
    steps, lr = 40, 3e-4
    p1, p2 = _run_route(False, steps, lr), _run_route(False, steps, lr)
    own = _run_route(True, steps, lr)
    spread = [max(abs(a - b), 1e-6) for a, b in zip(p1, p2)]
    dev = [abs(o - 0.5 * (a + b)) for o, a, b in zip(own, p1, p2)]
    ratio = [d / s for d, s in zip(dev, spread)]
    worst = int(np.argmax(ratio))
    report = {"steps": steps, "parent_run1": p1, "parent_run2": p2, "owned": own, "parent_spread_max": max(abs(a - b) for a, b in zip(p1, p2)),
              "owned_deviation_max": max(dev), "worst_ratio": ratio[worst], "worst_iteration": worst, "allowance": 4.0, "floor": 1e-6}
    print("\n[train iteration parity]", {k: v for k, v in report.items() if not isinstance(v, list)})
    try:
        with open(os.path.join(ROOT, "profiles", "train_iter_parity.json"), "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")
    except OSError:
        pass
    assert all(np.isfinite(own)), own
    assert all(d <= 4.0 * s for d, s in zip(dev, spread)), (worst, dev[worst], spread[worst])
    assert own[-1] < 0.6 * own[0], f"the owned-optimizer replay did not overfit the batch: {own[0]:.4f} -> {own[-1]:.4f}"


def test_wiring_errors_and_the_unowned_step_is_unchanged():
    import lavt_hip
    from lavt_hip import ops, _capi as K
    from lavt_hip.engine import TrainStep
    from lavt_hip.optim import FusedAdamW
    x, l, m, t = _batch()
    with lavt_hip.use_dtype(torch.bfloat16):
        model = _micro()
        ctx = ops.StepContext()
        step = TrainStep(model, x, l, m, t, world=1, use_graph=True, context=ctx)
        foreign = FusedAdamW([p for p in model.parameters()], lr=1e-4)                       # the default context: not the step's
        with pytest.raises(ValueError, match="never refreshed"):
            step.attach_optimizer(foreign)
        assert step.opt is None
        step.warmup_and_capture(eager_iters=2)
        assert step.captured
        with pytest.raises(RuntimeError, match="before warmup_and_capture"):
            step.make_optimizer(lr=1e-4)
        with pytest.raises(RuntimeError, match="before warmup_and_capture"):
            step.attach_optimizer(FusedAdamW([p for p in model.parameters()], lr=1e-4, context=ctx))
        # a step without an owned optimizer issues no optimizer launch, and the same number of launches every time
        plain = TrainStep(_micro(), x, l, m, t, world=1, use_graph=False, context=ops.StepContext())
        plain.warmup_and_capture(eager_iters=2)
        counts = []
        for _ in range(2):
            K.prof.start()
            plain.step()
            recs = K.prof.stop()
            assert not [r[0] for r in recs if "adamw" in r[0] or "grad_norm" in r[0]]
            counts.append(len(recs))
        assert counts[0] == counts[1] and counts[0] > 0
        owned = TrainStep(_micro(), x, l, m, t, world=1, use_graph=False, context=ops.StepContext())
        owned.make_optimizer(lr=1e-4, max_grad_norm=1.0)                                     # default groups: the reference's (backbone + classifier)
        assert len(owned.opt.param_groups) == 3
        owned.warmup_and_capture(eager_iters=2)
        K.prof.start()
        owned.step()
        names = [r[0] for r in K.prof.stop()]
        assert names.count("lavt_grad_norm") == 1 and names.count("lavt_adamw_step_chunks_guarded") == 1 and "lavt_adamw_step_chunks" not in names
        tail = names[names.index("lavt_grad_norm") + 1:]                                      # the update ends the body: only the refresh of the copies follows
        assert tail[0] == "lavt_adamw_step_chunks_guarded" and all(n in ("lavt_cast_multi", "lavt_cast", "lavt_pack_conv3x3", "lavt_ln_fold_multi") for n in tail[1:]), tail
        assert owned.opt.steps_taken() == 1
