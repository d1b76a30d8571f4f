"""AMSGrad on the fused AdamW (FusedAdamW(amsgrad=True), lavt_adamw_step_chunks_amsgrad) against torch.optim.AdamW(amsgrad=True) on the CPU: the update
rule, checkpoints in both directions, the guarded entry (bitwise equal to the unguarded one; skip and hold leave max_exp_avg_sq alone), the captured
step, and the step harness owning such an optimizer.

The gradients SHRINK (scales 1, 0.05, 0.05, 1, 0.02, 0.02) and beta2 is 0.95, so that the running maximum binds: with growing gradients and beta2 = 0.999
AMSGrad equals plain AdamW to within the gate and a kernel that ignored max_exp_avg_sq would pass.  Test 1 asserts that on the reference alone.

The non-finite inputs used here are ordinary floating-point values (Inf / NaN) in gradient buffers."""
import copy
import functools

import numpy as np
import pytest
import torch

from lavt_hip.detweights import det_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# flat state offsets (elements): 0, 561, 689, 824, 64824, 64831, 73023, 73024
#   (1000,64): 7 whole aligned chunks + a 6656 tail      (8192,): one whole chunk whose state is NOT 16-byte aligned (the element-wise path on a full chunk)
#   (12291,): an aligned whole chunk + a 4099 tail
SHAPES = [(33, 17), (128,), (5, 3, 3, 3), (1000, 64), (7,), (8192,), (1,), (12291,)]
SCALES = [1.0, 0.05, 0.05, 1.0, 0.02, 0.02]
COPIES = (0, 3)                                           # tensors with a bf16 'lin' compute copy
KW = dict(lr=1e-2, weight_decay=0.05, betas=(0.9, 0.95))
T, POWER = 10, 0.9


@pytest.fixture(autouse=True)
def _fp32():
    import lavt_hip
    lavt_hip.set_compute_dtype(torch.float32)
    yield
    lavt_hip.set_compute_dtype(torch.float32)


def _groups(ps):
    return [{"params": ps[:2], "weight_decay": 0.0}, {"params": ps[2:4]}, {"params": ps[4:], "lr": 3e-3}]


def _gate(q, p):
    """the project's own gate (test_fused_adamw_matches_torch)"""
    err = float((q.detach().cpu() - p.detach()).abs().max())
    return err, 2e-6 * max(1.0, float(p.abs().max()))


def _torch_run(params, grads, amsgrad, keep_at=None):
    ps = [torch.nn.Parameter(p.clone()) for p in params]
    opt = torch.optim.AdamW(_groups(ps), amsgrad=amsgrad, **KW)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda x: (1 - x / T) ** POWER)
    after, kept = [], None
    for k, gs in enumerate(grads):
        for p, gr in zip(ps, gs):
            p.grad = gr.clone()
        opt.step()
        sched.step()
        after.append([p.detach().clone() for p in ps])
        if keep_at == k + 1:
            kept = copy.deepcopy(opt.state_dict())
    return ps, opt, after, kept


@functools.lru_cache(maxsize=None)
def _reference():
    """computed once, read-only: the data, six torch AMSGrad steps (parameters after every step, the final moments, torch's state_dict after step 3) and
    the parameters of six plain torch AdamW steps"""
    g = torch.Generator().manual_seed(23)
    params = [torch.randn(*s, generator=g) for s in SHAPES]
    grads = [[torch.randn(*s, generator=g) * sc for s in SHAPES] for sc in SCALES]
    ps, opt, after, sd3 = _torch_run(params, grads, True, keep_at=3)
    v = [opt.state[p]["exp_avg_sq"].clone() for p in ps]
    x = [opt.state[p]["max_exp_avg_sq"].clone() for p in ps]
    plain = _torch_run(params, grads, False)[2][-1]
    return dict(params=params, grads=grads, after=after, v=v, x=x, sd3=sd3, plain=plain)


def _ours(params, guard=None, copies=True, **kw):
    """GPU clones of `params` (created in order), the bf16 copies, one FusedAdamW(amsgrad=True) over all of them"""
    from lavt_hip import ops
    from lavt_hip.optim import FusedAdamW
    ps = [torch.nn.Parameter(p.clone().to(DEV)) for p in params]
    if copies:
        for i in COPIES:
            ops.weights.get(ps[i], torch.bfloat16, "lin")
    opt = FusedAdamW(_groups(ps), amsgrad=True, total_steps=T, power=POWER, **KW, **kw)
    if guard == "hold":
        opt.hold(False)                                   # creates the control block: the guarded entry, no norm launch
    return ps, opt


def _set_grads(ps, gs, poison=None, at=(3, 12345)):
    for i, (q, gr) in enumerate(zip(ps, gs)):
        gr = gr.clone()
        if poison is not None and i == at[0]:
            gr.view(-1)[at[1]] = poison
        q.grad = gr.to(DEV)


def _state(opt, ps):
    """bitwise snapshot of everything an update may write: parameters, the three moments, the bf16 compute copies, step counter"""
    from lavt_hip import ops
    torch.cuda.synchronize()
    out = [p.detach().clone() for p in ps]
    for key in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
        out += [opt.state[p][key].clone() for p in ps]
    with ops.use_context(opt.context):
        out += [ops.weights.store[(id(p), torch.bfloat16, "lin")][1].clone() for p in ps if (id(p), torch.bfloat16, "lin") in ops.weights.store]
    out.append(opt._step.clone())
    return out


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


N_STATE = 4 * len(SHAPES) + len(COPIES) + 1


# ------------------------------------------------------------------------------------------------ 1. against torch
def test_amsgrad_matches_torch():
    """Six steps vs torch.optim.AdamW(amsgrad=True) + LambdaLR on the CPU.  Parameters: the project's gate, 2e-6 * max(1, |p|max), after every step.
    exp_avg_sq and max_exp_avg_sq per element after step 6: |a - b| <= 4e-6 * b -- both are sums of non-negative terms, at most 4 roundings per step
    per side, 6 steps: 2 * 24 * 2^-24 ~ 2.9e-6.  Then the checkpoint round trip: a fresh optimizer that loaded state_dict() stays bit-identical."""
    from lavt_hip import ops
    from lavt_hip.optim import FusedAdamW
    R = _reference()
    # the reference alone: the maximum binds, and AMSGrad is not plain AdamW on this data
    share = sum(int((x > v).sum()) for x, v in zip(R["x"], R["v"])) / sum(v.numel() for v in R["v"])
    print(f"\n[amsgrad] share of max_exp_avg_sq > exp_avg_sq after step 6: {share:.4f}")
    assert share >= 0.9, share
    for i, (a, b) in enumerate(zip(R["after"][-1], R["plain"])):
        diff, gate = float((a - b).abs().max()), 2e-6 * max(1.0, float(a.abs().max()))
        print(f"[amsgrad] tensor {i}: torch plain vs amsgrad differ by {diff / gate:.0f} x the gate")
        assert diff >= 10 * gate, (i, diff, gate)

    ps, opt = _ours(R["params"])
    worst = 0.0
    for k in range(6):
        _set_grads(ps, R["grads"][k])
        opt.step()
        for q, p in zip(ps, R["after"][k]):
            err, gate = _gate(q, p)
            worst = max(worst, err / gate)
            assert err <= gate, (k, tuple(p.shape), err, gate)
    print(f"[amsgrad] worst parameter error / gate over six steps: {worst:.3f}")
    assert opt.steps_taken() == 6
    st = [opt.state[q] for q in ps]
    assert st[5]["max_exp_avg_sq"].data_ptr() % 16 != 0                                    # (8192,): the unaligned whole chunk
    assert st[3]["max_exp_avg_sq"].data_ptr() % 16 == 0 and st[7]["max_exp_avg_sq"].data_ptr() % 16 == 0
    for key, ref in (("exp_avg_sq", R["v"]), ("max_exp_avg_sq", R["x"])):
        rel = max(float(((s[key].cpu() - b).abs() / b).max()) for s, b in zip(st, ref))
        print(f"[amsgrad] {key}: worst per-element relative error {rel:.3e} (gate 4e-6)")
        assert all(bool(((s[key].cpu() - b).abs() <= 4e-6 * b).all()) for s, b in zip(st, ref)), (key, rel)
    for i in COPIES:
        assert torch.equal(_bits(ops.weights.get(ps[i], torch.bfloat16, "lin")), _bits(ps[i].detach().to(torch.bfloat16)))

    sd = copy.deepcopy(opt.state_dict())                  # (what a checkpoint file holds: torch's own state_dict() hands out the live tensors)
    assert len(sd["state"]) == len(ps) and all("max_exp_avg_sq" in sd["state"][i] for i in range(len(ps)))
    assert all(g["amsgrad"] is True for g in sd["param_groups"])
    qs, fresh = _ours([q.detach().cpu() for q in ps])
    fresh.load_state_dict(sd)
    assert fresh.steps_taken() == 6
    assert fresh.state[qs[3]]["max_exp_avg_sq"].data_ptr() != st[3]["max_exp_avg_sq"].data_ptr()
    assert _same(_state(opt, ps), _state(fresh, qs))
    for side, o in ((ps, opt), (qs, fresh)):
        _set_grads(side, R["grads"][5])
        o.step()
    a, b = _state(opt, ps), _state(fresh, qs)
    assert len(a) == N_STATE and float(a[-1]) == 7.0
    assert _same(a, b)
    # an AMSGrad optimizer whose state was written without the maximum does not start it at zero
    bad_p, bad = _ours(R["params"], copies=False)
    _set_grads(bad_p, R["grads"][0])
    for q in bad_p:
        bad.state[q]["exp_avg"], bad.state[q]["exp_avg_sq"] = torch.zeros_like(q), torch.zeros_like(q)
    with pytest.raises(ValueError, match="max_exp_avg_sq"):
        bad.step()


# ------------------------------------------------------------------------------------------------ 2. resume from torch
def test_resume_from_a_torch_amsgrad_checkpoint():
    """three torch steps, torch's state_dict() loaded into FusedAdamW(amsgrad=True) on GPU clones of torch's parameters, three more steps on both sides"""
    R = _reference()
    ps, opt = _ours(R["after"][2])
    opt.load_state_dict(copy.deepcopy(R["sd3"]))
    assert opt.steps_taken() == 3
    for q, x in zip(ps, [R["sd3"]["state"][i]["max_exp_avg_sq"] for i in range(len(ps))]):
        assert torch.equal(opt.state[q]["max_exp_avg_sq"].cpu(), x)
    for k in range(3, 6):
        _set_grads(ps, R["grads"][k])
        opt.step()
        for q, p in zip(ps, R["after"][k]):
            err, gate = _gate(q, p)
            assert err <= gate, (k, tuple(p.shape), err, gate)
    assert opt.steps_taken() == 6


# ------------------------------------------------------------------------------------------------ 3. guarded = unguarded
def test_guarded_amsgrad_equals_unguarded_bitwise():
    """coefficient 1, skip 0, hold 0: lavt_adamw_step_chunks_amsgrad with a control block vs with NULL, on cloned state (one shared update body)"""
    from lavt_hip import _capi as K
    R = _reference()
    sides = []
    for guard in (None, "hold"):
        ps, opt = _ours(R["params"], guard=guard)
        assert (opt.guard is None) == (guard is None)
        K.prof.start()
        for k in range(3):
            _set_grads(ps, R["grads"][k])
            opt.step()
        names = [r[0] for r in K.prof.stop()]
        assert names.count("lavt_adamw_step_chunks_amsgrad") == 3 and not [n for n in names if n in ("lavt_adamw_step_chunks", "lavt_adamw_step_chunks_guarded", "lavt_grad_norm")]
        assert len(opt._tables[6]) == len(COPIES)
        sides.append(_state(opt, ps))
    assert len(sides[0]) == N_STATE
    assert any(bool((x > v).any()) for x, v in zip(sides[0][3 * len(SHAPES):4 * len(SHAPES)], sides[0][2 * len(SHAPES):3 * len(SHAPES)]))      # the maximum did bind
    assert _same(sides[0], sides[1])


# ------------------------------------------------------------------------------------------------ 4. skip and hold
@pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_nonfinite_amsgrad_step_is_skipped(bad):
    R = _reference()
    ps, opt = _ours(R["params"], skip_nonfinite=True)
    twin_p, twin = _ours(R["params"], skip_nonfinite=True)
    _set_grads(ps, R["grads"][0])
    opt.step()
    before = _state(opt, ps)
    assert len(before) == N_STATE and any(bool(x.any()) for x in before[3 * len(SHAPES):4 * len(SHAPES)])
    _set_grads(ps, R["grads"][1], poison=bad)
    opt.step()
    assert _same(_state(opt, ps), before)
    assert opt.steps_taken() == 1 and opt.skipped_steps() == 1 and float(opt.guard[2]) == 1.0
    assert not np.isfinite(opt.last_grad_norm())
    _set_grads(ps, R["grads"][2])
    opt.step()
    assert opt.steps_taken() == 2 and opt.skipped_steps() == 1 and float(opt.guard[2]) == 0.0
    for k in (0, 2):                                      # the twin never saw the bad step
        _set_grads(twin_p, R["grads"][k])
        twin.step()
    assert _same(_state(opt, ps), _state(twin, twin_p))
    for q, p in zip(ps, _torch_run(R["params"], [R["grads"][0], R["grads"][2]], True)[2][-1]):
        err, gate = _gate(q, p)
        assert err <= gate, (err, gate)


def test_hold_freezes_the_amsgrad_update_and_is_not_a_skip():
    R = _reference()
    for skip in (False, True):
        ps, opt = _ours(R["params"], skip_nonfinite=skip)
        twin_p, twin = _ours(R["params"], skip_nonfinite=skip)
        _set_grads(ps, R["grads"][0]), _set_grads(twin_p, R["grads"][0])
        opt.step(), twin.step()
        before = _state(opt, ps)
        opt.hold(True)
        _set_grads(ps, R["grads"][1])
        opt.step()
        _set_grads(ps, R["grads"][1], poison=float("nan"), at=(0, 5))          # held: not even a non-finite gradient is counted
        opt.step()
        assert _same(_state(opt, ps), before) and opt.steps_taken() == 1 and opt.skipped_steps() == 0
        opt.hold(False)
        _set_grads(ps, R["grads"][2]), _set_grads(twin_p, R["grads"][2])
        opt.step(), twin.step()
        assert opt.steps_taken() == 2 and opt.skipped_steps() == 0
        assert _same(_state(opt, ps), _state(twin, twin_p))          # resumed exactly where a never-held twin is


# ------------------------------------------------------------------------------------------------ 5. captured
def test_amsgrad_in_hip_graph():
    """1 eager step + 3 replays of step(check_tables=False) vs 4 eager steps, the shrinking gradients written into the same buffers before every step.
    Gate: test_fused_adamw_in_hip_graph's, 1e-7 * max(1, |p|max)."""
    R = _reference()
    eager_p, eager = _ours(R["params"])
    graph_p, captured = _ours(R["params"])
    for ps in (eager_p, graph_p):
        _set_grads(ps, R["grads"][0])
    eager.step()
    captured.step()                                       # builds the tables outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured.step(check_tables=False)
    for k in range(1, 4):                                 # capture itself executes nothing
        for ps in (eager_p, graph_p):
            for q, gr in zip(ps, R["grads"][k]):
                q.grad.copy_(gr.to(DEV))
        eager.step()
        g.replay()
    torch.cuda.synchronize()
    assert captured.steps_taken() == 4 and eager.steps_taken() == 4
    for p, q in zip(eager_p, graph_p):
        assert float((p.detach() - q.detach()).abs().max()) <= 1e-7 * max(1.0, float(p.detach().abs().max()))
    for q, p in zip(graph_p, R["after"][3]):
        err, gate = _gate(q, p)
        assert err <= gate, (err, gate)
    assert any(bool((captured.state[q]["max_exp_avg_sq"] > captured.state[q]["exp_avg_sq"]).any()) for q in graph_p)


# ------------------------------------------------------------------------------------------------ 6. the harness
def test_harness_owns_an_amsgrad_optimizer():
    """make_optimizer(amsgrad=True) + warmup_and_capture: captured; parameters bitwise unchanged, all three moment sets created and still zero (the
    optimizer is on hold for the eager iterations and the validation replays); then five replays are five AMSGrad iterations."""
    import lavt_hip
    from lavt_hip import ops
    from lavt_hip.engine import TrainStep
    from test_gpu_modules import _build          # the micro model of test_harness_owns_its_optimizer
    x, l, m, t = [v.to(DEV) for v in det_inputs(2, 64, 20, seed=17)]
    ctx = ops.StepContext()
    with lavt_hip.use_dtype(torch.bfloat16):
        model = _build(32, [2, 2, 2, 2], [1, 2, 4, 8], 7, dpr=0.0).train()
        step = TrainStep(model, x, l, m, t, world=1, use_graph=True, context=ctx)
        ps = [p for p in model.parameters()]
        opt = step.make_optimizer(ps, lr=3e-4, weight_decay=1e-2, amsgrad=True, max_grad_norm=1.0, skip_nonfinite=True)
        assert step.opt is opt and opt.amsgrad and all(g["amsgrad"] is True for g in opt.param_groups)
        before = [p.detach().clone() for p in ps]
        step.warmup_and_capture()
        torch.cuda.synchronize()
        assert step.captured
        assert all(torch.equal(_bits(p.detach()), _bits(b)) for p, b in zip(ps, before))
        assert opt.steps_taken() == 0 and opt.skipped_steps() == 0 and float(opt.guard[4]) == 0.0
        moments = [opt.state[p][k] for p in ps for k in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq") if k in opt.state[p]]
        assert len(moments) == 3 * len(ps) and all(not bool(mo.any()) for mo in moments)          # created by the warm-up, still all zero
        losses = [float(step.step()) for _ in range(5)]
        torch.cuda.synchronize()
        assert all(np.isfinite(losses)), losses
        assert opt.steps_taken() == 5 and opt.skipped_steps() == 0
        assert all(bool((opt.state[p]["max_exp_avg_sq"] >= opt.state[p]["exp_avg_sq"]).all()) for p in ps)
        assert any(bool(opt.state[p]["max_exp_avg_sq"].any()) for p in ps)
        assert any(not torch.equal(p.detach(), b) for p, b in zip(ps, before))


# ------------------------------------------------------------------------------------------------ 7. the plain path
def test_plain_path_carries_no_maximum():
    from lavt_hip.optim import FusedAdamW
    R = _reference()
    ps = [torch.nn.Parameter(p.clone().to(DEV)) for p in R["params"]]
    opt = FusedAdamW(_groups(ps), total_steps=T, power=POWER, **KW)
    _set_grads(ps, R["grads"][0])
    opt.step()
    assert all("max_exp_avg_sq" not in opt.state[p] and set(opt.state[p]) == {"step", "exp_avg", "exp_avg_sq"} for p in ps)
    assert all("max_exp_avg_sq" not in st for st in opt.state_dict()["state"].values())
    key, desc, hyper, n, chunks, nchunks, fused = opt._tables[:7]
    want_chunks = sum(-(-p.numel() // 8192) for p in ps)
    assert isinstance(key, tuple) and n == len(ps) and nchunks == want_chunks == 16 and fused == {}
    assert desc.shape == (len(ps), 6) and desc.dtype == torch.int64 and hyper.shape == (len(ps), 5) and hyper.dtype == torch.float32
    assert chunks.shape == (want_chunks, 2) and chunks.dtype == torch.int32
    assert opt._tables[7:] == (None, None)
    qs, ams = _ours(R["params"], copies=False)
    _set_grads(qs, R["grads"][0])
    ams.step()
    vmax = ams._tables[7]
    assert vmax.shape == (len(qs),) and vmax.dtype == torch.int64 and vmax.tolist() == [ams.state[q]["max_exp_avg_sq"].data_ptr() for q in qs]
