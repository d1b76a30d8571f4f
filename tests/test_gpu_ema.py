"""Weight EMA in the fused AdamW (FusedAdamW(ema_decay=0.9), lavt_adamw_step_chunks_ema, lavt_ema_swap) and live validation with a Predictor built on the
model that is being trained (DESIGN.md "Weight EMA").

Optimizer tests run on the data of tests/test_gpu_amsgrad.py (its SHAPES: whole aligned chunks, a whole chunk whose state is not 16-byte aligned, tails of
6656 and 4099, one element; two tensors with bf16 compute copies) against the CPU reference of tests/ema_reference.py: torch.optim.AdamW + LambdaLR +
AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(0.9)).  tests/test_ema_host.py shows, on the reference alone, that the average is >= 100 x the gate away
from the iterate: a kernel that ignored the stream cannot pass.

The non-finite inputs used here are ordinary floating-point values (Inf / NaN) in gradient buffers."""
import copy

import numpy as np
import pytest
import torch

from ema_reference import DECAY, EMA_GATE, reference
from test_gpu_amsgrad import COPIES, KW, POWER, SHAPES, T, _bits, _groups, _same, _set_grads

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FORMS = pytest.mark.parametrize("amsgrad", [False, True], ids=["plain", "amsgrad"])


def _ours(params, amsgrad=False, guard=None, ema_decay=DECAY, **kw):
    """GPU clones of `params` (created in order), the bf16 copies of COPIES, one FusedAdamW over all of them"""
    from lavt_hip import ops
    from lavt_hip.optim import FusedAdamW
    ps = [torch.nn.Parameter(p.clone().to(DEV)) for p in params]
    for i in COPIES:
        ops.weights.get(ps[i], torch.bfloat16, "lin")
    opt = FusedAdamW(_groups(ps), amsgrad=amsgrad, total_steps=T, power=POWER, ema_decay=ema_decay, **KW, **kw)
    if guard == "hold":
        opt.hold(False)                                   # creates the control block: the guarded entry, no norm launch
    return ps, opt


def _copies(opt, ps):
    from lavt_hip import ops
    with ops.use_context(opt.context):
        return [ops.weights.store[(id(ps[i]), torch.bfloat16, "lin")][1] for i in COPIES]


def _state(opt, ps):
    """bitwise snapshot of everything an update may write: parameters, the moments, the average, the bf16 compute copies, the step counter"""
    torch.cuda.synchronize()
    out = [p.detach().clone() for p in ps]
    for key in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq", "ema"):
        out += [opt.state[p][key].clone() for p in ps if key in opt.state[p]]
    out += [c.clone() for c in _copies(opt, ps)]
    out.append(opt._step.clone())
    return out


def _ema(opt, ps):
    torch.cuda.synchronize()
    return [opt.state[p]["ema"].clone() for p in ps]


# ------------------------------------------------------------------------------------------------ 1. against torch
@FORMS
def test_ema_matches_torch(amsgrad):
    """Six steps vs torch.optim.AdamW + LambdaLR + AveragedModel(get_ema_multi_avg_fn(0.9)) on the CPU.  After every step |e - ref| <= 3e-6 * max(1, |ref|max)
    (ema_reference.EMA_GATE: the parameter gate the average inherits as a convex combination, + 1e-6 for the spread between fp32 formulations of the
    rule); the parameters meet the project's own 2e-6 gate as without the average.  After step 1 the average IS the parameter, bit for bit."""
    from lavt_hip import _capi as K
    R = reference(amsgrad)
    ps, opt = _ours(R["params"], amsgrad=amsgrad)
    worst = 0.0
    K.prof.start()
    for k in range(6):
        _set_grads(ps, R["grads"][k])
        opt.step()
        torch.cuda.synchronize()
        for q, p, ref in zip(ps, R["after"][k], R["ema"][k]):
            e = opt.state[q]["ema"]
            assert e.shape == q.shape and e.dtype == torch.float32
            perr = float((q.detach().cpu() - p).abs().max())
            assert perr <= 2e-6 * max(1.0, float(p.abs().max())), (k, tuple(p.shape), perr)
            err, gate = float((e.cpu() - ref).abs().max()), EMA_GATE * max(1.0, float(ref.abs().max()))
            worst = max(worst, err / gate)
            assert err <= gate, (k, tuple(p.shape), err, gate)
        if k == 0:
            assert all(torch.equal(_bits(opt.state[q]["ema"]), _bits(q.detach())) for q in ps), "the first applied update copies"
    names = [r[0] for r in K.prof.stop()]
    print(f"\n[ema, amsgrad={amsgrad}] worst |e - ref| / gate over six steps: {worst:.3f}")
    assert names.count("lavt_adamw_step_chunks_ema") == 6
    assert not [n for n in names if n in ("lavt_adamw_step_chunks", "lavt_adamw_step_chunks_guarded", "lavt_adamw_step_chunks_amsgrad")]
    assert opt.steps_taken() == 6 and len(opt._tables) == 9 and opt._tables[8].tolist() == [opt.state[q]["ema"].data_ptr() for q in ps]
    st = [opt.state[q] for q in ps]
    assert st[5]["ema"].data_ptr() % 16 != 0                                    # (8192,): the unaligned whole chunk
    assert st[3]["ema"].data_ptr() % 16 == 0 and st[7]["ema"].data_ptr() % 16 == 0
    assert all(not torch.equal(s["ema"], q.detach()) for s, q in zip(st, ps))
    for i, c in zip(COPIES, _copies(opt, ps)):
        assert torch.equal(_bits(c), _bits(ps[i].detach().to(torch.bfloat16).reshape(c.shape)))

    # the checkpoint round trip: a fresh optimizer that loaded state_dict() stays bit-identical, the average included
    sd = copy.deepcopy(opt.state_dict())
    assert all("ema" in sd["state"][i] for i in range(len(ps))) and all(g["ema_decay"] == DECAY for g in sd["param_groups"])
    qs, fresh = _ours([q.detach().cpu() for q in ps], amsgrad=amsgrad)
    fresh.load_state_dict(sd)
    assert _same(_state(opt, ps), _state(fresh, qs))
    for side, o in ((ps, opt), (qs, fresh)):
        _set_grads(side, R["grads"][5])
        o.step()
    assert _same(_state(opt, ps), _state(fresh, qs)) and fresh.steps_taken() == 7


# ------------------------------------------------------------------------------------------------ 2. against fp64 on the device's own iterates
@FORMS
def test_ema_matches_fp64_on_the_devices_iterates(amsgrad):
    """The parameters after each step are read back and the average is recomputed from them in fp64 on the host: the rule alone, without the optimizer's
    own error.  Gate 1e-6 * max(1, |e|max): five fp32 updates, each one rounding of at most half an ulp of |e| (2^-24 |e|, ~6e-8 |e|), bounded by
    3e-7 |e| in total; the reference's own fp32-to-fp64 spread on this data is at most 1.2e-7."""
    R = reference(amsgrad)
    ps, opt = _ours(R["params"], amsgrad=amsgrad)
    e64, worst = None, 0.0
    for k in range(6):
        _set_grads(ps, R["grads"][k])
        opt.step()
        torch.cuda.synchronize()
        p64 = [q.detach().cpu().double() for q in ps]
        e64 = p64 if e64 is None else [e + (1.0 - DECAY) * (p - e) for e, p in zip(e64, p64)]
        for q, ref in zip(ps, e64):
            err, gate = float((opt.state[q]["ema"].cpu().double() - ref).abs().max()), 1e-6 * max(1.0, float(ref.abs().max()))
            worst = max(worst, err / gate)
            assert err <= gate, (k, tuple(q.shape), err, gate)
    print(f"\n[ema vs fp64, amsgrad={amsgrad}] worst |e - e64| / gate over six steps: {worst:.3f}")


# ------------------------------------------------------------------------------------------------ 3. the control block
@FORMS
def test_guarded_ema_equals_unguarded_bitwise(amsgrad):
    """coefficient 1, skip 0, hold 0: lavt_adamw_step_chunks_ema with a control block vs with NULL (one shared update body)"""
    R = reference(amsgrad)
    sides = []
    for guard in (None, "hold"):
        ps, opt = _ours(R["params"], amsgrad=amsgrad, guard=guard)
        assert (opt.guard is None) == (guard is None)
        for k in range(3):
            _set_grads(ps, R["grads"][k])
            opt.step()
        sides.append(_state(opt, ps))
    assert len(sides[0]) == (5 if amsgrad else 4) * len(SHAPES) + len(COPIES) + 1
    assert _same(sides[0], sides[1])


@pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_nonfinite_step_leaves_the_average_alone(bad):
    R = reference(False)
    ps, opt = _ours(R["params"], skip_nonfinite=True)
    twin_p, twin = _ours(R["params"], skip_nonfinite=True)
    for k in (0, 1):
        _set_grads(ps, R["grads"][k])
        opt.step()
    before = _state(opt, ps)
    assert not any(torch.equal(e, q.detach()) for e, q in zip(_ema(opt, ps), ps))          # past the copy: the average is its own stream
    _set_grads(ps, R["grads"][2], poison=bad)
    opt.step()
    assert _same(_state(opt, ps), before)
    assert opt.steps_taken() == 2 and opt.skipped_steps() == 1 and float(opt.guard[2]) == 1.0
    assert not np.isfinite(opt.last_grad_norm())
    _set_grads(ps, R["grads"][3])
    opt.step()
    for k in (0, 1, 3):                                   # the twin never saw the bad step
        _set_grads(twin_p, R["grads"][k])
        twin.step()
    assert opt.steps_taken() == 3 and opt.skipped_steps() == 1
    assert _same(_state(opt, ps), _state(twin, twin_p))


def test_a_skipped_first_step_still_copies_at_the_first_applied_one():
    """the copy rule follows the step counter, which a skipped step does not advance"""
    R = reference(False)
    ps, opt = _ours(R["params"], skip_nonfinite=True)
    _set_grads(ps, R["grads"][0], poison=float("nan"))
    opt.step()
    torch.cuda.synchronize()
    assert opt.steps_taken() == 0 and opt.skipped_steps() == 1
    assert all(torch.equal(_bits(e), _bits(p.to(DEV))) for e, p in zip(_ema(opt, ps), R["params"]))          # as created: the parameter
    _set_grads(ps, R["grads"][0])
    opt.step()
    assert opt.steps_taken() == 1
    assert all(torch.equal(_bits(e), _bits(q.detach())) for e, q in zip(_ema(opt, ps), ps))
    assert not any(torch.equal(q.detach().cpu(), p) for q, p in zip(ps, R["params"]))


def test_hold_leaves_the_average_alone_and_is_not_a_skip():
    R = reference(False)
    ps, opt = _ours(R["params"], skip_nonfinite=True)
    twin_p, twin = _ours(R["params"], skip_nonfinite=True)
    for k in (0, 1):
        _set_grads(ps, R["grads"][k]), _set_grads(twin_p, R["grads"][k])
        opt.step(), twin.step()
    before = _state(opt, ps)
    opt.hold(True)
    _set_grads(ps, R["grads"][2])
    opt.step()
    _set_grads(ps, R["grads"][2], poison=float("nan"), at=(0, 5))          # held: not even a non-finite gradient is counted
    opt.step()
    assert _same(_state(opt, ps), before) and opt.steps_taken() == 2 and opt.skipped_steps() == 0
    opt.hold(False)
    _set_grads(ps, R["grads"][3]), _set_grads(twin_p, R["grads"][3])
    opt.step(), twin.step()
    assert opt.steps_taken() == 3 and opt.skipped_steps() == 0
    assert _same(_state(opt, ps), _state(twin, twin_p))          # resumed exactly where a never-held twin is


@FORMS
def test_without_ema_decay_nothing_is_added(amsgrad):
    """ema_decay=None: no `ema` in the state or the checkpoint, eight tables, the entry points of an optimizer built without the argument.  The averaging
    optimizer runs another instantiation of the update body, so its parameters are not promised to carry the same bits: both meet the project's gate
    against torch (2e-6 * max(1, |p|max), test 1), hence each other within twice that."""
    from lavt_hip import _capi as K
    R = reference(amsgrad)
    ps, opt = _ours(R["params"], amsgrad=amsgrad, ema_decay=None)
    qs, avg = _ours(R["params"], amsgrad=amsgrad)
    K.prof.start()
    for k in range(3):
        _set_grads(ps, R["grads"][k])
        opt.step()
    names = [r[0] for r in K.prof.stop()]
    for k in range(3):
        _set_grads(qs, R["grads"][k])
        avg.step()
    old = "lavt_adamw_step_chunks_amsgrad" if amsgrad else "lavt_adamw_step_chunks"
    assert names.count(old) == 3 and "lavt_adamw_step_chunks_ema" not in names and "lavt_ema_swap" not in names
    assert all("ema" not in opt.state[p] for p in ps) and all("ema" not in st for st in opt.state_dict()["state"].values())
    assert opt._tables.ema is None and opt.ema_decay is None
    assert len(_state(avg, qs)) == len(_state(opt, ps)) + len(SHAPES)
    worst = 0.0
    for p, q in zip(ps, qs):
        err, gate = float((p.detach() - q.detach()).abs().max()), 4e-6 * max(1.0, float(p.detach().abs().max()))
        worst = max(worst, err / gate)
        assert err <= gate, (tuple(p.shape), err, gate)
    print(f"\n[ema off vs on, amsgrad={amsgrad}] worst parameter difference / (2 x the project's gate) after three steps: {worst:.4f}")


# ------------------------------------------------------------------------------------------------ 4. captured
@FORMS
def test_ema_in_hip_graph(amsgrad):
    """1 eager step + 3 replays of step(check_tables=False) equal 4 eager steps bit for bit, the average included"""
    R = reference(amsgrad)
    eager_p, eager = _ours(R["params"], amsgrad=amsgrad)
    graph_p, captured = _ours(R["params"], amsgrad=amsgrad)
    for ps in (eager_p, graph_p):
        _set_grads(ps, R["grads"][0])
    eager.step()
    captured.step()                                       # builds the tables outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured.step(check_tables=False)
        for call in (captured.swap_ema, captured.reset_ema):          # host calls: refused inside a capture, before anything is launched
            with pytest.raises(RuntimeError, match="capture"):
                call()
    for k in range(1, 4):                                 # capture itself executes nothing
        for ps in (eager_p, graph_p):
            for q, gr in zip(ps, R["grads"][k]):
                q.grad.copy_(gr.to(DEV))
        eager.step()
        g.replay()
    torch.cuda.synchronize()
    assert captured.steps_taken() == 4 and eager.steps_taken() == 4
    assert _same(_state(eager, eager_p), _state(captured, graph_p))
    for q, ref in zip(graph_p, R["ema"][3]):
        err = float((captured.state[q]["ema"].cpu() - ref).abs().max())
        assert err <= EMA_GATE * max(1.0, float(ref.abs().max())), (tuple(q.shape), err)


# ------------------------------------------------------------------------------------------------ 5. swap
@FORMS
def test_swap_exchanges_and_restores_every_bit(amsgrad):
    from lavt_hip import ops
    R = reference(amsgrad)
    ps, opt = _ours(R["params"], amsgrad=amsgrad)
    with pytest.raises(RuntimeError, match="first step"):
        opt.swap_ema()
    for k in range(3):
        _set_grads(ps, R["grads"][k])
        opt.step()
    before = _state(opt, ps)
    p0, e0 = [q.detach().clone() for q in ps], _ema(opt, ps)
    count = ops.raw_writes()
    opt.swap_ema()
    torch.cuda.synchronize()
    assert opt.ema_swapped and ops.raw_writes() > count
    assert all(torch.equal(_bits(q.detach()), _bits(e)) for q, e in zip(ps, e0)), "while swapped the parameters hold the former average"
    assert all(torch.equal(_bits(e), _bits(p)) for e, p in zip(_ema(opt, ps), p0))
    for i, c in zip(COPIES, _copies(opt, ps)):
        assert torch.equal(_bits(c), _bits(e0[i].to(torch.bfloat16).reshape(c.shape))), "the bf16 copies are the rounding of the swapped-in average"
    for call, kind in ((opt.step, "step"), (opt.state_dict, "state_dict"), (lambda: opt.load_state_dict({}), "load_state_dict"),
                       (lambda: opt.load_state_dict_in_place({}), "load_state_dict_in_place"), (opt.reset_ema, "reset_ema")):
        with pytest.raises(RuntimeError, match=kind):
            call()
    exported = opt.ema_state_dict(torch.nn.ParameterList(ps))          # the average in either swap state
    assert all(torch.equal(_bits(exported[str(i)]), _bits(e.cpu())) for i, e in enumerate(e0))
    opt.swap_ema()
    assert not opt.ema_swapped
    assert _same(_state(opt, ps), before)
    with opt.ema_weights():
        assert opt.ema_swapped and torch.equal(_bits(ps[3].detach()), _bits(e0[3]))
    assert not opt.ema_swapped and _same(_state(opt, ps), before)
    exported = opt.ema_state_dict(torch.nn.ParameterList(ps))
    assert all(torch.equal(_bits(exported[str(i)]), _bits(e.cpu())) and exported[str(i)].device.type == "cpu" for i, e in enumerate(e0))
    opt.reset_ema()
    assert all(torch.equal(_bits(e), _bits(p)) for e, p in zip(_ema(opt, ps), p0))
    assert all(torch.equal(_bits(q.detach()), _bits(p)) for q, p in zip(ps, p0))


# ------------------------------------------------------------------------------------------------ 6. the harness
EMA_KW = dict(ema_decay=DECAY)


def _ema_of(snap):
    return {k: v for k, v in snap.items() if k.endswith("|ema")}


def test_harness_accumulation_and_resume_carry_the_average():
    """TrainStep(deterministic=True, accumulate=2) + make_optimizer(ema_decay=0.9, max_grad_norm=1.0, skip_nonfinite=True) on the micro model of
    tests/test_gpu_train_state.py.  warmup_and_capture() leaves the average bitwise as it found it (created from the parameters, which the hold keeps);
    over four replays it changes on replays 2 and 4 only; a run saved after replay 3 (inside a cycle), rebuilt from other weights and resumed ends, after
    replay 6, on the bits of a run that never stopped -- the average included."""
    import lavt_hip
    from test_gpu_train_state import _assert_same, _batches2d, _eq, _micro2d, _snapshot, _start, _steps
    batches = _batches2d(6)
    with lavt_hip.use_dtype(torch.bfloat16):
        step, static = _start(_micro2d, 0, 1234, EMA_KW, accumulate=2)
        snap = _snapshot(step)
        ema = _ema_of(snap)
        assert len(ema) == len([p for p in step.model.parameters() if p.requires_grad]) > 0
        assert all(_eq(e, snap["p|" + k.split("|")[1]]) for k, e in ema.items()), "after the warm-up the average is the (unmoved) parameter"
        assert step.opt.steps_taken() == 0 and step.opt.skipped_steps() == 0
        moved, losses = [], []
        for i in range(4):
            losses += _steps(step, static, batches, i, i + 1)
            now = _ema_of(_snapshot(step))
            moved.append(sum(not _eq(now[k], ema[k]) for k in ema))
            ema = now
        print(f"\n[ema under accumulate=2] averages that moved in replays 1..4, of {len(ema)}: {moved}")
        assert moved[0] == 0 and moved[2] == 0 and moved[1] > len(ema) // 2 and moved[3] > len(ema) // 2, moved
        assert step.opt.steps_taken() == 2
        losses += _steps(step, static, batches, 4, 6)
        snap_a = _snapshot(step)
        del step

        step, static = _start(_micro2d, 0, 1234, EMA_KW, accumulate=2)
        _steps(step, static, batches, 0, 3)
        saved = step.state_dict()
        assert step.micro_step() == 1 and "acc" in saved["lavt_train_state"]
        assert all("ema" in st for st in saved["optimizer"]["state"].values()) and all(g["ema_decay"] == DECAY for g in saved["optimizer"]["param_groups"])
        assert "ema_decay" not in saved["lavt_train_state"]["config"]
        del step

        step, static = _start(_micro2d, 7, 99, EMA_KW, accumulate=2)
        addresses = {k: v.data_ptr() for p in step.model.parameters() for k, v in step.opt.state[p].items() if torch.is_tensor(v)}
        step.load_state_dict(saved)
        assert addresses == {k: v.data_ptr() for p in step.model.parameters() for k, v in step.opt.state[p].items() if torch.is_tensor(v)}
        loss_c = _steps(step, static, batches, 3, 6)
        assert all(_eq(a, c) for a, c in zip(losses[3:], loss_c))
        _assert_same(snap_a, _snapshot(step), "resumed after 3 of 6 micro-steps")
        with step.opt.ema_weights():
            with pytest.raises(RuntimeError, match="weight average"):
                step.step()


def test_harness_refuses_a_checkpoint_with_the_average_on_one_side_only():
    """an EMA run refuses the checkpoint of an EMA-free run and the other way round (ValueError naming ema, from the optimizer's check: the fingerprint
    has no such field), and nothing is written"""
    import lavt_hip
    from test_gpu_train_state import _assert_same, _batches2d, _micro2d, _snapshot, _start, _steps
    batches = _batches2d(1)
    with lavt_hip.use_dtype(torch.bfloat16):
        with_avg, static_a = _start(_micro2d, 0, 1234, EMA_KW)
        without, static_b = _start(_micro2d, 0, 1234, {})
        _steps(with_avg, static_a, batches, 0, 1), _steps(without, static_b, batches, 0, 1)
        sd_avg, sd_plain = with_avg.state_dict(), without.state_dict()
        assert sd_avg["lavt_train_state"]["config"] == sd_plain["lavt_train_state"]["config"]
        for step, bad in ((with_avg, sd_plain), (without, sd_avg)):
            before = _snapshot(step)
            with pytest.raises(ValueError, match="ema"):
                step.load_state_dict(bad)
            _assert_same(before, _snapshot(step), "after the refusal")


# ------------------------------------------------------------------------------------------------ 7. live validation
def _fresh_prediction(state, inputs):
    """mask and I / U of a new Predictor in its own context on a new model filled from `state`"""
    from lavt_hip import ops
    from lavt_hip.engine import Predictor
    from test_gpu_infer import _build
    model = _build(32, [2, 2, 2, 2], [1, 2, 4, 8], 7, dpr=0.0)
    model.load_state_dict(state)
    model.to(DEV).eval()
    x, l, m, t = (v.clone() for v in inputs)
    p = Predictor(model, x, l, m, target=t, use_graph=False, context=ops.StepContext())
    p.warmup_and_capture(eager_iters=1)
    mask, iu = p.step().clone(), p.iu.clone()
    torch.cuda.synchronize()
    return mask, iu


@pytest.mark.parametrize("ema_decay", [None, DECAY], ids=["iterate", "average"])
def test_a_predictor_on_the_model_being_trained_follows_it(ema_decay):
    """One model, two captured graphs: a Predictor (its own context) and a TrainStep with an owned optimizer (lr 3e-2, so that three updates move the
    mask).  After three training replays -- raw-pointer writes only: no version counter moves -- pred.step() must give, bit for bit, the mask and I / U
    of a fresh Predictor on a deep copy of the model's state; the fresh predictions before and after training must differ on >= 1 % of the pixels.
    With the average on: inside opt.ema_weights() the mask is that of a fresh Predictor on ema_state_dict(model); after it, the iterate's again."""
    import lavt_hip
    from lavt_hip import ops
    from lavt_hip.detweights import det_inputs
    from lavt_hip.engine import Predictor, TrainStep
    from test_gpu_infer import _build
    train_in = tuple(v.to(DEV) for v in det_inputs(2, 64, 20, seed=17))
    eval_in = tuple(v.to(DEV) for v in det_inputs(2, 64, 20, seed=18))
    with lavt_hip.use_dtype(torch.bfloat16):
        model = _build(32, [2, 2, 2, 2], [1, 2, 4, 8], 7, dpr=0.0).to(DEV).eval()
        pred = Predictor(model, *eval_in[:3], target=eval_in[3], context=ops.StepContext())
        pred.warmup_and_capture()
        assert pred.captured
        model.train()
        step = TrainStep(model, *train_in, context=ops.StepContext())
        kw = {} if ema_decay is None else {"ema_decay": ema_decay}
        opt = step.make_optimizer([p for p in model.parameters() if p.requires_grad], lr=3e-2, weight_decay=1e-2, max_grad_norm=1.0, skip_nonfinite=True, **kw)
        step.warmup_and_capture()
        assert step.captured
        model.eval()
        state0 = copy.deepcopy(model.state_dict())
        mask0, iu0 = _fresh_prediction(state0, eval_in)
        assert torch.equal(pred.step(), mask0) and torch.equal(pred.iu, iu0)          # (the warm-up moved the running statistics: seen as well)

        model.train()
        losses = [float(step.step()) for _ in range(3)]
        model.eval()
        mask = pred.step().clone()
        iu = pred.iu.clone()
        torch.cuda.synchronize()
        assert opt.steps_taken() == 3 and opt.skipped_steps() == 0 and all(np.isfinite(losses)), losses
        state1 = copy.deepcopy(model.state_dict())
        mask1, iu1 = _fresh_prediction(state1, eval_in)
        share = float((mask1 != mask0).float().mean())
        print(f"\n[live validation] fresh predictors before / after three updates differ on {100 * share:.2f} % of the pixels")
        assert share >= 0.01, share
        assert torch.equal(mask, mask1) and torch.equal(iu, iu1), f"the live predictor differs from a fresh one on {float((mask != mask1).float().mean()):.4f} of the pixels"
        if ema_decay is None:
            return

        avg_state = opt.ema_state_dict(model)
        assert avg_state.keys() == state1.keys() and all(torch.equal(avg_state[k], state1[k].cpu()) for k in state1 if "running_" in k or "num_batches" in k)
        mask_e, iu_e = _fresh_prediction(avg_state, eval_in)
        with opt.ema_weights():
            inside = pred.step().clone()
            iu_in = pred.iu.clone()
        torch.cuda.synchronize()
        print(f"[live validation] the average's mask differs from the iterate's on {100 * float((mask_e != mask1).float().mean()):.2f} % of the pixels")
        assert torch.equal(inside, mask_e) and torch.equal(iu_in, iu_e)
        assert torch.equal(pred.step(), mask1) and torch.equal(pred.iu, iu1)
        now = model.state_dict()
        raw = lambda t: t.detach().contiguous().reshape(-1).view(torch.uint8)          # noqa: E731
        assert all(now[k].dtype == v.dtype and torch.equal(raw(now[k]), raw(v)) for k, v in state1.items()), "two swaps restore the model"
