"""CPU tests of the checkpoint-and-resume feature's pure parts (DESIGN.md "Checkpoint and resume"): the fingerprint comparison of
TrainStep.load_state_dict (every field, the text naming it, nothing loaded when it raises), the names of the fp8 sites, the weights_only round trip and
the atomic write of lavt_hip.checkpoint's writer, and the checks FusedAdamW makes before an in-place load."""
import copy
import os
import weakref
from collections import OrderedDict

import pytest
import torch


def _model():
    torch.manual_seed(0)
    return torch.nn.Sequential(OrderedDict(lin=torch.nn.Linear(4, 3), bn=torch.nn.BatchNorm1d(3), out=torch.nn.Linear(3, 2)))


def _fake_step(accumulate=1, amsgrad=False, fp8=False):
    """a TrainStep past its warm-up as far as load_state_dict's checks can tell, on CPU tensors: everything those checks read, no device"""
    from lavt_hip import ops
    from lavt_hip.engine import TrainStep
    from lavt_hip.optim import FusedAdamW
    model = _model()
    step = TrainStep.__new__(TrainStep)
    step.model, step.context, step.world, step.accumulate = model, ops.StepContext(deterministic=True), 1, accumulate
    step.criterion, step.dice_rate, step.boundary_rate = "ce", 1.0, 0.05
    step._params, step._warmed, step._seen, step._dtype, step.acc, step.graph = list(model.parameters()), True, (0, 0), (torch.bfloat16, fp8), None, None
    decay = [p for n, p in model.named_parameters() if not n.startswith("bn.")]
    step.opt = FusedAdamW([{"params": [model.bn.weight, model.bn.bias], "weight_decay": 0.0}, {"params": decay}], lr=1e-3, amsgrad=amsgrad, total_steps=10)
    step.opt._owner = weakref.ref(step)
    step.opt._step = torch.zeros(1)
    for p in model.parameters():          # the flat state FusedAdamW._build creates on the device, here by hand
        step.opt.state[p] = {"step": step.opt._step, "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)}
        if amsgrad:
            step.opt.state[p]["max_exp_avg_sq"] = torch.zeros_like(p)
    if fp8:
        f8 = step.context.fp8
        f8.slot(id(model.out.weight), torch.device("cpu"))
        f8.slot((id(model.lin.weight), "dy"), torch.device("cpu"))
    return step


def _hand_made_state(step):
    """what state_dict() of `step` would hold, with other values in every tensor"""
    from lavt_hip.checkpoint import to_host
    sites = step._fp8_sites()
    return {"model": {k: v + 1 for k, v in to_host(step.model.state_dict()).items()},
            "optimizer": {**{k: (v if k != "state" else {i: {kk: (vv + 1) for kk, vv in st.items()} for i, st in v.items()})
                             for k, v in to_host(torch.optim.Optimizer.state_dict(step.opt)).items()},
                          "lavt_schedule": {"total_steps": 10.0, "power": 0.9, "steps_taken": 4}},
            "lavt_train_state": {"format": 1, "config": step._config(), "guard": None, "droppath": {}, "fp8": {n: torch.tensor([1.5, 2.5]) for n in sites},
                                 "torch_cuda_rng": torch.zeros(16, dtype=torch.uint8)}}


def _everything(step):
    out = [v.clone() for v in step.model.state_dict().values()]
    out += [v.clone() for st in step.opt.state.values() for v in st.values()]
    if step.context.fp8.prev is not None:
        out += [step.context.fp8.prev.clone(), step.context.fp8.cur.clone()]
    return out


def _unchanged(step, before):
    return all(torch.equal(a, b) for a, b in zip(_everything(step), before))


# ------------------------------------------------------------------------------------------------ fingerprint
OTHER = {"criterion": "mc_dice", "dice_rate": 0.75, "boundary_rate": 0.5, "accumulate": 3, "amsgrad": True, "max_grad_norm": 1.0, "skip_nonfinite": True,
         "deterministic": False, "compute_dtype": "torch.float32", "fp8": True, "world": 2}


def test_config_has_the_fields_of_the_fingerprint():
    from lavt_hip.checkpoint import CONFIG_FIELDS
    cfg = _fake_step(accumulate=2)._config()
    assert tuple(cfg) == CONFIG_FIELDS and set(OTHER) | {"param_groups"} == set(CONFIG_FIELDS)
    assert cfg["accumulate"] == 2 and cfg["compute_dtype"] == "torch.bfloat16" and cfg["deterministic"] is True and cfg["world"] == 1
    assert cfg["param_groups"] == [[["bn.weight", [3]], ["bn.bias", [3]]], [["lin.weight", [3, 4]], ["lin.bias", [3]], ["out.weight", [2, 3]], ["out.bias", [2]]]]


@pytest.mark.parametrize("field", sorted(OTHER))
def test_each_field_is_compared_named_and_nothing_is_loaded(field):
    from lavt_hip.checkpoint import compare_fingerprints
    step = _fake_step()
    state = _hand_made_state(step)
    state["lavt_train_state"]["config"][field] = OTHER[field]
    with pytest.raises(ValueError, match=f"config field '{field}' differs.*{field}={OTHER[field]!r}"):
        compare_fingerprints(state["lavt_train_state"]["config"], step._config())
    before = _everything(step)
    with pytest.raises(ValueError, match=f"TrainStep.load_state_dict: config field '{field}' differs"):
        step.load_state_dict(state)
    assert _unchanged(step, before)


def test_the_first_differing_field_is_the_one_named():
    from lavt_hip.checkpoint import compare_fingerprints
    step = _fake_step()
    saved = dict(step._config(), world=2, accumulate=3, amsgrad=True)
    with pytest.raises(ValueError, match="'accumulate' differs: the checkpoint was written with accumulate=3, this step runs with accumulate=1"):
        compare_fingerprints(saved, step._config())
    saved.pop("fp8")
    saved["accumulate"] = 1
    with pytest.raises(ValueError, match="'amsgrad'"):
        compare_fingerprints(saved, step._config())
    saved["amsgrad"] = False
    with pytest.raises(ValueError, match="no field 'fp8'"):
        compare_fingerprints(saved, step._config())


def _groups_case(edit):
    step = _fake_step()
    state = _hand_made_state(step)
    edit(state["lavt_train_state"]["config"]["param_groups"])
    return step, state


@pytest.mark.parametrize("edit,match", [
    (lambda g: g[1].pop(), r"group 1 has 3 parameters in the checkpoint and 4 in this step: out.bias \(2,\) is in this step only"),
    (lambda g: g[0].append(["bn.extra", [3]]), r"group 0 has 3 parameters in the checkpoint and 2 in this step: bn.extra \(3,\) is in the checkpoint only"),
    (lambda g: g[1][0].__setitem__(0, "linear.weight"), r"group 1, entry 0 is another parameter: the checkpoint has linear.weight \(3, 4\), this step lin.weight \(3, 4\)"),
    (lambda g: g[1][2].__setitem__(1, [2, 5]), r"group 1, entry 2 was reshaped: the checkpoint has out.weight \(2, 5\), this step out.weight \(2, 3\)"),
    (lambda g: g.append([]), "the checkpoint has 3 parameter groups, this step's optimizer 2"),
])
def test_parameter_list_missing_extra_renamed_reshaped(edit, match):
    step, state = _groups_case(edit)
    before = _everything(step)
    with pytest.raises(ValueError, match="config field 'param_groups' differs: " + match):
        step.load_state_dict(state)
    assert _unchanged(step, before)


def test_a_fingerprint_survives_the_file(tmp_path):
    """tuples and lists: a fingerprint read back from a file compares equal to the one it was written from"""
    from lavt_hip.checkpoint import compare_fingerprints, write_atomic
    cfg = _fake_step(accumulate=2, amsgrad=True)._config()
    cfg["param_groups"] = tuple(tuple((n, tuple(s)) for n, s in g) for g in cfg["param_groups"])
    write_atomic(str(tmp_path / "c.pt"), {"config": cfg})
    back = torch.load(str(tmp_path / "c.pt"), weights_only=True)["config"]
    compare_fingerprints(back, _fake_step(accumulate=2, amsgrad=True)._config())


def test_later_refusals_load_nothing_either():
    """past the fingerprint: a model entry of another shape, a moment of another shape, another schedule, an unknown fp8 site, a torn top level"""
    step = _fake_step(fp8=True)
    good = _hand_made_state(step)
    before = _everything(step)

    def case(edit, exc, match):
        state = copy.deepcopy(good)
        edit(state)
        with pytest.raises(exc, match=match):
            step.load_state_dict(state)
        assert _unchanged(step, before)
    case(lambda s: s["model"].update({"lin.weight": torch.zeros(3, 5)}), ValueError, r"'model' entry lin.weight is \(3, 5\) in the checkpoint, \(3, 4\)")
    case(lambda s: s["model"].pop("bn.running_mean"), ValueError, "'model' has no entry bn.running_mean")
    case(lambda s: s["model"].update({"bn.more": torch.zeros(1)}), ValueError, "entry bn.more that this model does not have")
    case(lambda s: s["optimizer"]["state"][0].update(exp_avg=torch.zeros(7)), ValueError, r"'exp_avg' of parameter 0 is \(7,\)")
    case(lambda s: s["optimizer"]["lavt_schedule"].update(total_steps=99.0), ValueError, "total_steps=99.0")
    case(lambda s: s["optimizer"]["param_groups"][1].update(lr=0.5), ValueError, "group 1 was saved with lr=0.5")
    case(lambda s: s["lavt_train_state"]["fp8"].update({"gone.weight|act": torch.zeros(2)}), ValueError, r"fp8 site 'gone.weight\|act' of the checkpoint does not exist")
    case(lambda s: s["lavt_train_state"]["fp8"].pop("lin.weight|dy"), ValueError, r"fp8 site 'lin.weight\|dy' of this step is not in the checkpoint")
    case(lambda s: s["lavt_train_state"].update(format=2), ValueError, "format 2")
    case(lambda s: s.pop("optimizer"), ValueError, "no 'optimizer'")


def test_load_before_the_warm_up_says_why():
    step = _fake_step()
    state = _hand_made_state(step)
    step._warmed, step._seen = False, None
    before = _everything(step)
    with pytest.raises(RuntimeError, match="call warmup_and_capture\\(\\) first.*advance forward-side state"):
        step.load_state_dict(state)
    assert _unchanged(step, before)


# ------------------------------------------------------------------------------------------------ the optimizer
def test_replacing_load_refuses_a_captured_owner_and_points_to_the_step():
    step = _fake_step()
    sd = copy.deepcopy(_hand_made_state(step)["optimizer"])
    ptrs = [st["exp_avg"].data_ptr() for st in step.opt.state.values()]
    step.graph = object()          # captured
    with pytest.raises(RuntimeError, match="has been captured.*TrainStep.load_state_dict"):
        step.opt.load_state_dict(sd)
    assert ptrs == [st["exp_avg"].data_ptr() for st in step.opt.state.values()] and step.opt.steps_taken() == 0
    step.graph = None              # attached, not captured: the path of every existing caller
    step.opt.load_state_dict(sd)
    assert step.opt.steps_taken() == 4 and ptrs != [st["exp_avg"].data_ptr() for st in step.opt.state.values()]


def test_in_place_plan_covers_every_moment_and_the_counters():
    step = _fake_step(amsgrad=True)
    sd = _hand_made_state(step)["optimizer"]
    sd["lavt_schedule"]["skipped_steps"] = 0
    plan, steps, skipped = step.opt.check_state_dict_in_place(sd)
    assert steps == 4.0 and skipped == 0.0 and len(plan) == 3 * 6
    mine = {t.data_ptr() for st in step.opt.state.values() for k, t in st.items() if k != "step"}
    assert {dst.data_ptr() for dst, _ in plan} == mine and all(src is not None and src.shape == dst.shape for dst, src in plan)
    other = _fake_step(amsgrad=False)
    with pytest.raises(ValueError, match="amsgrad"):
        other.opt.check_state_dict_in_place(sd)
    sd["lavt_schedule"]["skipped_steps"] = 2
    with pytest.raises(ValueError, match="2 skipped steps"):
        step.opt.check_state_dict_in_place(sd)          # no control block on this optimizer


# ------------------------------------------------------------------------------------------------ fp8 sites
def test_fp8_sites_are_named_by_the_consuming_parameter_not_by_slot():
    from lavt_hip.checkpoint import fp8_site_name, fp8_site_slots, match_fp8_sites
    from lavt_hip.ops import _Fp8State
    model = _model()
    names = {id(p): n for n, p in model.named_parameters()}
    w1, w2 = model.lin.weight, model.out.weight
    assert fp8_site_name(id(w1), names) == "lin.weight|act" and fp8_site_name((id(w2), "dy"), names) == "out.weight|dy"
    with pytest.raises(ValueError, match="not a parameter"):
        fp8_site_name(id(torch.zeros(1)), names)
    cpu = torch.device("cpu")
    a, b = _Fp8State(), _Fp8State()
    for key in (id(w1), (id(w1), "dy"), id(w2)):
        a.slot(key, cpu)
    for key in (id(w2), id(w1), (id(w1), "dy")):          # another order of first use: other slot numbers, the same names
        b.slot(key, cpu)
    sa, sb = fp8_site_slots(a.slots, names), fp8_site_slots(b.slots, names)
    assert sa == {"lin.weight|act": 0, "lin.weight|dy": 1, "out.weight|act": 2} and sb == {"out.weight|act": 0, "lin.weight|act": 1, "lin.weight|dy": 2}
    match_fp8_sites(sa, sb)
    step = _fake_step(fp8=True)
    assert step._fp8_sites() == {"out.weight|act": 0, "lin.weight|dy": 1}
    assert _fake_step(fp8=False)._fp8_sites() == {}


# ------------------------------------------------------------------------------------------------ the writer
class _Stub:
    """stands in for a TrainStep: hands out a hand-made state, keeps what it is given"""

    def __init__(self, state):
        self.state, self.loaded = state, None

    def state_dict(self):
        return self.state

    def load_state_dict(self, state):
        self.loaded = state


def test_weights_only_round_trip_through_the_writer(tmp_path):
    from lavt_hip.checkpoint import load_train_state, save_train_state
    step = _fake_step(fp8=True, accumulate=3)
    state = _hand_made_state(step)
    state["lavt_train_state"].update(guard=torch.arange(8, dtype=torch.float32), acc=torch.randn(11), acc_layout=[["lin.weight", 0], ["out.bias", 12]],
                                     droppath={"cuda:0": (1234, 56)})
    path = str(tmp_path / "run" ) + ".pt"
    save_train_state(path, _Stub(state), epoch=7, lr_scheduler={"last_epoch": 91, "base_lrs": [5e-5]}, note="after epoch 7")
    assert os.listdir(tmp_path) == ["run.pt"]          # the .tmp file is gone
    reader = _Stub(None)
    extra = load_train_state(path, reader)          # torch.load(weights_only=True) inside
    assert extra == {"epoch": 7, "lr_scheduler": {"last_epoch": 91, "base_lrs": [5e-5]}, "note": "after epoch 7"}
    assert set(reader.loaded) == {"model", "optimizer", "lavt_train_state", "epoch", "lr_scheduler", "note"}

    def same(a, b):
        if torch.is_tensor(a):
            return torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a, b)
        if isinstance(a, dict):
            return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
        if isinstance(a, (list, tuple)):
            return type(a) is type(b) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
        return type(a) is type(b) and a == b
    for k in ("model", "optimizer", "lavt_train_state"):
        assert same(state[k], reader.loaded[k]), k
    with pytest.raises(ValueError, match="'model' is written by the step itself"):
        save_train_state(path, _Stub(state), model={})


def test_the_write_is_atomic(tmp_path):
    from lavt_hip.checkpoint import write_atomic
    path = str(tmp_path / "ckpt.pt")
    write_atomic(path, {"epoch": 1})
    assert os.listdir(tmp_path) == ["ckpt.pt"]

    def torn(obj, f):
        open(f, "wb").write(b"half a file")
        raise OSError("disk full")
    with pytest.raises(OSError, match="disk full"):
        write_atomic(path, {"epoch": 2}, _save=torn)
    assert os.listdir(tmp_path) == ["ckpt.pt"]
    assert torch.load(path, weights_only=True) == {"epoch": 1}
    seen = []

    def watching(obj, f):
        seen.append((f, os.path.exists(path)))
        torch.save(obj, f)
    write_atomic(path, {"epoch": 3}, _save=watching)
    assert seen == [(path + ".tmp", True)] and torch.load(path, weights_only=True) == {"epoch": 3} and os.listdir(tmp_path) == ["ckpt.pt"]
