"""Training meters, the host side: lavt_hip.meters.reference_log -- the restatement of lavt_meter_append's arithmetic that the GPU tests compare the
device block with -- reproduces the reference's own SmoothedValue / MetricLogger / IoU (tests/golden/train_meter_cases.npz, written by
tests/golden/make_train_meter_golden.py) exactly; the three new symbols, their bindings, the documented block size, the keyword defaults, and the
state dict's trip through a file."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from meter_cases import PROPS, bits, cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {
    "lavt_meter_bytes": (["capacity"], [C.c_int32]),
    "lavt_meter_append": (["stats", "ctl", "step", "hyper", "total_steps", "power", "block", "capacity", "stream"],
                          [C.c_void_p] * 4 + [C.c_float] * 2 + [C.c_void_p, C.c_int32, C.c_void_p]),
    "lavt_grad_norm_tensors": (["ws", "nchunks", "first", "count", "ctl", "out", "bad", "stream"],
                               [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}


def _prefix(case, n):
    from lavt_hip.meters import reference_log
    c = cases()[case]
    return reference_log(c["losses"][:n], c["I"][:n], c["U"][:n], capacity=8, window_size=int(c["window"]), lrs=c["lrs"][:n])


@pytest.mark.parametrize("case", ["loss6", "run19"])
def test_the_restatement_reproduces_the_reference_exactly(case):
    """after every iteration: iou, seg_correct, cumulative I / U, the five SmoothedValue properties of loss and iou (floats bit for bit) and
    str(MetricLogger) (strings equal); capacity 8 < 19 iterations, so the window is also read across the ring's wrap-around"""
    from lavt_hip import meters as M
    c = cases()[case]
    n = len(c["losses"])
    for i in range(n):
        s = _prefix(case, i + 1)
        assert s.n == s.iterations == i + 1
        last = s.records(1)[0]
        assert bits(np.float64(last["iou"])) == bits(c["iou"][i]) and int(last["it"]) == i
        assert [int(v) for v in s.header[M.H_SEG0:M.H_SEG0 + 5]] == c["seg_correct"][i].tolist()
        assert (int(s.header[M.H_CUM_I]), int(s.header[M.H_CUM_U])) == (int(c["cum_I"][i]), int(c["cum_U"][i]))
        for meter, want in ((s.loss, c["loss_props"][i]), (s.iou, c["iou_props"][i])):
            got = np.array([getattr(meter, p) for p in PROPS], dtype=np.float64)
            assert np.array_equal(bits(got), bits(want)), (i, got.tolist(), want.tolist())
        assert str(s) == c["strings"][i]
    summary = s.summary()
    assert bits(np.float64(summary["mean_iou"])) == bits(c["mean_iou"])
    # the reference divides two integer tensors, i.e. in fp32 (train.py:500); the block holds the exact integers, the summary divides them in fp64
    assert np.float32(summary["overall_iou"]) == np.float32(c["overall_iou"])
    assert summary["iterations"] == n and summary["nonfinite_losses"] == 0
    assert [summary["precision"][t] for t in M.SEG_THRESHOLDS] == [float(v) * 100. / n for v in c["seg_correct"][-1]]


def test_the_issue_s_loss_sequence():
    s = _prefix("loss6", 6)
    assert (s.loss.median, s.loss.avg, s.loss.max, s.loss.value) == (0.75, 0.96875, 2.0, 2.0) and s.loss.global_avg == 4.625 / 6
    assert str(s.loss) == "0.7500 (0.7708)"


def test_the_fp64_division_is_what_passes_the_thresholds():
    """7/10 and 9/10 reach .7 and .9 only when divided in double precision: the fixture holds the reference's verdict, an fp32 division misses both"""
    from lavt_hip.meters import iou_of
    c = cases()["run19"]
    for (I, U), t in (((7, 10), 0.7), ((9, 10), 0.9)):
        assert iou_of(I, U) >= t > float(np.float32(I) / np.float32(U))
        i = next(k for k in range(len(c["I"])) if (c["I"][k], c["U"][k]) == (I, U))
        assert c["iou"][i] >= t
    assert iou_of(0, 0) == 0.0 and iou_of(0, 57) == 0.0


def test_a_non_finite_loss_is_counted_and_left_out_of_the_sum():
    from lavt_hip import meters as M
    s = M.reference_log([0.5, float("nan"), 0.25, float("inf")], [1, 1, 1, 1], [2, 2, 2, 2], capacity=4, window_size=4)
    assert s.header[M.H_LOSS_SUM] == 0.75 and s.header[M.H_LOSS_COUNT] == 2 and s.header[M.H_LOSS_NONFINITE] == 2 and s.loss.global_avg == 0.375
    assert [int(f) & M.LOSS_NONFINITE for f in s.ring["flags"]] == [0, 8, 0, 8]
    assert np.isnan(s.ring["loss"][1]) and np.isinf(s.ring["loss"][3])          # the ring keeps the raw values
    assert s.summary()["nonfinite_losses"] == 2 and s.summary()["mean_loss"] == 0.375


@pytest.mark.parametrize("name", sorted(NEW))
def test_symbols_are_declared_bound_and_exported(name):
    from lavt_hip import _capi
    header = open(os.path.join(ROOT, "include", "lavt_hip.h")).read()
    decl = re.search(r"\b(int|int64_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert decl, f"{name} is not declared in include/lavt_hip.h"
    args = [re.sub(r"/\*.*?\*/", "", a).strip() for a in decl.group(2).split(",")]
    names, ctypes_ = NEW[name]
    assert [a.split()[-1] for a in args] == names
    assert name in _capi.EXPORTED and hasattr(_capi._cdll, name)
    assert _capi._PROTOTYPES[name] == ctypes_
    assert getattr(_capi._cdll, name).restype is (C.c_int64 if decl.group(1) == "int64_t" else C.c_int)
    assert _capi.lib.lavt_abi_version() == _capi.EXPECTED_ABI == 7


def test_block_size_and_layout_are_the_documented_ones():
    from lavt_hip import _capi, meters as M
    header = open(os.path.join(ROOT, "include", "lavt_hip.h")).read()
    defs = {k: int(v.rstrip("u")) for k, v in re.findall(r"#define (LAVT_METER_\w+) (\w+)", header)}
    assert defs == {"LAVT_METER_HEADER_DOUBLES": M.HEADER_DOUBLES, "LAVT_METER_RECORD_BYTES": M.RECORD_BYTES, "LAVT_METER_APPLIED": M.APPLIED,
                    "LAVT_METER_SKIPPED": M.SKIPPED, "LAVT_METER_ACCUMULATING": M.ACCUMULATING, "LAVT_METER_LOSS_NONFINITE": M.LOSS_NONFINITE}
    for cap in (1, 8, 256, 100000):
        assert _capi.lib.lavt_meter_bytes(cap) == M.meter_bytes(cap) == 8 * 32 + 40 * cap
    assert _capi.lib.lavt_meter_bytes(0) == 0 and _capi.lib.lavt_meter_bytes(-3) == 0
    assert [(n, M.RECORD_DTYPE.fields[n][1]) for n in M.RECORD_DTYPE.names] == [("loss", 0), ("I", 4), ("U", 8), ("lr", 12), ("grad_norm", 16), ("flags", 20),
                                                                                  ("iou", 24), ("it", 32)]


def test_defaults_are_keyword_only_and_off():
    from lavt_hip.checkpoint import CONFIG_FIELDS
    from lavt_hip.engine import TrainStep
    from lavt_hip.meters import TrainMeters
    from lavt_hip.optim import FusedAdamW
    for cls, name, default in ((TrainStep, "meters", None), (FusedAdamW, "tensor_norms", False)):
        p = inspect.signature(cls.__init__).parameters[name]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is default
    p = inspect.signature(TrainMeters.__init__).parameters
    assert (p["capacity"].default, p["window_size"].default) == (256, 20)
    assert CONFIG_FIELDS == ("criterion", "dice_rate", "boundary_rate", "accumulate", "amsgrad", "max_grad_norm", "skip_nonfinite", "deterministic",
                             "compute_dtype", "fp8", "world", "param_groups")
    opt = FusedAdamW([torch.nn.Parameter(torch.zeros(3))])
    assert opt.tensor_norms is False and opt.guard is None and not opt._wants_norm()
    assert "tensor_norms" not in str(opt.state_dict())
    for call in (opt.grad_norms, opt.last_nonfinite):
        with pytest.raises(RuntimeError, match="tensor_norms=True"):
            call()
    for name in ("make_meters", "attach_meters"):
        assert callable(getattr(TrainStep, name))


def test_state_dict_loads_with_weights_only(tmp_path):
    """the state dict TrainMeters.state_dict() returns is Snapshot.state_dict() of the block's copy: CPU tensors and plain values"""
    from lavt_hip.meters import Snapshot, TrainMeters
    s = _prefix("run19", 19)
    sd = s.state_dict()
    assert "Snapshot(" in inspect.getsource(TrainMeters.state_dict) and ".state_dict()" in inspect.getsource(TrainMeters.state_dict)
    path = os.path.join(tmp_path, "meters.pt")
    torch.save({"meters": sd}, path)
    back = torch.load(path, map_location="cpu", weights_only=True)["meters"]
    assert back["capacity"] == 8 and back["window_size"] == 5 and back["format"] == 1
    raw = np.concatenate([back["header"].numpy().view(np.uint8), back["ring"].numpy()])
    again = Snapshot(raw, back["capacity"], back["window_size"])
    assert str(again) == str(s) and again.summary() == s.summary()
