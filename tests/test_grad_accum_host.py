"""CPU tests of gradient accumulation in the captured train step: TrainStep(accumulate=k) validates k in the constructor, before it touches any device;
lavt_grad_accumulate is declared in include/lavt_hip.h, bound in lavt_hip._capi with the argument types of its declaration and exported by the
library, under the unchanged ABI version."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _train_step(**kw):
    from lavt_hip.engine import TrainStep
    return TrainStep(None, None, None, None, None, **kw)          # the check of `accumulate` comes first: nothing of the model or the inputs is looked at


@pytest.mark.parametrize("bad", [0, -3, 2.5, 2.0, "2", None])
def test_bad_accumulate_raises_value_error(bad):
    with pytest.raises(ValueError, match="accumulate"):
        _train_step(accumulate=bad)


def test_accumulate_defaults_to_one_and_is_keyword_only():
    from lavt_hip.engine import TrainStep
    par = inspect.signature(TrainStep.__init__).parameters["accumulate"]
    assert par.default == 1 and par.kind is inspect.Parameter.KEYWORD_ONLY
    for name in ("micro_step", "reset_accumulation"):
        assert callable(getattr(TrainStep, name))
    from lavt_hip.optim import FusedAdamW
    assert callable(FusedAdamW.set_grad_source)


def test_grad_accumulate_is_declared_bound_and_exported():
    from lavt_hip import _capi
    header = open(os.path.join(ROOT, "include", "lavt_hip.h")).read()
    name = "lavt_grad_accumulate"
    decl = re.search(r"\bint\s+lavt_grad_accumulate\s*\(([^)]*)\)\s*;", header)
    assert decl, f"{name} is not declared in include/lavt_hip.h"
    assert name in _capi.EXPORTED, f"{name} is not bound in lavt_hip/_capi.py"
    assert hasattr(_capi._cdll, name), f"liblavt_hip.so does not export {name}"
    # the binding's argument types, one by one, against the declaration's
    ctype_of = {"const float*": C.c_void_p, "float*": C.c_void_p, "void*": C.c_void_p, "int64_t": C.c_int64, "int": C.c_int32}
    want = []
    for arg in decl.group(1).split(","):
        ty = re.sub(r"\s*\*\s*", "* ", arg.strip()).rsplit(" ", 1)[0].strip()          # drop the parameter's name
        want.append(ctype_of[ty])
    assert [a.strip().split()[-1] for a in decl.group(1).split(",")] == ["g", "acc", "n", "k", "ctl", "stream"]
    assert _capi._PROTOTYPES[name] == want == [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]
    assert getattr(_capi._cdll, name).restype is C.c_int
    assert _capi.lib.lavt_abi_version() == _capi.EXPECTED_ABI == 7


def test_control_block_documents_the_phase_slots():
    header = open(os.path.join(ROOT, "include", "lavt_hip.h")).read()
    assert re.search(r"\[5\] accumulating", header) and re.search(r"\[6\] micro index", header)
