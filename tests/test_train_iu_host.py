"""Host side of the hard-mask I / U pass of the training meters (DESIGN.md "Training meters"; include/lavt_hip.h: lavt_upsample_iu): the ABI surface,
the Python signatures, and the shared cases of tests/train_iu_ref.py -- that they are exact where they claim to be and contain what they are named
for.  No GPU: the kernels are checked by tests/test_gpu_train_iu.py."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

import train_iu_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
NEW = {
    "lavt_upsample_iu_ws": (["n", "Ho", "Wo"], [i32, i32, i32]),
    "lavt_upsample_iu": (["x", "target", "loss_src", "ws", "ws_words", "row", "B", "Hi", "Wi", "Ho", "Wo", "stream"],
                         [vp, vp, vp, vp, i64, vp, i32, i32, i32, i32, i32, vp]),
    "lavt_upsample_iu_sel": (["x", "sel", "nsel", "target", "loss_src", "ws", "ws_words", "row", "B", "Hi", "Wi", "Ho", "Wo", "stream"],
                             [vp, vp, i32, vp, vp, vp, i64, vp, i32, i32, i32, i32, i32, vp]),
}


@pytest.mark.parametrize("name", sorted(NEW))
def test_symbols_are_declared_bound_and_exported(name):
    from lavt_hip import _capi
    header = open(os.path.join(ROOT, "include", "lavt_hip.h")).read()
    decl = re.search(r"\b(int|int64_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert decl, f"{name} is not declared in include/lavt_hip.h"
    args = [re.sub(r"/\*.*?\*/", "", a).strip() for a in decl.group(2).split(",")]
    names, ctypes_ = NEW[name]
    lead = [] if name.endswith("_ws") else ["dtype"]
    assert [a.split()[-1].lstrip("*") for a in args] == lead + names
    assert name in _capi.EXPORTED and hasattr(_capi._cdll, name)
    assert _capi._PROTOTYPES[name] == ([i32] if lead else []) + ctypes_
    assert getattr(_capi._cdll, name).restype is (C.c_int64 if decl.group(1) == "int64_t" else C.c_int)
    assert _capi.lib.lavt_abi_version() == _capi.EXPECTED_ABI == 7


def test_the_header_states_the_row_and_its_source():
    header = open(os.path.join(ROOT, "include", "lavt_hip.h")).read()
    at = header.index("int64_t lavt_upsample_iu_ws")
    comment = header[header.rindex("/*", 0, at):at]
    assert "train.py:64-76" in comment and "{loss_src ? loss_src[0] : 0, 0, I, U}" in comment


def test_the_sel_prototype_is_the_plain_one_with_the_selection_behind_x():
    plain, sel = NEW["lavt_upsample_iu"], NEW["lavt_upsample_iu_sel"]
    assert sel[0] == plain[0][:1] + ["sel", "nsel"] + plain[0][1:] and sel[1] == plain[1][:1] + [vp, i32] + plain[1][1:]


def test_scratch_query():
    from lavt_hip import _capi as K
    assert K.lib.lavt_upsample_iu_ws(0, 480, 480) == 0 and K.lib.lavt_upsample_iu_ws(-3, 480, 480) == 0
    small, flagship, huge = K.lib.lavt_upsample_iu_ws(1, 1, 1), K.lib.lavt_upsample_iu_ws(2, 480, 480), K.lib.lavt_upsample_iu_ws(4096, 480, 480)
    assert 0 < small <= flagship <= huge
    assert small == 2 and flagship == 2 * 1800          # one int32 pair per workgroup of 256 pixels ...
    assert huge == 2 * 4096                             # ... on a capped grid (n * Ho * Wo = 9.4e8 here: the product is formed in 64 bits)
    assert K.lib.lavt_upsample_iu_ws(60000, 480, 480) == 2 * 4096          # 1.4e10 pixels: past 2^31


def test_python_signatures():
    from lavt_hip import ops
    from lib import _utils
    sig = inspect.signature(ops.upsample_iu)
    assert list(sig.parameters) == ["x", "target", "B", "Hi", "Wi", "Ho", "Wo", "sel", "loss"]
    assert sig.parameters["sel"].default is None and sig.parameters["loss"].default is None
    assert all(sig.parameters[k].default is inspect.Parameter.empty for k in ("x", "target", "B", "Hi", "Wi", "Ho", "Wo"))
    sig = inspect.signature(_utils.fused_iu)
    assert list(sig.parameters) == ["y", "target", "valid_indices", "loss"]
    assert sig.parameters["valid_indices"].default is None and sig.parameters["loss"].default is None


def test_cpu_tensors_are_refused():
    from lavt_hip import ops
    x, t = torch.zeros(4, 2), torch.zeros(1, 4, 4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="GPU memory only"):
        ops.upsample_iu(x, t, 1, 2, 2, 4, 4)


@pytest.mark.parametrize("name", sorted(R.EXACT_GEOMETRIES))
def test_exact_cases_are_exact_and_hold_what_they_are_named_for(name):
    logits, target = R.exact_case(name)
    B, Hi, Wi, Ho, Wo = R.EXACT_GEOMETRIES[name]
    assert logits.shape == (B, 2, Hi, Wi) and target.shape == (B, Ho, Wo)
    assert torch.equal(logits.bfloat16().float(), logits), "the logits must be representable in bf16"
    assert torch.equal(logits * 8, (logits * 8).round()) and float(logits.abs().max()) <= 3.0
    # fp32 and fp64 give the same upsampled VALUES, not only the same counts
    assert torch.equal(R.upsampled(logits, Ho, Wo, torch.float32).double(), R.upsampled(logits, Ho, Wo, torch.float64))
    assert R.train_iu(logits, target, dtype=torch.float32) == R.train_iu(logits, target, dtype=torch.float64)
    assert R.ties(logits, Ho, Wo) >= 1, "no exact tie pixel"
    assert R.ties(logits[:1], Ho, Wo) >= 1, "the planted ties are in sample 0"
    last = R.upsampled(logits[B - 1:], Ho, Wo)
    assert int(last.argmax(1).sum()) == 0, "the last sample predicts background everywhere"
    assert R.train_iu(logits[B - 1:], target[B - 1:]) == (0, 0)
    I, U = R.train_iu(logits, target)
    assert 0 < I < U < 2 ** 24
    # a tie is class 0: forcing the tied pixels to class 1 changes the counts, so the cases can tell `>` from `>=`
    out = R.upsampled(logits, Ho, Wo)
    ge = (out[:, 1] >= out[:, 0]).long()
    assert (int((ge * target).sum()), int((ge + target).sum() - (ge * target).sum())) != (I, U)


@pytest.mark.parametrize("name", sorted(R.MARGIN_GEOMETRIES))
def test_margin_cases_keep_their_margin(name):
    logits, target = R.margin_case(name)
    (B, Hi, Wi, Ho, Wo), _ = R.MARGIN_GEOMETRIES[name]
    assert torch.equal(logits.bfloat16().float(), logits)
    m = R.margin(logits, Ho, Wo)
    print(f"[{name}] smallest fp64 |up1 - up0| = {m:.3e}")
    assert m >= R.MIN_MARGIN
    assert R.train_iu(logits, target, dtype=torch.float32) == R.train_iu(logits, target, dtype=torch.float64)
    I, U = R.train_iu(logits, target)
    assert 0 < I < U < 2 ** 24


def test_selection_of_the_restatement():
    logits, target = R.exact_case("q_3x5x9_17x33")
    assert R.train_iu(logits, target, sel=[0, 1, 2]) == R.train_iu(logits, target)
    a, b = R.train_iu(logits[2:], target[:1]), R.train_iu(logits[:1], target[1:2])
    both = R.train_iu(logits, target[:2], sel=[2, 0])
    assert both == (a[0] + b[0], a[1] + b[1])
    assert R.train_iu(logits, target[:2], sel=[2, 9]) == a          # an out-of-range entry drops its sample, target included
    assert R.train_iu(logits, target[:2], sel=[-1, 7]) == (0, 0)
