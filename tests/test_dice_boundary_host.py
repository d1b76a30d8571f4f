"""Host-side checks of the fused Dice+Boundary criterion (no GPU): the torch restatement the GPU tests lean on (tests/dice_boundary_ref.py) against
the fixtures written by the reference's own DiceBoundaryLoss (tests/golden/make_boundary_golden.py), the C ABI additions under the unchanged ABI
version, and the keyword-only, default-valued surface in Python."""
import inspect
import os
import re

import pytest
import torch

import dice_boundary_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lavt_upsample_dice_boundary_ws", "lavt_upsample_dice_boundary_fwd", "lavt_upsample_dice_boundary_bwd", "lavt_upsample_dice_boundary_sel_fwd",
       "lavt_upsample_dice_boundary_sel_bwd")


@pytest.mark.parametrize("tag", R.TAGS)
def test_restatement_matches_the_reference_fixture(tag):
    """loss (and both parts) within 1e-6, d loss / d x within 1e-7 absolute, every element"""
    f = R.load(tag)
    loss, dice, bnd, dy = R.lowres(f["x"], f["target"], f["dims"], *f["rates"])
    err = float((dy - f["dy"]).abs().max())
    print(f"\n[dice_boundary restatement {tag}] loss {loss:.8f} ref {f['loss']:.8f}  max |dy - ref| {err:.3e} (max |ref| {float(f['dy'].abs().max()):.3e})")
    assert abs(loss - f["loss"]) <= 1e-6 and abs(dice - f["dice"]) <= 1e-6 and abs(bnd - f["boundary"]) <= 1e-6
    assert dy.shape == f["dy"].shape and err <= 1e-7


def test_fixtures_cover_the_cases_they_are_named_for():
    a, sat, fg, blob, only = (R.load(t) for t in ("a", "sat", "fg", "blob", "blob_bonly"))
    assert int(a["target"][-1].sum()) == 0 and int(a["target"][0].sum()) > 0
    assert sat["scale"] == 40.0 and bool((fg["target"] == 1).all()) and fg["boundary"] == pytest.approx(1.0)
    assert only["rates"] == (0.0, 1.0) and torch.equal(only["x"], blob["x"]) and torch.equal(only["target"], blob["target"])
    assert only["loss"] == pytest.approx(only["boundary"], abs=1e-7)
    assert R.load("same")["dims"][1:3] == R.load("same")["dims"][3:5]


def test_entry_points_are_declared_bound_and_exported():
    from lavt_hip import _capi
    header = open(os.path.join(ROOT, "include", "lavt_hip.h")).read()
    declared = set(re.findall(r"\b(lavt_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/lavt_hip.h"
        assert name in _capi.EXPORTED, f"{name} is not bound in lavt_hip/_capi.py"
        assert hasattr(_capi._cdll, name), f"liblavt_hip.so does not export {name}"
    assert _capi.lib.lavt_abi_version() == _capi.EXPECTED_ABI == 7
    # the scratch query is host arithmetic: 14 partial sums per 32 x 32 tile and sample, then the fp32 dz map
    assert _capi.lib.lavt_upsample_dice_boundary_ws(2, 120, 120) == 2 * (16 * 14 + 120 * 120)
    assert _capi.lib.lavt_upsample_dice_boundary_ws(3, 9, 7) == 3 * (14 + 63)
    assert _capi.lib.lavt_upsample_dice_boundary_ws(0, 9, 7) == 0


def test_python_surface():
    import losses
    from lavt_hip import ops
    from lavt_hip.engine import TrainStep
    from lib import _utils
    ts = inspect.signature(TrainStep.__init__).parameters
    for name, default in (("dice_rate", 1.0), ("boundary_rate", 0.05)):
        assert ts[name].kind is inspect.Parameter.KEYWORD_ONLY and ts[name].default == default
        assert inspect.signature(_utils.fused_dice_boundary_loss).parameters[name].default == default
        assert inspect.signature(ops.upsample_dice_boundary_loss).parameters[name].default == default
    assert list(inspect.signature(_utils.fused_dice_boundary_loss).parameters) == ["y", "target", "valid_indices", "dice_rate", "boundary_rate"]
    assert list(inspect.signature(ops.upsample_dice_boundary_loss).parameters) == ["x", "target", "B", "Hi", "Wi", "Ho", "Wo", "sel", "dice_rate", "boundary_rate"]
    assert inspect.signature(ops.upsample_dice_boundary_loss).parameters["sel"].default is None
    crit = losses.DiceBoundaryLoss()                        # the reference's constructor order: (boundary_rate, dice_rate)
    assert (crit.boundary_rate, crit.dice_rate) == (0.05, 1)
    crit = losses.DiceBoundaryLoss(0.2, 0.5)
    assert (crit.boundary_rate, crit.dice_rate) == (0.2, 0.5)
    with pytest.raises(NotImplementedError):
        losses.DiceFocalLoss()
    x, t = torch.zeros(2, 4, 3, 8, 8), torch.zeros(2, 8, 8, dtype=torch.int64)
    with pytest.raises(ValueError, match="dice_boundary"):
        TrainStep(None, x, None, None, t, loss="dice_focal")
