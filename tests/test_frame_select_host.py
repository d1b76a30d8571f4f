"""Host-side checks of annotated-frame selection (no GPU): the C ABI additions under the unchanged ABI version, the `i * t + ind` arithmetic of the
reference (train.py:283) with its host-side checks, and the keyword-only, default-off surface of TrainStep / Predictor / the fused losses."""
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lavt_upsample_ce_sel_fwd", "lavt_upsample_ce_sel_bwd", "lavt_upsample_dice_sel_fwd", "lavt_upsample_dice_sel_bwd", "lavt_gather_samples")


def test_selection_entry_points_are_declared_bound_and_exported():
    from lavt_hip import _capi
    header = open(os.path.join(ROOT, "include", "lavt_hip.h")).read()
    declared = set(re.findall(r"\b(lavt_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/lavt_hip.h"
        assert name in _capi.EXPORTED, f"{name} is not bound in lavt_hip/_capi.py"
        assert hasattr(_capi._cdll, name), f"liblavt_hip.so does not export {name}"
    assert _capi.lib.lavt_abi_version() == _capi.EXPECTED_ABI == 7


def _shell(cls, n_sel, clips, T):
    """an engine object with nothing but what set_valid_indices touches: the static index buffer and the image buffer that fixes the frame count"""
    obj = cls.__new__(cls)
    obj.valid_indices = torch.full((n_sel,), -1, dtype=torch.int32)
    obj.x = torch.zeros(clips, T, 3, 8, 8)
    return obj


@pytest.mark.parametrize("which", ["TrainStep", "Predictor"])
def test_set_valid_indices_maps_clip_frames_to_flat_rows(which):
    from lavt_hip import engine
    obj = _shell(getattr(engine, which), 2, 2, 4)
    obj.set_valid_indices([2, 1], 4)
    assert obj.valid_indices.tolist() == [2, 5] and obj.valid_indices.dtype == torch.int32
    obj.set_valid_indices([3, 0], 4)                      # usable again: the buffer is overwritten in place
    assert obj.valid_indices.tolist() == [3, 4]
    assert engine.flat_valid_indices([2, 1], 4, 8) == [2, 5]


@pytest.mark.parametrize("which", ["TrainStep", "Predictor"])
@pytest.mark.parametrize("per_clip,why", [([2, 7], "outside"), ([-1, 1], "outside"), ([5, 1], "twice"), ([2], "entries"), ([2, 1, 0], "entries")])
def test_set_valid_indices_refuses_bad_input(which, per_clip, why):
    """out of range (flat 11 of 8 frames; a negative frame), a duplicate ([5, 1] with T = 4 is row 5 twice), a wrong count -- and the buffer is untouched"""
    from lavt_hip import engine
    obj = _shell(getattr(engine, which), 2, 2, 4)
    with pytest.raises(ValueError, match=why):
        obj.set_valid_indices(per_clip, 4)
    assert obj.valid_indices.tolist() == [-1, -1]
    none = _shell(getattr(engine, which), 2, 2, 4)
    none.valid_indices = None
    with pytest.raises(ValueError, match="without"):
        none.set_valid_indices([2, 1], 4)


def test_new_parameters_are_keyword_only_and_default_to_todays_behaviour():
    from lavt_hip import ops
    from lavt_hip.engine import Predictor, TrainStep
    from lib import _utils
    ts = inspect.signature(TrainStep.__init__).parameters
    assert ts["loss"].kind is inspect.Parameter.KEYWORD_ONLY and ts["loss"].default == "ce"
    assert ts["valid_indices"].kind is inspect.Parameter.KEYWORD_ONLY and ts["valid_indices"].default is None
    pr = inspect.signature(Predictor.__init__).parameters
    assert pr["valid_indices"].kind is inspect.Parameter.KEYWORD_ONLY and pr["valid_indices"].default is None
    for fn in (_utils.fused_loss, _utils.fused_dice_loss):
        assert inspect.signature(fn).parameters["valid_indices"].default is None
    assert list(inspect.signature(_utils.fused_loss).parameters)[:3] == ["y", "target", "weight"]
    for fn in (ops.upsample_cross_entropy, ops.upsample_dice_loss):
        assert inspect.signature(fn).parameters["sel"].default is None
    for cls in (_utils.LAVT, _utils.LAVTOne, _utils.LAVTVideo):
        assert inspect.signature(cls.forward_lowres).parameters["frames"].default is None, cls.__name__
    assert callable(ops.gather_samples)


def test_train_step_refuses_an_unknown_loss_and_host_index_buffers():
    from lavt_hip.engine import TrainStep
    x, t = torch.zeros(2, 4, 3, 8, 8), torch.zeros(2, 8, 8, dtype=torch.int64)
    with pytest.raises(ValueError, match="mc_dice"):
        TrainStep(None, x, None, None, t, loss="dice_focal")
    with pytest.raises(RuntimeError, match="GPU memory only"):
        TrainStep(None, x, None, None, t, valid_indices=torch.zeros(2, dtype=torch.int32))
