"""Host-side checks of the inference path (no GPU): the C ABI additions, EvalMeter against a restatement of the reference's test loop
(test.py:84-108), and the refusals of lavt_hip.engine.Predictor."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lavt_conv_bn_fold", "lavt_splitk_reduce_epi", "lavt_upsample_mask")


def test_header_declares_and_library_exports_the_inference_entry_points():
    from lavt_hip import _capi
    header = open(os.path.join(ROOT, "include", "lavt_hip.h")).read()
    declared = set(re.findall(r"\b(lavt_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared, f"include/lavt_hip.h does not declare {name}"
        assert name in _capi.EXPORTED
        assert hasattr(_capi._cdll, name), f"liblavt_hip.so does not export {name}"
    assert _capi.lib.lavt_abi_version() == _capi.EXPECTED_ABI == 7
    assert "infer.hip" in open(os.path.join(ROOT, "lavt-rs_amd", "csrc", "Makefile")).read()


def _reference_loop(I, U):
    """test.py:84-108 restated: per-sample IoU (U == 0 -> 0), cumulative I / U, precision thresholds with >="""
    eval_seg_iou_list = [.5, .6, .7, .8, .9]
    cum_I, cum_U = 0, 0
    seg_correct = np.zeros(len(eval_seg_iou_list), dtype=np.int32)
    seg_total = 0
    mean_IoU = []
    for i, u in zip(I, U):
        if u == 0:
            this_iou = 0.0
        else:
            this_iou = i * 1.0 / u
        mean_IoU.append(this_iou)
        cum_I += i
        cum_U += u
        for n in range(len(eval_seg_iou_list)):
            seg_correct[n] += (this_iou >= eval_seg_iou_list[n])
        seg_total += 1
    out = {"mean_iou": np.mean(np.array(mean_IoU)) * 100.}
    for n, th in enumerate(eval_seg_iou_list):
        out[f"precision@{th}"] = seg_correct[n] * 100. / seg_total
    out["overall_iou"] = cum_I * 100. / cum_U
    return out


def test_eval_meter_matches_the_reference_loop():
    from lavt_hip.metrics import EvalMeter
    rng = np.random.default_rng(7)
    U = rng.integers(1, 50000, size=200)
    I = (U * rng.random(200)).astype(np.int64)
    # IoUs exactly on every threshold (>= counts them), one empty union, one perfect sample
    I = np.concatenate([I, [1, 3, 7, 4, 9, 0, 123]])
    U = np.concatenate([U, [2, 5, 10, 5, 10, 0, 123]])
    ref = _reference_loop(I.tolist(), U.tolist())
    meter = EvalMeter()
    iu = np.stack([I, U], 1)
    meter.update(torch.as_tensor(iu[:100], dtype=torch.int32))          # batches of per-sample counts, as Predictor.iu
    meter.update(iu[100:150])
    for row in iu[150:]:
        meter.update(row.tolist())
    got = meter.summary()
    assert set(got) == set(ref)
    for k in ref:
        assert got[k] == pytest.approx(ref[k], rel=1e-12, abs=1e-12), k
    # the threshold samples were counted with >=
    only = EvalMeter()
    only.update([[1, 2], [3, 5], [7, 10], [4, 5], [9, 10], [0, 0]])
    s = only.summary()
    assert [s[f"precision@{t}"] for t in (0.5, 0.6, 0.7, 0.8, 0.9)] == pytest.approx([500 / 6, 400 / 6, 300 / 6, 200 / 6, 100 / 6])
    assert "overall IoU" in str(only)


def _tiny_model():
    from lib._utils import LAVT
    from lib.backbone import MultiModalSwinTransformer
    from lib.mask_predictor import SimpleDecoding
    args = SimpleNamespace()
    bb = MultiModalSwinTransformer(embed_dim=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8], window_size=7, drop_path_rate=0.0, args=args)
    return LAVT(bb, SimpleDecoding(256, args))


def test_predictor_refuses_training_mode_and_cpu_tensors():
    from lavt_hip.engine import Predictor
    model = _tiny_model()
    x, l, m = torch.zeros(1, 3, 64, 64), torch.zeros(1, 768, 20), torch.ones(1, 20, 1)
    with pytest.raises(RuntimeError, match="training mode"):
        Predictor(model.train(), x, l, m)
    with pytest.raises(RuntimeError, match="GPU memory only"):
        Predictor(model.eval(), x, l, m)
    with pytest.raises(RuntimeError, match="eval mode"):
        model.train().classifier.forward_folded(None, None, None, None)


def test_forward_lowres_signatures_and_video_expand():
    import inspect
    from lib import _utils
    from lib.backbone import MultiModalSwinTransformer
    from lib.video_swin_transformer import MultiModalSwinTransformer3D
    for cls in (_utils.LAVT, _utils.LAVTOne, _utils.LAVTVideo):
        ps = inspect.signature(cls.forward_lowres).parameters
        assert ps["folded"].default is False and ps["expand"].default == 1, cls.__name__
    assert inspect.signature(MultiModalSwinTransformer.forward).parameters["expand"].default == 1
    assert inspect.signature(MultiModalSwinTransformer3D.forward).parameters["expand"].default == 1


def test_stage_halves_are_methods_not_shadowed_by_attributes():
    """MMBasicLayer keeps option strings as instance attributes (`fuse`, `version`): the two halves of its forward must stay callable beside them"""
    layer = _tiny_model().backbone.layers[0]
    assert callable(layer.run_blocks) and callable(layer.fuse_language)
    assert layer.fuse == "default"
