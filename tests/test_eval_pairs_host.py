"""Pair-list evaluation batches and the device-side evaluation meter, the host side (no GPU): the three new symbols and their bindings, the meter
block's documented layout against its numpy restatement, the new keywords, forward_lowres's refusals, and the snapshot decoder of
lavt_hip.metrics.DeviceEvalMeter against EvalMeter fed the same (I, U) list.  Predictor.set_image_of has no GPU-free constructor path: it is tested
in test_gpu_eval_pairs.py."""
import ctypes as C
import inspect
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, i32 = C.c_void_p, C.c_int32
NEW = {
    "lavt_upsample_mask_pairs": (["dtype", "x", "B", "Hi", "Wi", "Hm", "Wm", "Ho", "Wo", "mask", "target", "iu", "image_of", "n_images", "stream"],
                                 [i32, vp] + [i32] * 7 + [vp, vp, vp, vp, i32, vp]),
    "lavt_eval_meter_bytes": (["capacity"], [i32]),
    "lavt_eval_meter_append": (["iu", "image_of", "n_images", "n", "block", "capacity", "stream"], [vp, vp, i32, i32, vp, i32, vp]),
}


@pytest.mark.parametrize("name", sorted(NEW))
def test_symbols_are_declared_bound_and_exported(name):
    from lavt_hip import _capi
    header = open(os.path.join(ROOT, "include", "lavt_hip.h")).read()
    decl = re.search(r"\b(int|int64_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert decl, f"{name} is not declared in include/lavt_hip.h"
    args = [re.sub(r"/\*.*?\*/", "", a).strip() for a in decl.group(2).split(",")]
    names, ctypes_ = NEW[name]
    assert [a.split()[-1].lstrip("*") for a in args] == names
    assert name in _capi.EXPORTED and hasattr(_capi._cdll, name)
    assert _capi._PROTOTYPES[name] == ctypes_
    assert getattr(_capi._cdll, name).restype is (C.c_int64 if decl.group(1) == "int64_t" else C.c_int)
    assert _capi.lib.lavt_abi_version() == _capi.EXPECTED_ABI == 7


def test_the_pairs_entry_point_is_lavt_upsample_mask_with_two_more_arguments():
    from lavt_hip import _capi
    assert _capi._PROTOTYPES["lavt_upsample_mask_pairs"] == _capi._PROTOTYPES["lavt_upsample_mask"][:-1] + [vp, i32, vp]


def test_block_size_and_layout_are_the_documented_ones():
    from lavt_hip import _capi, metrics as M
    header = open(os.path.join(ROOT, "include", "lavt_hip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define (LAVT_EVAL_METER_\w+) (\w+)", header)}
    assert defs == {"LAVT_EVAL_METER_HEADER_DOUBLES": M.EVAL_HEADER_DOUBLES, "LAVT_EVAL_METER_RECORD_BYTES": M.EVAL_RECORD_BYTES}
    for cap in (1, 8, 4096, 100000):
        assert _capi.lib.lavt_eval_meter_bytes(cap) == M.eval_meter_bytes(cap) == 8 * 16 + 16 * cap
    assert _capi.lib.lavt_eval_meter_bytes(0) == 0 and _capi.lib.lavt_eval_meter_bytes(-3) == 0
    assert [(n, M.EVAL_RECORD_DTYPE.fields[n][1]) for n in M.EVAL_RECORD_DTYPE.names] == [("I", 0), ("U", 4), ("sample", 8)]
    assert (M.E_CAPACITY, M.E_HOLD, M.E_N, M.E_COUNT, M.E_IOU_SUM, M.E_CUM_I, M.E_CUM_U, M.E_CORRECT0) == tuple(range(8))
    assert M.E_CORRECT0 + len(M.THRESHOLDS) <= M.EVAL_HEADER_DOUBLES
    # the header's list of words names them in this order
    doc = header[header.index("Evaluation meter (csrc/meters.hip"):header.index("#define LAVT_EVAL_METER_HEADER_DOUBLES")]
    for text in ("[0] capacity", "[1] hold", "[2] n:", "[3] count", "[4] sum of iou", "[5] cumulative I", "[6] cumulative U", "[7..11] correct",
                 "offset 0 int32 I | 4 int32 U | 8 int64 running sample number"):
        assert text in doc, text


def test_the_new_keywords_default_to_none():
    from lavt_hip import ops
    from lavt_hip.engine import Predictor
    from lavt_hip.metrics import DeviceEvalMeter
    from lib import _utils
    from lib.backbone import MultiModalSwinTransformer
    for fn, names in ((MultiModalSwinTransformer.forward, ("image_of",)), (_utils.LAVT.forward_lowres, ("image_of",)), (_utils.LAVTOne.forward_lowres, ("image_of",)),
                      (_utils.LAVTVideo.forward_lowres, ("image_of",)), (ops.upsample_mask, ("image_of", "n_images")), (Predictor.__init__, ("image_of", "meter"))):
        ps = inspect.signature(fn).parameters
        for name in names:
            assert ps[name].default is None, (fn.__qualname__, name)
    for name in ("image_of", "meter"):
        assert inspect.signature(Predictor.__init__).parameters[name].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(MultiModalSwinTransformer.forward).parameters["expand"].default == 1
    for name in ("set_image_of", "make_meter", "attach_meter"):
        assert callable(getattr(Predictor, name))
    for name in ("poll", "read", "reset", "state_dict", "load_state_dict", "pause", "resume", "append"):
        assert callable(getattr(DeviceEvalMeter, name))


def test_the_meter_polls_with_the_training_meters_mechanism():
    """one poll / read, not two: both meters take them from the same base class"""
    from lavt_hip.meters import DeviceBlock, TrainMeters
    from lavt_hip.metrics import DeviceEvalMeter
    for name in ("poll", "read", "_collect", "_enqueue", "pause", "resume"):
        assert getattr(DeviceEvalMeter, name) is getattr(TrainMeters, name) is getattr(DeviceBlock, name), name


def _tiny_model():
    from lib._utils import LAVT
    from lib.backbone import MultiModalSwinTransformer
    from lib.mask_predictor import SimpleDecoding
    args = SimpleNamespace()
    bb = MultiModalSwinTransformer(embed_dim=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8], window_size=7, drop_path_rate=0.0, args=args)
    return LAVT(bb, SimpleDecoding(256, args))


def test_forward_lowres_refuses_image_of_with_expand_and_with_frames():
    model = _tiny_model().eval()
    x, l, m = torch.zeros(2, 3, 64, 64), torch.zeros(4, 768, 20), torch.ones(4, 20, 1)
    pairs = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="expand"):
        model.forward_lowres(x, l, m, folded=True, expand=2, image_of=pairs)
    with pytest.raises(ValueError, match="frames"):
        model.forward_lowres(x, l, m, folded=True, frames=torch.zeros(1, dtype=torch.int32), image_of=pairs)
    with pytest.raises(ValueError, match="expand"):
        model.backbone(x, l, m, expand=2, image_of=pairs)


def test_video_forward_lowres_refuses_image_of():
    from lib._utils import LAVTVideo
    model = LAVTVideo.__new__(LAVTVideo)
    torch.nn.Module.__init__(model)
    model.eval()
    with pytest.raises(NotImplementedError, match="image_of"):
        model.forward_lowres(torch.zeros(1, 2, 3, 64, 64), torch.zeros(1, 20, dtype=torch.long), torch.ones(1, 20), folded=True, image_of=torch.zeros(1, dtype=torch.int32))


IU = [(0, 0), (0, 9), (5, 5), (1, 2), (3, 5), (7, 10), (4, 5), (9, 10), (16777217, 33554433), (2147483646, 2147483647), (1073741824, 2147483647), (12, 57)]


@pytest.mark.parametrize("capacity", [5, 64])
def test_snapshot_decoder_equals_eval_meter_on_a_synthetic_block(capacity):
    """a block written by the host restatement of lavt_eval_meter_append (reference_block), decoded by EvalSnapshot, against EvalMeter fed the same
    list: counts exact, the text equal, the mean within n * 2^-53 * sum(iou) (a sequential fp64 sum against numpy's pairwise one)"""
    from lavt_hip.metrics import EvalMeter, EvalSnapshot, reference_block
    live = [True] * len(IU)
    live[2] = live[7] = False
    snap = reference_block(IU, capacity, live=live)
    kept = [r for r, f in zip(IU, live) if f]
    meter = EvalMeter()
    meter.update(kept)
    assert (snap.count, snap.n, snap.cum_I, snap.cum_U, snap.correct) == (meter.count, len(kept), meter.cum_I, meter.cum_U, [int(c) for c in meter.correct])
    assert snap.cum_U > 2 ** 32
    got, want = snap.summary(), meter.summary()
    assert list(got) == list(want)
    bound = len(kept) * 2.0 ** -53 * sum(meter.ious) / len(kept) * 100.0
    assert abs(got["mean_iou"] - want["mean_iou"]) <= bound
    for k in want:
        if k != "mean_iou":
            assert got[k] == want[k], k
    assert str(snap) == str(meter)
    recs = snap.records()
    tail = kept[-min(capacity, len(kept)):]
    assert [(int(r["I"]), int(r["U"])) for r in recs] == tail
    assert [int(r["sample"]) for r in recs] == list(range(len(kept) - len(tail), len(kept)))
    # the state dict is the block: through it the snapshot comes back
    sd = snap.state_dict()
    raw = np.concatenate([sd["header"].numpy().view(np.uint8), sd["ring"].numpy()])
    assert str(EvalSnapshot(raw, sd["capacity"])) == str(snap)
    with pytest.raises(RuntimeError, match="no samples"):
        reference_block([], 4).summary()


def test_counts_beyond_fp32_are_kept_as_integers():
    """(16777217, 33554433): neither count is an fp32 number (both round to a power of two and the quotient to exactly .5); the block keeps the
    integers and divides them in fp64, as EvalMeter does"""
    from lavt_hip.metrics import EvalMeter, reference_block
    I, U = 16777217, 33554433
    assert float(np.float32(I) / np.float32(U)) == 0.5 < I / U
    snap = reference_block([(I, U)], 2)
    meter = EvalMeter()
    meter.update([(I, U)])
    assert snap.correct == [int(c) for c in meter.correct] == [1, 0, 0, 0, 0]
    assert (int(snap.records()[0]["I"]), int(snap.records()[0]["U"])) == (I, U) and snap.summary() == meter.summary()
