"""Host-side checks of pair-list TRAIN batches (no GPU): the C ABI addition under the unchanged ABI version, what TrainStep(image_of=) and
set_image_of refuse before anything touches the GPU, what the models still refuse, and the torch restatement of lavt_gather_samples_bwd's contract
(tests/pair_train_ref.py, which the GPU test compares the kernel with) against index_add_ in fp64."""
import inspect
import os
import re
from types import SimpleNamespace

import pytest
import torch

from pair_train_ref import bounded_integer_samples, gather_bwd_index_add, gather_bwd_sequential, integer_samples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_gather_backward_is_declared_bound_and_exported():
    from lavt_hip import _capi
    header = open(os.path.join(ROOT, "include", "lavt_hip.h")).read()
    declared = set(re.findall(r"\b(lavt_[a-z0-9_]+)\s*\(", header))
    name = "lavt_gather_samples_bwd"
    assert name in declared, f"{name} is not declared in include/lavt_hip.h"
    assert name in _capi.EXPORTED, f"{name} is not bound in lavt_hip/_capi.py"
    assert hasattr(_capi._cdll, name), f"liblavt_hip.so does not export {name}"
    assert _capi.lib.lavt_abi_version() == _capi.EXPECTED_ABI == 7
    for cited in ("train.py:197-243", "data/dataset_refer_bert.py"):
        assert cited in header, f"the header does not cite {cited} for the pair gather's backward"


def _buffers(n=5, B=2):
    """CPU tensors of a pair-list batch: B images, n expressions, n targets"""
    return torch.zeros(B, 3, 8, 8), torch.zeros(n, 768, 20), torch.zeros(n, 20, 1), torch.zeros(n, 8, 8, dtype=torch.int64)


def test_train_step_refuses_bad_pair_buffers_before_anything_else():
    """the model is None: every refusal below comes before the first use of it (and of the GPU)"""
    from lavt_hip.engine import TrainStep
    x, l, m, t = _buffers()
    p = inspect.signature(TrainStep.__init__).parameters["image_of"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    with pytest.raises(RuntimeError, match="GPU memory only"):
        TrainStep(None, x, l, m, t, image_of=torch.zeros(5, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="GPU memory only"):
        TrainStep(None, x, l, m, t, image_of=[0, 1, 0, 1, 1])
    with pytest.raises(ValueError, match="int32"):
        TrainStep(None, x, l, m, t, image_of=torch.zeros(5, dtype=torch.int64))                     # dtype
    with pytest.raises(ValueError, match="image_of"):
        TrainStep(None, x, l, m, t, image_of=torch.zeros(5, 1, dtype=torch.int32))                  # shape
    with pytest.raises(ValueError, match="image_of"):
        TrainStep(None, x, l, m, t, image_of=torch.zeros(10, dtype=torch.int32)[::2])               # contiguity
    with pytest.raises(ValueError, match="per expression"):
        TrainStep(None, x, l, m, t, image_of=torch.zeros(4, dtype=torch.int32))                     # count against l
    with pytest.raises(ValueError, match="target"):
        TrainStep(None, x, l, m, t[:4], image_of=torch.zeros(5, dtype=torch.int32))                 # count against target
    with pytest.raises(ValueError, match="valid_indices"):
        TrainStep(None, x, l, m, t, image_of=torch.zeros(5, dtype=torch.int32), valid_indices=torch.zeros(2, dtype=torch.int32))


def _shell(cls, n, B):
    """an engine object with nothing but what set_image_of touches"""
    obj = cls.__new__(cls)
    obj.image_of = torch.full((n,), -7, dtype=torch.int32)
    obj.x = torch.zeros(B, 3, 8, 8)
    return obj


def test_set_image_of_writes_and_refuses():
    from lavt_hip.engine import Predictor, TrainStep
    step = _shell(TrainStep, 5, 2)
    step.set_image_of([1, 0, 1, 1, 0])
    assert step.image_of.tolist() == [1, 0, 1, 1, 0] and step.image_of.dtype == torch.int32
    for bad, why in (([1, -1, 1, 1, 0], "empty slots"), ([1, 2, 1, 1, 0], "images of the batch"), ([1, 0, 1, 1], "entries"), ([1, 0, 1, 1, 0, 0], "entries")):
        with pytest.raises(ValueError, match=why):
            step.set_image_of(bad)
        assert step.image_of.tolist() == [1, 0, 1, 1, 0], "a refused list is not written"
    none = _shell(TrainStep, 5, 2)
    none.image_of = None
    with pytest.raises(ValueError, match="without"):
        none.set_image_of([0] * 5)
    pred = _shell(Predictor, 5, 2)          # the shared host code: a Predictor keeps accepting -1, and only -1, outside the images
    pred.set_image_of([1, -1, 0, 0, -1])
    assert pred.image_of.tolist() == [1, -1, 0, 0, -1]
    for bad in ([1, -2, 0, 0, 0], [1, 2, 0, 0, 0], [0, 0]):
        with pytest.raises(ValueError):
            pred.set_image_of(bad)


def test_the_video_model_and_expand_are_still_refused_in_training():
    from lib import _utils
    from lib.backbone import MultiModalSwinTransformer
    video = _utils.LAVTVideo.__new__(_utils.LAVTVideo)
    torch.nn.Module.__init__(video)
    with pytest.raises(NotImplementedError, match="image_of"):
        video.forward_lowres(None, None, None, image_of=torch.zeros(2, dtype=torch.int32))
    bb = MultiModalSwinTransformer(embed_dim=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8], window_size=7, drop_path_rate=0.0, args=SimpleNamespace()).train()
    x, l, m = torch.zeros(2, 3, 64, 64), torch.zeros(4, 768, 20), torch.zeros(4, 20, 1)
    with pytest.raises(RuntimeError, match="expand > 1"):
        bb(x, l, m, expand=2)
    with pytest.raises(ValueError, match="expand"):
        bb(x, l, m, expand=2, image_of=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="language batch"):
        bb(x, l, m, image_of=torch.zeros(5, dtype=torch.int32))
    with pytest.raises(ValueError, match="expand"):
        _utils._check_image_of(2, None, torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="frames"):
        _utils._check_image_of(1, torch.zeros(1, dtype=torch.int32), torch.zeros(4, dtype=torch.int32))


def test_fingerprint_tells_pair_runs_from_plain_runs():
    from lavt_hip.checkpoint import CONFIG_FIELDS, compare_fingerprints
    plain = {f: 0 for f in CONFIG_FIELDS}
    plain["param_groups"] = []
    pair = dict(plain, pair_slots=6)
    compare_fingerprints(plain, dict(plain))
    compare_fingerprints(pair, dict(pair))
    for saved, current in ((plain, pair), (pair, plain), (pair, dict(plain, pair_slots=8))):
        with pytest.raises(ValueError, match="pair_slots"):
            compare_fingerprints(saved, current)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_the_restated_contract_equals_index_add(dtype):
    """integer data: the sequential fp32 sum with one rounding IS the fp64 index_add_; image 1 (nobody names it) is zero, -1 and 7 add nothing"""
    B, sel = 3, [2, 0, 2, -1, 2, 7, 0]
    for per in (1, 7, 1568):
        dy = integer_samples(per, len(sel), per, dtype)
        got = gather_bwd_sequential(dy, sel, B)
        assert got.dtype == dtype and torch.equal(got.double(), gather_bwd_index_add(dy, sel, B))
        assert not got[1].any()
        assert torch.equal(got[0].double(), (dy[1].double() + dy[6].double())) and got[2].abs().sum() > 0
    sel = [j % 2 for j in range(4001)]
    dy = bounded_integer_samples(3, sel, 2, 4, dtype)
    assert float(dy.abs().max()) <= 8 and torch.equal(gather_bwd_sequential(dy, sel, 2).double(), gather_bwd_index_add(dy, sel, 2))


def test_the_restated_order_is_sequential_and_rounds_once():
    """random fp32 data: ascending-j fp32 adds differ from other orders in the last bits (the order is part of the contract), and the bf16 result is the
    fp32 sum of the bf16 inputs rounded once -- not a bf16 running sum"""
    g = torch.Generator("cpu").manual_seed(11)
    dy = torch.randn(6, 1568, generator=g)
    sel = [1, 0, 1, 1, 0, 1]
    got = gather_bwd_sequential(dy, sel, 2)
    want1 = ((dy[0] + dy[2]) + dy[3]) + dy[5]
    assert torch.equal(got[1], want1) and torch.equal(got[0], dy[1] + dy[4])
    assert not torch.equal(got[1], dy[0] + (dy[2] + (dy[3] + dy[5]))), "1568 random sums: some other order differs somewhere"
    b = dy.bfloat16()
    got16 = gather_bwd_sequential(b, sel, 2)
    assert torch.equal(got16[1], (((b[0].float() + b[2].float()) + b[3].float()) + b[5].float()).bfloat16())
    running = ((b[0] + b[2]) + b[3]) + b[5]
    assert not torch.equal(got16[1], running), "a bf16 running sum rounds three times and differs somewhere"
