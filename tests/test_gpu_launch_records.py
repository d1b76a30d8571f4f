"""The launch sequences ops.py issues are the ones the parent commit issued.  Every scenario below runs under the in-process profiler (K.prof) and
yields one row [entry point, scope label, note["shape"] or None] per LAUNCH (an entry point whose last argument is the stream: the host-side size
queries -- *_ws, *_blocks, *_pieces -- are not launches and are left out).  tests/golden/launch_records_parent.json holds the rows of `record_all()`
run on the parent commit's tree; the test requires the same number of rows, the same entry point and scope in every row, and the same shape wherever
the fixture has one (a launch that carried no note on the parent may carry one now, never the other way round).

The model builders and inputs are those of test_gpu_deterministic.py; the eager steps have the shape of its eager_step_launches()."""
import ctypes as C
import json
import os

import pytest
import torch
import torch.nn.functional as F

from lavt_hip.detweights import det_inputs
from test_gpu_deterministic import _micro2d, _video

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_records_parent.json")


def _rows(recs):
    from lavt_hip import _capi as K
    out = []
    for name, scope, note, _ in recs:
        args = K._PROTOTYPES.get(name)
        if args and args[-1] is C.c_void_p:
            out.append([name, scope, note["shape"] if note else None])
    return out


def _record(fn):
    """fn twice to warm (compute-dtype weight copies, arenas, descriptor tables), the third call recorded"""
    from lavt_hip import _capi as K
    fn()
    fn()
    K.prof.start()
    try:
        fn()
    finally:
        recs = K.prof.stop()
    return _rows(recs)


def _eager_step(build, inputs, dtype, **step_kw):
    """one eager TrainStep iteration (fused loss, private context) after two warm-up iterations"""
    import lavt_hip
    from lavt_hip import _capi as K
    from lavt_hip import ops
    from lavt_hip.engine import TrainStep
    with lavt_hip.use_dtype(dtype):
        step = TrainStep(build(), *inputs, context=ops.StepContext(), use_graph=False, **step_kw)
        step.warmup_and_capture(eager_iters=2)
        K.prof.start()
        try:
            step.step()
        finally:
            recs = K.prof.stop()
    return _rows(recs)


def _step2d(loss, deterministic, dtype=torch.bfloat16):
    x, l, m, tgt = (t.to(DEV) for t in det_inputs(2, 64, 20, seed=5))
    vi = torch.tensor([1], dtype=torch.int32, device=DEV)
    return _eager_step(_micro2d, (x, l, m, tgt[[1]].contiguous()), dtype, loss=loss, valid_indices=vi, deterministic=deterministic)


def _step2d_fp8(deterministic):
    from lavt_hip import ops
    saved = ops._FP8_CONV_MIN_TILES
    ops._FP8_CONV_MIN_TILES = 0          # the micro decoder takes the e4m3 convolutions (test_gpu_deterministic's fp8 test)
    try:
        return _step2d("ce", deterministic, dtype="fp8")
    finally:
        ops._FP8_CONV_MIN_TILES = saved


def _step_video(deterministic):
    import lavt_hip
    with lavt_hip.use_dtype(torch.bfloat16):
        model, frames, ids, am, tgt = _video("pwam")
        vi = torch.tensor([2, 5], dtype=torch.int32, device=DEV)
        return _eager_step(lambda: model, (frames, ids, am, tgt[[2, 5]].contiguous()), torch.bfloat16, valid_indices=vi, deterministic=deterministic)


def _plain(dtype, deterministic):
    """forward + cross entropy + backward of the micro 2-D model with no step harness: no sinks, so the immediate LayerNorm and table-gradient paths"""
    import lavt_hip
    from lavt_hip import ops
    x, l, m, tgt = (t.to(DEV) for t in det_inputs(2, 64, 20, seed=5))
    w = torch.tensor([0.9, 1.1], device=DEV)
    with lavt_hip.use_dtype(dtype), ops.use_context(ops.StepContext(deterministic=deterministic)):
        model = _micro2d()

        def run():
            model.zero_grad(set_to_none=True)
            F.cross_entropy(model(x, l, m).float(), tgt, weight=w).backward()
        return _record(run)


CONV_SHAPES = {          # (B, H, W, C1, C2, Cout)
    "cat320": (1, 24, 24, 256, 64, 512),          # data gradient per source; the forward's reduction (9 x 320) is too short to split
    "cat512": (1, 24, 24, 256, 256, 512),         # the forward splits too
    "one512": (1, 24, 24, 512, 0, 512),           # single-source data gradient
}
# what ops._conv_split answers for these shapes with _CONV_KC_SPLITS "auto" / "0": forward, then the data gradient onto each source -- worked out from
# _conv_split / _kc_pieces: 576 rows = 5 row tiles of 128; forward onto 512 channels = 20 tiles, 8 channel blocks -> 8 pieces (160 workgroups <= 256),
# 5 blocks of 320 channels: 9 x 320 = 2880 < 4096, not split; data gradient onto 256 / 64 / 512 channels = 10 / 5 / 20 tiles, 8 blocks -> 8 pieces
CONV_SPLITS = {
    "cat320": {"auto": [(0, False), (8, True), (8, True)], "0": [(0, False), (3, False), (3, False)]},
    "cat512": {"auto": [(8, True), (8, True), (8, True)], "0": [(3, False), (3, False), (3, False)]},
    "one512": {"auto": [(8, True), (8, True)], "0": [(3, False), (3, False)]},
}


def _conv_split_answers(shape):
    from lavt_hip import ops
    B, H, W, C1, C2, Cout = shape
    M, bf = B * H * W, torch.bfloat16
    fwd = ops._conv_split(bf, M, Cout, C1 + C2, C1, C2, 9, None, 0)
    return [fwd] + [ops._conv_split(bf, M, Cn, Cout, Cout, 0, 9, None, 0) for Cn in ((C1, C2) if C2 else (C1,))]


def _with_kc(setting, fn):
    from lavt_hip import ops
    saved = ops._CONV_KC_SPLITS
    ops._CONV_KC_SPLITS = setting
    try:
        return fn()
    finally:
        ops._CONV_KC_SPLITS = saved


def _conv_inputs(shape):
    from test_gpu_ops import rnd
    B, H, W, C1, C2, Cout = shape
    M, Cin = B * H * W, C1 + C2
    x1 = rnd(M, C1, seed=1).to(DEV).to(torch.bfloat16)
    x2 = rnd(M, C2, seed=2).to(DEV).to(torch.bfloat16) if C2 else None
    w = rnd(Cout, Cin, 3, 3, seed=3, scale=(9 * Cin) ** -0.5).to(DEV)
    return x1, x2, w, rnd(M, Cout, seed=4).to(DEV).to(torch.bfloat16)


def _conv(shape, setting):
    import lavt_hip
    from lavt_hip import ops
    B, H, W = shape[:3]
    x1, x2, w, go = _conv_inputs(shape)

    def run():
        a = x1.clone().requires_grad_(True)
        b = x2.clone().requires_grad_(True) if x2 is not None else None
        p = torch.nn.Parameter(w.clone())
        ops.conv3x3(a, b, p, B, H, W).backward(go)
    with lavt_hip.use_dtype(torch.bfloat16), ops.use_context(ops.StepContext()):
        return _with_kc(setting, lambda: _record(run))


def _conv_folded(shape, setting):
    import lavt_hip
    from lavt_hip import ops
    B, H, W, C1, C2, Cout = shape
    x1, x2, w, _ = _conv_inputs(shape)
    conv = torch.nn.Conv2d(C1 + C2, Cout, 3, padding=1, bias=False).to(DEV)
    bn = torch.nn.BatchNorm2d(Cout).to(DEV).eval()
    with torch.no_grad():
        conv.weight.copy_(w)
    with lavt_hip.use_dtype(torch.bfloat16), ops.use_context(ops.StepContext()), torch.no_grad():
        return _with_kc(setting, lambda: _record(lambda: ops.conv3x3_bn_relu_folded(x1, x2, conv, bn, B, H, W)))


SCENARIOS = {
    "step2d-ce": lambda: _step2d("ce", None),
    "step2d-mc_dice": lambda: _step2d("mc_dice", None),
    "step2d-dice_boundary": lambda: _step2d("dice_boundary", None),
    "step2d-ce-det": lambda: _step2d("ce", True),
    "step2d-fp8": lambda: _step2d_fp8(None),
    "step2d-fp8-det": lambda: _step2d_fp8(True),
    "video-pwam": lambda: _step_video(None),
    "video-pwam-det": lambda: _step_video(True),
    "plain-bf16": lambda: _plain(torch.bfloat16, False),
    "plain-bf16-det": lambda: _plain(torch.bfloat16, True),
    "plain-fp32": lambda: _plain(torch.float32, False),
    "plain-fp32-det": lambda: _plain(torch.float32, True),
}
for _s in CONV_SHAPES:
    for _k in ("auto", "0"):
        SCENARIOS[f"conv-{_s}-kc{_k}"] = lambda s=_s, k=_k: _conv(CONV_SHAPES[s], k)
        if _s != "one512":
            SCENARIOS[f"folded-{_s}-kc{_k}"] = lambda s=_s, k=_k: _conv_folded(CONV_SHAPES[s], k)


def record_all():
    """{scenario: rows}: what the fixture holds, written by this function on the parent commit"""
    return {name: fn() for name, fn in SCENARIOS.items()}


@pytest.mark.parametrize("name", sorted(CONV_SHAPES))
@pytest.mark.parametrize("setting", ["auto", "0"])
def test_conv_shapes_split_as_recorded(name, setting):
    """the convolution scenarios cover the split contractions only while _conv_split cuts these shapes: a shape that stops splitting fails here"""
    assert _with_kc(setting, lambda: _conv_split_answers(CONV_SHAPES[name])) == CONV_SPLITS[name][setting]


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_launches_are_what_the_parent_commit_launched(name, monkeypatch):
    monkeypatch.delenv("LAVT_DETERMINISTIC", raising=False)
    want = json.load(open(FIXTURE))[name]
    got = SCENARIOS[name]()
    assert len(want) > 0
    assert [r[:2] for r in got] == [r[:2] for r in want], next(((i, a, b) for i, (a, b) in enumerate(zip(got, want)) if a[:2] != b[:2]), (len(got), len(want)))
    bad = [(i, a, b) for i, (a, b) in enumerate(zip(got, want)) if b[2] is not None and a[2] != b[2]]
    assert not bad, bad[:4]
