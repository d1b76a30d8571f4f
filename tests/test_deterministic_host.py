"""Host-side checks of deterministic mode (no GPU): the interface (LAVT_DETERMINISTIC, ops.StepContext(deterministic=), TrainStep(deterministic=)), the
routing choosers as pure functions, the refusals, and the audit that keeps the "Deterministic mode" table of DESIGN.md and the `atomicAdd` lines of
lavt-rs_amd/csrc in step."""
import inspect
import itertools
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lavt-rs_amd", "csrc")


def test_interface(monkeypatch):
    from lavt_hip import ops, runtime
    from lavt_hip.engine import TrainStep
    for fn in (TrainStep.__init__, ops.StepContext.__init__):
        p = inspect.signature(fn).parameters["deterministic"]
        assert p.default is None
    assert inspect.signature(TrainStep.__init__).parameters["deterministic"].kind is inspect.Parameter.KEYWORD_ONLY
    monkeypatch.delenv("LAVT_DETERMINISTIC", raising=False)
    assert runtime.deterministic() is False and ops.StepContext().deterministic is False
    monkeypatch.setenv("LAVT_DETERMINISTIC", "1")
    assert runtime.deterministic() is True and ops.StepContext().deterministic is True
    assert ops.StepContext(deterministic=False).deterministic is False
    monkeypatch.setenv("LAVT_DETERMINISTIC", "0")
    assert runtime.deterministic() is False and ops.StepContext(deterministic=True).deterministic is True
    # the helper every site asks follows the CURRENT context
    assert ops.deterministic() is ops.current_context().deterministic
    with ops.StepContext(deterministic=True):
        assert ops.deterministic() is True
        with ops.StepContext(deterministic=False):
            assert ops.deterministic() is False
        assert ops.deterministic() is True


def test_new_entry_points_are_bound_under_the_unchanged_abi_version():
    from lavt_hip import _capi
    new = ("lavt_gemm_tn_v2_eligible", "lavt_reduce_partials_det_stage", "lavt_reduce_partials_det", "lavt_reduce_partials_multi_det", "lavt_norm_bwd_stats_det",
           "lavt_window_attn_bwd_det_ws", "lavt_window_attn_bwd_det", "lavt_bert_embed_bwd_det")
    header = open(os.path.join(ROOT, "include", "lavt_hip.h")).read()
    for name in new:
        assert name in _capi._PROTOTYPES and re.search(r"\b%s\s*\(" % name, header), name
    assert _capi.lib.lavt_abi_version() == _capi.EXPECTED_ABI == 7          # new symbols only: no existing prototype or struct changed
    # the stage of the two-level reduction holds the most row slices the atomic form cuts (16), W floats each
    assert _capi.lib.lavt_reduce_partials_det_stage(192) == 16 * 192
    # exact-fp32 attention: one dS slab per (window, head) + the dense sum over the windows
    assert _capi.lib.lavt_window_attn_bwd_det_ws(_capi.F32, 72, 49, 2, 64, 1, 7, 7) == (72 + 1) * 2 * 49 * 64
    assert _capi.lib.lavt_window_attn_bwd_det_ws(_capi.BF16, 72, 49, 2, 64, 1, 7, 7) == _capi.lib.lavt_window_attn_bwd_ws(_capi.BF16, 72, 49, 2, 64, 1, 7, 7)


def test_weight_gradient_plan_never_splits_through_atomics():
    """ops.tn_plan is a pure function.  Deterministic mode: every plan either lends partial-tile scratch (the pieces are stored and added in index order) or
    forbids the split (split_k = 1), and never declares a zeroed C that a grouped launch may cut into atomic pieces (split_k = -1).  Default mode: the
    plan is what gemm_tn computed before the mode existed."""
    from lavt_hip.ops import _TN_PARTIALS_MAX, _TN_PARTIALS_MINK, tn_plan
    cases = itertools.product((torch.float32, torch.bfloat16), (64, 1024, _TN_PARTIALS_MINK, 28800), (1, 4), (None, (12, 12, 64)), (False, True), (False, True),
                              (0, 4160, _TN_PARTIALS_MAX, _TN_PARTIALS_MAX + 1), (False, True))
    for dtype, Kd, batch, conv, deferred, v2, need, enabled in cases:
        floats, split_k = tn_plan(dtype, Kd, batch, conv, deferred, v2, need, True, enabled)
        assert (floats == need and floats > 0 and split_k == 0) or (floats == 0 and split_k == 1), (dtype, Kd, batch, conv, deferred, v2, need, enabled)
        if floats:          # only a launch the LDS-DMA kernels take honours the scratch
            assert dtype == torch.bfloat16 and v2 and conv is None and enabled and need <= _TN_PARTIALS_MAX and (batch == 1 or not deferred)
        # the parent's rule, literally (ops.gemm_tn before tn_plan)
        floats0, split0 = tn_plan(dtype, Kd, batch, conv, deferred, v2, need, False, enabled)
        lend0 = (dtype == torch.bfloat16 and conv is None and (batch == 1 or not deferred) and Kd >= (_TN_PARTIALS_MINK if batch == 1 else 128) and enabled
                 and 0 < need <= (16 << 20))
        assert floats0 == (need if lend0 else 0) and split0 == (-1 if deferred else 0)
    # fp32 and short bf16 reductions get no scratch today: the two cases the GPU test runs
    assert tn_plan(torch.float32, 1000, 1, None, False, False, 4160, False) == (0, 0) and tn_plan(torch.float32, 1000, 1, None, False, False, 4160, True) == (0, 1)
    assert tn_plan(torch.bfloat16, 1024, 1, None, False, True, 8320, False) == (0, 0) and tn_plan(torch.bfloat16, 1024, 1, None, False, True, 8320, True) == (8320, 0)


def test_reduce_partials_plan_never_names_atomic_slices():
    """ops.reduce_partials_plan is a pure function.  Deterministic mode: for every caller and every row-block count the plan is the *_det form, names no
    atomic slice and lends a stage of at least 16 x W floats (what lavt_reduce_partials_det_stage asks for; the multi-set launch: eight slices of 128
    columns per column block).  Default mode: the entry point the parent called, whose reduction cuts reduce_partials_grid's slices (norm.hip) -- atomic
    from 48 row blocks on."""
    from lavt_hip import _capi
    from lavt_hip.ops import _RP_DET_SLICES, reduce_partials_plan, reduce_partials_slices
    assert [reduce_partials_slices(n) for n in (1, 47, 48, 127, 128, 383, 384, 767, 768, 2048)] == [1, 1, 2, 2, 4, 4, 8, 8, 16, 16]
    grid = re.search(r"reduce_partials_grid\(int nblk, int W\) \{ return dim3\(cdiv\(W, 32\), (.*?)\); \}", open(os.path.join(CSRC, "norm.hip")).read()).group(1)
    assert grid == "nblk >= 768 ? 16 : nblk >= 384 ? 8 : nblk >= 128 ? 4 : (nblk >= 48 ? 2 : 1)"          # the rule reduce_partials_slices restates
    parent = {"layernorm": "lavt_layernorm_bwd", "layernorm_xn": "lavt_layernorm_bwd_xn", "norm_stats": "lavt_norm_bwd_stats", "cls_head": "lavt_cls_head_bwd"}
    for kind, nblk, W in itertools.product(parent, (1, 47, 48, 128, 450, 768, 1024, 2048), (2, 192, 2048, 4096)):
        entries, atomic, stage = reduce_partials_plan(kind, nblk, W, True)
        assert atomic == 0 and stage >= 16 * W and stage >= _capi.lib.lavt_reduce_partials_det_stage(W) and stage == _RP_DET_SLICES * W
        assert entries[-1].endswith("_det") and all(e != parent[kind] for e in entries) and all(e in _capi._PROTOTYPES for e in entries)
        entries0, atomic0, stage0 = reduce_partials_plan(kind, nblk, W, False)
        assert entries0 == (parent[kind],) and stage0 == 0
        want = nblk if kind == "cls_head" else reduce_partials_slices(nblk)          # the classifier head adds from every workgroup
        assert atomic0 == (want if want > 1 else 0)
    for cb in (1, 33, 1000):
        assert reduce_partials_plan("multi", 0, 0, True, column_blocks=cb) == (("lavt_reduce_partials_multi_det",), 0, cb * 8 * 128)
        assert reduce_partials_plan("multi", 0, 0, False, column_blocks=cb) == (("lavt_reduce_partials_multi",), 8, 0)


def test_scratch_is_lent_by_the_library_s_own_eligibility_rule():
    """lavt_gemm_tn_v2_eligible answers for the launcher itself (tn_v2_eligible of gemm_tn_v2.hip): bf16 with a zeros page and 16-byte rows, a row scale only
    if binary, no row map on a convolution, 32-bit element offsets.  ops.gemm_tn lends scratch in deterministic mode only where it says yes."""
    import ctypes as C

    from lavt_hip import _capi as K

    def ask(**kw):
        p = K.GemmTN()
        p.dtype, p.I, p.J, p.K, p.batch, p.lda, p.ldb, p.zeros = K.BF16, 64, 64, 1024, 1, 64, 64, 1
        for k, v in kw.items():
            setattr(p, k, v)
        return K.lib.lavt_gemm_tn_v2_eligible(C.byref(p))
    assert ask() == 1
    assert ask(dtype=K.F32) == 0 and ask(zeros=None) == 0 and ask(lda=68) == 0 and ask(ldb=12) == 0
    assert ask(a_rowscale=1) == 0 and ask(a_rowscale=1, a_rowscale_binary=1) == 1
    assert ask(a_rowmap=1, conv_kc=64) == 0 and ask(K=1 << 26, lda=64) == 0
    src = open(os.path.join(ROOT, "lavt-rs_amd", "lavt_hip", "ops.py")).read()
    assert "lavt_gemm_tn_v2_eligible(C.byref(p))" in src


def test_train_step_refuses_what_the_mode_does_not_cover():
    from lavt_hip import ops
    from lavt_hip.engine import TrainStep
    x = torch.zeros(2, 3, 8, 8)
    t = torch.zeros(2, 8, 8, dtype=torch.long)
    ctx = ops.StepContext()
    with pytest.raises(NotImplementedError, match="world > 1"):
        TrainStep(None, x, None, None, t, world=2, deterministic=True, context=ctx)
    assert ctx.deterministic is False          # a refused construction leaves the context's mode alone
    with pytest.raises(NotImplementedError, match="world > 1"):          # the context's own mode counts the same
        TrainStep(None, x, None, None, t, world=2, context=ops.StepContext(deterministic=True))


def _enclosing(text):
    """name of the __global__ / __device__ function whose definition is the last one in `text` (the source up to an atomicAdd line)"""
    seg = text[max(text.rfind("__global__"), text.rfind("__device__")):]
    seg = re.sub(r"__launch_bounds__\([^)]*\)", "", seg)
    m = re.search(r"\b(\w+)\s*\(", seg)
    return m.group(1) if m else None


def _float_atomic_sites():
    sites = set()
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith((".hip", ".h")) or name == "infer.hip":          # infer.hip: integer I / U counts (exact, order-independent)
            continue
        lines = open(os.path.join(CSRC, name)).read().split("\n")
        for i, line in enumerate(lines):
            code = line.split("//")[0]
            if "atomicAdd(" in code:
                sites.add((name, _enclosing("\n".join(lines[:i]))))
    return sites


def test_design_table_lists_every_float_atomic_site():
    """Every `atomicAdd` line on a float target in lavt-rs_amd/csrc is a row of the "Deterministic mode" table of DESIGN.md, keyed by file and enclosing
    kernel, with a guard; the table names no site that no longer exists.  A text comparison (like the environment-switch test)."""
    sites = _float_atomic_sites()
    assert all(k for _, k in sites), sites
    # the integer sites that stay are really integer
    text = open(os.path.join(CSRC, "infer.hip")).read()
    assert all(re.search(r"atomicAdd\(iu \+", ln) for ln in text.split("\n") if "atomicAdd(" in ln.split("//")[0]) and "int* __restrict__ iu" in text
    doc = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = doc.split("## 9. Deterministic mode", 1)[1].split("\n## ", 1)[0]
    rows = re.findall(r"^\| `([a-z_0-9]+\.(?:hip|h))` \| `(\w+)` \| ([^|]+) \| ([^|]+) \|$", section, flags=re.M)
    table = {(f, k) for f, k, _, _ in rows}
    assert table == sites, (sorted(sites - table), sorted(table - sites))
    assert all(len(guard.strip()) > 20 and len(today.strip()) > 10 for _, _, today, guard in rows)
