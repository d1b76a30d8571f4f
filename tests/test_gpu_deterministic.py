"""Deterministic mode on the GPU (DESIGN.md "Deterministic mode").  Per float-atomic site: at the smallest shape at which the default kernel takes its
atomic branch, three calls on identical inputs give identical bits (torch.equal), and the result meets the reference and the gate of the op's existing
parity test (tests/test_gpu_ops.py: run_pair with that test's arguments).  End to end: two builds of a captured training iteration from one state dict
give identical losses, gradients, parameters, Adam moments and BatchNorm buffers, and an eager build gives the same bits as the replays.  A run whose
bits differ is a test failure: nothing here repeats a launch until something differs."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lavt_hip.detweights import det_inputs, fill_state_dict_
from test_gpu_ops import rnd, run_pair

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = [torch.float32, torch.bfloat16]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _det():
    from lavt_hip import ops
    return ops.StepContext(deterministic=True)


def _thrice(fn, inputs, dtype, seed=99):
    """fn(**gpu inputs) -> output; the output and every input gradient of three calls on identical inputs, each from fresh leaf tensors: bitwise equal"""
    runs = []
    for _ in range(3):
        gpu = {}
        for k, (t, kind) in inputs.items():
            if kind == "const":
                gpu[k] = t.to(DEV) if isinstance(t, torch.Tensor) else t
                continue
            g = t.to(DEV)
            gpu[k] = (g.to(dtype) if kind == "act" else g).requires_grad_(True)
        y = fn(**gpu)
        go = rnd(*y.shape, seed=seed).to(DEV).to(y.dtype)
        y.backward(go)
        torch.cuda.synchronize()
        runs.append([y.detach().clone()] + [gpu[k].grad.clone() for k, (_, kind) in inputs.items() if kind != "const"])
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert torch.equal(a, b), f"bits differ between two calls on identical inputs (max abs {float((a.float() - b.float()).abs().max()):.3e})"


def _site(fn, ref, inputs, dtype, name, **gate):
    import lavt_hip
    with lavt_hip.use_dtype(dtype), _det():
        _thrice(fn, inputs, dtype)
        run_pair(fn, ref, inputs, dtype, name=name, **gate)


# ================================================================================================ per site
def _rows_for_blocks(dtype, C, want):
    """smallest row count whose LayerNorm backward runs `want` workgroups (lavt_layernorm_bwd_blocks is monotone in rows)"""
    from lavt_hip import _capi as K
    lo, hi = 1, 1 << 20
    while lo < hi:
        mid = (lo + hi) // 2
        if K.lib.lavt_layernorm_bwd_blocks(K.dt(dtype), mid, C) >= want:
            hi = mid
        else:
            lo = mid + 1
    assert K.lib.lavt_layernorm_bwd_blocks(K.dt(dtype), lo, C) == want
    return lo


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("nblk", [48, 768])
def test_layernorm_row_slices(dtype, nblk):
    """norm.hip reduce_partials_kernel: `if (gridDim.y > 1) atomicAdd(dst + ..., t)`, gridDim.y from reduce_partials_grid: `nblk >= 768 ? 16 : nblk >= 384 ?
    8 : nblk >= 128 ? 4 : (nblk >= 48 ? 2 : 1)` -- 48 row blocks are the first two slices, 768 the sixteen.  C = 96.  Reference and gate:
    test_gpu_ops.test_layernorm (run_pair defaults)."""
    from lavt_hip import ops
    C = 96
    rows = _rows_for_blocks(dtype, C, nblk)
    inputs = {"x": (rnd(rows, C, seed=1) + 0.3, "act"), "g": (1 + 0.1 * rnd(C, seed=2), "param"), "b": (0.1 * rnd(C, seed=3), "param")}
    _site(lambda x, g, b: ops.layer_norm(x, g, b), lambda x, g, b: F.layer_norm(x, (C,), g, b), inputs, dtype, "layernorm (deterministic)")


@pytest.mark.parametrize("dtype", DT)
def test_norm_statistics_row_blocks(dtype):
    """norm.hip colstats_kernel: `if (partials) {...} else { atomicAdd(o1 + ...); atomicAdd(o2 + ...) }` (scratch too small) and the reduce_partials slices
    behind it (75 row blocks at 2 x 3136 x 96: two slices).  Reference and gate: test_gpu_ops.test_instance_norm, its (2, 3136, 96, with_mul) case."""
    from lavt_hip import ops
    B, T, C = 2, 3136, 96

    def ref(x, mul):
        z = x.view(B, T, C)
        y = (z - z.mean(1, keepdim=True)) / torch.sqrt(z.var(1, unbiased=False, keepdim=True) + 1e-5)
        return y.reshape(B * T, C) * mul
    inputs = {"x": (rnd(B * T, C, seed=1) * 2 + 0.5, "act"), "mul": (rnd(B * T, C, seed=2), "act")}
    _site(lambda x, mul: ops.instance_norm(x, B, T, mul=mul), ref, inputs, dtype, "instance norm (deterministic)", bf16=5e-2)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("window,dims,heads", [((1, 7, 7), (1, 42, 42), 2), ((2, 7, 7), (2, 14, 14), 2)])
def test_table_gradient(dtype, window, dims, heads):
    """bf16: dtable_body.h dtable_block `atomicAdd(hist + (bi - bs[j + r]), a[r] + b[r])` (LDS, every launch) and attention_mfma.hip wattn_dtable_finish
    `if (gridDim.z > 1) atomicAdd(dtable + ...)` (more than 16 records).  7x7: 72 windows = 3 window groups of <= 32 (dtable_geometry), 39 records; 2x7x7:
    a 3-D window.  fp32: attention.hip window_attn_bwd_kernel `if (dtable) atomicAdd(dtable + relpos_index(...) * heads + h, ds)` and the LDS
    `atomicAdd(dKs + j * KV_LD + d, dk[t][d])` across waves, every launch.  Reference and gate: test_gpu_ops.test_window_attention(_3d) (run_pair defaults)."""
    from lavt_hip import ops
    from oracle import lavt_video_oracle as OV
    N, C = window[0] * window[1] * window[2], heads * 32
    nW = (dims[0] // window[0]) * (dims[1] // window[1]) * (dims[2] // window[2])
    Bw = 2 * nW
    idx = OV.rel_pos_index_3d(*window).reshape(-1)
    R = (2 * window[0] - 1) * (2 * window[1] - 1) * (2 * window[2] - 1)

    def ref(qkv, table):
        q, k, v = qkv.view(Bw, N, 3, heads, 32).permute(2, 0, 3, 1, 4)
        a = (q * 32 ** -0.5) @ k.transpose(-1, -2) + table[idx].view(N, N, heads).permute(2, 0, 1)[None]
        return (a.softmax(-1) @ v).transpose(1, 2).reshape(Bw * N, C)
    inputs = {"qkv": (rnd(Bw * N, 3 * C, seed=1), "act"), "table": (rnd(R, heads, seed=2, scale=0.5), "param")}
    _site(lambda qkv, table: ops.window_attention(qkv, table, None, window, heads, N=N), ref, inputs, dtype, "window attention (deterministic)")


@pytest.mark.parametrize("dtype,M", [(torch.float32, 1000), (torch.bfloat16, 1024)])
def test_weight_gradient_split(dtype, M):
    """fp32: gemm.hip gemm_tn_kernel `atomicAdd(C + ii * p.ldc + col, ...)` from the classic split rule of lavt_gemm_tn_route (gemm_tn_plan.hip), `split = 768 / (tiles * batch)` pieces (capped at one per 4 K
    tiles): 1000 rows on one 64x64 tile split, and fp32 is never lent scratch.  bf16: gemm_tn_v2.hip tn_tile_range `if (atomic) atomicAdd(dst, ...)`,
    `o.atomic = !to_parts && (nsplit > 1 || p.accumulate)`: 1024 rows = 16 K tiles = 2 pieces (>= 8 K tiles each), below _TN_PARTIALS_MINK = 2048 no
    scratch.  Reference and gate: test_gpu_ops.test_linear_plain (run_pair defaults)."""
    from lavt_hip import ops
    N, Kd = 64, 64
    inputs = {"x": (rnd(M, Kd, seed=1), "act"), "w": (rnd(N, Kd, seed=2, scale=Kd ** -0.5), "param"), "b": (rnd(N, seed=3), "param")}
    _site(lambda x, w, b: ops.linear(x, w, b), lambda x, w, b: F.linear(x, w, b), inputs, dtype, "linear (deterministic)")


@pytest.mark.parametrize("dtype", DT)
def test_embedding_backward(dtype):
    """text.hip bert_embed_bwd_kernel: `atomicAdd(w + c, g); atomicAdd(p + c, g); atomicAdd(t + c, g)` on every launch (repeated ids, every position once per
    sentence, two token types).  4 sentences x 22 tokens: id 7 occurs 9 times, id 40 once.  Reference and gate: test_gpu_ops.test_bert_embed (three
    embedding lookups and their scatter-add gradients; output within 2e-2 (bf16) / 1e-6 of the scale, gradients within 1e-5 x max + 1e-6)."""
    import lavt_hip
    from lavt_hip import ops
    B, N, H, V = 4, 22, 768, 64
    ids = torch.randint(8, 40, (B, N), generator=torch.Generator().manual_seed(3))
    ids.view(-1)[::10] = 7
    ids[2, 5] = 40
    assert int((ids == 7).sum()) >= 8 and int((ids == 40).sum()) == 1
    tt = torch.zeros(B, N, dtype=torch.long)
    tt[:, 15:] = 1
    ids, tt = ids.to(DEV), tt.to(DEV)
    w = rnd(B * N, H, seed=5).to(DEV)
    runs = []
    with lavt_hip.use_dtype(dtype), _det():
        for _ in range(3):
            ps = [torch.nn.Parameter(rnd(V, H, seed=1).to(DEV)), torch.nn.Parameter(rnd(32, H, seed=2).to(DEV)), torch.nn.Parameter(rnd(2, H, seed=3).to(DEV))]
            out = ops.bert_embed(ids, tt, ps[0], ps[1], ps[2], N, dtype)
            (out.float() * w).sum().backward()
            torch.cuda.synchronize()
            runs.append([out.detach()] + [p.grad for p in ps])
    for r in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(runs[0], r)), "bits differ between two calls on identical inputs"
    ref_p = [p.detach().clone().requires_grad_(True) for p in ps]
    ref = (ref_p[0][ids] + ref_p[2][tt] + ref_p[1][:N][None]).view(B * N, H)
    (ref * (w.to(dtype).float() if dtype == torch.bfloat16 else w)).sum().backward()
    tol = 2e-2 if dtype == torch.bfloat16 else 1e-6
    assert float((out.detach().float() - ref.detach()).abs().max()) <= tol * float(ref.detach().abs().max())
    for p, r in zip(ps, ref_p):
        assert float((p.grad - r.grad).abs().max()) <= 1e-5 * float(r.grad.abs().max()) + 1e-6


@pytest.mark.parametrize("dtype", DT)
def test_classifier_head_backward(dtype):
    """elementwise.hip cls_head_bwd_kernel (non-PART): `atomicAdd(dw + e, red[e])` / `atomicAdd(db + threadIdx.x, ...)` from every workgroup of every launch
    outside the step harness.  Shapes, reference and gate: test_gpu_ops.test_cls_head_and_logits_up (run_pair defaults)."""
    from lavt_hip import ops
    B, h, w, C, H, W = 2, 14, 12, 64, 56, 48

    def ref(x, wt, b):
        y = F.conv2d(x.view(B, h, w, C).permute(0, 3, 1, 2), wt, b)
        return F.interpolate(y, size=(H, W), mode="bilinear", align_corners=True)
    inputs = {"x": (rnd(B * h * w, C, seed=1), "act"), "wt": (rnd(2, C, 1, 1, seed=2, scale=C ** -0.5), "param"), "b": (rnd(2, seed=3), "param")}
    _site(lambda x, wt, b: ops.logits_upsample(ops.cls_head(x, wt, b), B, h, w, H, W), ref, inputs, dtype, "cls head + upsample (deterministic)")


def test_multi_set_reduction_over_more_than_64_sets():
    """norm.hip reduce_partials_multi_kernel: `atomicAdd((w + i >= C ? o2 : o1) + ..., tv[i])` from the eight row slices of every column block, every
    launch.  ops._reduce_partials_multi in deterministic mode over 70 sets (two launches of lavt_reduce_partials_multi_det: 64 + 6 rows of the descriptor
    table), widths 1 (the classifier head's bias set), 24, 96, 130 and 1024, 1 to 450 row blocks: three calls give identical bits, and the sums ADDED to
    non-zero outputs meet the fp64 sums within fp32 summation error (2e-4 of the scale: test_gpu_ops's fp32 gate)."""
    from lavt_hip import ops
    gen = torch.Generator().manual_seed(11)
    sets = []
    for i in range(70):
        C = (1, 24, 96, 130, 1024)[i % 5]
        nblk = (1, 7, 48, 450, 129, 33, 8)[i % 7]
        parts = torch.randn(nblk, 2 * C, generator=gen).to(DEV)
        init = torch.randn(2, C, generator=gen).to(DEV)
        sets.append((parts, nblk, C, init))
    with _det():
        runs = []
        for _ in range(3):
            outs = [init.clone() for _, _, _, init in sets]
            items = [(p.data_ptr(), nblk, C, o[0].data_ptr(), o[1].data_ptr()) for (p, nblk, C, _), o in zip(sets, outs)]
            desc = torch.tensor(items, dtype=torch.int64).to(DEV)
            ops._reduce_partials_multi(desc, items)
            torch.cuda.synchronize()
            runs.append(outs)
    for r in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(runs[0], r)), "bits differ between two calls on identical inputs"
    for (parts, nblk, C, init), got in zip(sets, runs[0]):
        ref = init.double() + parts.double().sum(0).view(2, C)
        err = float((got.double() - ref).abs().max())
        assert err <= 2e-4 * max(float(ref.abs().max()), 1.0), (nblk, C, err)


class _Collect:
    """stands in for ops.wgrads in gemm_tn(defer=): keeps the members instead of queueing them"""

    def __init__(self):
        self.items, self.keep = [], []

    def add(self, p, tensors, extra=False, rider=None):
        self.items.append(p)
        self.keep.append(tensors)


def test_two_addend_colsum_is_order_independent():
    """The one float atomic deterministic mode keeps: the windowed qkv bias gradient shared by the two members of the token-order launch (ops._WmsaFused.backward,
    colsum_atomic=True): the padded-row side member and the weight-gradient member each add ONE column sum per element into a zeroed vector, and
    0 + a + b == 0 + b + a in IEEE arithmetic.  200 repetitions of that grouped launch give one bit pattern; the sum is the fp64 column sum of all rows
    within the bf16 gate of test_gpu_ops (3e-2 x 1.5 of the scale)."""
    import ctypes as C

    import lavt_hip
    from lavt_hip import _capi as K
    from lavt_hip import ops
    Cc, M, P = 1024, 450, 702          # a stage-3 Swin-B block at batch 2: 450 tokens, 702 padded window rows; 816 tiles: the group forms
    with lavt_hip.use_dtype(torch.bfloat16), _det():
        dqkv = rnd(M + P, 3 * Cc, seed=1).to(DEV).to(torch.bfloat16)
        xn = rnd(M, Cc, seed=2).to(DEV).to(torch.bfloat16)
        perm = torch.randperm(M + P, generator=torch.Generator().manual_seed(4)).to(torch.int32).to(DEV)
        inv, padrows = perm[:M].contiguous(), perm[M:].contiguous()
        wbuf = torch.zeros(3 * Cc, Cc, device=DEV)
        bbuf = torch.zeros(3 * Cc, device=DEV)
        dummy = torch.empty(3 * Cc * 8, device=DEV)
        q = _Collect()
        ops.gemm_tn(torch.bfloat16, 3 * Cc, 8, P, dqkv, 3 * Cc, ops._zero_page_tensor(torch.device(DEV)), 0, dummy, 8, a_rowmap=padrows, colsum=bbuf, colsum_atomic=True,
                    defer=q, extra=True)
        ops.gemm_tn(torch.bfloat16, 3 * Cc, Cc, M, dqkv, 3 * Cc, xn, Cc, wbuf, Cc, a_rowmap=inv, colsum=bbuf, colsum_atomic=True, defer=q)
        assert all(p.split_k >= 0 for p in q.items)          # deterministic mode: no member may be cut into atomic pieces
        ops.assign_partials(q.items, torch.device(DEV))
        arr = (K.GemmTN * 2)(*q.items)
        first = None
        for _ in range(200):
            bbuf.zero_()
            K.check(K.lib.lavt_gemm_tn_grouped(arr, 2, K.stream()))
            got = bbuf.clone()
            first = got if first is None else first
            assert torch.equal(got, first)
        torch.cuda.synchronize()
    ref = dqkv.double().sum(0).cpu()
    err = float((first.double().cpu() - ref).abs().max())
    assert err <= 3e-2 * 1.5 * float(ref.abs().max()), err


# ================================================================================================ end to end
def _micro2d(sd=None):
    from test_gpu_modules import _build
    model = _build(32, [2, 2, 2, 2], [1, 2, 4, 8], 7, dpr=0.0)
    if sd is not None:
        model.load_state_dict(sd)
    return model.train()


def _state(model, opt):
    out = {"p|" + n: p.detach().clone() for n, p in model.named_parameters()}
    out.update({"b|" + n: b.detach().clone() for n, b in model.named_buffers()})
    for n, p in model.named_parameters():
        for k, v in opt.state.get(p, {}).items():
            if torch.is_tensor(v):
                out[f"m|{n}|{k}"] = v.detach().clone()
    return out


def _run(build, inputs, dtype, use_graph, replays, seed=4321, fp8=False, **step_kw):
    """one build from `build()` in a private deterministic context: warm-up (+ capture) and `replays` iterations -> (losses, gradients after the last
    iteration, gradients after the first, parameters + buffers + optimizer state)"""
    import lavt_hip
    from lavt_hip import ops
    from lavt_hip.engine import TrainStep
    ctx = ops.StepContext()
    with lavt_hip.use_dtype("fp8" if fp8 else dtype):
        model = build()
        step = TrainStep(model, *inputs, context=ctx, use_graph=use_graph, deterministic=True, **step_kw)
        assert ctx.deterministic and lavt_hip.fp8_enabled() == fp8
        opt = step.make_optimizer([p for p in model.parameters() if p.requires_grad], lr=3e-4, weight_decay=1e-2, max_grad_norm=1.0, skip_nonfinite=True)
        step.warmup_and_capture()
        assert step.captured == use_graph
        with pytest.raises(RuntimeError, match="before warmup_and_capture"):
            step.set_deterministic(False)
        # identical state: the warm-up left parameters and optimizer state untouched (FusedAdamW.hold) but advanced the BatchNorm buffers and the
        # DropPath generator -- the buffers are put back, the generator reseeded
        with ops.use_context(ctx):
            ops.droppath_reseed(seed, torch.device(DEV))
        model.load_state_dict(build.sd)
        if fp8:          # the delayed-scaling |max| history is state too: the warm-up (and the validation replays of a capture) advanced it
            assert ctx.fp8.slots, "the e4m3 sites must have been reached"
            ctx.fp8.prev.zero_()
            ctx.fp8.cur.zero_()
        losses, first = [], None
        for it in range(replays):
            losses.append(step.step().clone())
            if it == 0:
                torch.cuda.synchronize()
                first = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
        torch.cuda.synchronize()
        grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
        state = _state(model, opt)
        if fp8:
            state.update({"fp8|prev": ctx.fp8.prev[:len(ctx.fp8.slots)].clone(), "fp8|cur": ctx.fp8.cur[:len(ctx.fp8.slots)].clone()})
        return torch.stack(losses), grads, first, state


def _same(a, b, what):
    assert a.keys() == b.keys(), what
    bad = [k for k in a if not torch.equal(a[k], b[k])]
    assert not bad, f"{what}: {len(bad)} of {len(a)} tensors differ, e.g. {bad[:6]}"


@pytest.mark.parametrize("dtype", DT)
def test_captured_iteration_2d_is_bit_reproducible(golden, dtype):
    """The micro model and batch of tests/golden/e2e_tiny_train.npz, TrainStep(deterministic=True) with an owned FusedAdamW (clip 1.0, non-finite skip): two
    builds from one state dict, warm-up + capture + 4 replays each -> the 4 losses, the gradients after the last replay, all parameters, both moments and
    the BatchNorm buffers are torch.equal; a third build with use_graph=False gives the same bits (eager equals replay).  fp32: the first iteration's
    gradients meet the fixture within test_gpu_modules.test_e2e_micro_train_grads_golden's gate (2e-3 x the gradient's norm + 5e-6 on its digest)."""
    from test_gpu_modules import grad_digest
    g = golden("e2e_tiny_train")
    x, l, m, tgt = (t.to(DEV) for t in det_inputs(2, 64, 20, seed=int(g["seed"])))
    sd = {k: v.clone() for k, v in _micro2d().state_dict().items()}

    def build():
        return _micro2d(sd)
    build.sd = sd
    a = _run(build, (x, l, m, tgt), dtype, True, 4)
    b = _run(build, (x, l, m, tgt), dtype, True, 4)
    e = _run(build, (x, l, m, tgt), dtype, False, 4)
    for other, what in ((b, "second captured build"), (e, "eager build")):
        assert torch.equal(a[0], other[0]), (what, a[0].tolist(), other[0].tolist())
        _same(a[1], other[1], what + ": gradients after the last iteration")
        _same(a[3], other[3], what + ": parameters, buffers, moments")
    assert any(not torch.equal(a[3]["p|" + n], sd[n].to(DEV)) for n, _ in _micro2d(sd).named_parameters()), "the iterations must have trained"
    if dtype == torch.float32:
        assert abs(float(a[0][0]) - float(g["loss"])) < 1e-4
        nograd = set(g["nograd"].tolist())
        bad = []
        for k, gr in a[2].items():
            if k in nograd:
                continue
            ref = torch.as_tensor(g["g|" + k])
            err = float((grad_digest(gr) - ref).abs().max())
            if not err <= 2e-3 * max(float(ref[0]), 1e-6) + 5e-6:
                bad.append((k, err, float(ref[0])))
        assert not bad, f"{len(bad)} parameter gradients off the fixture: {bad[:8]}"


def test_captured_iteration_fp8_is_bit_reproducible(golden, monkeypatch):
    """The same micro model and batch with LAVT_FP8=1's arithmetic (bf16 + e4m3 decoder convolutions; the fill threshold lowered so that the micro decoder
    takes them, as test_gpu_ops's fp8 tests do): the |max| history starts from zeros in every build; two captured builds and an eager one, 4 iterations ->
    losses, gradients, parameters, moments, BatchNorm buffers and the |max| history torch.equal."""
    from lavt_hip import ops
    monkeypatch.setattr(ops, "_FP8_CONV_MIN_TILES", 0)
    g = golden("e2e_tiny_train")
    x, l, m, tgt = (t.to(DEV) for t in det_inputs(2, 64, 20, seed=int(g["seed"])))
    sd = {k: v.clone() for k, v in _micro2d().state_dict().items()}

    def build():
        return _micro2d(sd)
    build.sd = sd
    a = _run(build, (x, l, m, tgt), torch.bfloat16, True, 4, fp8=True)
    b = _run(build, (x, l, m, tgt), torch.bfloat16, True, 4, fp8=True)
    e = _run(build, (x, l, m, tgt), torch.bfloat16, False, 4, fp8=True)
    for other, what in ((b, "second captured build"), (e, "eager build")):
        assert torch.equal(a[0], other[0]), (what, a[0].tolist(), other[0].tolist())
        _same(a[1], other[1], what + ": gradients after the last iteration")
        _same(a[3], other[3], what + ": parameters, buffers, moments, |max| history")
    assert bool(torch.isfinite(a[0]).all()) and float(a[3]["fp8|prev"].abs().max()) > 0


def _video(tag, sd=None):
    """LAVTVideo around the micro Video-Swin of test_gpu_modules._build_video (PWAM | SepTPWAM) with the stub text encoder of test_gpu_frame_select"""
    from lib._utils import LAVTVideo
    from test_gpu_modules import _build_video
    parts = _build_video(tag)
    frames, l, m, tgt = det_inputs(2, 64, 22, seed=1234, frames=4)
    l = l.to(DEV)

    class _Text(torch.nn.Module):
        def forward(self, ids, attention_mask=None):
            return (l.permute(0, 2, 1),)

    model = LAVTVideo.__new__(LAVTVideo)
    torch.nn.Module.__init__(model)
    model.backbone, model.classifier, model.text_encoder = parts["backbone"], parts["classifier"], _Text()
    model.lazy_pred, model.seg_last = False, False
    if sd is not None:
        model.load_state_dict(sd)
    ids, am = torch.zeros(2, 22, dtype=torch.long, device=DEV), m.squeeze(-1).contiguous().to(DEV)
    return model.train(), frames.to(DEV), ids, am, tgt.to(DEV)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("tag", ["pwam", "sept"])
def test_captured_iteration_video_is_bit_reproducible(tag, dtype):
    """The micro Video-Swin of e2e_video_micro_{pwam,sept} (2 clips x 4 frames x 64^2) with valid_indices = frames [2, 5]: two captured builds and an eager
    one, 2 iterations each -> losses and gradients torch.equal."""
    model, frames, ids, am, tgt = _video(tag)
    sd = {k: v.clone() for k, v in model.state_dict().items()}

    def build():
        return _video(tag, sd)[0]
    build.sd = sd
    vi = torch.tensor([2, 5], dtype=torch.int32, device=DEV)
    kw = dict(valid_indices=vi)
    inputs = (frames, ids, am, tgt[[2, 5]].contiguous())
    a = _run(build, inputs, dtype, True, 2, **kw)
    b = _run(build, inputs, dtype, True, 2, **kw)
    e = _run(build, inputs, dtype, False, 2, **kw)
    for other, what in ((b, "second captured build"), (e, "eager build")):
        assert torch.equal(a[0], other[0]), (what, a[0].tolist(), other[0].tolist())
        _same(a[1], other[1], what + ": gradients")
        _same(a[2], other[2], what + ": gradients of the first iteration")


def test_lavt_one_embedding_gradient_is_applied_reproducibly():
    """lavt_one with the micro BERT of test_gpu_modules.test_lavt_one_micro_matches_oracle_chain (1 layer, 12 heads, hidden 768 -- the width PWAM's language
    projections read; the 128-wide encoder of bert_micro_n22.npz does not fit LAVTOne), 22 tokens, trained with lang_enc_params="embeddings+encoder-all",
    so that the embedding scatter's gradient reaches the update: two captured builds, 2 iterations -> equal parameters (the word embedding among them,
    and it moved)."""
    import lavt_hip
    from bert.modeling_bert import BertConfig, BertModel
    from lavt_hip import ops
    from lavt_hip.engine import TrainStep
    from lavt_hip.optim import lavt_param_groups
    from lib._utils import LAVTOne
    from lib.backbone import MultiModalSwinTransformer
    from lib.mask_predictor import SimpleDecoding
    N = 22
    x, _, m, tgt = det_inputs(2, 64, N, seed=9)
    mask = m.squeeze(-1).long()
    ids = torch.randint(1, 64, mask.shape, generator=torch.Generator().manual_seed(5)) * mask

    def build():
        args = SimpleNamespace(lazy_pred=False)
        bb = MultiModalSwinTransformer(embed_dim=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8], window_size=7, drop_path_rate=0.0, args=args)
        model = LAVTOne(bb, SimpleDecoding(256, args), SimpleNamespace(ck_bert="/nonexistent", bert_random_init=True))
        model.text_encoder = BertModel(BertConfig(vocab_size=64, hidden_size=768, num_hidden_layers=1, num_attention_heads=12, intermediate_size=256,
                                                  max_position_embeddings=32, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0), add_pooling_layer=False)
        fill_state_dict_(model)
        return model.to(DEV).train()
    word = "text_encoder.embeddings.word_embeddings.weight"
    finals = []
    for _ in range(2):
        ctx = ops.StepContext()
        with lavt_hip.use_dtype(torch.bfloat16):
            model = build()
            sd0 = {k: v.clone() for k, v in model.state_dict().items()}
            start = sd0[word]
            step = TrainStep(model, x.to(DEV), ids.to(DEV), mask.to(DEV), tgt.to(DEV), context=ctx, deterministic=True)
            step.make_optimizer(lavt_param_groups(model, lang_enc_params="embeddings+encoder-all"), lr=3e-4, weight_decay=1e-2, max_grad_norm=1.0, skip_nonfinite=True)
            step.warmup_and_capture()
            assert step.captured
            model.load_state_dict(sd0)          # (the warm-up advanced the BatchNorm buffers)
            for _ in range(2):
                step.step()
            torch.cuda.synchronize()
            finals.append({n: p.detach().clone() for n, p in model.named_parameters()})
            assert not torch.equal(finals[-1][word], start), "the embedding gradient must have been applied"
    _same(finals[0], finals[1], "lavt_one parameters after 2 iterations")


# ================================================================================================ the default mode is untouched
def eager_step_launches():
    """the C entry points one eager fused-loss step of the micro 2-D model launches in the DEFAULT mode, in order, with their scope labels (K.prof)"""
    import lavt_hip
    from lavt_hip import _capi as K
    from lavt_hip import ops
    from lavt_hip.engine import TrainStep
    x, l, m, tgt = (t.to(DEV) for t in det_inputs(2, 64, 20, seed=5))
    ctx = ops.StepContext()
    with lavt_hip.use_dtype(torch.bfloat16):
        step = TrainStep(_micro2d(), x, l, m, tgt, context=ctx, use_graph=False)
        step.warmup_and_capture(eager_iters=2)
        K.prof.start()
        step.step()
        recs = K.prof.stop()
    return [[name, scope] for name, scope, _, _ in recs]


def test_default_mode_launches_what_the_parent_commit_launched(monkeypatch):
    """LAVT_DETERMINISTIC unset: the launches of one eager step of the micro 2-D model (bf16, fused loss) are the list recorded on the parent commit
    (tests/golden/default_step_launches_micro2d.json: names and scopes only, written by eager_step_launches() on that commit)."""
    monkeypatch.delenv("LAVT_DETERMINISTIC", raising=False)
    want = json.load(open(os.path.join(GOLDEN, "default_step_launches_micro2d.json")))
    got = eager_step_launches()
    assert len(got) > 100
    assert got == want, next(((i, a, b) for i, (a, b) in enumerate(zip(got, want)) if a != b), (len(got), len(want)))
