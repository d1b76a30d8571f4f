"""GPU parity of every liblavt_hip op (through the C ABI) against plain fp32 PyTorch-on-CPU statements of
the same op (autograd gives the gradient oracle).  fp32 path: tight tolerances (exact-fp32 MFMA);
bf16 path: tolerance relative to the output scale (bf16 has 8 significant bits).

Run on the GPU box:  python -m pytest tests -m gpu -x -q
"""
import math

import numpy as np
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DT = [torch.float32, torch.bfloat16]


def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m 'not gpu' elsewhere)"
    return torch.device("cuda:0")


def lavt_hip_dtype(dtype):
    import lavt_hip
    return lavt_hip.use_dtype(dtype)


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator("cpu").manual_seed(seed)) * scale


def tol(dtype, ref, f32=2e-4, bf16=3e-2):
    scale = float(ref.abs().max())
    return f32 * max(scale, 1.0) if dtype == torch.float32 else bf16 * max(scale, 1e-3)


def assert_close(got, ref, dtype, name="", f32=2e-4, bf16=3e-2, l2=None):
    """max-norm gate relative to the reference's scale; `l2` adds the norm-wise gate ||got - ref||_2 <= l2 * ||ref||_2 (both sides of run_pair start
    from the same bf16-representable values, so a bf16 output differs from the fp32 reference by its final rounding -- 2^-9 / sqrt(3) = 1.1e-3 rms --
    plus the summation order: a kernel that drops or misplaces a few terms moves the norm-wise error long before it moves a loose max-norm)"""
    got = got.detach().float().cpu()
    ref = ref.detach().float()
    assert got.shape == ref.shape, f"{name}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    err = float((got - ref).abs().max())
    t = tol(dtype, ref, f32, bf16)
    assert math.isfinite(err) and err <= t, f"{name}: max abs err {err:.3e} > {t:.3e} (ref scale {float(ref.abs().max()):.3e})"
    if l2 is not None:
        rel = float((got - ref).norm()) / max(float(ref.norm()), 1e-30)
        assert rel <= l2, f"{name}: relative l2 error {rel:.3e} > {l2:.1e}"


def border_rows(B, H, W):
    """row indices (NHWC token order) of the image-border pixels: where a 3x3 tap that must read the zero halo reads a neighbour instead"""
    y, x = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    m = ((y == 0) | (y == H - 1) | (x == 0) | (x == W - 1)).reshape(-1)
    return torch.cat([torch.nonzero(m).reshape(-1) + b * H * W for b in range(B)])


def assert_border_close(got, ref, bhw, tol_rel, name=""):
    """border-only max check of an [B*H*W, C] map at a tight tolerance (relative to the whole map's scale): one wrong halo tap is ~0.07 x max|ref|"""
    got, ref = got.detach().float().cpu(), ref.detach().float()
    rows = border_rows(*bhw)
    err = float((got[rows] - ref[rows]).abs().max())
    scale = float(ref.abs().max())
    assert err <= tol_rel * scale, f"{name}: border pixels differ by {err / scale:.3e} x max|ref| > {tol_rel:.1e}"


def run_pair(hip_fn, ref_fn, inputs, dtype, requires=None, f32=2e-4, bf16=3e-2, name="", l2=None, border=None, border_tol=8e-3):
    """inputs: dict name -> (cpu fp32 tensor, kind) with kind in {'act','param','const'}.
    act tensors are cast to `dtype` on the GPU, params stay fp32.  Compares outputs and all gradients.
    l2: norm-wise gate on the output and on every gradient (assert_close); border = (B, H, W): the output and every activation gradient are
    [B*H*W, C] maps whose border pixels get their own max check at `border_tol` x max|ref| (x 1.5 for gradients)."""
    from lavt_hip import ops
    d = dev()
    cpu, gpu = {}, {}
    for k, (t, kind) in inputs.items():
        if kind == "const":
            cpu[k], gpu[k] = t, (t.to(d) if isinstance(t, torch.Tensor) else t)
            continue
        c = t.clone()
        if dtype == torch.bfloat16:
            c = c.to(torch.bfloat16).float()          # both sides start from the same bf16-representable values
        c.requires_grad_(True)
        g = c.detach().to(d)
        if kind == "act":
            g = g.to(dtype)
        g.requires_grad_(True)
        cpu[k], gpu[k] = c, g
    ops.weights.invalidate()
    y_ref = ref_fn(**cpu)
    y = hip_fn(**gpu)
    assert_close(y, y_ref, dtype, name + " forward", f32, bf16, l2)
    if border is not None and dtype == torch.bfloat16:
        assert_border_close(y, y_ref, border, border_tol, name + " forward")
    go = rnd(*y_ref.shape, seed=99)
    if dtype == torch.bfloat16:
        go = go.to(torch.bfloat16).float()
    y_ref.backward(go)
    y.backward(go.to(d).to(y.dtype))
    torch.cuda.synchronize()
    for k, (t, kind) in inputs.items():
        if kind == "const":
            continue
        assert gpu[k].grad is not None, f"{name}: no grad for {k}"
        assert_close(gpu[k].grad, cpu[k].grad, dtype, f"{name} grad[{k}]", f32 * 5, bf16 * 1.5, l2)
        if border is not None and dtype == torch.bfloat16 and kind == "act" and gpu[k].grad.dim() == 2 and gpu[k].grad.shape[0] == border[0] * border[1] * border[2]:
            assert_border_close(gpu[k].grad, cpu[k].grad, border, border_tol * 1.5, f"{name} grad[{k}]")


# ------------------------------------------------------------------------------------------------ GEMM
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("M,N,Kd", [(300, 200, 96), (3072, 1024, 128), (77, 24, 48), (640, 384, 512)])
def test_linear_plain(dtype, M, N, Kd):
    from lavt_hip import ops
    inputs = {"x": (rnd(M, Kd, seed=1), "act"), "w": (rnd(N, Kd, seed=2, scale=Kd ** -0.5), "param"), "b": (rnd(N, seed=3), "param")}
    run_pair(lambda x, w, b: ops.linear(x, w, b), lambda x, w, b: F.linear(x, w, b), inputs, dtype, name=f"linear {M}x{N}x{Kd}")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("tile", ["128", "64"])
def test_gemm_forced_tiles(dtype, tile, monkeypatch, request):
    """Both tile configurations of every GEMM family (NT k-contiguous, NT k-major, TN) and of the implicit-GEMM conv."""
    from lavt_hip import ops, _capi as K
    monkeypatch.setenv("LAVT_GEMM_TILE", tile)
    K.lib.lavt_tuning_reload()             # the library reads its switches once per process; re-read after changing one
    request.addfinalizer(lambda: (os.environ.pop("LAVT_GEMM_TILE", None), K.lib.lavt_tuning_reload()))
    M, N, Kd = 700, 328, 264
    inputs = {"x": (rnd(M, Kd, seed=1), "act"), "w": (rnd(N, Kd, seed=2, scale=Kd ** -0.5), "param"), "b": (rnd(N, seed=3), "param")}
    run_pair(lambda x, w, b: ops.linear(x, w, b), lambda x, w, b: F.linear(x, w, b), inputs, dtype, name=f"linear tile {tile}")
    B, H, W, C1, C2, Cout = 2, 13, 11, 96, 32, 136
    inputs = {"x1": (rnd(B * H * W, C1, seed=1), "act"), "x2": (rnd(B * H * W, C2, seed=2), "act"),
              "w": (rnd(Cout, C1 + C2, 3, 3, seed=3, scale=(9 * (C1 + C2)) ** -0.5), "param")}

    def ref(x1, w, x2):
        y = F.conv2d(torch.cat([x1, x2], 1).view(B, H, W, C1 + C2).permute(0, 3, 1, 2), w, padding=1)
        return y.permute(0, 2, 3, 1).reshape(B * H * W, Cout)
    run_pair(lambda x1, w, x2: ops.conv3x3(x1, x2, w, B, H, W), ref, inputs, dtype, name=f"conv tile {tile}", bf16=4e-2)


@pytest.mark.parametrize("tile,stages", [("512", "0"), ("128", "4"), ("128", "2")])
def test_gemm_pipelined_k_loop(tile, stages, monkeypatch, request):
    """csrc/gemm_nt_pipe.hip (software-pipelined K loop, 8 waves: fragment reads one MFMA group ahead, one barrier per K tile, DMA issue spread between
    the MFMAs of the last group, taps-fastest K order for convolutions) in its three configurations -- 256x256 tile, 128x128 tile with a 4- and a
    2-stage ring -- and its three DMA modes: plain (K % 64 == 0), tap-walking convolution (channels % 64 == 0, with a concat source and with a
    tap-split reduction), general decode (K tail / odd channel counts); k-contiguous (forward) and k-major (data gradient) weight reads."""
    from lavt_hip import ops, _capi as K
    for k, v in (("LAVT_GEMM_TILE", tile), ("LAVT_GEMM_STAGES", stages), ("LAVT_GEMM_PIPE", "3")):
        monkeypatch.setenv(k, v)
    K.lib.lavt_tuning_reload()
    request.addfinalizer(lambda: ([os.environ.pop(k, None) for k in ("LAVT_GEMM_TILE", "LAVT_GEMM_STAGES", "LAVT_GEMM_PIPE")], K.lib.lavt_tuning_reload()))
    dtype = torch.bfloat16
    for (M, N, Kd) in ((700, 328, 256), (700, 328, 264), (130, 520, 64), (1000, 256, 1024)):
        inputs = {"x": (rnd(M, Kd, seed=1), "act"), "w": (rnd(N, Kd, seed=2, scale=Kd ** -0.5), "param"), "b": (rnd(N, seed=3), "param")}
        run_pair(lambda x, w, b: ops.linear(x, w, b), lambda x, w, b: F.linear(x, w, b), inputs, dtype, name=f"pipe linear {M}x{N}x{Kd} tile {tile}/{stages}", l2=5e-3)
    # (the 1024 + 512 and 512 -> 512 cases: few pixels, long reduction -- split-K over channel blocks, conv_kc_split, forward across the concat boundary and backward)
    # (no fp32 instantiation of this kernel exists, so its index arithmetic -- tap walking, halo zeros through out-of-range buffer offsets, channel-split
    # pieces -- is gated norm-wise (5e-3) and on the border pixels alone (8e-3 x max|ref|) next to the max-norm; the last shapes are the products' own:
    # Swin-T's 384 + 96 -> 384 concat convolution at 2 x 120 x 120 and, on the default configuration, Swin-B's 512 -> 512 at 4 x 120 x 120)
    # (round 5: channel counts that are not a multiple of 64 take the tap walk with a partial last block -- MODE 3 -- when the concat boundary sits on a
    # 64-channel block: 384 + 96 (Swin-T conv1_2), a single source of 96 / 160 channels, 128 + 40 (a 5-chunk tail))
    real = ((2, 120, 120, 384, 96, 384), (1, 20, 20, 96, 0, 128), (2, 9, 20, 160, 0, 256), (1, 24, 24, 128, 40, 256)) + (((4, 120, 120, 512, 0, 512),) if tile == "512" else ())
    for (B, H, W, C1, C2, Cout) in ((2, 13, 11, 128, 64, 136), (2, 13, 11, 96, 32, 136), (1, 30, 30, 512, 0, 128), (2, 9, 20, 64, 0, 256), (1, 24, 24, 256, 128, 256),
                                    (1, 20, 20, 1024, 512, 128), (1, 16, 16, 512, 0, 512)) + real:
        Cin = C1 + C2
        inputs = {"x1": (rnd(B * H * W, C1, seed=1), "act"), "w": (rnd(Cout, Cin, 3, 3, seed=3, scale=(9 * Cin) ** -0.5), "param")}
        if C2:
            inputs["x2"] = (rnd(B * H * W, C2, seed=2), "act")

        def ref(x1, w, x2=None):
            x = x1 if x2 is None else torch.cat([x1, x2], 1)
            y = F.conv2d(x.view(B, H, W, Cin).permute(0, 3, 1, 2), w, padding=1)
            return y.permute(0, 2, 3, 1).reshape(B * H * W, Cout)
        run_pair(lambda x1, w, x2=None: ops.conv3x3(x1, x2, w, B, H, W), ref, inputs, dtype, name=f"pipe conv {B}x{H}x{W} {C1}+{C2}->{Cout} tile {tile}/{stages}", bf16=4e-2,
                 l2=5e-3, border=(B, H, W))
    # two channel pieces of four 64-channel blocks each: the second piece starts in the first concat source and crosses into the second
    monkeypatch.setattr(ops, "_CONV_KC_SPLITS", "2")
    B, H, W, C1, C2, Cout = 1, 24, 24, 320, 192, 128
    Cin = C1 + C2
    assert ops._conv_split(dtype, B * H * W, Cout, Cin, C1, C2, 9, None, 0) == (2, True)
    inputs = {"x1": (rnd(B * H * W, C1, seed=1), "act"), "x2": (rnd(B * H * W, C2, seed=2), "act"), "w": (rnd(Cout, Cin, 3, 3, seed=3, scale=(9 * Cin) ** -0.5), "param")}

    def ref2(x1, w, x2):
        y = F.conv2d(torch.cat([x1, x2], 1).view(B, H, W, Cin).permute(0, 3, 1, 2), w, padding=1)
        return y.permute(0, 2, 3, 1).reshape(B * H * W, Cout)
    run_pair(lambda x1, w, x2: ops.conv3x3(x1, x2, w, B, H, W), ref2, inputs, dtype, name=f"pipe conv, 2 channel pieces across the concat boundary, tile {tile}/{stages}", bf16=4e-2,
             l2=5e-3, border=(B, H, W))
    monkeypatch.setattr(ops, "_CONV_KC_SPLITS", "auto")
    # Conv3d of SepTPWAM (27 taps, bias + GELU epilogue, tap-split forward at few rows)
    from lavt_hip._capi import ACT_GELU
    B, D, H, W, Cin, Cout, ks = 1, 4, 6, 6, 64, 64, (3, 3, 3)
    inputs = {"x": (rnd(B * D * H * W, Cin, seed=1), "act"), "w": (rnd(Cout, Cin, *ks, seed=3, scale=(27 * Cin) ** -0.5), "param"), "b": (0.1 * rnd(Cout, seed=4), "param")}

    def ref3(x, w, b):
        y = F.conv3d(x.view(B, D, H, W, Cin).permute(0, 4, 1, 2, 3), w, b, padding=1)
        return F.gelu(y.permute(0, 2, 3, 4, 1).reshape(B * D * H * W, Cout))
    run_pair(lambda x, w, b: ops.conv3d(x, w, b, B, D, H, W, act=ACT_GELU), ref3, inputs, dtype, name=f"pipe conv3d tile {tile}/{stages}", bf16=4e-2, l2=5e-3)


@pytest.mark.parametrize("tile,stages", [("512", "0"), ("128", "4")])
@pytest.mark.parametrize("B,H,W,C1,C2,Cout", [(2, 13, 11, 128, 64, 136), (1, 30, 30, 128, 0, 256), (2, 16, 8, 64, 0, 64)])
def test_conv_epilogue_column_statistics(tile, stages, B, H, W, C1, C2, Cout, monkeypatch, request):
    """BatchNorm statistics from the convolution's epilogue (lavt_gemm_nt_t.colstats, csrc/gemm_nt_pipe.hip + lavt_colstats_finish_blocks): per block of
    rows the column sums and the second moments about the block's own mean, combined in parallel-variance form.  Row counts that leave a block partly
    or wholly empty, columns that do not fill the last tile; a large common offset (|mean| / sigma ~ 50) must not cost the variance its digits.  Then the
    conv -> BatchNorm -> ReLU pair through the product ops (reference lib/mask_predictor.py:60-97) against PyTorch, forward and every gradient."""
    from lavt_hip import ops, _capi as K
    for k, v in (("LAVT_GEMM_TILE", tile), ("LAVT_GEMM_STAGES", stages), ("LAVT_GEMM_PIPE", "3")):
        monkeypatch.setenv(k, v)
    K.lib.lavt_tuning_reload()
    request.addfinalizer(lambda: ([os.environ.pop(k, None) for k in ("LAVT_GEMM_TILE", "LAVT_GEMM_STAGES", "LAVT_GEMM_PIPE")], K.lib.lavt_tuning_reload()))
    bf = torch.bfloat16
    Cin, M = C1 + C2, B * H * W
    w = rnd(Cout, Cin, 3, 3, seed=3, scale=(9 * Cin) ** -0.5)
    w[:, 0, 1, 1] += 4.0                                    # with x[:, 0] = 12.5 below: every output channel carries a common offset of ~50 sigma
    x1 = rnd(M, C1, seed=1)
    x1[:, 0] = 12.5
    x2 = rnd(M, C2, seed=2) if C2 else None
    with lavt_hip_dtype(bf):
        with torch.no_grad():
            y = ops.conv3x3(x1.to(dev()).to(bf), x2.to(dev()).to(bf) if C2 else None, w.to(dev()), B, H, W)
        assert ops.conv_stats.take(y) is None, "no statistics epilogue outside autograd"
        y = ops.conv3x3(x1.to(dev()).to(bf), x2.to(dev()).to(bf) if C2 else None, w.to(dev()), B, H, W)
        st = ops.conv_stats.take(y)
        assert st is not None, "the forced pipelined tile has the statistics epilogue"
        parts, nblk, rpb = st
        assert nblk * rpb >= M and (nblk - 1) * rpb < M + rpb
        mean = torch.empty(Cout, dtype=torch.float32, device=dev())
        rstd = torch.empty_like(mean)
        s12 = torch.empty(2, Cout, dtype=torch.float32, device=dev())
        K.check(K.lib.lavt_colstats_finish_blocks(K.ptr(parts), nblk, rpb, M, Cout, 1e-5, K.ptr(mean), K.ptr(rstd), K.ptr(s12[0]), K.ptr(s12[1]), None, None, 0.0, K.stream()))
    torch.cuda.synchronize()
    xf = (x1 if x2 is None else torch.cat([x1, x2], 1)).to(bf).float()
    yr = F.conv2d(xf.view(B, H, W, Cin).permute(0, 3, 1, 2), w.to(bf).float(), padding=1).permute(0, 2, 3, 1).reshape(M, Cout)
    mu, var = yr.mean(0), yr.var(0, unbiased=False)
    assert float(mu.abs().mean() / var.sqrt().mean()) > 20      # the offset case is what this test is about
    assert float((mean.cpu() - mu).abs().max()) <= 2e-3 * float(mu.abs().max())
    assert float((rstd.cpu() * (var + 1e-5).sqrt() - 1).abs().max()) <= 2e-3, float((rstd.cpu() * (var + 1e-5).sqrt() - 1).abs().max())
    assert float((s12[0].cpu() - yr.sum(0)).abs().max()) <= 2e-3 * float(yr.sum(0).abs().max())
    assert float((s12[1].cpu() / (var * M) - 1).abs().max()) <= 4e-3

    bn = torch.nn.BatchNorm2d(Cout)
    with torch.no_grad():
        bn.weight.copy_(1.0 + 0.2 * rnd(Cout, seed=7)); bn.bias.copy_(0.1 * rnd(Cout, seed=8))
    bn_ref = torch.nn.BatchNorm2d(Cout)
    bn_ref.load_state_dict(bn.state_dict())
    bn = bn.to(dev())
    w0 = rnd(Cout, Cin, 3, 3, seed=3, scale=(9 * Cin) ** -0.5)
    inputs = {"x1": (rnd(M, C1, seed=1), "act"), "w": (w0, "param")}
    if C2:
        inputs["x2"] = (rnd(M, C2, seed=2), "act")

    def hip(x1, w, x2=None):
        y = ops.conv3x3(x1, x2, w, B, H, W)
        return ops.batch_norm_relu(y, bn)

    def ref(x1, w, x2=None):
        x = x1 if x2 is None else torch.cat([x1, x2], 1)
        y = F.conv2d(x.view(B, H, W, Cin).permute(0, 3, 1, 2), w, padding=1)
        return F.relu(bn_ref(y)).permute(0, 2, 3, 1).reshape(M, Cout)
    hits0 = ops.conv_stats.hits
    run_pair(hip, ref, inputs, bf, name=f"conv+bn (epilogue statistics) tile {tile}", bf16=8e-2)      # (two bf16 ops: the BatchNorm backward scales the conv's rounding by gamma * rstd)
    assert ops.conv_stats.hits == hits0 + 1, "the BatchNorm took its statistics from the convolution's epilogue"
    assert float((bn.running_mean.cpu() - bn_ref.running_mean).abs().max()) <= 2e-3 and float((bn.running_var.cpu() - bn_ref.running_var).abs().max()) <= 2e-3


@pytest.mark.parametrize("dtype", DT)
def test_linear_gelu_residual(dtype):
    from lavt_hip import ops
    from lavt_hip._capi import ACT_GELU, ACT_RELU
    M, N, Kd = 520, 256, 64
    inputs = {"x": (rnd(M, Kd, seed=1), "act"), "w": (rnd(N, Kd, seed=2, scale=Kd ** -0.5), "param"), "b": (rnd(N, seed=3), "param"),
              "r": (rnd(M, N, seed=4), "act")}
    run_pair(lambda x, w, b, r: ops.linear(x, w, b, residual=r, act=ACT_GELU),
             lambda x, w, b, r: F.gelu(F.linear(x, w, b)) + r, inputs, dtype, name="linear+gelu+res")
    inputs = {"x": inputs["x"], "w": inputs["w"]}
    run_pair(lambda x, w: ops.linear(x, w, None, act=ACT_RELU), lambda x, w: F.relu(F.linear(x, w)), inputs, dtype, name="linear+relu")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("B,H,W,ws,shift", [(2, 10, 9, 7, 3), (1, 15, 15, 12, 6), (2, 14, 14, 7, 0), (2, 24, 24, 12, 6)])
def test_linear_window_gather_scatter(dtype, B, H, W, ws, shift):
    """qkv-style gather (zero rows for padding) and proj-style scatter + residual + per-sample DropPath factor."""
    from lavt_hip import ops, rowmaps
    C, N = 64, 96
    wmap_np = rowmaps.window_map_np(B, H, W, ws, shift)
    wmap = torch.from_numpy(wmap_np).to(dev())
    idx = torch.from_numpy(wmap_np.astype(np.int64))
    M = idx.numel()

    def ref_gather(x, w, b):
        xz = torch.cat([x, torch.zeros(1, x.shape[1])], 0)
        return F.linear(xz[idx], w, b)          # idx -1 -> the appended zero row
    inputs = {"x": (rnd(B * H * W, C, seed=1), "act"), "w": (rnd(N, C, seed=2, scale=C ** -0.5), "param"), "b": (rnd(N, seed=3), "param")}
    run_pair(lambda x, w, b: ops.linear(x, w, b, in_map=wmap, rows=M), ref_gather, inputs, dtype, name="gather linear")

    fac = torch.tensor([0.0, 1.0 / 0.7][:B] if B > 1 else [1.0 / 0.7])
    fac_d = fac.to(dev())

    def ref_scatter(a, w, b, r):
        y = F.linear(a, w, b) * fac.repeat_interleave(M // B)[:, None]
        keep = idx >= 0
        out = r.clone()
        out = out.index_add(0, idx[keep], y[keep])
        return out
    inputs = {"a": (rnd(M, N, seed=5), "act"), "w": (rnd(C, N, seed=6, scale=N ** -0.5), "param"), "b": (rnd(C, seed=7), "param"),
              "r": (rnd(B * H * W, C, seed=8), "act")}
    run_pair(lambda a, w, b, r: ops.linear(a, w, b, residual=r, out_map=wmap, rows=M, out_rows=B * H * W, row_scale=fac_d, row_scale_div=M // B),
             ref_scatter, inputs, dtype, name="scatter linear")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("B,H,W,C1,C2,Cout", [(2, 9, 7, 64, 32, 64), (1, 30, 30, 128, 0, 128), (2, 16, 16, 384, 96, 128), (2, 64, 64, 64, 32, 256)])
def test_conv3x3(dtype, B, H, W, C1, C2, Cout):
    from lavt_hip import ops
    Cin = C1 + C2
    inputs = {"x1": (rnd(B * H * W, C1, seed=1), "act"), "w": (rnd(Cout, Cin, 3, 3, seed=3, scale=(9 * Cin) ** -0.5), "param")}
    if C2:
        inputs["x2"] = (rnd(B * H * W, C2, seed=2), "act")

    def ref(x1, w, x2=None):
        x = x1 if x2 is None else torch.cat([x1, x2], 1)
        y = F.conv2d(x.view(B, H, W, Cin).permute(0, 3, 1, 2), w, padding=1)
        return y.permute(0, 2, 3, 1).reshape(B * H * W, Cout)
    run_pair(lambda x1, w, x2=None: ops.conv3x3(x1, x2, w, B, H, W), ref, inputs, dtype, name="conv3x3", bf16=4e-2)


@pytest.mark.parametrize("B,H,W,C1,C2,Cout", [(2, 30, 30, 128, 64, 128), (1, 60, 60, 64, 64, 128), (2, 24, 96, 64, 0, 128), (2, 120, 120, 128, 64, 256),
                                              (1, 16, 128, 64, 0, 128), (3, 7, 33, 64, 0, 128), (1, 5, 120, 64, 0, 128), (2, 120, 120, 512, 0, 512),
                                              (2, 20, 24, 64, 32, 128), (1, 16, 120, 384, 96, 384)])
def test_conv3x3_wgrad_fused_taps(B, H, W, C1, C2, Cout, monkeypatch):
    """csrc/conv_wgrad.hip (nine taps fused: image rows of X in a rolling LDS window with zero halo columns / a zero slot for rows outside the
    image, the tap shift as an LDS address, partial tiles + one reducing / transposing kernel) against the fp32 weight gradient of F.conv2d and
    against the tap-shifted TN GEMM form it replaces: every row count per k-step (W = 30 .. 128), two concat sources, image borders inside a
    piece (B > 1), a piece count that does not divide the rows, the decoder's own 2 x 120 x 120 x 512 -> 512 shape, and a skip source whose
    channels do not fill the last 64-channel tile (Swin-T's conv1_2: 384 + 96)."""
    from lavt_hip import ops, _capi as K
    Cin = C1 + C2
    assert int(K.lib.lavt_conv3x3_wgrad_ws(B, H, W, Cout, Cin, C1 if C2 else Cin)) > 0
    bf = torch.bfloat16
    x1 = rnd(B * H * W, C1, seed=1).to(bf)
    x2 = rnd(B * H * W, C2, seed=2).to(bf) if C2 else None
    dy = rnd(B * H * W, Cout, seed=3).to(bf)
    w = rnd(Cout, Cin, 3, 3, seed=4, scale=(9 * Cin) ** -0.5)

    def run(fused):
        monkeypatch.setenv("LAVT_CONV_WGRAD_TAPS", "1" if fused else "0")
        wd = w.to(dev()).requires_grad_(True)
        a1 = x1.to(dev()).requires_grad_(True)
        a2 = x2.to(dev()).requires_grad_(True) if C2 else None
        with lavt_hip_dtype(bf):
            y = ops.conv3x3(a1, a2, wd, B, H, W)
            y.backward(dy.to(dev()))
        torch.cuda.synchronize()
        return wd.grad.detach().cpu()
    got, old = run(True), run(False)
    x = (x1 if x2 is None else torch.cat([x1, x2], 1)).float().view(B, H, W, Cin).permute(0, 3, 1, 2)
    ref = torch.nn.grad.conv2d_weight(x, (Cout, Cin, 3, 3), dy.float().view(B, H, W, Cout).permute(0, 3, 1, 2), padding=1)
    scale = float(ref.abs().max())
    assert float((got - ref).abs().max()) <= 2e-3 * scale, float((got - ref).abs().max()) / scale       # exact bf16 products, fp32 sums: summation order only
    assert float((old - ref).abs().max()) <= 2e-3 * scale
    assert float((got - ref).norm() / ref.norm()) <= 2e-4                                               # norm-wise: a dropped / doubled row of one piece shows here first
    # the three tap rows / columns that touch the halo, each against its own scale (a wrong zero row or column lands in exactly these taps)
    for ky, kx in ((0, 1), (2, 1), (1, 0), (1, 2), (0, 0), (2, 2)):
        assert float((got[:, :, ky, kx] - ref[:, :, ky, kx]).abs().max()) <= 2e-3 * float(ref[:, :, ky, kx].abs().max()), (ky, kx)
    # border taps really see zeros: the corner pixel's contribution to tap (dy, dx) = (-1, -1) is absent
    assert torch.isfinite(got).all()


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("B,D,H,W,Cin,Cout,ks", [(2, 4, 6, 5, 32, 32, (3, 3, 3)), (1, 8, 9, 7, 64, 32, (3, 1, 1)), (1, 3, 8, 8, 32, 64, (1, 3, 3)),
                                                 (2, 4, 2, 2, 256, 256, (3, 3, 3)), (1, 8, 24, 24, 128, 128, (3, 3, 3))])
def test_conv3d(dtype, B, D, H, W, Cin, Cout, ks):
    """Conv3d (stride 1, 'same' padding, bias, optional GELU) of SepTPWAM as an implicit GEMM over NDHWC rows
    (lib/video_swin_transformer.py:1331-1343)"""
    from lavt_hip import ops
    from lavt_hip._capi import ACT_GELU
    taps = ks[0] * ks[1] * ks[2]
    inputs = {"x": (rnd(B * D * H * W, Cin, seed=1), "act"), "w": (rnd(Cout, Cin, *ks, seed=3, scale=(taps * Cin) ** -0.5), "param"),
              "b": (0.1 * rnd(Cout, seed=4), "param")}

    def ref(x, w, b):
        y = F.conv3d(x.view(B, D, H, W, Cin).permute(0, 4, 1, 2, 3), w, b, padding=tuple(k // 2 for k in ks))
        return F.gelu(y.permute(0, 2, 3, 4, 1).reshape(B * D * H * W, Cout))
    run_pair(lambda x, w, b: ops.conv3d(x, w, b, B, D, H, W, act=ACT_GELU), ref, inputs, dtype, name="conv3d", bf16=4e-2)


# ------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("ws,heads,H,shift", [(7, 3, 14, 3), (7, 2, 14, 0), (12, 4, 24, 6), (12, 2, 12, 6)])
def test_window_attention(dtype, ws, heads, H, shift):
    from lavt_hip import ops, rowmaps
    from oracle import lavt_oracle as O
    N, C = ws * ws, heads * 32
    nW = (H // ws) ** 2
    Bw = 2 * nW
    region_np = rowmaps.region_ids_np(H, H, ws, shift) if shift else None
    region = torch.from_numpy(region_np).to(dev()) if shift else None
    mask = O.shift_mask(H, H, ws, shift) if shift else None
    idx = O.rel_pos_index(ws).reshape(-1)

    def ref(qkv, table):
        q, k, v = qkv.view(Bw, N, 3, heads, 32).permute(2, 0, 3, 1, 4)
        a = (q * 32 ** -0.5) @ k.transpose(-1, -2) + table[idx].view(N, N, heads).permute(2, 0, 1)[None]
        if mask is not None:
            a = (a.view(Bw // nW, nW, heads, N, N) + mask[None, :, None]).view(Bw, heads, N, N)
        return (a.softmax(-1) @ v).transpose(1, 2).reshape(Bw * N, C)
    inputs = {"qkv": (rnd(Bw * N, 3 * C, seed=1), "act"), "table": (rnd((2 * ws - 1) ** 2, heads, seed=2, scale=0.5), "param")}
    run_pair(lambda qkv, table: ops.window_attention(qkv, table, region, ws, heads), ref, inputs, dtype, name="window attention")

@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("dims,window,heads,shifted", [((8, 14, 7), (8, 7, 7), 2, 1), ((8, 7, 7), (8, 7, 7), 1, 0), ((3, 14, 14), (8, 7, 7), 2, 1),
                                                       ((16, 7, 7), (8, 7, 7), 2, 1), ((4, 12, 12), (8, 12, 12), 1, 0)])
def test_window_attention_3d(dtype, dims, window, heads, shifted):
    """Video-Swin windows: 392 / 576 tokens (composed path), 147 tokens of a clipped window (fused path; the bias is the
    top-left block of the FULL window's index matrix, lib/video_swin_transformer.py:150)"""
    from lavt_hip import ops, rowmaps
    from oracle import lavt_video_oracle as OV
    win, shift = rowmaps.clip_window(dims, window, tuple(w // 2 for w in window) if shifted else (0, 0, 0))
    N, C = win[0] * win[1] * win[2], heads * 32
    nW = (dims[0] // win[0]) * (dims[1] // win[1]) * (dims[2] // win[2])
    Bw = 2 * nW
    moved = any(shift)
    region = torch.from_numpy(rowmaps.region_ids3d_np(*dims, win, shift)).to(dev()) if moved else None
    mask = OV.shift_mask_3d(*dims, win, shift) if moved else None
    idx = OV.rel_pos_index_3d(*window)[:N, :N].reshape(-1)
    R = (2 * window[0] - 1) * (2 * window[1] - 1) * (2 * window[2] - 1)

    def ref(qkv, table):
        q, k, v = qkv.view(Bw, N, 3, heads, 32).permute(2, 0, 3, 1, 4)
        a = (q * 32 ** -0.5) @ k.transpose(-1, -2) + table[idx].view(N, N, heads).permute(2, 0, 1)[None]
        if mask is not None:
            a = (a.view(Bw // nW, nW, heads, N, N) + mask[None, :, None]).view(Bw, heads, N, N)
        return (a.softmax(-1) @ v).transpose(1, 2).reshape(Bw * N, C)
    inputs = {"qkv": (rnd(Bw * N, 3 * C, seed=1), "act"), "table": (rnd(R, heads, seed=2, scale=0.5), "param")}
    run_pair(lambda qkv, table: ops.window_attention(qkv, table, region, window, heads, N=N), ref, inputs, dtype, name="window attention 3d")
    if dtype == torch.bfloat16 and 160 < N <= 400:          # bf16 routes these to the fused 25-tile kernels: keep the composed path covered too
        os.environ["LAVT_ATTN_COMPOSED"] = "1"
        try:
            run_pair(lambda qkv, table: ops.window_attention(qkv, table, region, window, heads, N=N), ref, inputs, dtype, name="window attention 3d (composed)")
        finally:
            del os.environ["LAVT_ATTN_COMPOSED"]


# ------------------------------------------------------------------------------------------------ norms
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("rows,C", [(50, 96), (333, 128), (64, 1024), (9, 2048)])
def test_layernorm(dtype, rows, C):
    from lavt_hip import ops
    inputs = {"x": (rnd(rows, C, seed=1) + 0.3, "act"), "g": (1 + 0.1 * rnd(C, seed=2), "param"), "b": (0.1 * rnd(C, seed=3), "param")}
    run_pair(lambda x, g, b: ops.layer_norm(x, g, b), lambda x, g, b: F.layer_norm(x, (C,), g, b), inputs, dtype, name="layernorm")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("B,H,W,C", [(2, 8, 6, 32), (2, 7, 5, 64), (1, 15, 15, 128)])
def test_merge_layernorm(dtype, B, H, W, C):
    from lavt_hip import ops, rowmaps
    gm = torch.from_numpy(rowmaps.merge_map_np(B, H, W)).to(dev())

    def ref(x, g, b):
        z = F.pad(x.view(B, H, W, C), (0, 0, 0, W % 2, 0, H % 2))
        z = torch.cat([z[:, 0::2, 0::2], z[:, 1::2, 0::2], z[:, 0::2, 1::2], z[:, 1::2, 1::2]], -1).reshape(-1, 4 * C)
        return F.layer_norm(z, (4 * C,), g, b)
    inputs = {"x": (rnd(B * H * W, C, seed=1), "act"), "g": (1 + 0.1 * rnd(4 * C, seed=2), "param"), "b": (0.1 * rnd(4 * C, seed=3), "param")}
    run_pair(lambda x, g, b: ops.layer_norm(x, g, b, gather=gm), ref, inputs, dtype, name="merge layernorm")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("B,T,C,with_mul", [(2, 90, 64, False), (2, 3136, 96, True), (1, 225, 1024, True)])
def test_instance_norm(dtype, B, T, C, with_mul):
    from lavt_hip import ops

    def ref(x, mul=None):
        z = x.view(B, T, C)
        y = (z - z.mean(1, keepdim=True)) / torch.sqrt(z.var(1, unbiased=False, keepdim=True) + 1e-5)
        y = y.reshape(B * T, C)
        return y * mul if mul is not None else y
    inputs = {"x": (rnd(B * T, C, seed=1) * 2 + 0.5, "act")}
    if with_mul:
        inputs["mul"] = (rnd(B * T, C, seed=2), "act")
    run_pair(lambda x, mul=None: ops.instance_norm(x, B, T, mul=mul), ref, inputs, dtype, name="instance norm", bf16=5e-2)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("training", [True, False])
def test_batchnorm_relu(dtype, training):
    from lavt_hip import ops
    R, C = 2 * 12 * 12, 64
    bn_ref = torch.nn.BatchNorm2d(C)
    bn_hip = torch.nn.BatchNorm2d(C)
    with torch.no_grad():
        for bn in (bn_ref, bn_hip):
            bn.weight.copy_(1 + 0.2 * rnd(C, seed=2)); bn.bias.copy_(0.2 * rnd(C, seed=3))
            bn.running_mean.copy_(0.1 * rnd(C, seed=4)); bn.running_var.copy_(1 + 0.3 * rnd(C, seed=5).abs())
    bn_ref.train(training); bn_hip.train(training)
    bn_hip.to(dev())
    x = rnd(R, C, seed=1) * 1.5 + 0.2
    xc = (x.to(dtype).float() if dtype == torch.bfloat16 else x).clone().requires_grad_(True)
    xg = xc.detach().to(dev()).to(dtype).requires_grad_(True)
    y_ref = F.relu(bn_ref(xc.view(2, 12, 12, C).permute(0, 3, 1, 2))).permute(0, 2, 3, 1).reshape(R, C)
    y = ops.batch_norm_relu(xg, bn_hip)
    assert_close(y, y_ref, dtype, "bn forward", bf16=4e-2)
    go = rnd(R, C, seed=9)
    y_ref.backward(go)
    y.backward(go.to(dev()).to(dtype))
    assert_close(xg.grad, xc.grad, dtype, "bn dx", 1e-3, 5e-2)
    assert_close(bn_hip.weight.grad, bn_ref.weight.grad, dtype, "bn dgamma", 1e-3, 5e-2)
    assert_close(bn_hip.bias.grad, bn_ref.bias.grad, dtype, "bn dbeta", 1e-3, 5e-2)
    if training:
        assert_close(bn_hip.running_mean, bn_ref.running_mean, torch.float32, "running_mean", 1e-4 if dtype == torch.float32 else 2e-2)
        assert_close(bn_hip.running_var, bn_ref.running_var, torch.float32, "running_var", 1e-4 if dtype == torch.float32 else 3e-2)
        assert int(bn_hip.num_batches_tracked) == 1


# ------------------------------------------------------------------------------------------------ PWAM pieces
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("G", [1, 2])
def test_pwam_attention(dtype, G):
    from lavt_hip import ops
    B, T, C, n_l, LD = 2, 90, 64, 20, 32
    valid = [9, 15]
    m = torch.zeros(B, n_l)
    for b, n in enumerate(valid):
        m[b, :n] = 1
    maskbias = torch.full((B, LD), -1e4)
    maskbias[:, :n_l] = 1e4 * m - 1e4

    def pad(t):       # (B*LD, C) with rows >= n_l (and masked words) zero, as the K/V projections produce
        z = torch.zeros(B, LD, C)
        z[:, :n_l] = t.view(B, n_l, C) * m[:, :, None]
        return z.view(B * LD, C)

    def ref(q, k, v):
        qh = q.view(B, T, G, C // G).transpose(1, 2)
        kh = k.view(B, LD, G, C // G)[:, :n_l].permute(0, 2, 3, 1)
        vh = v.view(B, LD, G, C // G)[:, :n_l].transpose(1, 2)
        s = (qh @ kh) * C ** -0.5 + (1e4 * m[:, None, None, :] - 1e4)
        return (s.softmax(-1) @ vh).transpose(1, 2).reshape(B * T, C)
    inputs = {"q": (rnd(B * T, C, seed=1), "act"), "k": (pad(rnd(B * n_l, C, seed=2)), "act"), "v": (pad(rnd(B * n_l, C, seed=3)), "act")}
    mb = maskbias.to(dev())
    # gradients of k/v are only meaningful on valid rows: compare through a masked loss by masking the reference grads too
    from lavt_hip import ops as _o
    d = dev()
    cpu = {k: t.clone().requires_grad_(True) for k, (t, _) in inputs.items()}
    if dtype == torch.bfloat16:
        cpu = {k: t.detach().to(torch.bfloat16).float().requires_grad_(True) for k, t in cpu.items()}
    gpu = {k: t.detach().to(d).to(dtype).requires_grad_(True) for k, t in cpu.items()}
    y_ref = ref(**cpu)
    y = _o.pwam_attention(gpu["q"], gpu["k"], gpu["v"], mb, B, T, n_l, G)
    assert_close(y, y_ref, dtype, "pwam attention")
    go = rnd(B * T, C, seed=7)
    y_ref.backward(go)
    y.backward(go.to(d).to(dtype))
    rowmask = torch.zeros(B, LD, 1)
    rowmask[:, :n_l] = m[:, :, None]
    rowmask = rowmask.view(B * LD, 1)
    assert_close(gpu["q"].grad, cpu["q"].grad, dtype, "pwam dq", 1e-3)
    assert_close(gpu["k"].grad.float().cpu() * rowmask, cpu["k"].grad * rowmask, dtype, "pwam dk", 1e-3)
    assert_close(gpu["v"].grad.float().cpu() * rowmask, cpu["v"].grad * rowmask, dtype, "pwam dv", 1e-3)
    assert float((gpu["k"].grad.float().cpu() * (1 - rowmask)).abs().max()) == 0.0      # masked / padded words get exactly 0


@pytest.mark.parametrize("dtype", DT)
def test_gate(dtype):
    from lavt_hip import ops
    n = (300, 64)
    inputs = {"x": (rnd(*n, seed=1), "act"), "g": (rnd(*n, seed=2), "act"), "r": (rnd(*n, seed=3), "act")}
    run_pair(lambda x, g, r: ops.gate(x, g, r), lambda x, g, r: x + torch.tanh(g) * r, inputs, dtype, name="gate")


# ------------------------------------------------------------------------------------------------ decoder / boundary pieces
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("Hi,Wi,Ho,Wo", [(4, 4, 8, 8), (15, 15, 30, 30), (7, 5, 14, 9), (3, 3, 3, 7)])
def test_bilinear(dtype, Hi, Wi, Ho, Wo):
    from lavt_hip import ops
    B, C = 2, 32

    def ref(x):
        y = F.interpolate(x.view(B, Hi, Wi, C).permute(0, 3, 1, 2), size=(Ho, Wo), mode="bilinear", align_corners=True)
        return y.permute(0, 2, 3, 1).reshape(B * Ho * Wo, C)
    run_pair(lambda x: ops.bilinear(x, B, Hi, Wi, Ho, Wo), ref, {"x": (rnd(B * Hi * Wi, C, seed=1), "act")}, dtype, name="bilinear")


@pytest.mark.parametrize("B,C,Hi,Wi,Ho,Wo", [(2, 512, 60, 60, 120, 120), (3, 192, 15, 15, 30, 30), (1, 128, 7, 5, 14, 9), (2, 64, 3, 3, 3, 7), (2, 1024, 15, 15, 30, 30),
                                              (1, 256, 9, 11, 9, 40), (2, 128, 6, 6, 1, 1), (1, 64, 1, 8, 5, 8)])
def test_bilinear_row_staged_equals_element_indexed(B, C, Hi, Wi, Ho, Wo, monkeypatch, request):
    """the row-staged bf16 upsample (input row pairs through LDS-DMA, csrc/elementwise.hip bilinear_rows_fwd_kernel) against the element-indexed kernel it
    replaces -- the same expression, so at most one bf16 rounding step apart where hipcc contracts the two kernels' multiply-adds differently (0.1 % of the
    elements) -- and against F.interpolate(align_corners=True) with the same error as the old kernel; decoder shapes, odd ratios, a single output row /
    column, a single input row"""
    from lavt_hip import ops, _capi as K
    x = rnd(B * Hi * Wi, C, seed=1).to(torch.bfloat16).to(dev())

    def run(rows):
        monkeypatch.setenv("LAVT_BILINEAR_ROWS", rows)
        K.lib.lavt_tuning_reload()
        y = torch.empty(B * Ho * Wo, C, dtype=torch.bfloat16, device=dev())
        K.check(K.lib.lavt_bilinear_fwd(K.BF16, K.ptr(x), K.ptr(y), B, Hi, Wi, Ho, Wo, C, K.stream()))
        torch.cuda.synchronize()
        return y.cpu()
    request.addfinalizer(lambda: (os.environ.pop("LAVT_BILINEAR_ROWS", None), K.lib.lavt_tuning_reload()))
    new, old = run("1"), run("0")
    d = (new.float() - old.float()).abs()
    assert float((d / old.float().abs().clamp_min(1e-3)).max()) <= 2.0 ** -7 and float((d > 0).float().mean()) < 0.01
    ref = F.interpolate(x.float().cpu().view(B, Hi, Wi, C).permute(0, 3, 1, 2), size=(Ho, Wo), mode="bilinear", align_corners=True).permute(0, 2, 3, 1).reshape(B * Ho * Wo, C)
    assert float((new.float() - ref).abs().max()) <= 1.05 * float((old.float() - ref).abs().max()) + 1e-6
    assert float((new.float() - ref).abs().max()) <= 2e-2 * float(ref.abs().max())


@pytest.mark.parametrize("dtype", DT)
def test_cls_head_and_logits_up(dtype):
    from lavt_hip import ops
    B, h, w, C, H, W = 2, 14, 12, 64, 56, 48

    def ref(x, wt, b):
        y = F.conv2d(x.view(B, h, w, C).permute(0, 3, 1, 2), wt, b)
        return F.interpolate(y, size=(H, W), mode="bilinear", align_corners=True)
    inputs = {"x": (rnd(B * h * w, C, seed=1), "act"), "wt": (rnd(2, C, 1, 1, seed=2, scale=C ** -0.5), "param"), "b": (rnd(2, seed=3), "param")}
    run_pair(lambda x, wt, b: ops.logits_upsample(ops.cls_head(x, wt, b), B, h, w, H, W), ref, inputs, dtype, name="cls head + upsample")


@pytest.mark.parametrize("dtype", DT)
def test_patch_embed(dtype):
    from lavt_hip import ops
    B, H, W, C0 = 2, 30, 27, 48

    def ref(img, wt, b):
        x = F.pad(img, (0, (-W) % 4, 0, (-H) % 4))
        return F.conv2d(x, wt, b, stride=4).flatten(2).transpose(1, 2).reshape(-1, C0)
    inputs = {"img": (rnd(B, 3, H, W, seed=1), "param"), "wt": (rnd(C0, 3, 4, 4, seed=2, scale=48 ** -0.5), "param"), "b": (rnd(C0, seed=3), "param")}
    run_pair(lambda img, wt, b: ops.patch_embed(img, wt, b, dtype), ref, inputs, dtype, name="patch embed")


@pytest.mark.parametrize("dtype", DT)
def test_transpose_boundary(dtype):
    from lavt_hip import ops
    x = rnd(2, 70, 45, seed=1)
    run_pair(lambda x: ops.transpose_last2(x), lambda x: x.transpose(1, 2).contiguous(), {"x": (x, "act")}, dtype, name="transpose")


def test_cpu_tensor_is_refused():
    from lavt_hip import ops
    with pytest.raises(RuntimeError, match="GPU memory only"):
        ops.linear(torch.zeros(8, 8), torch.zeros(8, 8))


# ------------------------------------------------------------------------------------------------ fused upsample + CE + I/U
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("B,Hi,Wi,Ho,Wo", [(2, 16, 16, 64, 64), (1, 30, 30, 120, 117), (2, 7, 9, 28, 36), (1, 120, 120, 480, 480)])
def test_upsample_cross_entropy(dtype, B, Hi, Wi, Ho, Wo):
    """fused bilinear(align_corners) upsample + F.cross_entropy(weight=[0.9, 1.1]) + I/U counts vs the unfused torch ops
    (lib/_utils.py:21, losses.py:7-11, train.py:64-76); some targets carry the ignore value"""
    from lavt_hip import ops
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B * Hi * Wi, 2, generator=g)
    tgt = torch.randint(0, 2, (B, Ho, Wo), generator=g)
    tgt[0, :2, :3] = -100
    if dtype == torch.bfloat16:
        x = x.to(dtype).float()
    xr = x.clone().requires_grad_(True)
    up = F.interpolate(xr.view(B, Hi, Wi, 2).permute(0, 3, 1, 2), size=(Ho, Wo), mode="bilinear", align_corners=True)
    ref = F.cross_entropy(up, tgt, weight=torch.tensor([0.9, 1.1]))
    (3.0 * ref).backward()
    pred = up.argmax(1)
    I, U = int(((pred == 1) & (tgt == 1)).sum()), int(((pred == 1) | (tgt == 1)).sum())
    xg = x.to(dev()).to(dtype).requires_grad_(True)
    loss, stats = ops.upsample_cross_entropy(xg, tgt.to(dev()), B, Hi, Wi, Ho, Wo, (0.9, 1.1))
    (3.0 * loss).backward()
    stats = stats.cpu()
    assert abs(float(loss) - float(ref)) <= 2e-5 * max(1.0, abs(float(ref)))
    assert abs(float(stats[1]) - float(torch.tensor([0.9, 1.1])[tgt[tgt >= 0]].sum())) <= 1e-3 * float(stats[1])
    # identical inputs on both sides; a pixel whose two upsampled logits agree to the last ulp may flip with the FMA contraction (1 of 173 541 seen)
    assert abs(int(stats[2]) - I) <= 2 and abs(int(stats[3]) - U) <= 2
    tol = 1e-5 if dtype == torch.float32 else 1e-2
    err = float((xg.grad.float().cpu() - xr.grad).abs().max()) / float(xr.grad.abs().max())
    assert err <= tol, err


# ------------------------------------------------------------------------------------------------ fused AdamW + poly schedule
def _adamw_problem():
    g = torch.Generator().manual_seed(11)
    shapes = [(33, 17), (128,), (5, 3, 3, 3), (1000, 64), (7,)]
    params = [torch.randn(*s, generator=g) for s in shapes]
    grads = [[torch.randn(*s, generator=g) * (0.1 + k) for s in shapes] for k in range(6)]
    return params, grads


def test_fused_adamw_matches_torch():
    """lavt_adamw_step vs torch.optim.AdamW + LambdaLR((1 - it/T)^0.9) (train.py:688-700): 6 steps, 3 groups (one without weight decay)"""
    from lavt_hip.optim import FusedAdamW
    params, grads = _adamw_problem()
    T = 10

    def groups(ps):
        return [{"params": ps[:2], "weight_decay": 0.0}, {"params": ps[2:4]}, {"params": ps[4:], "lr": 3e-3}]
    ref_p = [torch.nn.Parameter(p.clone()) for p in params]
    ref = torch.optim.AdamW(groups(ref_p), lr=1e-2, weight_decay=0.05)
    sched = torch.optim.lr_scheduler.LambdaLR(ref, lambda x: (1 - x / T) ** 0.9)
    our_p = [torch.nn.Parameter(p.clone().to(dev())) for p in params]
    ours = FusedAdamW(groups(our_p), lr=1e-2, weight_decay=0.05, total_steps=T, power=0.9)
    for k in range(6):
        for p, q, gr in zip(ref_p, our_p, grads[k]):
            p.grad = gr.clone()
            q.grad = gr.clone().to(dev())
        ref.step()
        sched.step()
        ours.step()
        for p, q in zip(ref_p, our_p):
            err = float((q.detach().cpu() - p.detach()).abs().max())
            assert err <= 2e-6 * max(1.0, float(p.abs().max())), (k, err)
    assert ours.steps_taken() == 6 and abs(ours.current_lr_factor() - (1 - 6 / T) ** 0.9) < 1e-6
    sd = ours.state_dict()
    assert set(sd["state"][0]) >= {"step", "exp_avg", "exp_avg_sq"} and sd["lavt_schedule"]["steps_taken"] == 6
    again = FusedAdamW(groups([torch.nn.Parameter(p.detach().clone()) for p in our_p]), lr=1e-2, weight_decay=0.05)
    again.load_state_dict(sd)
    assert again.steps_taken() == 6 and again.total_steps == T


def test_fused_adamw_keeps_the_compute_copies_current():
    """FusedAdamW's update kernel writes the bf16 compute copies of the Linear weights itself (lavt_adamw_step_chunks, `copy` column) and refreshes the
    LayerNorm folds in one launch (lavt_ln_fold_multi): after a step every cached copy equals what a fresh cast / fold of the updated parameters gives"""
    from lavt_hip import ops
    from lavt_hip.optim import FusedAdamW
    g = torch.Generator().manual_seed(11)
    mk = lambda *sh: torch.nn.Parameter((torch.randn(*sh, generator=g) * 0.3).to(dev()))
    W, b, gamma, beta, W2 = mk(192, 128), mk(192), mk(128), mk(128), mk(20000, 64)          # W2: several chunks + a partial last one
    c1, c2 = ops.weights.get(W, torch.bfloat16, "lin"), ops.weights.get(W2, torch.bfloat16, "lin")
    Wg, wsum, biasp = ops.weights.get_lnfold(W, b, gamma, beta)
    ptrs = (c1.data_ptr(), c2.data_ptr(), Wg.data_ptr())
    opt = FusedAdamW([W, b, gamma, beta, W2], lr=3e-2, weight_decay=1e-2)
    for it in range(2):
        for p in (W, b, gamma, beta, W2):
            p.grad = torch.randn(p.shape, generator=g).to(dev())
        before = W.detach().clone()
        opt.step()
    torch.cuda.synchronize()
    assert len(opt._tables[6]) == 2 and float((W - before).abs().max()) > 1e-3
    c1n, c2n = ops.weights.get(W, torch.bfloat16, "lin"), ops.weights.get(W2, torch.bfloat16, "lin")
    Wgn, wsumn, biaspn = ops.weights.get_lnfold(W, b, gamma, beta)
    assert (c1n.data_ptr(), c2n.data_ptr(), Wgn.data_ptr()) == ptrs                           # static addresses (hipGraph replays)
    assert torch.equal(c1n, W.detach().to(torch.bfloat16)) and torch.equal(c2n.view(-1), W2.detach().to(torch.bfloat16).view(-1))
    ref_g = (W.detach() * gamma.detach()[None, :]).to(torch.bfloat16)
    assert torch.equal(Wgn, ref_g)
    assert float((wsumn - ref_g.float().sum(1)).abs().max()) <= 1e-4 * float(ref_g.float().abs().sum(1).max())
    ref_b = b.detach() + W.detach() @ beta.detach()
    assert float((biaspn - ref_b).abs().max()) <= 1e-4 * max(float(ref_b.abs().max()), 1.0)


def test_fused_adamw_in_hip_graph():
    """the device-side step counter keeps the schedule moving when the optimizer step is replayed from a captured hipGraph"""
    from lavt_hip.optim import FusedAdamW
    params, grads = _adamw_problem()
    eager_p = [torch.nn.Parameter(p.clone().to(dev())) for p in params]
    graph_p = [torch.nn.Parameter(p.clone().to(dev())) for p in params]
    for ps in (eager_p, graph_p):
        for q, gr in zip(ps, grads[0]):
            q.grad = gr.clone().to(dev())
    eager = FusedAdamW(eager_p, lr=1e-2, total_steps=8)
    captured = FusedAdamW(graph_p, lr=1e-2, total_steps=8)
    for _ in range(4):
        eager.step()
    captured.step()                                   # builds the tables outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured.step(check_tables=False)
    for _ in range(3):                                # capture itself executes nothing
        g.replay()
    torch.cuda.synchronize()
    assert captured.steps_taken() == 4
    for p, q in zip(eager_p, graph_p):
        assert float((p - q).abs().max()) <= 1e-7 * max(1.0, float(p.abs().max()))


def test_fused_adamw_refuses_a_table_from_before_the_bucket_relayout():
    """GradBuckets lays its flat buffer out again in the second zero() (a parameter nothing reported in step 1 joins the late bucket): every p.grad
    may move.  step(check_tables=False) skips the host-side pointer scan, so it must refuse the descriptor table built on the old layout instead of
    reading gradients at stale offsets; a step with check_tables=True rebuilds it and the update then equals torch.optim.AdamW's."""
    from lavt_hip.ddp import GradBuckets
    from lavt_hip.optim import FusedAdamW
    torch.manual_seed(0)
    net = torch.nn.Sequential(*[torch.nn.Linear(16, 16, bias=False) for _ in range(4)]).to(dev())
    twin = torch.nn.Sequential(*[torch.nn.Linear(16, 16, bias=False) for _ in range(4)]).to(dev())
    twin.load_state_dict(net.state_dict())
    ps, dead = list(net.parameters()), 2
    gb = GradBuckets(net, bucket_mib=2 * 256 * 4 / (1 << 20))          # two weights per bucket: the dead one gates bucket 0 in step 1
    opt = FusedAdamW(ps, lr=1e-2, total_steps=0)
    ref = torch.optim.AdamW(twin.parameters(), lr=1e-2)
    g = [torch.randn(16, 16, generator=torch.Generator("cpu").manual_seed(i)).to(dev()) for i in range(4)]

    def backward():
        gb.zero()
        for i in reversed(range(4)):
            if i != dead:
                ps[i].grad.copy_(g[i])
                gb._on_grad(ps[i])
        gb.finish()
    backward()
    before = [p.grad.data_ptr() for p in ps]
    opt.step()                                       # tables built on the first layout
    backward()                                       # second zero(): relayout
    assert [p.grad.data_ptr() for p in ps] != before
    with pytest.raises(RuntimeError, match="laid out again"):
        opt.step(check_tables=False)
    opt.step()                                       # rebuilds
    opt.step(check_tables=False)                     # and the rebuilt table is accepted
    for i, q in enumerate(twin.parameters()):
        q.grad = torch.zeros_like(q) if i == dead else g[i].clone()
    for _ in range(3):
        ref.step()
    torch.cuda.synchronize()
    for p, q in zip(ps, twin.parameters()):
        assert float((p - q).abs().max()) <= 2e-6 * max(1.0, float(q.abs().max()))


# ------------------------------------------------------------------------------------------------ grouped weight-gradient launch
def test_gemm_tn_grouped_matches_individual():
    """lavt_gemm_tn_grouped (one launch; the deferred members declare zeroed outputs, so the 41-K-tile qkv / proj reductions are cut in two and
    meet through atomics while fc1 / fc2 store plainly) vs the same problems through lavt_gemm_tn: a Swin block's four weight gradients incl.
    a gathered operand, a row mask folded into alpha and a bias column sum"""
    import ctypes as C
    from lavt_hip import _capi as K, ops
    g = torch.Generator().manual_seed(21)
    M, Mw, Cc = 1800, 2592, 512
    bf = torch.bfloat16
    wmap = torch.randint(0, M, (Mw,), generator=g, dtype=torch.int32).to(dev())
    mask = (torch.rand(2, generator=g) > 0.3).float().to(dev())               # per-sample DropPath mask (0 / 1), value folded into alpha
    probs = []          # (I, J, Kd, A, B, kwargs)
    def mk(rows, cols):
        return (torch.randn(rows, cols, generator=g) * 0.5).to(dev()).to(bf)
    probs.append((4 * Cc, Cc, M, mk(M, 4 * Cc), mk(M, Cc), dict()))                                              # fc1
    probs.append((Cc, 4 * Cc, M, mk(M, Cc), mk(M, 4 * Cc), dict(a_rowscale=mask, a_rowscale_div=M // 2, a_rowscale_binary=True, alpha=1.25)))   # fc2 + DropPath
    probs.append((3 * Cc, Cc, Mw, mk(Mw, 3 * Cc), mk(M, Cc), dict(b_rowmap=wmap)))                               # qkv (gathered input)
    probs.append((Cc, Cc, Mw, mk(M, Cc), mk(Mw, Cc), dict(a_rowmap=wmap)))                                       # proj (gathered gradient)
    outs_ref, outs_grp, structs, keep = [], [], [], []
    class _Q:
        def add(self, p, t, extra=False): structs.append(p); keep.append(t)
    for I, J, Kd, A, B, kw in probs:
        ref = torch.zeros(I, J, device=dev()); cs_ref = torch.zeros(I, device=dev())
        ops.gemm_tn(bf, I, J, Kd, A, I, B, J, ref, J, colsum=cs_ref, **kw)
        out = torch.zeros(I, J, device=dev()); cs = torch.zeros(I, device=dev())
        ops.gemm_tn(bf, I, J, Kd, A, I, B, J, out, J, colsum=cs, defer=_Q(), **kw)
        outs_ref.append((ref, cs_ref)); outs_grp.append((out, cs))
    arr = (K.GemmTN * len(structs))(*structs)
    K.check(K.lib.lavt_gemm_tn_grouped(arr, len(structs), K.stream()))
    torch.cuda.synchronize()
    for (r, cr), (o, co) in zip(outs_ref, outs_grp):
        scale = float(r.abs().max())
        assert float((r - o).abs().max()) <= 2e-3 * scale, float((r - o).abs().max()) / scale        # fp32 summation order only
        assert float((cr - co).abs().max()) <= 2e-3 * float(cr.abs().max())


@pytest.mark.parametrize("stages,Kd,min_tiles", [("4", 1800, "8"), ("4", 7200, "8"), ("4", 456, "8"), ("3", 1800, "8"), ("3", 7200, "8"),
                                                  ("4", 7200, "4096"), ("4", 28800, "4096"), ("4", 450, "8"), ("4", 900, "8"), ("4", 900, "4096")])
def test_gemm_tn_grouped_pipelined_tiles(Kd, stages, min_tiles, monkeypatch, request):
    """csrc/gemm_tn_pipe.hip (round 5: the grouped weight-gradient launch on 128x128 software-pipelined tiles -- buffer-descriptor LDS-DMA of two
    k-major operand tiles, transposing fragment reads one MFMA group ahead, row maps through scalar loads, the DropPath mask as a keep bit per
    sample, column sums on the matrix cores) against fp32 torch and against gemm_tn_v2.hip's 64x64 launch (LAVT_TN_PIPE=0): six members with
    every feature at once -- tiles that overhang I and J (I = 192, J = 328), a K tail of 8 rows (1800 = 28 x 64 + 8; 456 = 7 x 64 + 8), gathered
    reductions whose length is not a multiple of 8 (450 = the last stage's tokens, 900 = batch 4's: the row maps end inside a wave's eight entries), a long chain
    (7200 = 113 K tiles), gathered A rows with masked (-1) entries, gathered B rows, a row mask folded into alpha, accumulate into a non-zero C,
    a column-sum-only member adding atomically into a bias gradient it shares with a second member, an unaligned C (4-byte stores) -- in both ring depths.
    min_tiles = 4096: the same group CUT INTO K PIECES (the form long reductions on few output tiles take: every member through its partials scratch,
    pieces of equal length, one reduction kernel)."""
    from lavt_hip import _capi as K, ops
    monkeypatch.setenv("LAVT_TN_PIPE_STAGES", stages)
    monkeypatch.setenv("LAVT_TN_PIPE_MIN_TILES", min_tiles)
    monkeypatch.setenv("LAVT_TN_PIPE_MIN_KTILES", "1")          # (the planner keeps uncut groups of < 12 K tiles per tile on the 64x64 launch: here they take the pipelined one)
    request.addfinalizer(lambda: ([os.environ.pop(k, None) for k in ("LAVT_TN_PIPE", "LAVT_TN_PIPE_STAGES", "LAVT_TN_PIPE_MIN_TILES", "LAVT_TN_PIPE_MIN_KTILES")], K.lib.lavt_tuning_reload()))
    g = torch.Generator().manual_seed(77)
    bf = torch.bfloat16
    Ms = Kd + 640                                                               # rows of the gathered sources
    def mk(rows, cols):
        return (torch.randn(rows, cols, generator=g) * 0.5).to(dev()).to(bf)
    amap = torch.randint(-1, Ms, (Kd,), generator=g, dtype=torch.int32).to(dev())
    bmap = torch.randint(0, Ms, (Kd,), generator=g, dtype=torch.int32).to(dev())
    nsmp = 4 if Kd % 4 == 0 else 2
    mask = torch.tensor([1.0, 0.0, 1.0, 1.0][:nsmp]).to(dev())
    shared_bias = lambda: torch.zeros(384, device=dev())
    flat = torch.zeros(512 * 512 + 3, device=dev())
    def members(bias):
        return [
            (2048, 512, mk(Kd, 2048), mk(Kd, 512), dict(), None),                                                              # plain (fc1)
            (512, 2048, mk(Kd, 512), mk(Kd, 2048), dict(a_rowscale=mask, a_rowscale_div=Kd // nsmp, a_rowscale_binary=True, alpha=1.25), None),   # row mask (fc2 + DropPath)
            (192, 328, mk(Ms, 192), mk(Ms, 328), dict(a_rowmap=amap, b_rowmap=bmap, accumulate=True), None),                  # both gathered, overhanging tiles, accumulate
            (384, 8, mk(Ms, 384), None, dict(a_rowmap=bmap, colsum_atomic=True), bias),                                        # column sums only (padded rows' bias share)
            (384, 256, mk(Ms, 384), mk(Kd, 256), dict(a_rowmap=amap, colsum_atomic=True), bias),                               # gathered A + shared bias gradient
            (512, 512, mk(Kd, 512), mk(Kd, 512), dict(), "unaligned"),                                                         # C at a 12-byte offset
        ]
    def run(pipe):
        monkeypatch.setenv("LAVT_TN_PIPE", "2" if pipe == "1" else "0")
        K.lib.lavt_tuning_reload()
        g.manual_seed(77)
        torch.randint(-1, Ms, (Kd,), generator=g); torch.randint(0, Ms, (Kd,), generator=g)          # (same operand stream in both runs)
        bias = shared_bias()
        structs, keep, outs = [], [], []
        class _Q:
            def add(self, p, t, extra=False, rider=None): structs.append(p); keep.append(t)
        for I, J, A, B, kw, extra in members(bias):
            if extra == "unaligned":
                flat.zero_()
                out = flat[3:3 + I * J].view(I, J)
            else:
                out = torch.full((I, J), 0.25 if kw.get("accumulate") else 0.0, device=dev())
            cs = extra if torch.is_tensor(extra) else torch.zeros(I, device=dev())
            if B is None:
                ops.gemm_tn(bf, I, 8, Kd, A, I, ops._zero_page_tensor(dev()), 0, out, 8, colsum=cs, defer=_Q(), extra=True, **kw)
            else:
                ops.gemm_tn(bf, I, J, Kd, A, I, B, J, out, J, colsum=cs, defer=_Q(), **kw)
            outs.append((out, cs, A, B, kw))
        ops.assign_partials(structs, dev())
        arr = (K.GemmTN * len(structs))(*structs)
        K.check(K.lib.lavt_gemm_tn_grouped(arr, len(structs), K.stream()))
        torch.cuda.synchronize()
        return [(o.clone(), c.clone(), A, B, kw) for o, c, A, B, kw in outs]
    new, old = run("1"), run("0")
    rows = torch.arange(Kd, device=dev())
    for idx, ((o, c, A, B, kw), (o0, c0, _, _, _)) in enumerate(zip(new, old)):
        Af = A.float()
        if "a_rowmap" in kw:
            m = kw["a_rowmap"].long()
            Af = torch.where(m[:, None] >= 0, Af[m.clamp(min=0)], torch.zeros(1, device=dev()))
        if "a_rowscale" in kw:
            Af = Af * mask[(rows // kw["a_rowscale_div"]).clamp(max=nsmp - 1)][:, None] * kw["alpha"]
        if B is not None:
            Bf = B.float()[kw["b_rowmap"].long()] if "b_rowmap" in kw else B.float()
            ref = Af.t() @ Bf + (0.25 if kw.get("accumulate") else 0.0)
            scale = float(ref.abs().max())
            assert torch.isfinite(o).all(), idx
            assert float((o - ref).abs().max()) <= 2e-3 * scale, (idx, float((o - ref).abs().max()) / scale)
            assert float((o - ref).norm() / ref.norm()) <= 1e-4, idx                                    # exact bf16 products, fp32 sums
            assert float((o - o0).abs().max()) <= 1e-3 * scale, idx                                    # and the 64x64 launch agrees
        else:
            assert float(o.abs().max()) == 0.0
    bias_ref = sum(torch.where(kw["a_rowmap"].long()[:, None] >= 0, A.float()[kw["a_rowmap"].long().clamp(min=0)], torch.zeros(1, device=dev())).sum(0)
                   for o, c, A, B, kw in new if kw.get("colsum_atomic"))
    for res in (new, old):
        got = res[3][1]
        assert float((got - bias_ref).abs().max()) <= 2e-3 * float(bias_ref.abs().max())
    for idx in (0, 1, 2, 5):
        c, A, kw = new[idx][1], new[idx][2], new[idx][4]
        Af = A.float()
        if "a_rowmap" in kw:
            m = kw["a_rowmap"].long()
            Af = torch.where(m[:, None] >= 0, Af[m.clamp(min=0)], torch.zeros(1, device=dev()))
        if "a_rowscale" in kw:
            Af = Af * mask[(rows // kw["a_rowscale_div"]).clamp(max=nsmp - 1)][:, None] * kw["alpha"]
        cref = Af.sum(0)
        assert float((c - cref).abs().max()) <= 2e-3 * float(cref.abs().max()), idx


@pytest.mark.parametrize("B,H,ws,shift,Cc", [(2, 30, 12, 6, 512), (2, 15, 12, 0, 1024), (3, 10, 7, 3, 256), (8, 30, 12, 6, 512)])
def test_gemm_tn_token_order_matches_window_order(B, H, ws, shift, Cc):
    """The windowed members of a Swin block's grouped weight-gradient launch in TOKEN order (contraction over the real tokens through the inverse
    window map; the padded window rows -- zero input rows whose dq / dk / dv still count for the qkv bias gradient -- summed by a column-sum-only
    side member, both added atomically: lavt_gemm_tn_t.colsum_atomic) against the same gradients in window order."""
    import ctypes as C
    from lavt_hip import _capi as K, ops, rowmaps
    g = torch.Generator().manual_seed(5)
    bf = torch.bfloat16
    wmap = rowmaps.window_map(B, H, H, ws, shift, dev())
    inv, pad = rowmaps.window_inverse(B, H, H, ws, shift, dev()), rowmaps.window_pad_rows(B, H, H, ws, shift, dev())
    T, Mw = B * H * H, wmap.numel()
    assert pad.numel() == Mw - T and bool((wmap[inv.long()] == torch.arange(T, device=dev())).all())
    def mk(rows, cols):
        return (torch.randn(rows, cols, generator=g) * 0.5).to(dev()).to(bf)
    dqkv, xn, dy, o = mk(Mw, 3 * Cc), mk(T, Cc), mk(T, Cc), mk(Mw, Cc)
    fc = [(4 * Cc, Cc, T, mk(T, 4 * Cc), mk(T, Cc)), (Cc, 4 * Cc, T, mk(T, Cc), mk(T, 4 * Cc))]          # the block's MLP members fill the launch
    structs, keep = [], []
    class _Q:
        def add(self, p, t, extra=False): structs.append(p); keep.append(t)
    # window order (reference form)
    w_qkv, b_qkv, w_proj, b_proj = (torch.zeros(3 * Cc, Cc, device=dev()), torch.zeros(3 * Cc, device=dev()), torch.zeros(Cc, Cc, device=dev()), torch.zeros(Cc, device=dev()))
    ops.gemm_tn(bf, 3 * Cc, Cc, Mw, dqkv, 3 * Cc, xn, Cc, w_qkv, Cc, b_rowmap=wmap, colsum=b_qkv)
    ops.gemm_tn(bf, Cc, Cc, Mw, dy, Cc, o, Cc, w_proj, Cc, a_rowmap=wmap, colsum=b_proj)
    # token order, one grouped launch
    t_qkv, tb_qkv, t_proj, tb_proj = (torch.zeros_like(w_qkv), torch.zeros_like(b_qkv), torch.zeros_like(w_proj), torch.zeros_like(b_proj))
    outs = []
    for I, J, Kd, A, Bm in fc:
        out = torch.zeros(I, J, device=dev()); outs.append((out, A, Bm))
        ops.gemm_tn(bf, I, J, Kd, A, I, Bm, J, out, J, defer=_Q())
    ops.gemm_tn(bf, Cc, Cc, T, dy, Cc, o, Cc, t_proj, Cc, b_rowmap=inv, colsum=tb_proj, defer=_Q())
    dummy = torch.zeros(3 * Cc, 8, device=dev())          # (zeros: a member cut into partial tiles ADDS its -- zero -- sum to what C holds)
    ops.gemm_tn(bf, 3 * Cc, 8, pad.numel(), dqkv, 3 * Cc, ops._zero_page_tensor(dev()), 0, dummy, 8, a_rowmap=pad, colsum=tb_qkv, colsum_atomic=True, defer=_Q(), extra=True)
    ops.gemm_tn(bf, 3 * Cc, Cc, T, dqkv, 3 * Cc, xn, Cc, t_qkv, Cc, a_rowmap=inv, colsum=tb_qkv, colsum_atomic=True, defer=_Q())
    assert len(structs) == 5
    if B == 8:          # the reference's default batch per GPU: 3168 padded rows and 7200 tokens -- BOTH members that add into the qkv bias gradient are
        assert pad.numel() >= 3136 and structs[3].partials and structs[4].partials      # cut into pieces through partial tiles (their sums met in a plain += of one launch)
    ops.assign_partials(structs, dev())
    arr = (K.GemmTN * len(structs))(*structs)
    K.check(K.lib.lavt_gemm_tn_grouped(arr, len(structs), K.stream()))
    torch.cuda.synchronize()
    for nm, r, t in (("qkv.weight", w_qkv, t_qkv), ("qkv.bias", b_qkv, tb_qkv), ("proj.weight", w_proj, t_proj), ("proj.bias", b_proj, tb_proj)):
        scale = float(r.abs().max())
        assert float((r - t).abs().max()) <= 2e-3 * scale, (nm, float((r - t).abs().max()) / scale)      # fp32 summation order only
    assert float(dummy.abs().max()) == 0.0
    for out, A, Bm in outs:
        ref = A.float().t() @ Bm.float()
        assert float((out - ref).abs().max()) <= 2e-3 * float(ref.abs().max())
    # the qkv bias gradient really contains the padded rows' share
    share = dqkv[pad.long()].float().sum(0)
    assert float(share.abs().max()) > 0 and float((tb_qkv - b_qkv).abs().max()) < 0.05 * float(share.abs().max())


@pytest.mark.parametrize("B,H,ws,shift,Cc", [(2, 30, 12, 6, 512), (2, 15, 12, 0, 1024), (4, 30, 12, 6, 512), (2, 60, 12, 6, 256)])
def test_gemm_tn_grouped_streamk(B, H, ws, shift, Cc):
    """Stream-K form of a Swin block's grouped weight-gradient launch (lavt_gemm_tn_grouped_sk: 128x128 tiles, equal runs of K-tile iterations per
    persistent workgroup, split tiles through scratch slots + a fixed-order fix-up) on the five token-order members (row maps, matrix-core
    column sums, the column-sum-only side member adding atomically into the shared bias gradient) against fp32 torch, and bit-identical
    between two runs (no atomics in the split reductions)."""
    from lavt_hip import _capi as K, ops, rowmaps
    g = torch.Generator().manual_seed(7)
    bf = torch.bfloat16
    wmap = rowmaps.window_map(B, H, H, ws, shift, dev())
    inv, pad = rowmaps.window_inverse(B, H, H, ws, shift, dev()), rowmaps.window_pad_rows(B, H, H, ws, shift, dev())
    T, Mw = B * H * H, wmap.numel()
    def mk(rows, cols):
        return (torch.randn(rows, cols, generator=g) * 0.5).to(dev()).to(bf)
    dqkv, xn, dy, o = mk(Mw, 3 * Cc), mk(T, Cc), mk(T, Cc), mk(Mw, Cc)
    dpre, x2, dy2, h = mk(T, 4 * Cc), mk(T, Cc), mk(T, Cc), mk(T, 4 * Cc)

    def run():
        structs, keep = [], []
        class _Q:
            def add(self, p, t, extra=False): structs.append(p); keep.append(t)
        outs = {k: torch.zeros(*shp, device=dev()) for k, shp in (("fc1.w", (4 * Cc, Cc)), ("fc1.b", (4 * Cc,)), ("fc2.w", (Cc, 4 * Cc)), ("fc2.b", (Cc,)), ("proj.w", (Cc, Cc)),
                                                                   ("proj.b", (Cc,)), ("qkv.w", (3 * Cc, Cc)), ("qkv.b", (3 * Cc,)))}
        ops.gemm_tn(bf, Cc, 4 * Cc, T, dy2, Cc, h, 4 * Cc, outs["fc2.w"], 4 * Cc, colsum=outs["fc2.b"], defer=_Q())
        ops.gemm_tn(bf, 4 * Cc, Cc, T, dpre, 4 * Cc, x2, Cc, outs["fc1.w"], Cc, colsum=outs["fc1.b"], defer=_Q())
        ops.gemm_tn(bf, Cc, Cc, T, dy, Cc, o, Cc, outs["proj.w"], Cc, b_rowmap=inv, colsum=outs["proj.b"], defer=_Q())
        dummy = torch.zeros(3 * Cc, 8, device=dev())
        if pad.numel():                 # (no side member when the grid is a whole number of windows: 60 = 5 x 12)
            ops.gemm_tn(bf, 3 * Cc, 8, pad.numel(), dqkv, 3 * Cc, ops._zero_page_tensor(dev()), 0, dummy, 8, a_rowmap=pad, colsum=outs["qkv.b"], colsum_atomic=True, defer=_Q(), extra=True)
        ops.gemm_tn(bf, 3 * Cc, Cc, T, dqkv, 3 * Cc, xn, Cc, outs["qkv.w"], Cc, a_rowmap=inv, colsum=outs["qkv.b"], colsum_atomic=True, defer=_Q())
        arr = (K.GemmTN * len(structs))(*structs)
        need = int(K.lib.lavt_gemm_tn_grouped_sk_ws(arr, len(structs)))
        assert need > 0, "the Swin-block group must qualify for the stream-K launch"
        scr = torch.full((need,), float("nan"), device=dev())             # stale scratch must never leak into a result
        K.check(K.lib.lavt_gemm_tn_grouped_sk(arr, len(structs), K.ptr(scr), scr.numel(), K.stream()))
        torch.cuda.synchronize()
        return outs
    a, b = run(), run()
    f = lambda t: t.float()
    ref = {"fc2.w": f(dy2).t() @ f(h), "fc2.b": f(dy2).sum(0), "fc1.w": f(dpre).t() @ f(x2), "fc1.b": f(dpre).sum(0),
           "proj.w": f(dy).t() @ f(o)[inv.long()], "proj.b": f(dy).sum(0), "qkv.w": f(dqkv)[inv.long()].t() @ f(xn), "qkv.b": f(dqkv).sum(0)}
    for k, r in ref.items():
        scale = float(r.abs().max())
        assert torch.isfinite(a[k]).all(), k
        assert float((a[k] - r).abs().max()) <= 2e-3 * scale, (k, float((a[k] - r).abs().max()) / scale)
        if k != "qkv.b":                      # (two members add into qkv.b atomically: two addends into zeros, order-independent -- also identical)
            assert torch.equal(a[k], b[k]), f"{k}: two runs differ"
    assert torch.equal(a["qkv.b"], b["qkv.b"])


@pytest.mark.parametrize("Cc,T", [(512, 1800), (128, 28800), (256, 7200), (1024, 450), (512, 1804), (256, 3600)])
def test_grouped_wgrad_with_layernorm_rider(Cc, T):
    """lavt_gemm_tn_grouped_ln: the partial-sum LayerNorm backward as rider workgroups of a Swin block's grouped weight-gradient launch (C = 1024 and
    groups that do not form fall back to two launches inside the call; (512, 1800) rides on the 128x128 pipelined launch of round 5 as two 256-thread
    units per 512-thread workgroup, (512, 1804) with an odd unit count -- the spare half repeats the last unit --, (256, 3600) with 32 lanes per row)
    -- dx and the per-workgroup d gamma / d beta partials bit-identical to
    lavt_layernorm_bwd_partial on its own, the weight gradients identical to lavt_gemm_tn_grouped."""
    from lavt_hip import _capi as K, ops
    g = torch.Generator().manual_seed(11)
    bf = torch.bfloat16
    def mk(rows, cols, s=0.5):
        return (torch.randn(rows, cols, generator=g) * s).to(dev()).to(bf)
    dy2, h, dpre, x2, dyp, o, dqkv, xn = mk(T, Cc), mk(T, 4 * Cc), mk(T, 4 * Cc), mk(T, Cc), mk(T, Cc), mk(T, Cc), mk(T, 3 * Cc), mk(T, Cc)
    dxn, x, dres = mk(T, Cc), mk(T, Cc, 1.0), mk(T, Cc)
    gamma = (1.0 + 0.1 * torch.randn(Cc, generator=g)).to(dev())
    mean, rstd = x.float().mean(1), torch.rsqrt(x.float().var(1, unbiased=False) + 1e-5)
    nblk = int(K.lib.lavt_layernorm_bwd_blocks(K.BF16, T, Cc))

    def run(ride):
        structs, keep = [], []
        class _Q:
            def add(self, p, t, extra=False, rider=None): structs.append(p); keep.append(t)
        outs = [torch.zeros(Cc, 4 * Cc, device=dev()), torch.zeros(4 * Cc, Cc, device=dev()), torch.zeros(Cc, Cc, device=dev()), torch.zeros(3 * Cc, Cc, device=dev())]
        bs = [torch.zeros(Cc, device=dev()), torch.zeros(4 * Cc, device=dev()), torch.zeros(Cc, device=dev()), torch.zeros(3 * Cc, device=dev())]
        ops.gemm_tn(bf, Cc, 4 * Cc, T, dy2, Cc, h, 4 * Cc, outs[0], 4 * Cc, colsum=bs[0], defer=_Q())
        ops.gemm_tn(bf, 4 * Cc, Cc, T, dpre, 4 * Cc, x2, Cc, outs[1], Cc, colsum=bs[1], defer=_Q())
        ops.gemm_tn(bf, Cc, Cc, T, dyp, Cc, o, Cc, outs[2], Cc, colsum=bs[2], defer=_Q())
        ops.gemm_tn(bf, 3 * Cc, Cc, T, dqkv, 3 * Cc, xn, Cc, outs[3], Cc, colsum=bs[3], defer=_Q())
        ops.assign_partials(structs, dev())
        arr = (K.GemmTN * len(structs))(*structs)
        dx = torch.empty_like(x)
        ws = torch.full((nblk * 2 * Cc,), float("nan"), device=dev())
        if ride:
            K.check(K.lib.lavt_gemm_tn_grouped_ln(arr, len(structs), K.ptr(dxn), K.ptr(x), K.ptr(gamma), K.ptr(mean), K.ptr(rstd), K.ptr(dx), K.ptr(ws), ws.numel(),
                                                  K.ptr(dres), T, Cc, K.stream()))
        else:
            K.check(K.lib.lavt_gemm_tn_grouped(arr, len(structs), K.stream()))
            K.check(K.lib.lavt_layernorm_bwd_partial(K.BF16, K.ptr(dxn), K.ptr(x), None, K.ptr(gamma), K.ptr(mean), K.ptr(rstd), K.ptr(dx), K.ptr(ws), ws.numel(),
                                                     K.ptr(dres), T, Cc, K.stream()))
        torch.cuda.synchronize()
        return outs + bs + [dx, ws]
    a, b = run(True), run(False)
    for i, (u, v) in enumerate(zip(a, b)):
        assert torch.isfinite(u.float()).all(), i
        if i < 8 and not torch.equal(u, v):
            # (weight / bias gradients of a group that is cut into K pieces: with riders on board the launch leaves a fifth of the chip to them, so its
            # pieces are longer than without -- the same sums in another fp32 order; uncut groups are bit-identical)
            assert float((u - v).abs().max()) <= 2e-5 * float(v.abs().max()), f"tensor {i}: ridden and separate launches differ beyond fp32 summation order"
            continue
        assert torch.equal(u, v), f"tensor {i}: ridden and separate launches differ"
    # and the LayerNorm backward itself against fp32 torch
    xh = (x.float() - mean[:, None]) * rstd[:, None]
    gg = dxn.float() * gamma
    ref = rstd[:, None] * (gg - gg.mean(1, keepdim=True) - xh * (gg * xh).mean(1, keepdim=True)) + dres.float()
    assert float((a[8].float() - ref).abs().max()) <= 3e-2 * float(ref.abs().max())


def test_gemm_tn_split_through_partial_tiles(monkeypatch):
    """Long-K weight gradients on few output tiles (PWAM's 1x1 convolutions: K = 28 800 rows on 4 tiles): the K pieces store plain partial tiles
    into the lent scratch and a second kernel adds them into C (lavt_gemm_tn_t.partials, ABI v3) -- against the atomic form of the same launch
    and against fp32 torch; C accumulates (it holds a previous value), colsum and a gathered operand with masked rows included.  Then four such
    problems through lavt_gemm_tn_grouped (every member cut into pieces of 8 K tiles, one reduction kernel)."""
    from lavt_hip import _capi as K, ops
    bf = torch.bfloat16
    g = torch.Generator().manual_seed(33)
    Kd = 28800
    def mk(rows, cols):
        return (torch.randn(rows, cols, generator=g) * 0.25).to(dev()).to(bf)
    rmap = torch.randint(-1, 7200, (Kd,), generator=g, dtype=torch.int32).to(dev())         # gathered B rows, some masked (-1)
    cases = [(128, 128, mk(Kd, 128), mk(Kd, 128), {}), (128, 256, mk(Kd, 128), mk(7200, 256), dict(b_rowmap=rmap)), (512, 128, mk(Kd, 512), mk(Kd, 128), {})]
    def run(I, J, A, B, kw, parts):
        monkeypatch.setenv("LAVT_TN_PARTIALS", "1" if parts else "0")
        out = torch.full((I, J), 0.5, device=dev()); cs = torch.full((I,), -2.0, device=dev())
        ops.gemm_tn(bf, I, J, Kd, A, I, B, J, out, J, colsum=cs, accumulate=True, **kw)
        torch.cuda.synchronize()
        return out, cs
    for I, J, A, B, kw in cases:
        Bf = B.float()
        if "b_rowmap" in kw:
            Bf = torch.where(rmap[:, None] >= 0, B.float()[rmap.clamp(min=0).long()], torch.zeros(1, device=dev()))
        ref, cref = A.float().t() @ Bf + 0.5, A.float().sum(0) - 2.0
        (o1, c1), (o0, c0) = run(I, J, A, B, kw, True), run(I, J, A, B, kw, False)
        scale = float(ref.abs().max())
        for o, c in ((o1, c1), (o0, c0)):
            assert float((o - ref).abs().max()) <= 2e-3 * scale, float((o - ref).abs().max()) / scale
            assert float((c - cref).abs().max()) <= 2e-3 * float(cref.abs().max())
        assert float((o1 - o0).abs().max()) <= 1e-4 * scale                                  # fp32 summation order only
    # grouped: four long-K members in one launch
    monkeypatch.setenv("LAVT_TN_PARTIALS", "1")
    structs, keep, outs = [], [], []
    class _Q:
        def add(self, p, t, extra=False): structs.append(p); keep.append(t)
    members = [cases[0], cases[1], cases[2], (128, 128, mk(Kd, 128), mk(Kd, 128), {})]
    for I, J, A, B, kw in members:
        out = torch.zeros(I, J, device=dev()); cs = torch.zeros(I, device=dev())
        ops.gemm_tn(bf, I, J, Kd, A, I, B, J, out, J, colsum=cs, defer=_Q(), **kw)
        outs.append((out, cs))
    need = [int(q.partials_floats) for q in structs]
    assert all(n > 0 for n in need)
    scr = torch.empty(sum(need), device=dev())
    off = 0
    for q, n in zip(structs, need):                 # what ops._WgradQueue.flush does: disjoint regions of one scratch
        q.partials = scr.data_ptr() + 4 * off
        off += n
    arr = (K.GemmTN * len(structs))(*structs)
    K.check(K.lib.lavt_gemm_tn_grouped(arr, len(structs), K.stream()))
    torch.cuda.synchronize()
    for (I, J, A, B, kw), (o, c) in zip(members, outs):
        Bf = B.float()
        if "b_rowmap" in kw:
            Bf = torch.where(rmap[:, None] >= 0, B.float()[rmap.clamp(min=0).long()], torch.zeros(1, device=dev()))
        ref, cref = A.float().t() @ Bf, A.float().sum(0)
        assert float((o - ref).abs().max()) <= 2e-3 * float(ref.abs().max())
        assert float((c - cref).abs().max()) <= 2e-3 * float(cref.abs().max())


def test_syncbn_combine_kernel():
    """lavt_syncbn_combine (gathered per-rank (sum, centred M2) pairs -> mean / rstd of the global batch + running estimates, one launch) against
    statistics computed directly over the concatenated batch, and against ops.combine_rank_stats (the torch form the gloo tests drive)"""
    from lavt_hip import _capi as K, ops
    g = torch.Generator().manual_seed(7)
    world, rows, Cc, eps, mom = 4, 300, 96, 1e-5, 0.1
    x = (torch.randn(world, rows, Cc, generator=g) * 2.0 + 5.0).to(dev())                 # large mean: E[x^2] - E[x]^2 would lose digits
    allst = torch.stack([torch.stack([xr.sum(0), ((xr - xr.mean(0)) ** 2).sum(0)]) for xr in x]).view(world, 2, 1, Cc).contiguous()
    rm, rv = torch.zeros(Cc, device=dev()), torch.ones(Cc, device=dev())
    mean, rstd = ops._HipBnKernels.combine_finalize(allst, rows, eps, rm, rv, mom)
    torch.cuda.synchronize()
    flat = x.reshape(-1, Cc)
    n = flat.shape[0]
    mu, var = flat.mean(0), flat.var(0, unbiased=False)
    assert float((mean - mu).abs().max()) < 1e-5 and float((rstd - (var + eps).rsqrt()).abs().max()) < 1e-5
    assert float((rm - mom * mu).abs().max()) < 1e-5 and float((rv - (0.9 + mom * var * n / (n - 1))).abs().max()) < 1e-4
    comb = ops.combine_rank_stats(allst, rows).view(2, Cc)
    assert float((comb[0] / n - mean).abs().max()) < 1e-5 and float((comb[1] / n - var).abs().max()) < 1e-4


# ------------------------------------------------------------------------------------------------ text side + composed-attention helpers
@pytest.mark.parametrize("dtype", DT)
def test_bert_embed(dtype):
    """lavt_bert_embed_fwd/bwd vs three nn.Embedding lookups and their scatter-add gradients (repeated ids and positions collide)"""
    from lavt_hip import ops
    B, N, H, V = 3, 20, 96, 50
    g = torch.Generator().manual_seed(4)
    ids = torch.randint(0, V, (B, N), generator=g)
    ids[1, 5:9] = ids[0, 2]                      # repeated ids
    tt = torch.randint(0, 2, (B, N), generator=g)
    ps = [torch.nn.Parameter(rnd(V, H, seed=1).to(dev())), torch.nn.Parameter(rnd(32, H, seed=2).to(dev())), torch.nn.Parameter(rnd(2, H, seed=3).to(dev()))]
    out = ops.bert_embed(ids.to(dev()), tt.to(dev()), ps[0], ps[1], ps[2], N, dtype)
    w = rnd(B * N, H, seed=5).to(dev())
    (out.float() * w).sum().backward()
    ref_p = [p.detach().clone().requires_grad_(True) for p in ps]
    ref = (ref_p[0][ids.to(dev())] + ref_p[2][tt.to(dev())] + ref_p[1][:N][None]).view(B * N, H)
    (ref * (w.to(dtype).float() if dtype == torch.bfloat16 else w)).sum().backward()
    tol = 2e-2 if dtype == torch.bfloat16 else 1e-6
    assert float((out.float() - ref).abs().max()) <= tol * float(ref.abs().max())
    for p, r in zip(ps, ref_p):
        assert float((p.grad - r.grad).abs().max()) <= 1e-5 * float(r.grad.abs().max()) + 1e-6


@pytest.mark.parametrize("dtype", DT)
def test_dropout(dtype):
    """lavt_dropout: kept elements scaled by 1/(1-p) (+ residual), dropped ones zero; backward uses the same mask"""
    from lavt_hip import ops
    torch.manual_seed(11)
    x = rnd(64, 96, seed=1).to(dev()).to(dtype).requires_grad_(True)
    r = rnd(64, 96, seed=2).to(dev()).to(dtype).requires_grad_(True)
    y = ops.dropout(x, 0.25, True, residual=r)
    y.sum().backward()
    kept = x.grad != 0                           # the backward applies the same keep mask: gradient 1/(1-p) on kept elements, 0 elsewhere
    assert 0.6 < float(kept.float().mean()) < 0.9
    assert float((x.grad.float()[kept] - 1 / 0.75).abs().max()) < 1e-2
    ref = r.detach().float() + kept.float() * x.detach().float() / 0.75
    tol = 2e-2 if dtype == torch.bfloat16 else 1e-6
    assert float((y.detach().float() - ref).abs().max()) <= tol * float(ref.abs().max())
    assert float((r.grad.float() - 1).abs().max()) == 0.0
    assert ops.dropout(x, 0.25, False) is x


@pytest.mark.parametrize("dtype", DT)
def test_attn_dbias_sum(dtype):
    """lavt_attn_dbias_sum: sum over windows of the score gradients, padded rows skipped"""
    from lavt_hip import _capi as K
    nwin, heads, N, rpw, ld = 5, 3, 21, 24, 24
    ds = rnd(nwin, heads, rpw, ld, seed=8).to(dev()).to(dtype)
    out = torch.full((heads, N, ld), 7.0, device=dev())
    K.check(K.lib.lavt_attn_dbias_sum(K.dt(dtype), K.ptr(ds), K.ptr(out), nwin, heads, N, rpw, ld, K.stream()))
    ref = ds.float()[:, :, :N].sum(0)
    assert float((out - ref).abs().max()) <= 1e-5 * float(ref.abs().max())


# ---------------------------------------------------------------------------------------------- MultiClassDiceLoss
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("tag", ["a", "b", "same"])
def test_upsample_dice_golden(golden, tag, dtype):
    """lavt_upsample_dice_{fwd,bwd} vs the reference's MultiClassDiceLoss on the upsampled logits (losses.py:38-77): loss and d loss / d y"""
    from lib._utils import fused_dice_loss
    g = golden(f"dice_{tag}")
    B, h, w, H, W = g["dims"].tolist()
    y = (torch.randn(B, 2, h, w, generator=torch.Generator("cpu").manual_seed(int(g["seeds"][0]))) * 2.0)
    tgt = (torch.randn(B, H, W, generator=torch.Generator("cpu").manual_seed(int(g["seeds"][1]))) > 0.3).long()
    tgt[B - 1] = 0
    yd = y.to(dev()).to(dtype).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2).requires_grad_(True)     # NCHW-shaped view of NHWC memory, as the decoder returns it
    loss, stats = fused_dice_loss(yd, tgt.to(dev()))
    loss.backward()
    tol = 1e-5 if dtype == torch.float32 else 3e-3
    assert abs(float(loss) - float(g["loss"])) < tol
    ref = torch.as_tensor(g["dy"])
    assert float((yd.grad.float().cpu() - ref).abs().max()) <= (1e-6 if dtype == torch.float32 else 0.02 * float(ref.abs().max()))
    per = stats[2:].view(B, 6).cpu()
    assert torch.equal(per[:, 5], (tgt == 1).flatten(1).sum(1).float()) and float(per[B - 1, 1]) == 0.0


def test_losses_module_criteria_on_full_resolution_logits(golden):
    """`losses.cross_entropy_loss` / `losses.MultiClassDiceLoss()` called as train.py:225 does (criterion(output, target), output (B,2,H,W))"""
    import losses
    from oracle import lavt_oracle as O
    g = torch.Generator("cpu").manual_seed(17)
    out = (torch.randn(2, 2, 40, 36, generator=g) * 2).requires_grad_(True)
    tgt = (torch.randn(2, 40, 36, generator=g) > 0).long()
    o2 = out.detach().to(dev()).requires_grad_(True)
    for crit, ref_fn in ((losses.cross_entropy_loss, O.weighted_ce), (losses.MultiClassDiceLoss(), O.multiclass_dice)):
        out.grad = o2.grad = None
        ref = ref_fn(out, tgt)
        ref.backward()
        got = crit(o2, tgt.to(dev()))
        got.backward()
        assert abs(float(got) - float(ref)) < 1e-5
        assert float((o2.grad.cpu() - out.grad).abs().max()) < 1e-6
    with pytest.raises(NotImplementedError):
        losses.DiceFocalLoss()


def test_fused_mlp_node_matches_two_linears(monkeypatch):
    """ops.mlp's single-node form (LAVT_FUSED_MLP=1: fc2's data-gradient GEMM applies GELU'(pre) in its epilogue, lavt_gemm_nt dact_pre)
    against the two-op form: output and every gradient, with a DropPath row mask and a residual"""
    from lavt_hip import ops
    g = torch.Generator().manual_seed(3)
    M, Cc = 1800, 128
    bf = torch.bfloat16
    x0 = (torch.randn(M, Cc, generator=g)).to(dev()).to(bf)
    res0 = (torch.randn(M, Cc, generator=g)).to(dev()).to(bf)
    ws = [torch.randn(4 * Cc, Cc, generator=g) * Cc ** -0.5, torch.randn(4 * Cc, generator=g) * 0.1, torch.randn(Cc, 4 * Cc, generator=g) * (4 * Cc) ** -0.5,
          torch.randn(Cc, generator=g) * 0.1]
    mask = torch.tensor([1.25, 0.0], device=dev())
    dy = torch.randn(M, Cc, generator=g).to(dev()).to(bf)
    outs = []
    for fused in ("0", "1"):
        monkeypatch.setenv("LAVT_FUSED_MLP", fused)
        x, res = x0.clone().requires_grad_(True), res0.clone().requires_grad_(True)
        ps = [torch.nn.Parameter(w.clone().to(dev())) for w in ws]
        y = ops.mlp(x, ps[0], ps[1], ps[2], ps[3], residual=res, row_scale=mask, row_scale_div=M // 2, row_scale_value=1.25)
        y.backward(dy)
        outs.append([y.detach().float(), x.grad.float(), res.grad.float()] + [p.grad for p in ps])
    for a, b in zip(*outs):
        assert float((a - b).abs().max()) <= 2e-2 * float(a.abs().max()) + 1e-6


# ---------------------------------------------------------------------------------------------- fp8 (BASELINE.json configs[4])
def test_fp8_quantizer_bit_exact_and_delayed_scaling():
    """lavt_fp8_quantize vs torch's float8_e4m3fn cast (round to nearest even, saturating at +-448): identical bytes; the |max| seen by one
    call becomes the scale of the next step after lavt_fp8_advance"""
    from lavt_hip import ops
    from oracle import fp8_oracle as F8
    st = ops._Fp8State()
    x = (rnd(512, 128, seed=3) * 3.0).to(torch.bfloat16)
    x[0, 0], x[1, 1] = 1000.0, -777.0                                    # beyond +-448 at scale 1: must saturate, not become NaN
    q0, _ = st.quantize(x.to(dev()), "site")                            # uncalibrated: scale 1
    assert torch.equal(q0.cpu(), F8.quantize_bytes(x, 0.0))
    st.advance()
    amax = float(x.float().abs().max())
    assert float(st.prev[0]) == amax and float(st.cur[0]) == 0.0
    q1, _ = st.quantize(x.to(dev()), "site")
    assert torch.equal(q1.cpu(), F8.quantize_bytes(x, amax))


def test_fp8_twins_written_by_producers_equal_the_quantiser(monkeypatch):
    """configs[4]: BatchNorm + ReLU (lavt_norm_apply_q8) and the bilinear upsample (lavt_bilinear_fwd_q8) write the e4m3 twin of their bf16 output themselves,
    the BatchNorm backward apply pass (lavt_norm_bwd_apply_amax) records |max| of the gradient it stores: the bytes must be the ones lavt_fp8_quantize /
    lavt_fp8_quantize_current produce from the same bf16 tensors (oracle: fp8_oracle.quantize_bytes), the |max| bookkeeping the same, and the consuming
    convolution must pick the twin up instead of launching a quantiser."""
    import lavt_hip
    from lavt_hip import ops
    from oracle import fp8_oracle as F8
    monkeypatch.setattr(ops, "_FP8_CONV_MIN_TILES", 0)
    B, Hi, H, C = 2, 12, 24, 128
    x = rnd(B * Hi * Hi, C, seed=1).to(torch.bfloat16)
    w = torch.nn.Parameter((rnd(C, C, 3, 3, seed=2) * (9 * C) ** -0.5).to(dev()))
    bn = torch.nn.BatchNorm2d(C).to(dev())
    with torch.no_grad():
        bn.weight.copy_(1.0 + 0.2 * rnd(C, seed=3)); bn.bias.copy_(0.3 * rnd(C, seed=4))
    ops.fp8.__init__()
    with lavt_hip.use_dtype("fp8"):
        site = ops.fp8_act_site(w, B * H * H, C)
        assert site == id(w)
        for it in range(2):                                                  # second pass: calibrated scale
            ops.fp8.advance()
            up = ops.bilinear(x.to(dev()), B, Hi, Hi, H, H, fp8_site=site)
            q_up, a_up = ops.fp8.twins[(up.data_ptr(), up.numel())][:2]
            got = ops.fp8.quantize(up, site)
            assert got[0] is q_up and not ops.fp8.twins                     # picked up, no second quantisation
        amax_up = float(up.float().abs().max())
        assert torch.equal(q_up.cpu(), F8.quantize_bytes(up.cpu(), amax_up))   # (the same tensor both passes: the delayed scale is its own |max|)
        assert float(ops.fp8.cur[ops.fp8.slots[site]]) == amax_up
        # BatchNorm + ReLU twin, and the gradient |max| of its backward
        ops.fp8.__init__()
        dsite = ops.fp8_dy_site(w, B * H * H, C)
        for it in range(2):
            ops.fp8.advance()
            xin = up.detach().clone().requires_grad_(True)
            y = ops.batch_norm_relu(xin, bn, fp8_site=site, fp8_dy_site=dsite)
            q_y = ops.fp8.twins.pop((y.data_ptr(), y.numel()))[0]
            dy = (rnd(B * H * H, C, seed=9) * 1e-3).to(torch.bfloat16).to(dev())
            dx, = torch.autograd.grad(y, xin, dy)
        assert torch.equal(q_y.cpu(), F8.quantize_bytes(y.detach().cpu(), float(y.detach().float().abs().max())))
        a_ptr = ops.fp8.dy_amax[(dx.data_ptr(), dx.numel())][0]
        i = ops.fp8.slots[dsite]
        assert a_ptr == ops.fp8.cur.data_ptr() + 4 * i
        assert float(ops.fp8.cur[i]) == float(dx.float().abs().max())
        qd, ap = ops.fp8.quantize_current(dx, dsite)
        assert ap == a_ptr and torch.equal(qd.cpu(), F8.quantize_bytes(dx.cpu(), float(dx.float().abs().max())))
        # without fp8 sites nothing is registered
        ops.fp8.advance()
        ops.batch_norm_relu(up.detach(), bn)
        assert not ops.fp8.twins and not ops.fp8.dy_amax
        # outside the step harness (no advance() per step: the reference's eager loop, several backward passes per optimizer step) the producers register
        # nothing and the gradient is quantised against ITS OWN |max| on every call -- shrinking gradients are not flushed by a stale running maximum
        ops.fp8.end_step()
        for k, scale in enumerate((1e-3, 1e-6)):
            xin = up.detach().clone().requires_grad_(True)
            y = ops.batch_norm_relu(xin, bn, fp8_site=site, fp8_dy_site=dsite)
            dy = (rnd(B * H * H, C, seed=9) * scale).to(torch.bfloat16).to(dev())
            dx, = torch.autograd.grad(y, xin, dy)
            assert not ops.fp8.twins and not ops.fp8.dy_amax
            qd, ap = ops.fp8.quantize_current(dx, dsite)
            assert torch.equal(qd.cpu(), F8.quantize_bytes(dx.cpu(), float(dx.float().abs().max()))), f"pass {k}: current scaling outside the harness"


@pytest.mark.parametrize("cat", [False, True])
def test_fp8_conv3x3_matches_quantised_oracle(cat, monkeypatch):
    """decoder 3x3 convolution on e4m3 operands (v_mfma_scale_f32_16x16x128_f8f6f4, unit block scales): both concat sources against one scale,
    weights with current scaling; against the fp32 convolution of the quantise-dequantised tensors"""
    import lavt_hip
    from lavt_hip import ops
    from oracle import fp8_oracle as F8
    B, H, W, C1, C2, Cout = 2, 20, 24, 128, (128 if cat else 0), 256
    monkeypatch.setattr(ops, "_FP8_CONV_MIN_TILES", 0)                 # (the product keeps maps this small in bf16)
    x1 = (rnd(B * H * W, C1, seed=1)).to(torch.bfloat16)
    x2 = (rnd(B * H * W, C2, seed=2) * 2.0).to(torch.bfloat16) if cat else None
    w = rnd(Cout, C1 + C2, 3, 3, seed=5) * (9 * (C1 + C2)) ** -0.5
    wd = torch.nn.Parameter(w.clone().to(dev()))
    ops.fp8.__init__()
    with lavt_hip.use_dtype("fp8"):
        assert lavt_hip.fp8_enabled()
        for it in range(2):                                              # second call: calibrated scale (delayed scaling)
            ops.fp8.advance()
            with torch.no_grad():
                y = ops.conv3x3(x1.to(dev()), x2.to(dev()) if cat else None, wd, B, H, W)
    assert not lavt_hip.fp8_enabled()
    xs = torch.cat([x1, x2], 1) if cat else x1
    amax_x, amax_w = float(xs.float().abs().max()), float(w.abs().max())
    ref = F8.conv3x3_fp8(xs.float().view(B, H, W, -1).permute(0, 3, 1, 2), w, amax_x, amax_w).permute(0, 2, 3, 1).reshape(B * H * W, Cout)
    err = float((y.float().cpu() - ref).abs().max())
    assert err <= 1e-2 * float(ref.abs().max()), err / float(ref.abs().max())
    assert float((y.float().cpu() - ref).norm() / ref.norm()) <= 5e-3                                   # bf16 rounding of the output: 1.1e-3 rms
    assert_border_close(y, ref, (B, H, W), 8e-3, "fp8 conv forward")
    exact = F.conv2d(xs.float().view(B, H, W, -1).permute(0, 3, 1, 2), w, padding=1).permute(0, 2, 3, 1).reshape(B * H * W, Cout)
    rel = float((y.float().cpu() - exact).norm() / exact.norm())
    assert rel < 0.06, rel                                               # e4m3 has 3 mantissa bits: ~3-4 % rms on a 1000-term contraction


@pytest.mark.parametrize("cat", [False, True])
@pytest.mark.parametrize("shape", [(2, 20, 24, 128, 256), (2, 48, 48, 256, 512)])
def test_fp8_conv3x3_data_gradient_matches_quantised_oracle(cat, shape, monkeypatch):
    """e4m3 data gradient of the decoder convolutions (dY quantised with current scaling against its own |max|, weights as the transposed
    [Cin][taps][Cout] e4m3 copy; the larger shape takes the software-pipelined kernel): against the fp32 transposed convolution of the
    quantise-dequantised tensors; the weight gradient stays bf16 and must equal the bf16 path's"""
    import lavt_hip
    from lavt_hip import ops
    from oracle import fp8_oracle as F8
    B, H, W, C1, Cout = shape
    C2 = 128 if cat else 0
    monkeypatch.setattr(ops, "_FP8_CONV_MIN_TILES", 0)                 # (the product keeps maps this small in bf16)
    x1 = rnd(B * H * W, C1, seed=1).to(torch.bfloat16)
    x2 = (rnd(B * H * W, C2, seed=2) * 2.0).to(torch.bfloat16) if cat else None
    w = rnd(Cout, C1 + C2, 3, 3, seed=5) * (9 * (C1 + C2)) ** -0.5
    dy = (rnd(B * H * W, Cout, seed=7) * 1e-3).to(torch.bfloat16)          # gradient-sized values: nothing would survive a scale-1 quantisation
    dy[3, 5] = 0.05                                                        # one outlier sets the scale: the bulk sits ~50x below |max|
    ops.fp8.__init__()
    grads = {}
    for mode in ("fp8", "bf16"):
        wd = torch.nn.Parameter(w.clone().to(dev()))
        with lavt_hip.use_dtype(mode):
            for it in range(2):                                            # second pass: calibrated scales
                ops.fp8.advance()
                a1 = x1.to(dev()).requires_grad_(True)
                a2 = x2.to(dev()).requires_grad_(True) if cat else None
                wd.grad = None
                y = ops.conv3x3(a1, a2, wd, B, H, W)
                y.backward(dy.to(dev()))
        torch.cuda.synchronize()
        grads[mode] = (torch.cat([a1.grad, a2.grad], 1) if cat else a1.grad).float().cpu(), wd.grad.float().cpu()
    amax_dy, amax_w = float(dy.float().abs().max()), float(w.abs().max())
    ref = F8.conv3x3_fp8_dgrad(dy.float().view(B, H, W, Cout).permute(0, 3, 1, 2), w, amax_dy, amax_w).permute(0, 2, 3, 1).reshape(B * H * W, -1)
    dx, dw = grads["fp8"]
    err = float((dx - ref).abs().max())
    assert err <= 1e-2 * float(ref.abs().max()), err / float(ref.abs().max())     # bf16 rounding of the output
    assert float((dx - ref).norm() / ref.norm()) <= 5e-3
    assert_border_close(dx, ref, (B, H, W), 8e-3, "fp8 conv data gradient")
    exact = F.conv_transpose2d(dy.float().view(B, H, W, Cout).permute(0, 3, 1, 2), w, padding=1).permute(0, 2, 3, 1).reshape(B * H * W, -1)
    rel = float((dx - exact).norm() / exact.norm())
    assert rel < 0.08, rel
    assert float((grads["bf16"][0] - exact).norm() / exact.norm()) < 0.01
    if W <= 32:
        assert float((dw - grads["bf16"][1]).abs().max()) <= 1e-6 * float(dw.abs().max()) + 1e-12      # weight gradient: the same bf16 kernel in both modes (narrow maps)
    else:                                                                                               # e4m3 weight gradient (test_fp8_conv3x3_weight_gradient_* pins it)
        assert float((dw - grads["bf16"][1]).norm() / grads["bf16"][1].norm()) < 0.08


@pytest.mark.parametrize("B,H,W,C1,C2,Cout", [(2, 120, 120, 128, 64, 256), (1, 60, 60, 64, 64, 128), (2, 24, 96, 64, 0, 128), (1, 5, 120, 64, 0, 128), (3, 6, 33, 64, 0, 128),
                                              (1, 16, 128, 64, 0, 128), (2, 14, 64, 128, 0, 128), (1, 16, 120, 384, 96, 384), (2, 120, 120, 512, 0, 512), (4, 60, 60, 512, 128, 512),
                                              (3, 8, 65, 64, 16, 128)])
def test_fp8_conv3x3_weight_gradient_matches_quantised_oracle(B, H, W, C1, C2, Cout, monkeypatch):
    """e4m3 weight gradient of the decoder convolutions (csrc/conv_wgrad.hip, conv_wgrad3x3_f8_kernel: the nine taps fused on
    v_mfma_f32_16x16x128_f8f6f4, pixel-major operands through ds_read_b64_tr_b8, a K step = one image row of 65-128 pixels or two of 33-64) against the
    fp32 weight gradient of the quantise-dequantised tensors: products of e4m3 values are exact in fp32, so only the summation order differs.  X with
    delayed scaling (the forward's copy, both concat sources against one |max|), dY with current scaling (the data gradient's copy); every width
    class, image borders inside a piece, a row count the pieces do not divide, a skip source that does not fill its 64-channel tile."""
    import lavt_hip
    from lavt_hip import ops, _capi as K
    from oracle import fp8_oracle as F8
    Cin = C1 + C2
    assert K.lib.lavt_conv3x3_wgrad_f8_ok(B, H, W, Cout, Cin, C1 if C2 else Cin) == 1
    monkeypatch.setattr(ops, "_FP8_CONV_MIN_TILES", 0)
    x1 = rnd(B * H * W, C1, seed=1).to(torch.bfloat16)
    x2 = (rnd(B * H * W, C2, seed=2) * 2.0).to(torch.bfloat16) if C2 else None
    w = rnd(Cout, Cin, 3, 3, seed=5) * (9 * Cin) ** -0.5
    dy = (rnd(B * H * W, Cout, seed=7) * 1e-3).to(torch.bfloat16)
    dy[3, 5] = 0.02
    ops.fp8.__init__()
    wd = torch.nn.Parameter(w.clone().to(dev()))
    with lavt_hip.use_dtype("fp8"):
        for it in range(2):                                                # second pass: calibrated activation scale
            ops.fp8.advance()
            a1 = x1.to(dev()).requires_grad_(True)
            a2 = x2.to(dev()).requires_grad_(True) if C2 else None
            wd.grad = None
            y = ops.conv3x3(a1, a2, wd, B, H, W)
            y.backward(dy.to(dev()))
    torch.cuda.synchronize()
    got = wd.grad.float().cpu()
    xs = (torch.cat([x1, x2], 1) if C2 else x1).float().view(B, H, W, Cin).permute(0, 3, 1, 2)
    dyn = dy.float().view(B, H, W, Cout).permute(0, 3, 1, 2)
    ref = F8.conv3x3_fp8_wgrad(xs, dyn, float(xs.abs().max()), float(dyn.abs().max()))
    scale = float(ref.abs().max())
    assert torch.isfinite(got).all()
    assert float((got - ref).abs().max()) <= 1e-3 * scale, float((got - ref).abs().max()) / scale
    assert float((got - ref).norm() / ref.norm()) <= 2e-4
    for ky, kx in ((0, 1), (2, 1), (1, 0), (1, 2), (0, 0), (2, 2)):          # the taps that touch the halo, each against its own scale
        assert float((got[:, :, ky, kx] - ref[:, :, ky, kx]).abs().max()) <= 1e-3 * float(ref[:, :, ky, kx].abs().max()), (ky, kx)
    exact = torch.nn.grad.conv2d_weight(xs, (Cout, Cin, 3, 3), dyn, padding=1)
    assert float((got - exact).norm() / exact.norm()) < 0.08                 # e4m3 operands: ~3-4 % rms each


@pytest.mark.parametrize("shape", [(4608, 256, 384), (6656, 1024, 512), (26368, 1024, 512)])
def test_fp8_linear_matches_quantised_oracle(monkeypatch, shape):
    """the Linear form of the fp8 contraction (off by default: ops._FP8_LINEAR_MIN_ROWS) against the quantised oracle; the second and third shapes
    take the plain-issue form of the software-pipelined fp8 kernel (128x128 and 256x256 tiles), the first gemm_v2's K loop"""
    import lavt_hip
    from lavt_hip import ops
    from oracle import fp8_oracle as F8
    monkeypatch.setattr(ops, "_FP8_LINEAR_MIN_ROWS", 4096)
    M, Kd, N = shape
    x = rnd(M, Kd, seed=7).to(torch.bfloat16)
    w, b = rnd(N, Kd, seed=8) * Kd ** -0.5, rnd(N, seed=9) * 0.1
    wd, bd = torch.nn.Parameter(w.clone().to(dev())), torch.nn.Parameter(b.clone().to(dev()))
    ops.fp8.__init__()
    with lavt_hip.use_dtype("fp8"):
        for it in range(2):
            ops.fp8.advance()
            xd = x.to(dev()).requires_grad_(True)
            y = ops.linear(xd, wd, bd)
        y.float().sum().backward()                                       # backward runs on the bf16 tensors
    ref = F8.linear_fp8(x, w, b, float(x.float().abs().max()), float(w.abs().max()))
    assert float((y.detach().float().cpu() - ref).abs().max()) <= 1e-2 * float(ref.abs().max())
    assert float((xd.grad.float().cpu() - w.sum(0).to(torch.bfloat16).float()).abs().max()) <= 3e-2 * float(w.sum(0).abs().max())


def test_fp16_autocast_runs_as_bf16(monkeypatch):
    """The reference's AMP hook is torch.cuda.amp.autocast() = float16 + GradScaler (train.py:452-459).  This path has no fp16 kernels: an fp16
    autocast region computes in bf16 with one warning per process, so `--use_amp` runs unchanged -- forward, scaled backward, unscale; a bf16
    region selects bf16 silently; LAVT_STRICT_FP16_AUTOCAST=1 raises."""
    import warnings
    from lavt_hip import ops, runtime
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert runtime.compute_dtype() == torch.bfloat16
    runtime._warned_fp16[0] = False
    x, w, b = rnd(96, 64, seed=1), rnd(48, 64, seed=2, scale=0.125), rnd(48, seed=3)
    wd, bd = w.to(dev()).requires_grad_(True), b.to(dev()).requires_grad_(True)
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        with torch.autocast("cuda", dtype=torch.float16):
            assert runtime.compute_dtype() == torch.bfloat16
            y = ops.linear(x.to(dev()).to(runtime.compute_dtype()), wd, bd)          # (the model casts its inputs to the compute dtype at the door)
            assert runtime.compute_dtype() == torch.bfloat16
        assert len([r for r in rec if "float16" in str(r.message)]) == 1
    assert y.dtype == torch.bfloat16
    loss = y.float().pow(2).mean()
    scaler.scale(loss).backward()
    opt = torch.optim.SGD([wd, bd], lr=0.0)
    scaler.unscale_(opt)
    ref_w = torch.autograd.grad(F.linear(x, w.requires_grad_(True), b).pow(2).mean(), w)[0]
    assert float((wd.grad.cpu() - ref_w).abs().max()) <= 3e-2 * float(ref_w.abs().max())
    monkeypatch.setenv("LAVT_STRICT_FP16_AUTOCAST", "1")
    with torch.autocast("cuda", dtype=torch.float16):
        with pytest.raises(RuntimeError, match="float16"):
            runtime.compute_dtype()


def test_forward_glue_kernels():
    """The O(batch) glue of a forward as single launches: language mask -> float rows + the -1e4 word bias (lib/backbone.py:1360) for float and
    int64 masks, and timm's drop_path factors floor(keep + u) / keep -- bit-identical to the torch expressions they replace."""
    from lavt_hip import ops
    g = torch.Generator().manual_seed(3)
    B, n_l = 3, 20
    m = (torch.rand(B, n_l, 1, generator=g) > 0.4)
    for mm in (m.float(), m.long(), m):
        rows, bias = ops.lang_mask(mm.to(dev()), B, n_l)
        mf = m.float().reshape(B, n_l)
        ref = torch.full((B, ops.KV_LD), -1e4)
        ref[:, :n_l] = 1e4 * mf - 1e4
        assert torch.equal(rows.cpu(), mf.reshape(-1)) and torch.equal(bias.cpu(), ref)
    u = torch.rand(48, 2, generator=g)
    keep = (1.0 - torch.linspace(0.0125, 0.3, 48))[:, None]
    f = ops.droppath_factors(u.to(dev()), keep.to(dev()))
    assert torch.equal(f.cpu(), torch.floor(keep + u) / keep)


def _philox4x32_10_first(seed, ctr, n):
    """numpy restatement of the generator of lavt_droppath_draw (Philox4x32-10, Salmon et al. 2011; key = seed, counter = (ctr lo, ctr hi, e, 0)): word 0"""
    import numpy as np
    M0, M1, W0, W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), 0x9E3779B9, 0xBB67AE85
    c0 = np.full(n, ctr & 0xffffffff, dtype=np.uint64); c1 = np.full(n, ctr >> 32, dtype=np.uint64)
    c2 = np.arange(n, dtype=np.uint64); c3 = np.zeros(n, dtype=np.uint64)
    k0, k1 = seed & 0xffffffff, (seed >> 32) & 0xffffffff
    mask = np.uint64(0xffffffff)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & mask, p1 >> np.uint64(32), p1 & mask
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + W0) & 0xffffffff, (k1 + W1) & 0xffffffff
    return c0.astype(np.uint32)


def test_droppath_draw_on_device():
    """lavt_droppath_draw: the DropPath factors of a forward with the uniform draw made in the kernel (no torch.rand under capture) -- bit-identical to a
    numpy restatement of Philox4x32-10 for three consecutive draws (the kernel advances its own counter), reseedable, and the drop rate is what
    timm's drop_path gives (reference lib/backbone.py:240-245)."""
    import numpy as np
    from lavt_hip import ops
    keep = (1.0 - torch.linspace(0.0125, 0.3, 48))[:, None].to(dev())
    B = 2
    ops.droppath_draw(keep, B)                                   # (creates the state)
    ops.droppath_reseed(1234567890123)
    kf = keep.cpu().numpy()
    for ctr in range(3):
        f = ops.droppath_draw(keep, B).cpu().numpy()
        x = _philox4x32_10_first(1234567890123, ctr, 48 * B)
        u = ((x >> 8).astype(np.float32) * np.float32(1.0 / 16777216.0)).reshape(48, B)
        assert np.array_equal(f, np.floor(kf + u) / kf), ctr
    keep2 = torch.full((64, 1), 0.7, device=dev())
    drops = sum(float((ops.droppath_draw(keep2, 64) == 0).float().mean()) for _ in range(20)) / 20
    assert abs(drops - 0.3) < 0.02, drops
    g = torch.cuda.CUDAGraph()
    out = []
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            fg = ops.droppath_draw(keep2, 64)
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        out.append(fg.clone())
    assert not torch.equal(out[0], out[1]), "a replay must draw fresh factors"


# ------------------------------------------------------------------------------------------ PWAM word-side reductions as by-products (round 6)
def _pwam_words_ref(q, k, mean, rstd, maskbias, n_l, alpha):
    """fp32 statement of lavt_pwam_words_fwd on the bf16 operands: softmax_{j < n_l}(alpha * IN(q) K^T + maskbias), lib/backbone.py:1349-1361"""
    B, T, C = q.shape
    qn = (q.float() - mean[:, None, :]) * rstd[:, None, :]
    s = alpha * torch.einsum("btc,bjc->btj", qn, k.float()) + maskbias[:, None, :]
    s[:, :, n_l:] = -float("inf")
    return torch.softmax(s, dim=-1)


@pytest.mark.parametrize("B,T,C,n_l", [(2, 14400, 128, 20), (2, 3600, 256, 13), (2, 900, 512, 20), (3, 225, 1024, 7), (2, 50, 64, 32), (4, 14400, 96, 20), (1, 40000, 128, 20)])
def test_pwam_words_moments_by_product(B, T, C, n_l):
    """lavt_pwam_words_fwd_moments: P as lavt_pwam_words_fwd writes it, and records whose sum is P^T P / colsum(P) of THAT bf16 P (1 .. 64 records per
    sample, both workgroup sizes, rows that are no multiple of a tile, masked words); lavt_pwam_lang_fwd_records on the records = lavt_pwam_lang_fwd on
    the TN product of the round-5 path; run-to-run identical."""
    from lavt_hip import _capi as K
    from lavt_hip import ops
    d = dev()
    bf = torch.bfloat16
    q = (rnd(B, T, C, seed=1) * 1.5 + 0.3).to(bf).to(d)
    k = torch.zeros(B, 32, C)
    k[:, :n_l] = rnd(B, n_l, C, seed=2)
    k = k.to(bf).to(d)
    mean = q.float().mean(1)
    rstd = (q.float().var(1, unbiased=False) + 1e-5).rsqrt()
    mb = torch.zeros(B, 32)
    mb[:, n_l:] = -1e4
    mb[0, max(n_l - 3, 1):n_l] = -1e4              # masked words inside n_l: probability exactly zero rows / columns of the moments
    mb = mb.to(d)
    alpha = C ** -0.5
    P0 = torch.empty(B * T, 32, dtype=bf, device=d)
    K.check(K.lib.lavt_pwam_words_fwd(K.ptr(q), C, K.ptr(k), C, K.ptr(mean), K.ptr(rstd), K.ptr(mb), K.ptr(P0), B, T, C, n_l, alpha, K.stream()))
    R = int(K.lib.lavt_pwam_words_records(B, T, C))
    assert 1 <= R <= 64
    outs = []
    for _ in range(2):
        P = torch.empty_like(P0)
        rec = torch.full((B, R, 1056), float("nan"), device=d)
        K.check(K.lib.lavt_pwam_words_fwd_moments(K.ptr(q), C, K.ptr(k), C, K.ptr(mean), K.ptr(rstd), K.ptr(mb), K.ptr(P), K.ptr(rec), B, T, C, n_l, alpha, K.stream()))
        torch.cuda.synchronize()
        outs.append((P, rec))
    P, rec = outs[0]
    assert torch.equal(P, P0), "the by-product does not change P"
    assert torch.equal(outs[1][1], rec), "records are run-to-run identical"
    ref = _pwam_words_ref(q.cpu(), k.cpu(), mean.cpu(), rstd.cpu(), mb.cpu(), n_l, alpha)
    assert_close(P.reshape(B, T, 32), ref, bf, "P", bf16=2e-2)
    Pd = P.reshape(B, T, 32).double()
    tot = rec.double().sum(1)
    pp_ref = torch.einsum("btj,btk->bjk", Pd, Pd)
    assert float((tot[:, :1024].reshape(B, 32, 32) - pp_ref).abs().max()) <= 2e-6 * T, "sum of the records = P^T P"
    assert float((tot[:, 1024:] - Pd.sum(1)).abs().max()) <= 2e-6 * T, "sum of the records = colsum(P)"
    # the language kernel on the records against the same kernel on the explicit TN product
    V = torch.zeros(B, 32, C)
    V[:, :n_l] = rnd(B, n_l, C, seed=3)
    V = V.to(bf).to(d)
    Wo = (rnd(C, C, seed=4) * C ** -0.5).to(bf).to(d)
    PP = torch.zeros(B, 32, 32, device=d)
    sumP = torch.zeros(B, 32, device=d)
    ops.gemm_tn(bf, 32, 32, T, P, 32, P, 32, PP, 32, batch=B, strideA=T * 32, strideB=T * 32, strideC=1024, colsum=sumP, strideColsum=32)

    def lang(use_rec):
        o = dict(VWc=torch.empty(B, C, 32, dtype=bf, device=d), VWw=torch.empty(B, 32, C, dtype=bf, device=d), beta=torch.empty(B, C, device=d),
                 rw=torch.empty(B, C, device=d), pbar=torch.empty(B, 32, device=d), cov=torch.empty(B, 32, 32, device=d))
        K.check(K.lib.lavt_pwam_lang_fwd_records(K.ptr(V), C, K.ptr(Wo), None if use_rec else K.ptr(PP), None if use_rec else K.ptr(sumP), K.ptr(rec) if use_rec else None,
                                                 R if use_rec else 0, K.ptr(o["VWc"]), K.ptr(o["VWw"]), K.ptr(o["beta"]), K.ptr(o["rw"]), K.ptr(o["pbar"]), K.ptr(o["cov"]),
                                                 B, T, C, 1e-5, K.stream()))
        torch.cuda.synchronize()
        return o
    a, b_ = lang(True), lang(False)
    pb_ref = Pd.mean(1)
    cov_ref = pp_ref / T - pb_ref[:, :, None] * pb_ref[:, None, :]
    assert float((a["pbar"].double() - pb_ref).abs().max()) <= 2e-6, "Pbar"
    assert float((a["cov"].double() - cov_ref).abs().max()) <= 5e-6, "Cov"
    for kname in ("beta", "rw"):
        assert_close(a[kname], b_[kname].cpu(), torch.float32, kname, f32=2e-3)
    assert_close(a["VWc"], b_["VWc"].float().cpu(), bf, "VWc", bf16=1e-2)
    assert torch.equal(a["VWc"].transpose(1, 2).contiguous(), a["VWw"]), "both layouts of VW' hold the same values"


@pytest.mark.parametrize("B,T,C", [(2, 14400, 128), (2, 3600, 256), (2, 900, 512), (3, 225, 1024), (2, 50, 96), (1, 5000, 64)])
def test_pwam_mix1_word_reduction_by_product(B, T, C):
    """lavt_pwam_mix1: d vpre / d what as lavt_pwam_mix(1) writes them, records whose sum is H^T = dwhat^T P and colsum(dwhat) of THAT bf16 d what
    (1 .. 32 records per sample, a last channel group of 32, rows that are no multiple of a tile); lavt_pwam_lang_bwd1_records on the records =
    lavt_pwam_lang_bwd1 on the explicit TN product; run-to-run identical."""
    from lavt_hip import _capi as K
    from lavt_hip import ops
    d = dev()
    bf = torch.bfloat16
    P = torch.softmax(rnd(B * T, 32, seed=1) * 2.0, dim=-1)
    P[:, 20:] = 0.0
    P = (P / P.sum(-1, keepdim=True)).to(bf).to(d)
    VWc = (rnd(B, C, 32, seed=2) * 0.7).to(bf).to(d)
    beta = (rnd(B, C, seed=3) * 0.3).to(d)
    bv = (rnd(C, seed=4) * 0.2).to(d)
    vpre = rnd(B * T, C, seed=5).to(bf).to(d)
    dmm = (rnd(B * T, C, seed=6) * 1e-2).to(bf).to(d)

    def old():
        g = torch.empty(B * T, 2 * C, dtype=bf, device=d)
        dwh = torch.empty(B * T, C, dtype=bf, device=d)
        K.check(K.lib.lavt_pwam_mix(1, K.ptr(P), K.ptr(VWc), K.ptr(beta), None, K.ptr(bv), K.ptr(vpre), C, K.ptr(dmm), C, K.ptr(g), 2 * C, K.ptr(dwh), C, B, T, C, K.stream()))
        return g, dwh

    R = int(K.lib.lavt_pwam_mix1_records(B, T, C))
    assert 1 <= R <= 32

    def new():
        g = torch.empty(B * T, 2 * C, dtype=bf, device=d)
        dwh = torch.empty(B * T, C, dtype=bf, device=d)
        rec = torch.full((B, R, C * 33), float("nan"), device=d)
        K.check(K.lib.lavt_pwam_mix1(K.ptr(P), K.ptr(VWc), K.ptr(beta), K.ptr(bv), K.ptr(vpre), C, K.ptr(dmm), C, K.ptr(g), 2 * C, K.ptr(dwh), C, K.ptr(rec), B, T, C, K.stream()))
        torch.cuda.synchronize()
        return g, dwh, rec
    g0, w0 = old()
    g1, w1, rec = new()
    g2, w2, rec2 = new()
    assert torch.equal(rec, rec2) and torch.equal(w1, w2), "run-to-run identical"
    assert_close(w1, w0.float().cpu(), bf, "d what", bf16=1e-2)
    assert_close(g1[:, :C], g0[:, :C].float().cpu(), bf, "d vpre", bf16=1e-2)
    wd, Pd = w1.reshape(B, T, C).double(), P.reshape(B, T, 32).double()
    tot = rec.double().sum(1)
    H_ref = torch.einsum("btc,btj->bcj", wd, Pd)
    scale = float(H_ref.abs().max())
    assert float((tot[:, :C * 32].reshape(B, C, 32) - H_ref).abs().max()) <= 2e-5 * scale, "sum of the records = dwhat^T P"
    assert float((tot[:, C * 32:] - wd.sum(1)).abs().max()) <= 2e-5 * float(wd.sum(1).abs().max()), "sum of the records = colsum(dwhat)"
    # the language kernel on the records against the same kernel on the explicit product of the same d what
    HT = torch.zeros(B, C, 32, device=d)
    s = torch.zeros(B, C, device=d)
    ops.gemm_tn(bf, C, 32, T, w1, C, P, 32, HT, 32, batch=B, strideA=T * C, strideB=T * 32, strideC=C * 32, colsum=s, strideColsum=C)
    rw = (1.0 + 0.1 * rnd(B, C, seed=7).abs()).to(d)
    pbar = P.reshape(B, T, 32).float().mean(1)
    cov = torch.einsum("btj,btk->bjk", P.reshape(B, T, 32).float(), P.reshape(B, T, 32).float()) / T - pbar[:, :, None] * pbar[:, None, :]
    nq = int(K.lib.lavt_pwam_q_parts(C))

    def lang(use_rec):
        dVW = torch.empty(B * 32, C, dtype=bf, device=d)
        Qp = torch.empty(B * nq * 1056, device=d)
        K.check(K.lib.lavt_pwam_lang_bwd1_records(None if use_rec else K.ptr(HT), None if use_rec else K.ptr(s), K.ptr(rec) if use_rec else None, R if use_rec else 0,
                                                  K.ptr(VWc), K.ptr(rw), K.ptr(pbar), K.ptr(cov), K.ptr(dVW), K.ptr(Qp), B, T, C, K.stream()))
        torch.cuda.synchronize()
        return dVW, Qp.reshape(B, nq, 1056).sum(1)
    dv_a, q_a = lang(True)
    dv_b, q_b = lang(False)
    assert_close(dv_a, dv_b.float().cpu(), bf, "dVW", bf16=1e-2)
    assert_close(q_a, q_b.cpu(), torch.float32, "Q / u", f32=2e-3)
