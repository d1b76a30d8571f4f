"""GPU checks of the streaming bf16 window attention (csrc/attention_stream.hip, ops._WindowAttnStream): Video-Swin --window12 windows of up to
1152 tokens (lib/video_swin_transformer.py:137-168 with window_size (8, 12, 12)) -- parity of the forward, lse and every gradient with the fp32 CPU
statement, the online-softmax rescale branch forced, the route, the memory it saves, bitwise reproducible backward, a block and a captured step."""
import os
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from test_gpu_ops import assert_close, dev, rnd, run_pair

pytestmark = pytest.mark.gpu
W12 = (8, 12, 12)


def _case(dims, heads, shifted, batch=2):
    from lavt_hip import rowmaps
    from oracle import lavt_video_oracle as OV
    win, shift = rowmaps.clip_window(dims, W12, tuple(w // 2 for w in W12) if shifted else (0, 0, 0))
    N = win[0] * win[1] * win[2]
    nW = (dims[0] // win[0]) * (dims[1] // win[1]) * (dims[2] // win[2])
    moved = any(shift)
    region = torch.from_numpy(rowmaps.region_ids3d_np(*dims, win, shift)).to(dev()) if moved else None
    mask = OV.shift_mask_3d(*dims, win, shift) if moved else None
    idx = OV.rel_pos_index_3d(*W12)[:N, :N].reshape(-1)
    return SimpleNamespace(N=N, nW=nW, Bw=batch * nW, region=region, mask=mask, idx=idx, heads=heads, C=heads * 32,
                           R=(2 * W12[0] - 1) * (2 * W12[1] - 1) * (2 * W12[2] - 1))


def _scores(cs, qkv, table):
    q, k, v = qkv.view(cs.Bw, cs.N, 3, cs.heads, 32).permute(2, 0, 3, 1, 4)
    a = (q * 32 ** -0.5) @ k.transpose(-1, -2) + table[cs.idx].view(cs.N, cs.N, cs.heads).permute(2, 0, 1)[None].to(q.dtype)
    if cs.mask is not None:
        a = (a.view(cs.Bw // cs.nW, cs.nW, cs.heads, cs.N, cs.N) + cs.mask[None, :, None].to(q.dtype)).view(cs.Bw, cs.heads, cs.N, cs.N)
    return a, v


def _ref(cs):
    def ref(qkv, table):
        a, v = _scores(cs, qkv, table)
        return (a.softmax(-1) @ v).transpose(1, 2).reshape(cs.Bw * cs.N, cs.C)
    return ref


def _grad_fn_name(y):
    return type(y.grad_fn).__name__


@pytest.mark.parametrize("dims,heads,shifted", [((8, 12, 12), 2, 0), ((8, 24, 24), 2, 1), ((16, 12, 12), 1, 1), ((4, 12, 12), 1, 0),
                                                ((8, 10, 10), 2, 0), ((5, 12, 11), 1, 0), ((7, 24, 24), 2, 1)])
def test_stream_parity(dims, heads, shifted):
    """forward, lse and the qkv / table gradients against the fp32 CPU statement, through run_pair's bf16 gates"""
    from lavt_hip import ops, _capi as K
    cs = _case(dims, heads, shifted)
    assert cs.N > ops.FUSED_ATTN_MAX_N_BF16
    inputs = {"qkv": (rnd(cs.Bw * cs.N, 3 * cs.C, seed=1), "act"), "table": (rnd(cs.R, heads, seed=2, scale=0.5), "param")}
    seen = []

    def hip(qkv, table):
        y = ops.window_attention(qkv, table, cs.region, W12, heads, N=cs.N)
        seen.append(_grad_fn_name(y))
        return y
    run_pair(hip, _ref(cs), inputs, torch.bfloat16, name=f"stream attention {dims}", l2=2e-2)
    assert seen == ["_WindowAttnStreamBackward"], seen
    # lse: natural-log domain, [nwin][heads][N]
    qkv = inputs["qkv"][0].to(torch.bfloat16)
    table = inputs["table"][0]
    a, _ = _scores(cs, qkv.float(), table)
    lse_ref = torch.logsumexp(a, -1)
    qg = qkv.to(dev())
    out = torch.empty(cs.Bw * cs.N, cs.C, dtype=torch.bfloat16, device=dev())
    lse = torch.empty(cs.Bw, heads, cs.N, dtype=torch.float32, device=dev())
    nw_img = cs.region.shape[0] if cs.region is not None else 0
    K.check(K.lib.lavt_window_attn_stream_fwd(K.BF16, K.ptr(qg), K.ptr(cs.region), nw_img, K.ptr(out), K.ptr(lse), K.ptr(table.to(dev())),
                                              *W12, cs.Bw, cs.N, heads, 32, 32 ** -0.5, K.stream()))
    torch.cuda.synchronize()
    assert float((lse.cpu() - lse_ref).abs().max()) < 2e-3 * max(1.0, float(lse_ref.abs().max()))


def test_stream_online_rescale_forced():
    """Guide rule 26: the running maximum of some query rows jumps at a LATE key tile (a Q row spiked against one K row near the end of the
    window), so the rescale of the accumulated O and sum is exercised with a large factor; full tensors against an fp64 CPU reference."""
    from lavt_hip import ops
    cs = _case((8, 12, 12), 1, 0, batch=1)
    qkv = rnd(cs.N, 96, seed=7, scale=0.5)
    u = torch.ones(32) / 32 ** 0.5
    for r in range(8):
        i, j = 7 + 131 * r, cs.N - 1 - 37 * r          # keys in tiles 13..17 of 18
        qkv[i, :32] = 6.0 * u
        qkv[j, 32:64] = 6.0 * u                         # score 36 / sqrt(32) = 6.4 (x log2 e in the kernel's domain) above the rest
        qkv[j, 64:] = 3.0 - r
    table = rnd(cs.R, 1, seed=8, scale=0.5)
    qkv = qkv.to(torch.bfloat16).double()
    qc = qkv.clone().requires_grad_(True)
    tc = table.double().clone().requires_grad_(True)
    y_ref = _ref(cs)(qc, tc)
    go = rnd(*y_ref.shape, seed=99).to(torch.bfloat16).double()
    y_ref.backward(go)
    qg = qkv.float().to(dev()).to(torch.bfloat16).requires_grad_(True)
    tg = table.to(dev()).requires_grad_(True)
    y = ops.window_attention(qg, tg, None, W12, 1, N=cs.N)
    assert _grad_fn_name(y) == "_WindowAttnStreamBackward"
    y.backward(go.float().to(dev()).to(torch.bfloat16))
    torch.cuda.synchronize()
    assert_close(y, y_ref.float(), torch.bfloat16, "rescale forward", l2=2e-2)
    spiked = [7 + 131 * r for r in range(8)]
    err = float((y.detach().float().cpu()[spiked] - y_ref.detach().float()[spiked]).abs().max())
    assert err < 3e-2 * float(y_ref.detach().abs().max()), f"spiked rows off by {err}"
    assert_close(qg.grad, qc.grad.float(), torch.bfloat16, "rescale dqkv", bf16=4.5e-2, l2=3e-2)
    assert_close(tg.grad, tc.grad.float(), torch.bfloat16, "rescale dtable", bf16=4.5e-2, l2=3e-2)


def test_stream_route():
    from lavt_hip import ops
    cs = _case((8, 12, 12), 2, 0, batch=1)
    qkv = rnd(cs.N, 3 * cs.C, seed=1).to(dev()).to(torch.bfloat16).requires_grad_(True)
    table = rnd(cs.R, 2, seed=2).to(dev()).requires_grad_(True)
    prev = os.environ.pop("LAVT_ATTN_COMPOSED", None)
    try:
        assert _grad_fn_name(ops.window_attention(qkv, table, None, W12, 2, N=cs.N)) == "_WindowAttnStreamBackward"
        os.environ["LAVT_ATTN_COMPOSED"] = "1"
        assert _grad_fn_name(ops.window_attention(qkv, table, None, W12, 2, N=cs.N)) == "_WindowAttnComposedBackward"
        # fp32 stays on the composed route, bf16 <= 400 tokens on the fused kernels
        del os.environ["LAVT_ATTN_COMPOSED"]
        assert _grad_fn_name(ops.window_attention(qkv.detach().float().requires_grad_(True), table, None, W12, 2, N=cs.N)) == "_WindowAttnComposedBackward"
        q392 = rnd(392, 3 * cs.C, seed=3).to(dev()).to(torch.bfloat16).requires_grad_(True)
        t392 = rnd(13 * 13 * 15, 2, seed=4).to(dev()).requires_grad_(True)
        assert _grad_fn_name(ops.window_attention(q392, t392, None, (8, 7, 7), 2, N=392)) == "_WindowAttnBackward"
    finally:
        os.environ.pop("LAVT_ATTN_COMPOSED", None)
        if prev is not None:
            os.environ["LAVT_ATTN_COMPOSED"] = prev


def test_stream_memory_stage0_layer():
    """A stage-0-like layer (dims (8, 48, 48), 4 heads, C = 128, 16 windows of 1152 tokens): forward + backward allocate < 64 MB beyond the inputs and
    outputs.  The composed route holds S and P ([64, 1152, 1152] bf16, 170 MB each)."""
    from lavt_hip import ops
    nwin, N, heads, C = 16, 1152, 4, 128
    R = 15 * 23 * 23
    torch.cuda.synchronize()
    qkv = (torch.randn(nwin * N, 3 * C, device=dev()) * 0.5).to(torch.bfloat16).requires_grad_(True)
    table = (torch.randn(R, heads, device=dev()) * 0.5).requires_grad_(True)
    go = torch.randn(nwin * N, C, device=dev()).to(torch.bfloat16)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    y = ops.window_attention(qkv, table, None, W12, heads, N=N)
    assert _grad_fn_name(y) == "_WindowAttnStreamBackward"
    y.backward(go)
    torch.cuda.synchronize()
    io = y.numel() * 2 + qkv.numel() * 2 + table.numel() * 4          # out, dqkv, table gradient
    extra = torch.cuda.max_memory_allocated() - base - io
    assert extra < 64 * 2 ** 20, f"{extra / 2 ** 20:.1f} MB beyond inputs and outputs"


def test_stream_backward_bitwise_reproducible():
    from lavt_hip import ops
    cs = _case((8, 24, 24), 2, 1, batch=1)
    qkv = rnd(cs.Bw * cs.N, 3 * cs.C, seed=11).to(dev()).to(torch.bfloat16).requires_grad_(True)
    table = rnd(cs.R, 2, seed=12, scale=0.5).to(dev()).requires_grad_(True)
    go = rnd(cs.Bw * cs.N, cs.C, seed=13).to(dev()).to(torch.bfloat16)
    res = []
    for _ in range(2):
        y = ops.window_attention(qkv, table, cs.region, W12, 2, N=cs.N)
        res.append(torch.autograd.grad(y, (qkv, table), go))
    torch.cuda.synchronize()
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


@pytest.mark.parametrize("shifted", [0, 1])
def test_stream_video_block_vs_composed(shifted):
    """SwinTransformerBlock3D(64, 2, (8, 12, 12)) in bf16: output, input gradient and every parameter gradient on the streaming route against the same
    block on the composed route"""
    import lavt_hip
    from lavt_hip.detweights import fill_state_dict_
    from lib.video_swin_transformer import SwinTransformerBlock3D

    def run(composed):
        blk = SwinTransformerBlock3D(64, 2, W12, (4, 6, 6) if shifted else (0, 0, 0))
        fill_state_dict_(blk)
        blk.to(dev())
        x = rnd(1, 8, 24, 24, 64, seed=21).to(dev()).requires_grad_(True)
        if composed:
            os.environ["LAVT_ATTN_COMPOSED"] = "1"
        try:
            with lavt_hip.use_dtype(torch.bfloat16):
                y = blk(x)
                y.float().square().sum().backward()
        finally:
            os.environ.pop("LAVT_ATTN_COMPOSED", None)
        torch.cuda.synchronize()
        return y.detach().float().cpu(), x.grad.float().cpu(), {n: p.grad.float().cpu() for n, p in blk.named_parameters() if p.grad is not None}
    ys, xs, gs = run(False)
    yc, xc, gc = run(True)
    assert_close(ys, yc, torch.bfloat16, "block output", bf16=3e-2, l2=1e-2)
    assert_close(xs, xc, torch.bfloat16, "block dx", bf16=4.5e-2, l2=2e-2)
    assert gs.keys() == gc.keys() and len(gs) > 0
    for n in gs:
        assert_close(gs[n], gc[n], torch.bfloat16, f"block grad {n}", bf16=4.5e-2, l2=3e-2)


class _VideoLowres(torch.nn.Module):
    """(clip, l_feats, l_mask) -> logits, as LAVTVideo.forward_backbone + upsample; `forward_lowres` absent: the step uses the plain loss"""

    def __init__(self, backbone, classifier):
        super().__init__()
        self.backbone, self.classifier = backbone, classifier

    def forward(self, x, l, m):
        from lib._utils import _upsample_logits
        f = self.backbone(x.permute(0, 2, 1, 3, 4), l, m)
        return _upsample_logits(self.classifier(f[3], f[2], f[1], f[0]), x.shape[-2:])


def _micro_video_w12():
    from lavt_hip import ops
    from lavt_hip.detweights import fill_state_dict_
    ops.weights.invalidate()            # (a new model's parameters may reuse a freed one's ids: no stale compute-dtype copies)
    from lib.mask_predictor import SimpleDecoding
    from lib.video_swin_transformer import MultiModalSwinTransformer3D
    a = SimpleNamespace()
    bb = MultiModalSwinTransformer3D(patch_size=(1, 4, 4), embed_dim=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8], window_size=W12,
                                     drop_path_rate=0.0, patch_norm=True, out_indices=(0, 1, 2, 3), num_heads_fusion=[1, 1, 1, 1], fusion_drop=0.0, args=a)
    model = _VideoLowres(bb, SimpleDecoding(256, a))
    fill_state_dict_(model)
    return model.to(dev()).train()


def _grad_rel(a, b):
    return float((a.float() - b.float()).norm()) / max(float(b.float().norm()), 1e-12)


def test_stream_micro_video_w12_captured_step(monkeypatch):
    """A micro Video-Swin LAVT with window (8, 12, 12) (stages 0 and 1 on the streaming kernels) trains under TrainStep(use_graph=True).

    What is compared, and why this way (measured on MI355X with this model, bf16):
      * two EAGER runs of the same route already differ by 2-3 % relative l2 in some parameter gradients (kernels outside the attention core sum in
        no fixed order; the train-mode norms of this small random network amplify last-bit differences) -- the same on the fused 8x7x7 route;
      * the eager streaming and eager composed routes differ in the loss by 3e-4 relative, and then by up to 60 % in parameter gradients -- also in
        stage 3 (N = 72, fused kernels), whose gradients no streaming backward kernel touches: forward rounding differences amplified, not an
        attention-gradient error.  Route equivalence of the gradients is therefore checked where it is well conditioned: the op against the fp32
        CPU statement (test_stream_parity) and a block against the composed route (test_stream_video_block_vs_composed).
    Here: the forward (logits against the fp32 path, loss) against the eager composed route; the captured replay's loss and every parameter gradient against an eager
    step on the same (streaming) route, at 3x the measured run-to-run floor; two replays against each other."""
    import lavt_hip
    from lavt_hip import ops
    from lavt_hip.detweights import det_inputs
    from lavt_hip.engine import TrainStep
    routes = []
    plain = ops.window_attention

    def counting(*a, **k):
        y = plain(*a, **k)
        routes.append(_grad_fn_name(y))
        return y
    monkeypatch.setattr(ops, "window_attention", counting)
    noise = ("image_lang_att.f_key.0.bias", "image_lang_att.f_value.0.bias")      # analytically zero gradients (rounding noise): as in
    w = torch.tensor([0.9, 1.1], device=dev())                                      # test_gpu_modules.test_train_step_gradients_match_plain_autograd
    lavt_hip.set_compute_dtype(torch.bfloat16)
    try:
        x, l, m, t = det_inputs(1, 96, 20, seed=5, frames=8)
        x, l, m, t = x.to(dev()), l.to(dev()), m.to(dev()), t.to(dev())
        lavt_hip.set_compute_dtype(torch.float32)
        with torch.no_grad():
            logits_32 = _micro_video_w12()(x, l, m).float()         # exact-fp32 path: the yardstick of both bf16 routes' forward
        lavt_hip.set_compute_dtype(torch.bfloat16)
        monkeypatch.setenv("LAVT_ATTN_COMPOSED", "1")
        with torch.no_grad():
            logits_c = _micro_video_w12()(x, l, m)
            loss_c = float(F.cross_entropy(logits_c, t, weight=w))
        monkeypatch.delenv("LAVT_ATTN_COMPOSED")
        assert "_WindowAttnStreamBackward" not in routes
        routes.clear()
        ref_model = _micro_video_w12()
        logits = ref_model(x, l, m)
        loss = F.cross_entropy(logits, t, weight=w)
        loss.backward()
        torch.cuda.synchronize()
        assert routes.count("_WindowAttnStreamBackward") == 4, routes          # the two blocks of stages 0 and 1
        # Train-mode logits of this network are ~5 % (max) / 3.5 % (l2) away from the fp32 path on EITHER bf16 route -- the fused 8x7x7 route too:
        # the streaming route must be no further from fp32 than the composed one
        def dist(a):
            a = a.detach().float()
            return float((a - logits_32).abs().max()) / float(logits_32.abs().max()), float((a - logits_32).norm()) / float(logits_32.norm())
        (ms, ls), (mc, lc) = dist(logits), dist(logits_c)
        assert ms <= 1.25 * mc + 5e-3 and ls <= 1.25 * lc + 5e-3 and ls < 6e-2, ((ms, ls), (mc, lc))
        assert abs(float(loss.detach()) - loss_c) < 2e-3 * abs(loss_c)
        ref = {n: p.grad.clone() for n, p in ref_model.named_parameters() if p.grad is not None and not n.endswith(noise)}
        model = _micro_video_w12()
        step = TrainStep(model, x, l, m, t, use_graph=True, fused_loss=False)
        step.warmup_and_capture(eager_iters=1)
        assert step.captured
        step.step()
        torch.cuda.synchronize()
        loss1 = float(step.loss)
        g1 = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None and not n.endswith(noise)}
        common = [n for n in ref if n in g1]
        assert len(common) >= 0.9 * len(ref) and len(common) > 100, (len(common), len(ref), len(g1))
        assert abs(loss1 - float(loss)) <= 1e-5 * abs(float(loss))
        bad = [(n, _grad_rel(g1[n], ref[n])) for n in common if _grad_rel(g1[n], ref[n]) > 0.1]
        assert not bad, bad[:10]
        step.step()
        torch.cuda.synchronize()
        assert abs(float(step.loss) - loss1) <= 1e-5 * abs(loss1)
        bad = [(n, _grad_rel(p.grad, g1[n])) for n, p in model.named_parameters() if n in g1 and _grad_rel(p.grad, g1[n]) > 0.1]
        assert not bad, bad[:10]
    finally:
        lavt_hip.set_compute_dtype(torch.float32)
