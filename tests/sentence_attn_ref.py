"""The HF `BertSelfAttention` core (transformers 3.0.2 modeling_bert.py) with an explicit dropout keep mask, as a torch statement -- the reference of
tests/test_sentence_attention_host.py and tests/test_gpu_sentence_attention.py:

    scores = q k^T / sqrt(hd) + keybias[:, None, None, :]        keybias = (1 - attention_mask) * -10000
    P  = softmax(scores, -1);   Pd = P * keep * drop_scale        (nn.Dropout with a given mask)
    out = Pd v

on the token-major layout of lavt_sentence_attn_fwd: qkv [B*N, 3H] with columns q | k | v, each heads x hd; out [B*N, H].  `reference` evaluates it in
fp64 (the truth) or in fp32 (what a correct fp32 implementation with another summation order may differ from the truth by), both on the CPU, and
returns out and -- through autograd -- dq, dk, dv as [B*N, H] each."""
import torch

CASES = ((1, 1, 2), (2, 20, 12), (3, 22, 2), (2, 33, 2), (2, 64, 2))          # (B, N, heads); hd = 64
HD = 64


def sentence_attention_ok(N, hd):
    """the geometry the fused kernels cover (include/lavt_hip.h)"""
    return hd == 64 and 1 <= N <= 64


def reference(qkv, keybias, dout, B, N, heads, keep=None, drop_scale=1.0, dtype=torch.float64):
    """qkv [B*N, 3H], keybias [B, N], dout [B*N, H], keep uint8 [B, heads, N, N] or None -> (out, dq, dk, dv), each [B*N, H] in `dtype` on the CPU"""
    H = qkv.shape[1] // 3
    hd = H // heads
    x = qkv.detach().cpu().to(dtype).clone().requires_grad_(True)
    q, k, v = (x[:, i * H:(i + 1) * H].view(B, N, heads, hd).permute(0, 2, 1, 3) for i in range(3))          # [B, heads, N, hd]
    scores = torch.matmul(q, k.transpose(-1, -2)) / (hd ** 0.5) + keybias.detach().cpu().to(dtype).view(B, 1, 1, N)
    p = torch.softmax(scores, dim=-1)
    if keep is not None:
        p = p * (keep.detach().cpu().to(dtype) * drop_scale)
    out = torch.matmul(p, v).permute(0, 2, 1, 3).reshape(B * N, H)
    out.backward(dout.detach().cpu().to(dtype))
    g = x.grad
    return out.detach(), g[:, :H].clone(), g[:, H:2 * H].clone(), g[:, 2 * H:].clone()


def ragged_mask(B, N, seed):
    """attention mask int64 [B, N]: a prefix of ones per sample -- sample 0 has the full length, the last sample length 1 (when B > 1), the others random"""
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(1, N + 1, (B,), generator=g)
    lens[0] = N
    if B > 1:
        lens[-1] = 1
    return (torch.arange(N)[None, :] < lens[:, None]).long()


def keybias_of(mask):
    return (1.0 - mask.to(torch.float32)) * -10000.0


def case_inputs(B, N, heads, seed, with_keep, p=0.1):
    """(qkv, keybias, dout, keep or None, drop_scale): fp32 CPU tensors drawn from a fixed seed"""
    g = torch.Generator().manual_seed(seed)
    H = heads * HD
    qkv = torch.randn(B * N, 3 * H, generator=g)
    dout = torch.randn(B * N, H, generator=g)
    keep = (torch.rand(B, heads, N, N, generator=g) >= p).to(torch.uint8) if with_keep else None
    return qkv, keybias_of(ragged_mask(B, N, seed + 1)), dout, keep, (1.0 / (1.0 - p) if with_keep else 1.0)
