"""lavt_sentence_attn_fwd / _bwd (csrc/text.hip) and ops.sentence_attention against the fp64 statement of tests/sentence_attn_ref.py.

Gates (none is taken from the code under test):
  fp32   for each of out, dq, dk, dv:  max |x - ref64| <= 10 * max |ref32 - ref64|, both references from the helper on the same inputs; the factor 10
         covers another summation order (the margin of test_gpu_dice_boundary.py)
  bf16   inputs bf16-rounded on both sides; the fp32 gate plus 2^-8 * max |ref64|: one rounding of the stored result, the half-ulp bound doubled
Exact probes: with one live key per sample the probabilities are exactly one-hot, so out, dv are copies / integer sums and dq, dk are exactly zero --
any head, sample, token or column-offset mis-indexing breaks bit equality.  Outputs and gradient buffers are NaN-prefilled before every raw call."""
import pytest
import torch

import sentence_attn_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = (torch.float32, torch.bfloat16)
_REFS = {}


def _abi(qkv, keybias, dout, keep, drop_scale, B, N, heads, dtype, hd=R.HD):
    """one forward + backward through the C ABI on NaN-prefilled outputs -> (out, dqkv) as fp32 CPU tensors"""
    from lavt_hip import _capi as K
    H = heads * hd
    q, kb, do = qkv.to(DEV).to(dtype).contiguous(), keybias.to(DEV).contiguous(), dout.to(DEV).to(dtype).contiguous()
    kp = None if keep is None else keep.to(DEV).contiguous()
    out = torch.full((B * N, H), float("nan"), dtype=dtype, device=DEV)
    dqkv = torch.full((B * N, 3 * H), float("nan"), dtype=dtype, device=DEV)
    K.check(K.lib.lavt_sentence_attn_fwd(K.dt(dtype), K.ptr(q), K.ptr(kb), K.ptr(kp), drop_scale, K.ptr(out), B, N, heads, hd, K.stream()))
    K.check(K.lib.lavt_sentence_attn_bwd(K.dt(dtype), K.ptr(q), K.ptr(kb), K.ptr(kp), drop_scale, K.ptr(do), K.ptr(dqkv), B, N, heads, hd, K.stream()))
    torch.cuda.synchronize()
    return out.float().cpu(), dqkv.float().cpu()


def _refs(case, with_keep, dtype):
    """the case's inputs (rounded to `dtype`) and its two references, computed once and shared"""
    key = (case, with_keep, dtype)
    if key not in _REFS:
        B, N, heads = case
        qkv, keybias, dout, keep, scale = R.case_inputs(B, N, heads, seed=11 + 7 * N + heads, with_keep=with_keep)
        qkv, dout = qkv.to(dtype).float(), dout.to(dtype).float()
        args = (qkv, keybias, dout, B, N, heads, keep, scale)
        _REFS[key] = ((qkv, keybias, dout, keep, scale), R.reference(*args, dtype=torch.float64), R.reference(*args, dtype=torch.float32))
    return _REFS[key]


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
@pytest.mark.parametrize("with_keep", (False, True), ids=("nodrop", "keep"))
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "B%d_N%d_h%d" % c)
def test_against_the_fp64_statement(case, with_keep, dtype):
    B, N, heads = case
    H = heads * R.HD
    (qkv, keybias, dout, keep, scale), ref64, ref32 = _refs(case, with_keep, dtype)
    out, dqkv = _abi(qkv, keybias, dout, keep, scale, B, N, heads, dtype)
    got = (out, dqkv[:, :H], dqkv[:, H:2 * H], dqkv[:, 2 * H:])
    for name, x, r64, r32 in zip(("out", "dq", "dk", "dv"), got, ref64, ref32):
        gate = 10.0 * float((r32.double() - r64).abs().max())
        if dtype == torch.bfloat16:
            gate += 2.0 ** -8 * float(r64.abs().max())
        err = float((x.double() - r64).abs().max())
        print(f"{case} keep={with_keep} {dtype} {name}: max|x - ref64| = {err:.3e}, gate {gate:.3e}")
        assert torch.isfinite(x).all(), f"{name}: an element was not written (NaN prefill) or is not finite"
        assert err <= gate, f"{name}: {err:.3e} > {gate:.3e}"


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
def test_one_live_key_is_an_exact_copy_and_an_exact_sum(dtype):
    B, N, heads = 3, 22, 2
    H = heads * R.HD
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(B * N, 3 * H, generator=g).to(dtype).float()
    dout = torch.randint(-3, 4, (B * N, H), generator=g).float()
    live = [4, 0, 21]                                         # the one live key of every sample: an inner token, the first, the last
    mask = torch.zeros(B, N, dtype=torch.long)
    for b, j in enumerate(live):
        mask[b, j] = 1
    out, dqkv = _abi(qkv, R.keybias_of(mask), dout, None, 1.0, B, N, heads, dtype)
    v = qkv[:, 2 * H:].view(B, N, H)
    want_out = torch.stack([v[b, j].expand(N, H) for b, j in enumerate(live)]).reshape(B * N, H)
    assert torch.equal(out, want_out), "out[b, i, head h] must be v[b, j_b, head h] bit for bit"
    want_dv = torch.zeros(B, N, H)
    for b, j in enumerate(live):
        want_dv[b, j] = dout.view(B, N, H)[b].sum(0)
    assert torch.equal(dqkv[:, 2 * H:], want_dv.reshape(B * N, H)), "dv: the live row holds the column sums of dout, every other row is zero"
    assert bool((dqkv[:, :2 * H] == 0).all()), "dq and dk are exactly zero under one-hot probabilities"


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
def test_keep_of_ones_is_no_dropout_and_runs_repeat_bit_for_bit(dtype):
    B, N, heads = 2, 33, 2
    (qkv, keybias, dout, keep, scale), _, _ = _refs((B, N, heads), True, dtype)
    plain = _abi(qkv, keybias, dout, None, 1.0, B, N, heads, dtype)
    ones = _abi(qkv, keybias, dout, torch.ones_like(keep), 1.0, B, N, heads, dtype)
    assert torch.equal(plain[0], ones[0]) and torch.equal(plain[1], ones[1])
    a, b = _abi(qkv, keybias, dout, keep, scale, B, N, heads, dtype), _abi(qkv, keybias, dout, keep, scale, B, N, heads, dtype)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(a[0], plain[0])          # (the mask does something)


@pytest.mark.parametrize("N,hd,heads", ((72, 64, 2), (20, 32, 4)), ids=("N72", "hd32"))
def test_outside_the_geometry_the_op_is_the_composed_route_and_the_entry_point_refuses(N, hd, heads):
    from lavt_hip import _capi as K, ops
    B, H = 2, heads * hd
    g = torch.Generator().manual_seed(9)
    qkv = torch.randn(B * N, 3 * H, generator=g).to(DEV)
    dout = torch.randn(B * N, H, generator=g).to(DEV)
    keybias = R.keybias_of(R.ragged_mask(B, N, 2)).to(DEV)
    res = []
    for fn in (ops.sentence_attention, ops.masked_self_attention):
        x = qkv.clone().requires_grad_(True)
        y = fn(x, keybias, B, N, heads)
        y.backward(dout)
        res.append((y.detach().clone(), x.grad.clone()))
    torch.cuda.synchronize()
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    out = torch.full((B * N, H), float("nan"), device=DEV)
    dqkv = torch.full((B * N, 3 * H), float("nan"), device=DEV)
    assert K.lib.lavt_sentence_attn_fwd(K.F32, K.ptr(qkv), K.ptr(keybias), None, 1.0, K.ptr(out), B, N, heads, hd, K.stream()) == -22
    assert K.lib.lavt_sentence_attn_bwd(K.F32, K.ptr(qkv), K.ptr(keybias), None, 1.0, K.ptr(dout), K.ptr(dqkv), B, N, heads, hd, K.stream()) == -22
    assert b"64" in K.lib.lavt_last_error()
    torch.cuda.synchronize()
    assert bool(out.isnan().all()) and bool(dqkv.isnan().all()), "a refused call launches nothing"


def test_the_op_matches_the_raw_entry_points_and_draws_its_mask_from_torchs_generator():
    from lavt_hip import ops
    B, N, heads = 2, 20, 12
    (qkv, keybias, dout, keep, scale), _, _ = _refs((B, N, heads), True, torch.float32)
    want = _abi(qkv, keybias, dout, keep, scale, B, N, heads, torch.float32)
    x = qkv.to(DEV).requires_grad_(True)
    y = ops.sentence_attention(x, keybias.to(DEV), B, N, heads, p_drop=0.1, keep=keep.to(DEV))
    y.backward(dout.to(DEV))
    assert torch.equal(y.detach().cpu(), want[0]) and torch.equal(x.grad.cpu(), want[1])
    runs = []
    for _ in range(2):
        torch.manual_seed(77)
        with torch.no_grad():
            runs.append(ops.sentence_attention(qkv.to(DEV), keybias.to(DEV), B, N, heads, p_drop=0.1).cpu())
    assert torch.equal(runs[0], runs[1]) and not torch.equal(runs[0], want[0])
