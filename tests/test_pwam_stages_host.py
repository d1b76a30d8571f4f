"""The fp64 stage statements of the fused PWAM kernels (tests/pwam_stages.py) checked themselves, CPU only.

(1) Chain against autograd: the stage functions, chained in the order of ops._PwamGate.forward / .backward with plain fp64 GEMMs between them, reproduce
    the unfused formulation `plain` and its autograd gradients to 1e-8 -- the two algebraic collapses (instance norm of q folded into the keys;
    IN(w) rebuilt from Pbar and Cov(P)) hold, and every reference the GPU tests use is the arithmetic of the model.
(2) Mutation self-test: the "kernel" is the floor evaluation (fp32, bf16 roundings of the contract) with one defect injected, at the smallest case of
    test_gpu_pwam_stages.py that the defect can touch.  The gate must reject every defect with a factor 2 to spare (E >= 2 K_STAGE F) and pass the
    unmutated floor."""
import functools

import pytest
import torch

import pwam_stages as S

F64 = torch.float64


# ------------------------------------------------------------------------------------------------ (1) chain against autograd
def _chain_case(B, T, C, n_l, masked):
    """masked: {sample: [word, ...]} words < n_l that carry -1e4"""
    g = torch.Generator("cpu").manual_seed(0)

    def rnd(*s, scale=1.0):
        return (scale * torch.randn(*s, generator=g, dtype=F64)).requires_grad_(True)
    mb = torch.zeros(B, S.J, dtype=F64)
    mb[:, n_l:] = -1e4
    for b, ws in masked.items():
        mb[b, ws] = -1e4
    live = (mb > -1.0).to(F64)[:, :, None]
    p = dict(x=rnd(B, T, C), Kl=(torch.randn(B, S.J, C, generator=g, dtype=F64) * live).requires_grad_(True),
             Vl=(torch.randn(B, S.J, C, generator=g, dtype=F64) * live).requires_grad_(True),
             Wv=rnd(C, C), bv=rnd(C), Wq=rnd(C, C), bq=rnd(C), Wo=rnd(C, C), bo=rnd(C), Wm=rnd(C, C), bm=rnd(C), W1=rnd(C, C, scale=0.3), W2=rnd(C, C, scale=0.3))
    return p, mb, torch.randn(B, T, C, generator=g, dtype=F64), torch.randn(B, T, C, generator=g, dtype=F64)


@pytest.mark.parametrize("B,T,C,n_l,masked", [(2, 37, 32, 5, {1: [3, 4]}), (1, 16, 64, 32, {0: [4, 29]})])
def test_stage_chain_reproduces_autograd(B, T, C, n_l, masked):
    p, mb, dr_out, dxg = _chain_case(B, T, C, n_l, masked)
    r_ref, xg_ref = S.plain(p["x"], p["Kl"], p["Vl"], mb, n_l, *(p[k] for k in "Wv bv Wq bq Wo bo Wm bm W1 W2".split()))
    names = list(p)
    ref = dict(zip(names, torch.autograd.grad((r_ref * dr_out).sum() + (xg_ref * dxg).sum(), [p[k] for k in names], allow_unused=True)))
    with torch.no_grad():
        x, Kl, Vl, Wv, bv, Wq, bq, Wo, Wm, bm, W1, W2 = (p[k] for k in "x Kl Vl Wv bv Wq bq Wo Wm bm W1 W2".split())
        alpha = C ** -0.5
        ein = torch.einsum
        # ---- forward, ops._PwamGate.forward
        vpre = x @ Wv.T                                   # (the bias joins in the mix kernel)
        q = x @ Wq.T + bq
        mean, rstd = q.mean(1), torch.rsqrt(q.var(1, unbiased=False) + S.EPS)
        wf = S.words_fwd(q, Kl, mean, rstd, mb, n_l, alpha)
        lf = S.lang_fwd(Vl, Wo, wf["PP"], wf["sumP"], T)
        assert torch.equal(lf["VWc"].transpose(1, 2), lf["VWw"])
        mm = S.mix0(wf["P"], lf["VWc"], lf["beta"], bv, vpre)["mm"]
        rpre = mm @ Wm.T + bm
        r = S._gelu(rpre)
        g1 = torch.relu(r @ W1.T)
        g2 = g1 @ W2.T
        xg = x + torch.tanh(g2) * r
        # ---- backward, ops._PwamGate.backward
        th = torch.tanh(g2)
        dg2 = dxg * r * (1 - th * th)
        dpre1 = (dg2 @ W2) * (g1 > 0)
        drpre = (dr_out + dxg * th + dpre1 @ W1) * S._gelu_grad(rpre)
        dmm = drpre @ Wm
        m1 = S.mix1(wf["P"], lf["VWc"], lf["beta"], bv, vpre, dmm)
        lb1 = S.lang_bwd1(m1["HT"], m1["s"], lf["VWc"], lf["rw"], lf["pbar"], lf["cov"], T)
        dS = S.words_bwd(m1["dwhat"], lf["VWw"], lb1["Q"], lb1["u"], lf["pbar"], wf["P"])["dS"]
        lb2 = S.lang_bwd2(ein("btj,btc->bjc", dS, q), dS.sum(1), Kl, mean, rstd, T, alpha)
        dq = S.mix2(dS, lb2["K2c"], lb2["c0"], lb2["c1"], q)["dq"]
        dvpre = m1["dvpre"]
        got = dict(x=dxg + dvpre @ Wv + dq @ Wq, Kl=lb2["dK"], Vl=lb1["dVW"] @ Wo, Wv=ein("btn,btk->nk", dvpre, x), bv=dvpre.sum((0, 1)),
                   Wq=ein("btn,btk->nk", dq, x), bq=dq.sum((0, 1)), Wo=ein("bjc,bje->ce", lb1["dVW"], Vl), bo=torch.zeros(C, dtype=F64),
                   Wm=ein("btn,btk->nk", drpre, mm), bm=drpre.sum((0, 1)), W1=ein("btn,btk->nk", dpre1, r), W2=ein("btn,btk->nk", dg2, g1))

    def close(a, b, name):
        e, sc = float((a - b).abs().max()), float(b.abs().max())
        assert e <= 1e-8 * max(sc, 1.0), (name, e, sc)
    close(r, r_ref.detach(), "r")
    close(xg, xg_ref.detach(), "xg")
    for k in names:
        close(got[k], ref[k] if ref[k] is not None else torch.zeros_like(got[k]), k)
    # masked and padding words: no probability, no key / value gradient
    dead = (mb < -1.0)
    assert float(wf["P"][dead[:, None, :].expand_as(wf["P"])].abs().max()) == 0.0
    assert float(got["Kl"][dead].abs().max()) == 0.0 and float(ref["Kl"][dead].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ (2) mutation self-test
@functools.lru_cache(maxsize=None)
def _case(*a, **k):
    return S.Case(*a, **k)


def _eval(fn, args, **k):
    """(reference, floor) of one stage"""
    return S.reference(fn, *args, **k), S.floor(fn, *args, **k)


def _check(pairs, ref, flo, must=None):
    """pairs: {output name: mutated floor tensor}.  The unmutated floor is accepted on every output; the mutated one is rejected on every output
    named in `must` (default: all of pairs) -- a kernel's gate is the conjunction over its outputs, so one rejecting output fails its test."""
    for name, mut in pairs.items():
        S.gate(name, flo[name], ref[name], flo[name], scale=S.scale_of(name, ref))
    for name in (pairs if must is None else must):
        sc = S.scale_of(name, ref)
        assert S.rejects(name, pairs[name], ref[name], flo[name], sc), (name, S.row_error(pairs[name], ref[name], sc), S.K_STAGE[name], S.row_error(flo[name], ref[name], sc))


def _with(args, idx, value):
    a = list(args)
    a[idx] = value
    return tuple(a)


def test_mutation_01_tail_tile_rows():
    """rows of the last partial tile take row T - 1's values: every row-streaming kernel at its smallest case, T = 5 (rows 0..4 of the only tile).
    n_l = 3, the mix kernels' GPU case: at n_l = 1 every P row is (1, 0, ...), so what, dS and c1 vanish and mm, d vpre, dS, dq are identically zero."""
    c = _case(2, 5, 32, 3)
    for fn, args, names in ((S.words_fwd, c.words_fwd_args, ["P"]), (S.mix0, c.mix0_args(), ["mm"]), (S.mix1, c.mix1_args(), ["dvpre", "dwhat"]),
                            (S.mix2, c.mix2_args, ["dq"]), (S.words_bwd, c.words_bwd_args, ["dS"])):
        ref, flo = _eval(fn, args)
        for n in names:
            assert float(ref[n].abs().max()) > 0.0, n
        _check({n: S.tail_rows_from_last(flo[n], 5) for n in names}, ref, flo)


def test_mutation_02_last_word_left_out():
    c = _case(2, 37, 96, 17)
    ref, flo = _eval(S.words_fwd, c.words_fwd_args)
    mut = S.floor(S.words_fwd, *_with(c.words_fwd_args, 5, 16))
    _check({k: mut[k] for k in ("P", "PP", "sumP")}, ref, flo)


def test_mutation_03_word_slot_n_l_let_in():
    """with -1e4 at the padding words the kernel's j < n_l bound is redundant; the case with open padding (maskbias 0 there) is the one that holds it"""
    c = _case(2, 37, 96, 17, open_padding=True)
    ref, flo = _eval(S.words_fwd, c.words_fwd_args)
    mut = S.floor(S.words_fwd, *_with(c.words_fwd_args, 5, 18))
    _check({k: mut[k] for k in ("P", "PP", "sumP")}, ref, flo)


def test_mutation_04_masked_word_inside_unmasked():
    c = _case(2, 48, 192, 32, masked_inside=True)
    ref, flo = _eval(S.words_fwd, c.words_fwd_args)
    mb = c.i["maskbias"].clone()
    mb[0, 1] = 0.0
    mut = S.floor(S.words_fwd, *_with(c.words_fwd_args, 4, mb))
    _check({k: mut[k] for k in ("P", "PP", "sumP")}, ref, flo)


def test_mutation_05_k_step_dropped_in_later_tiles():
    """one 32-channel k-step missing from the contraction, for the rows of tiles beyond a wave's first only.  Forward: (1, 2100, 672, 20) with records,
    32 workgroups x 4 waves x 16 rows = 2048 rows in the first pass.  Backward: two samples of (64, 1100, 160, 20), where the per-batch cap leaves
    16 workgroups = 1024 rows in the first pass (the set of later rows does not depend on the number of samples evaluated here)."""
    c = _case(1, 2100, 672, 20)
    ref, flo = _eval(S.words_fwd, c.words_fwd_args)
    q = c.i["q"].clone()
    q[..., 32:64] = 0.0
    mut = S.floor(S.words_fwd, *_with(c.words_fwd_args, 0, q))["P"]
    P = flo["P"].clone()
    P[:, 2048:] = mut[:, 2048:]
    _check({"P": P}, ref, flo)
    c = _case(2, 1100, 160, 20)
    ref, flo = _eval(S.words_bwd, c.words_bwd_args)
    dw = c.m1["dwhat"].clone()
    dw[..., 32:64] = 0.0
    mut = S.floor(S.words_bwd, *_with(c.words_bwd_args, 0, dw))["dS"]
    dS = flo["dS"].clone()
    dS[:, 1024:] = mut[:, 1024:]
    _check({"dS": dS}, ref, flo)


def test_mutation_06_beta_omitted():
    c = _case(2, 5, 32, 3)          # (the mix kernels' smallest GPU case; at n_l = 1 what = P VW' + beta is identically zero)
    assert float(c.lf["beta"].abs().min()) > 0.0
    zero = torch.zeros_like(c.lf["beta"])
    ref, flo = _eval(S.mix0, c.mix0_args())
    _check({"mm": S.floor(S.mix0, *_with(c.mix0_args(), 2, zero))["mm"]}, ref, flo)
    ref, flo = _eval(S.mix1, c.mix1_args())
    _check({"dvpre": S.floor(S.mix1, *_with(c.mix1_args(), 2, zero))["dvpre"]}, ref, flo)


@pytest.mark.parametrize("how", ["not written", "copied from the first span"])
def test_mutation_07_last_32_channel_span(how):
    c = _case(2, 37, 96, 17)          # C % 64 == 32

    def mutate(t):
        t = t.clone()
        t[..., 64:] = 0.0 if how == "not written" else t[..., :32]          # (the GPU tests pre-fill with NaN: an unwritten span is an infinite error there)
        return t
    for fn, args, names in ((S.mix0, c.mix0_args(), ["mm"]), (S.mix1, c.mix1_args(), ["dvpre", "dwhat"]), (S.mix2, c.mix2_args, ["dq"])):
        ref, flo = _eval(fn, args)
        _check({n: mutate(flo[n]) for n in names}, ref, flo)


def test_mutation_08_one_record_omitted():
    """from each records sum: P^T P / colsum(P) into lang_fwd, H^T / s into lang_bwd1, Q / u into words_bwd.  The stage functions take totals: the
    mutated kernel's total lacks the last of the unevenly split records."""
    c = _case(2, 37, 32, 20)
    # lang_fwd, nrec = 32 (the smallest share is 1 / 64 of the total)
    ref, flo = _eval(S.lang_fwd, c.lang_fwd_args)
    rp, rs = S.split_records(c.wf["PP"], 32, 1), S.split_records(c.wf["sumP"], 32, 1)
    mut = S.floor(S.lang_fwd, *_with(_with(c.lang_fwd_args, 2, rp[:, :-1].double().sum(1)), 3, rs[:, :-1].double().sum(1)))
    # (beta = -Pbar VW' cancels to near zero in some channel, where the bf16 rounding of VW' is its whole error: its floor is ~0.2 and cannot show this)
    _check({k: mut[k] for k in ("pbar", "cov", "rw", "VWc", "beta")}, ref, flo, must=("pbar", "cov", "rw"))
    # lang_bwd1
    ref, flo = _eval(S.lang_bwd1, c.lang_bwd1_args)
    rh, rs = S.split_records(c.m1["HT"], 32, 2), S.split_records(c.m1["s"], 32, 2)
    mut = S.floor(S.lang_bwd1, *_with(_with(c.lang_bwd1_args, 0, rh[:, :-1].double().sum(1)), 1, rs[:, :-1].double().sum(1)))
    _check({k: mut[k] for k in ("dVW", "Q", "u")}, ref, flo)
    # words_bwd: lavt_pwam_q_parts(96) = 6 records
    c17 = _case(2, 37, 96, 17)          # (at (2, 5, 32, 1) dS is identically 0 whatever Q is -- P = 1 makes softmax' vanish -- so the first case that can show it)
    ref, flo = _eval(S.words_bwd, c17.words_bwd_args)
    rq, ru = S.split_records(c17.lb1["Q"], 6, 3), S.split_records(c17.lb1["u"], 6, 3)
    mut = S.floor(S.words_bwd, *_with(_with(c17.words_bwd_args, 2, rq[:, :-1].double().sum(1)), 3, ru[:, :-1].double().sum(1)))
    _check({"dS": mut["dS"]}, ref, flo)


def test_mutation_09_quads_left_unswapped():
    c = _case(2, 37, 96, 17)
    for fn, args, names in ((S.words_fwd, c.words_fwd_args, ["P"]), (S.words_bwd, c.words_bwd_args, ["dS"]), (S.mix0, c.mix0_args(), ["mm"]),
                            (S.mix1, c.mix1_args(), ["dvpre", "dwhat"]), (S.mix2, c.mix2_args, ["dq"])):
        ref, flo = _eval(fn, args)
        _check({n: S.unswap_quads(flo[n]) for n in names}, ref, flo)


def test_mutation_10_q_c1_term_omitted():
    c = _case(2, 5, 32, 1)
    c17 = _case(2, 37, 96, 17)          # (n_l = 1: dS = 0, so c1 = 0 and the term is not there to omit)
    ref, flo = _eval(S.mix2, c17.mix2_args)
    _check({"dq": S.floor(S.mix2, *_with(c17.mix2_args, 3, torch.zeros_like(c17.lb2["c1"])))["dq"]}, ref, flo)
    assert float(c.lb2["c1"].abs().max()) == 0.0


def test_mutation_11_softmax_dot_over_16_words():
    c = _case(2, 37, 96, 17)
    ref, flo = _eval(S.words_bwd, c.words_bwd_args)
    dP, P = S.words_bwd_dP(*c.words_bwd_args, dtype=torch.float32, round_bf16=True)
    mut = S.bf(P * (dP - (P[..., :16] * dP[..., :16]).sum(-1, keepdim=True)))
    _check({"dS": mut}, ref, flo)


def test_gate_factors_follow_the_measured_ratios():
    """K_STAGE is twice the largest E / F measured on MI355X (the table beside the GPU tests), never under 1: the two tables cannot drift apart"""
    from test_gpu_pwam_stages import MEASURED
    assert set(MEASURED) == set(S.K_STAGE)
    for n, ratio in MEASURED.items():
        assert S.K_STAGE[n] == S.k_from_measured(ratio), (n, S.K_STAGE[n], ratio)


def test_rejects_is_strict():
    """a defect that changes nothing is never counted as caught, not even where reference and floor are identically zero"""
    c = _case(2, 5, 32, 1)
    ref, flo = _eval(S.mix0, c.mix0_args())
    assert float(ref["mm"].abs().max()) == 0.0 and not S.rejects("mm", S.tail_rows_from_last(flo["mm"], 5), ref["mm"], flo["mm"])
