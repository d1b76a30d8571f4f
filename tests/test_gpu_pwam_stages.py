"""Every kernel of csrc/pwam.hip alone, through the C ABI, against its fp64 statement in tests/pwam_stages.py.

A test builds synthetic inputs on the CPU (bf16 tensors rounded first, so both sides start from the same values; what an earlier stage would have
produced comes from that stage's FUNCTION, never from its kernel: a test fails for its own kernel only), calls the one kernel, and holds every
output to the gate of pwam_stages: row error E <= K_STAGE x F, F the row error of the fp32 / bf16 floor of the same case.  A second run must be
bit-identical.  Outputs are pre-filled with NaN (an unwritten element is an infinite error), strided buffers carry NaN outside the columns the
kernel owns (inputs: a read outside them poisons the result; outputs: they must come back untouched).

The cases are the smallest that enter each branch of the kernels: the k-loop forms of the words kernel (prefetch of 16 / 8 steps, 16-at-a-time,
4-at-a-time, remainder), the later tiles of a wave (records cap; per-batch cap), both workgroup sizes, the tail loop of the language forward above
C = 1024, the 16-at-a-time record loops at 1 / 15 / 16 / 17 / 32 records, a last channel group of 32, word counts 1, 3, 17 (cutting a lane quad), 32,
T < 16, and the product's strides.

Out of scope: the grid cap of lavt_pwam_mix (8192 workgroups) is reached only at T * C above about 33 M per sample; no stage of the image or video
model does that.

Measured E / F on MI355X, the largest over each kernel's cases (pwam_stages.K_STAGE = 2 x that, rounded up, never under 1): MEASURED below.
Every bf16 output sits at 1.000: its row error IS the final bf16 rounding, and the kernel rounds the same fp32 value the floor rounds.  The fp32 side
outputs differ from the floor by summation order: rw 1.41 (C = 32; dominant-word cases 0.64 / 1.05 / 1.10 / 1.09), cov 1.12, Q 1.23, c1 0.76.
u of lavt_pwam_lang_bwd1 is judged against the sum of its absolute terms (pwam_stages.SCALED): u[j] = sum_c VW'[c][j] s[c] / T cancels over the channels,
and against |u[j]| itself -- 1.9e-4 on the worst word at C = 96 where the median is 2.1e-2 -- the kernel stood at 3.2 .. 5.7 x a floor that itself moved by a
factor 6 with the order in which the records were split; against the terms it stands at 1.00 or under.  No ratio is above 3."""
import pytest
import torch

import pwam_stages as S

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
NAN = float("nan")

# largest E / F per output over the cases of this file, as measured on MI355X (the table K_STAGE in pwam_stages.py is derived from)
MEASURED = {"P": 1.000, "PP": 1.000, "sumP": 1.000, "VWc": 1.000, "VWw": 1.000, "beta": 1.000, "rw": 1.408, "pbar": 1.000, "cov": 1.123, "mm": 1.000,
            "dvpre": 1.000, "dwhat": 1.000, "HT": 1.000, "s": 1.000, "dVW": 1.000, "Q": 1.226, "u": 1.000, "dS": 1.000, "dK": 1.000, "K2c": 1.000, "c0": 1.000,
            "c1": 0.762, "dq": 1.000}


def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m 'not gpu' elsewhere)"
    return torch.device("cuda:0")


def _K():
    from lavt_hip import _capi as K
    return K


def to_bf(t, ld=None):
    """[..., n] fp32 holding bf16 values -> device bf16 rows [rows, ld] (columns >= n NaN)"""
    rows = t.reshape(-1, t.shape[-1])
    if ld is None or ld == rows.shape[1]:
        return rows.to(BF).to(dev()).contiguous()
    buf = torch.full((rows.shape[0], ld), NAN, dtype=BF)
    buf[:, :rows.shape[1]] = rows.to(BF)
    return buf.to(dev())


def to_f(t):
    return t.float().contiguous().to(dev())


def out(*shape, dtype=BF):
    return torch.full(shape, NAN, dtype=dtype, device=dev())


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def same(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def judge(kernel, case, got, ref, flo, names):
    """print every figure, then fail on every output that misses pwam_stages.gate"""
    fails = []
    for n in names:
        E, Fl, ok = S.gate(n, got[n].float().cpu().reshape(ref[n].shape), ref[n], flo[n], report=True, scale=S.scale_of(n, ref))
        ratio = E / Fl if Fl > 0 else (0.0 if E == 0 else float("inf"))
        print(f"[pwam-stage] {kernel} {case} {n}: E {E:.3e} F {Fl:.3e} E/F {ratio:.3f} K {S.K_STAGE[n]:g}")
        if not ok:
            fails.append((n, E, Fl, ratio))
    assert not fails, (kernel, case, fails)


def twice(run):
    a = run()
    torch.cuda.synchronize()
    b = run()
    torch.cuda.synchronize()
    assert same(a, b), "second run is not bit-identical"
    return a


# ------------------------------------------------------------------------------------------------ words forward
WORDS_FWD = [
    # (B, T, C, n_l, flags)
    (2, 5, 32, 1, ""),                       # (P is the constant row (1, 0, ...): holds only that T < 16 writes exact 1 / 0)
    (2, 5, 32, 3, ""),                       # T < 16 with rows that differ
    (2, 37, 96, 17, ""),
    (2, 37, 96, 17, "wide"),                 # ldq, ldk wider than C
    (2, 37, 96, 17, "open"),                 # maskbias 0 at the padding words: only the kernel's j < n_l bound keeps them out
    (2, 48, 192, 32, "inside"),              # two masked words inside n_l in sample 0
    (1, 31, 768, 3, ""),                     # 24 k-steps: prefetch 16 + two 4-at-a-time
    (2, 37, 1056, 20, ""),                   # 33 k-steps: prefetch 16 + 16-at-a-time + remainder
    (2, 1100, 96, 20, ""),                   # the 1024-thread form
    (1, 8300, 224, 20, ""),                  # 1024-thread form, later tiles, 7 k-steps
    (1, 2100, 672, 20, ""),                  # 256-thread form with records, later tiles, 21 k-steps
    (64, 1100, 32, 20, "norec"),             # without records: later tiles through the per-batch cap
]


@pytest.mark.parametrize("B,T,C,n_l,flags", WORDS_FWD)
def test_words_fwd(B, T, C, n_l, flags):
    """lavt_pwam_words_fwd, and lavt_pwam_words_fwd_moments with the records checked as totals."""
    K = _K()
    c = S.Case(B, T, C, n_l, masked_inside=flags == "inside", open_padding=flags == "open")
    ldq, ldk = (C + 24, C + 40) if flags == "wide" else (C, C)
    q, k = to_bf(c.i["q"], ldq), to_bf(c.i["K"], ldk)
    mean, rstd, mb = to_f(c.i["mean"]), to_f(c.i["rstd"]), to_f(c.i["maskbias"])
    ref, flo = S.reference(S.words_fwd, *c.words_fwd_args), S.floor(S.words_fwd, *c.words_fwd_args)

    def plain():
        P = out(B * T, 32)
        K.check(K.lib.lavt_pwam_words_fwd(K.ptr(q), ldq, K.ptr(k), ldk, K.ptr(mean), K.ptr(rstd), K.ptr(mb), K.ptr(P), B, T, C, n_l, c.alpha, K.stream()))
        return (P,)
    (P,) = twice(plain)
    judge("words_fwd", c.name + flags, {"P": P}, ref, flo, ["P"])
    if flags == "norec":
        return
    R = int(K.lib.lavt_pwam_words_records(B, T, C))
    assert 1 <= R <= 32

    def moments():
        P = out(B * T, 32)
        rec = out(B, R, 1056, dtype=torch.float32)
        K.check(K.lib.lavt_pwam_words_fwd_moments(K.ptr(q), ldq, K.ptr(k), ldk, K.ptr(mean), K.ptr(rstd), K.ptr(mb), K.ptr(P), K.ptr(rec), B, T, C, n_l, c.alpha, K.stream()))
        return P, rec
    P, rec = twice(moments)
    tot = rec.double().sum(1).cpu()
    judge("words_fwd_moments", c.name + flags, {"P": P, "PP": tot[:, :1024], "sumP": tot[:, 1024:]}, ref, flo, ["P", "PP", "sumP"])


# ------------------------------------------------------------------------------------------------ words backward
def _records(total_a, total_b, n, seed):
    """[B, n, a + b] fp32 records splitting two totals unevenly, their exact totals (the reference's input) and their fp32 totals added in index order
    (the floor's input: the consuming kernel adds the records that way)"""
    ra, rb = S.split_records(total_a, n, seed), S.split_records(total_b, n, seed + 1)
    B = ra.shape[0]
    rec = torch.cat([ra.reshape(B, n, -1), rb.reshape(B, n, -1)], -1)
    return rec, (S.sum_records(ra, torch.float64), S.sum_records(rb, torch.float64)), (S.sum_records(ra, torch.float32), S.sum_records(rb, torch.float32))


@pytest.mark.parametrize("B,T,C,n_l", [(2, 5, 32, 1), (2, 5, 32, 3), (2, 37, 96, 17), (1, 31, 768, 20), (2, 37, 1056, 20),          # (n_l = 1: dS is identically 0)
                                       (64, 1100, 160, 20)])          # later tiles (per-batch cap), fresh P loads, 5 k-steps from ks = 0
def test_words_bwd(B, T, C, n_l):
    """lavt_pwam_words_bwd; Qp given as lavt_pwam_q_parts(C) records that split the stage function's Q and u unevenly."""
    K = _K()
    c = S.Case(B, T, C, n_l)
    nq = int(K.lib.lavt_pwam_q_parts(C))
    rec, exact, added = _records(c.lb1["Q"], c.lb1["u"], nq, 11)
    a = c.words_bwd_args
    ref, flo = S.reference(S.words_bwd, *a[:2], *exact, *a[4:]), S.floor(S.words_bwd, *a[:2], *added, *a[4:])
    dwh, VWw, Qp, pbar, P = to_bf(c.m1["dwhat"]), to_bf(c.lf["VWw"]), to_f(rec), to_f(c.lf["pbar"]), to_bf(c.wf["P"])

    def run():
        dS = out(B * T, 32)
        K.check(K.lib.lavt_pwam_words_bwd(K.ptr(dwh), C, K.ptr(VWw), K.ptr(Qp), K.ptr(pbar), K.ptr(P), K.ptr(dS), B, T, C, K.stream()))
        return (dS,)
    (dS,) = twice(run)
    judge("words_bwd", c.name, {"dS": dS}, ref, flo, ["dS"])


# ------------------------------------------------------------------------------------------------ mix kernels
MIX = [(2, 5, 32), (2, 37, 96), (1, 50, 160), (2, 33, 256), (1, 4200, 96)]          # the last: lavt_pwam_mix1 waves walk several tiles


@pytest.mark.parametrize("B,T,C", MIX)
@pytest.mark.parametrize("bias", [True, False])
def test_mix0(B, T, C, bias):
    K = _K()
    c = S.Case(B, T, C, 20 if T > 5 else 3)
    a = c.mix0_args(bias)
    ref, flo = S.reference(S.mix0, *a), S.floor(S.mix0, *a)
    P, VWc, beta, xb, X = to_bf(a[0]), to_bf(a[1]), to_f(a[2]), to_f(a[3]) if bias else None, to_bf(a[4])

    def run():
        mm = out(B * T, C)
        K.check(K.lib.lavt_pwam_mix(0, K.ptr(P), K.ptr(VWc), K.ptr(beta), None, K.ptr(xb), K.ptr(X), C, None, 0, K.ptr(mm), C, None, 0, B, T, C, K.stream()))
        return (mm,)
    (mm,) = twice(run)
    judge("mix0", f"{c.name} bias={bias}", {"mm": mm}, ref, flo, ["mm"])


@pytest.mark.parametrize("B,T,C", MIX)
@pytest.mark.parametrize("bias", [True, False])
def test_mix1(B, T, C, bias):
    """lavt_pwam_mix mode 1, and lavt_pwam_mix1 without and with records (H^T and s checked as totals); d vpre goes into the left half of [M, 2C]
    (ld0 = 2C, the product's stride), whose right half must stay as it was."""
    K = _K()
    c = S.Case(B, T, C, 20 if T > 5 else 3)
    a = c.mix1_args(bias)
    ref, flo = S.reference(S.mix1, *a), S.floor(S.mix1, *a)
    P, VWc, beta, xb, X, D = to_bf(a[0]), to_bf(a[1]), to_f(a[2]), to_f(a[3]) if bias else None, to_bf(a[4]), to_bf(a[5])
    R = int(K.lib.lavt_pwam_mix1_records(B, T, C))
    assert 1 <= R <= 32
    M = B * T
    fill = torch.arange(M * C, dtype=torch.float32).reshape(M, C).remainder(251.0).to(BF).to(dev())

    def run(kind):
        g = out(M, 2 * C)
        g[:, C:] = fill
        dwh = out(M, C)
        rec = out(B, R, C * 33, dtype=torch.float32) if kind == "rec" else None
        if kind == "mix":
            K.check(K.lib.lavt_pwam_mix(1, K.ptr(P), K.ptr(VWc), K.ptr(beta), None, K.ptr(xb), K.ptr(X), C, K.ptr(D), C, K.ptr(g), 2 * C, K.ptr(dwh), C, B, T, C, K.stream()))
        else:
            K.check(K.lib.lavt_pwam_mix1(K.ptr(P), K.ptr(VWc), K.ptr(beta), K.ptr(xb), K.ptr(X), C, K.ptr(D), C, K.ptr(g), 2 * C, K.ptr(dwh), C, K.ptr(rec), B, T, C, K.stream()))
        return (g, dwh) + ((rec,) if rec is not None else ())
    for kind in ("mix", "norec", "rec"):
        o = twice(lambda: run(kind))
        assert torch.equal(o[0][:, C:], fill), "the right half of [M, 2C] is not the kernel's to write"
        got, names = {"dvpre": o[0][:, :C], "dwhat": o[1]}, ["dvpre", "dwhat"]
        if kind == "rec":
            tot = o[2].double().sum(1).cpu()
            got.update(HT=tot[:, :C * 32], s=tot[:, C * 32:])
            names += ["HT", "s"]
        judge({"mix": "mix(1)", "norec": "mix1", "rec": "mix1+rec"}[kind], f"{c.name} bias={bias}", got, ref, flo, names)


@pytest.mark.parametrize("B,T,C", MIX)
def test_mix2(B, T, C):
    """lavt_pwam_mix mode 2 writing dq at column offset C of [M, 2C], as the product does; the left half must stay as it was."""
    K = _K()
    c = S.Case(B, T, C, 20 if T > 5 else 3)
    a = c.mix2_args
    ref, flo = S.reference(S.mix2, *a), S.floor(S.mix2, *a)
    dS, K2c, c0, c1, q = to_bf(a[0]), to_bf(a[1]), to_f(a[2]), to_f(a[3]), to_bf(a[4])
    M = B * T
    fill = torch.arange(M * C, dtype=torch.float32).reshape(M, C).remainder(251.0).to(BF).to(dev())

    def run():
        g = out(M, 2 * C)
        g[:, :C] = fill
        K.check(K.lib.lavt_pwam_mix(2, K.ptr(dS), K.ptr(K2c), K.ptr(c0), K.ptr(c1), None, K.ptr(q), C, None, 0, g.data_ptr() + 2 * C, 2 * C, None, 0, B, T, C, K.stream()))
        return (g,)
    (g,) = twice(run)
    assert torch.equal(g[:, :C], fill), "the left half of [M, 2C] is not the kernel's to write"
    judge("mix2", c.name, {"dq": g[:, C:]}, ref, flo, ["dq"])


# ------------------------------------------------------------------------------------------------ language side
LANG_OUT = ["VWc", "VWw", "beta", "rw", "pbar", "cov"]


def _lang_fwd(K, V, ldv, Wo, PP, sumP, rec, nrec, B, T, C):
    o = dict(VWc=out(B, C, 32), VWw=out(B, 32, C), beta=out(B, C, dtype=torch.float32), rw=out(B, C, dtype=torch.float32),
             pbar=out(B, 32, dtype=torch.float32), cov=out(B, 32, 32, dtype=torch.float32))
    K.check(K.lib.lavt_pwam_lang_fwd_records(K.ptr(V), ldv, K.ptr(Wo), K.ptr(PP), K.ptr(sumP), K.ptr(rec), nrec, K.ptr(o["VWc"]), K.ptr(o["VWw"]), K.ptr(o["beta"]),
                                             K.ptr(o["rw"]), K.ptr(o["pbar"]), K.ptr(o["cov"]), B, T, C, S.EPS, K.stream()))
    return o


@pytest.mark.parametrize("C", [32, 96, 672, 1536, 2048])          # above 1024: the tail loop of the reduction
def test_lang_fwd(C):
    """lavt_pwam_lang_fwd on (P^T P, colsum P) and lavt_pwam_lang_fwd_records on synthetic records at 1 / 15 / 16 / 17 / 32 records; ldv wider than C."""
    K = _K()
    B, T = 2, 37
    c = S.Case(B, T, C, 20, masked_inside=True)
    ldv = C + 24
    V, Wo = to_bf(c.i["V"], ldv), to_bf(c.i["Wo"])
    for nrec in (0, 1, 15, 16, 17, 32):
        if nrec == 0:
            exact = added = (c.wf["PP"], c.wf["sumP"])
            rec, dPP, dsum = None, to_f(exact[0]), to_f(exact[1])
        else:
            rec, exact, added = _records(c.wf["PP"], c.wf["sumP"], nrec, 20 + nrec)
            rec, dPP, dsum = to_f(rec), None, None
        ref, flo = S.reference(S.lang_fwd, c.i["V"], c.i["Wo"], *exact, T), S.floor(S.lang_fwd, c.i["V"], c.i["Wo"], *added, T)
        keys = LANG_OUT

        def run():
            o = _lang_fwd(K, V, ldv, Wo, dPP, dsum, rec, nrec, B, T, C)
            return tuple(o[k] for k in keys)
        o = dict(zip(keys, twice(run)))
        assert torch.equal(o["VWc"].transpose(1, 2).contiguous(), o["VWw"]), "both layouts of VW' hold the same values"
        # beta against ITS OWN outputs.  The gate above cannot hold beta tightly: beta = -Pbar VW' cancels to near zero in some channel, where the bf16
        # rounding of VW' (which the fp64 reference does not make) is the whole value -- floor errors of 0.2 .. 1.5.  What the mix kernels need is
        # beta = -sum_j Pbar_j VW'_j of the STORED VW' (so that what = (P - Pbar) VW' has zero mean): an fp32 dot product of 32 terms, so
        # |beta + sum_j Pbar_j VW'_j| <= 32 * 2^-24 * sum_j |Pbar_j VW'_j| (n * u * sum |terms|, the standard bound for any summation order).
        terms = o["pbar"].double().cpu()[:, None, :] * o["VWc"].double().cpu()
        resid = (o["beta"].double().cpu() + terms.sum(-1)).abs()
        assert bool((resid <= 32 * 2.0 ** -24 * terms.abs().sum(-1)).all()), ("beta is not -Pbar VW' of the stored VW'", float(resid.max()))
        judge("lang_fwd", f"{c.name} nrec={nrec}", o, ref, flo, keys)


@pytest.mark.parametrize("lead", [0, 6, 9, 12])
def test_lang_fwd_dominant_word(lead):
    """The collapsed covariance Cov = P^T P / T - Pbar Pbar^T in fp32 loses rw = rsqrt(var_w + eps) when one word dominates every pixel of a sample
    (DESIGN.md lists the figures).  This judges the IMPLEMENTATION, not the formula: the kernel's per-channel error of rw against fp64 may not exceed
    K_STAGE['rw'] x that of the fp32 CPU evaluation of the same formula.  T = 14400, C = 128, n_l = 20, word 0's logit raised by `lead`, VW' scale 8."""
    K = _K()
    B, T, C, n_l = 1, 14400, 128, 20
    logit = S.randn(B, T, n_l, seed=31)
    logit[..., 0] += lead
    P = torch.zeros(B, T, 32)
    P[..., :n_l] = torch.softmax(logit, -1)
    P = S.bf(P).double()
    PP, sumP = torch.einsum("btj,btk->bjk", P, P).float(), P.sum(1).float()
    V = torch.zeros(B, 32, C)
    V[:, :n_l] = 8.0 * S.randn(B, n_l, C, seed=32)
    V, Wo = S.bf(V), S.bf(S.randn(C, C, seed=33) * C ** -0.5)
    a = (V, Wo, PP, sumP, T)
    ref, flo = S.reference(S.lang_fwd, *a), S.floor(S.lang_fwd, *a)
    dV, dWo, dPP, dsum = to_bf(V), to_bf(Wo), to_f(PP), to_f(sumP)
    o = _lang_fwd(K, dV, C, dWo, dPP, dsum, None, 0, B, T, C)
    torch.cuda.synchronize()
    E, Fl = S.row_error(o["rw"].cpu(), ref["rw"]), S.row_error(flo["rw"], ref["rw"])
    print(f"[pwam-dominant] lead {lead}: P0 mean {float(P[..., 0].mean()):.4f}  rw error kernel {E:.3e}  fp32 formula (floor) {Fl:.3e}  E/F {E / Fl:.3f}  "
          f"fp64 var_w {float(ref['var'].min()):.3e} .. {float(ref['var'].max()):.3e}")
    assert E <= S.K_STAGE["rw"] * Fl, (lead, E, Fl)


@pytest.mark.parametrize("C", [32, 96, 672, 1536])
def test_lang_bwd1(C):
    """lavt_pwam_lang_bwd1 on (H^T, s) and lavt_pwam_lang_bwd1_records on synthetic records at 1 / 15 / 16 / 17 / 32 records; Q and u are compared as the
    sum over the lavt_pwam_q_parts(C) records the kernel leaves."""
    K = _K()
    B, T = 2, 37
    c = S.Case(B, T, C, 20, masked_inside=True)
    nq = int(K.lib.lavt_pwam_q_parts(C))
    VWc, rw, pbar, cov = to_bf(c.lf["VWc"]), to_f(c.lf["rw"]), to_f(c.lf["pbar"]), to_f(c.lf["cov"])
    for nrec in (0, 1, 15, 16, 17, 32):
        if nrec == 0:
            exact = added = (c.m1["HT"], c.m1["s"])
            rec, dHT, ds = None, to_f(exact[0]), to_f(exact[1])
        else:
            rec, exact, added = _records(c.m1["HT"], c.m1["s"], nrec, 40 + nrec)
            rec, dHT, ds = to_f(rec), None, None
        ref, flo = S.reference(S.lang_bwd1, *exact, *c.lang_bwd1_args[2:]), S.floor(S.lang_bwd1, *added, *c.lang_bwd1_args[2:])

        def run():
            dVW, Qp = out(B * 32, C), out(B, nq, 1056, dtype=torch.float32)
            K.check(K.lib.lavt_pwam_lang_bwd1_records(K.ptr(dHT), K.ptr(ds), K.ptr(rec), nrec, K.ptr(VWc), K.ptr(rw), K.ptr(pbar), K.ptr(cov), K.ptr(dVW), K.ptr(Qp),
                                                      B, T, C, K.stream()))
            return dVW, Qp
        dVW, Qp = twice(run)
        tot = Qp.double().sum(1).cpu()
        judge("lang_bwd1", f"{c.name} nrec={nrec}", {"dVW": dVW, "Q": tot[:, :1024], "u": tot[:, 1024:]}, ref, flo, ["dVW", "Q", "u"])


@pytest.mark.parametrize("C", [32, 96, 288])
def test_lang_bwd2(C):
    """lavt_pwam_lang_bwd2 with ldk and lddk wider than C; the dK rows of padded and masked words are exactly zero."""
    K = _K()
    B, T = 2, 37
    c = S.Case(B, T, C, 20, masked_inside=True)
    a = c.lang_bwd2_args
    ref, flo = S.reference(S.lang_bwd2, *a), S.floor(S.lang_bwd2, *a)
    ldk, lddk = C + 24, C + 40
    G, sdS, Kd, mean, rstd = to_f(a[0]), to_f(a[1]), to_bf(a[2], ldk), to_f(a[3]), to_f(a[4])

    def run():
        dK, K2c, c0, c1 = out(B * 32, lddk), out(B, C, 32), out(B, C, dtype=torch.float32), out(B, C, dtype=torch.float32)
        K.check(K.lib.lavt_pwam_lang_bwd2(K.ptr(G), K.ptr(sdS), K.ptr(Kd), ldk, K.ptr(mean), K.ptr(rstd), K.ptr(dK), lddk, K.ptr(K2c), K.ptr(c0), K.ptr(c1),
                                          B, T, C, c.alpha, K.stream()))
        return dK, K2c, c0, c1
    dK, K2c, c0, c1 = twice(run)
    assert bool(torch.isnan(dK[:, C:]).all()), "columns beyond C of the dK rows are not the kernel's to write"
    dK = dK[:, :C].reshape(B, 32, C)
    dead = (c.i["maskbias"] < -1.0).to(dev())
    assert int(dead.sum()) == 2 * 12 + 2 and float(dK[dead].abs().max()) == 0.0, "dK of padded and masked words must be exactly zero"
    judge("lang_bwd2", c.name, {"dK": dK, "K2c": K2c, "c0": c0, "c1": c1}, ref, flo, ["dK", "K2c", "c0", "c1"])
