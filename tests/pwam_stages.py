"""One fp64 statement per kernel of the fused PWAM path (csrc/pwam.hip; contracts: the comment block above lavt_pwam_words_fwd in include/lavt_hip.h).
CPU only, pure torch, nothing imported from the product or from oracle/.

Every stage function takes exactly the tensors its kernel receives (records as their totals) and returns, as a dict, exactly what the kernel must
write.  Two switches: `dtype` (float64 / float32: the precision of every intermediate) and `round_bf16` (rounds what the kernel's contract says is
bf16: every stored bf16 output and the operands the kernel documents as bf16 for the matrix cores -- K'' in the words forward, -Q in the words
backward, VW').  dtype=float64, round_bf16=False is the REFERENCE; dtype=float32, round_bf16=True is the FLOOR: the same arithmetic at the kernel's
precision, evaluated by torch.  `plain` is the unfused formulation with autograd (what the reference model computes); test_pwam_stages_host.py chains
the stage functions against it, so the references are themselves checked.

Metric (`row_error`): the MAXIMUM OVER ROWS of ||got[r] - ref[r]||_2 / max(||ref[r]||_2, a), a = 1e-3 x the median norm of the reference's non-zero
rows (for u of lavt_pwam_lang_bwd1, a sum that cancels, ||ref[r]|| is replaced by the sum of the absolute terms).  Rows are pixels for [B, T, n] tensors, channels for [B, C] and [B, C, 32], word rows for [B, 32, n] and single words for [B, 32]: a fault
confined to one tail tile, one lane quad, one channel span or one word moves it; a global norm hides such a fault.  A row that must be exactly zero
(masked and padding words) and is not gives an error of the order 1 / 1e-3.

Gate (`gate`): E(got, ref) <= K_STAGE[output] * F with F = E(floor, ref) of the same case."""
import math

import torch
import torch.nn.functional as F

J = 32                      # word slots
EPS = 1e-5
LOG2E = 1.4426950408889634
BF = torch.bfloat16

# Gate factors, one per kernel output: twice the largest E / F measured on MI355X over that kernel's cases of test_gpu_pwam_stages.py (the measured
# ratios are listed in that file's docstrings), and never under 1.
K_STAGE = {
    # lavt_pwam_words_fwd(_moments)
    "P": 2.0, "PP": 2.0, "sumP": 2.0,
    # lavt_pwam_lang_fwd(_records)
    "VWc": 2.0, "VWw": 2.0, "beta": 2.0, "rw": 2.82, "pbar": 2.0, "cov": 2.25,
    # lavt_pwam_mix mode 0
    "mm": 2.0,
    # lavt_pwam_mix mode 1 / lavt_pwam_mix1
    "dvpre": 2.0, "dwhat": 2.0, "HT": 2.0, "s": 2.0,
    # lavt_pwam_lang_bwd1(_records)
    "dVW": 2.0, "Q": 2.46, "u": 2.0,
    # lavt_pwam_words_bwd
    "dS": 2.0,
    # lavt_pwam_lang_bwd2
    "dK": 2.0, "K2c": 2.0, "c0": 2.0, "c1": 1.53,
    # lavt_pwam_mix mode 2
    "dq": 2.0,
}


SCALED = {"u": "u_scale"}          # outputs whose rows are judged against a scale from the reference instead of their own norm


def scale_of(name, ref):
    return ref[SCALED[name]] if name in SCALED else None


def bf(x):
    """the value a bf16 store leaves, in x's dtype"""
    return x.to(torch.float32).to(BF).to(x.dtype)


def _r(x, on):
    return bf(x) if on else x


def _gelu(z):
    return 0.5 * z * (1.0 + torch.erf(z * 0.7071067811865476))


def _gelu_grad(z):
    return 0.5 * (1.0 + torch.erf(z * 0.7071067811865476)) + z * torch.exp(-0.5 * z * z) * 0.3989422804014327


# ------------------------------------------------------------------------------------------------ stage functions
def words_fwd(q, K, mean, rstd, maskbias, n_l, alpha, dtype=torch.float64, round_bf16=False):
    """lavt_pwam_words_fwd(_moments): q [B, T, C] raw, K [B, 32, C], mean / rstd [B, C] of q over T, maskbias [B, 32].
    P = softmax_{j < n_l}(q K''^T + s0), K'' = alpha rstd K (bf16 for the matrix cores, with the log2 e of the exp2 folded in), s0 = maskbias - mu K''^T;
    word slots >= n_l get exactly 0.  PP = P^T P [B, 32, 32] and sumP = colsum(P) [B, 32] of the P that was stored."""
    q, K, mean, rstd, mb = (t.to(dtype) for t in (q, K, mean, rstd, maskbias))
    K2 = _r(K * (rstd[:, None, :] * (alpha * LOG2E)), round_bf16)
    s0 = mb * LOG2E - torch.einsum("bc,bjc->bj", mean, K2)
    S = torch.einsum("btc,bjc->btj", q, K2) + s0[:, None, :]
    S = S[..., :n_l]
    e = torch.exp2(S - S.max(-1, keepdim=True).values)
    P = torch.zeros(q.shape[0], q.shape[1], J, dtype=dtype)
    P[..., :n_l] = e / e.sum(-1, keepdim=True)
    P = _r(P, round_bf16)
    return {"P": P, "PP": torch.einsum("btj,btk->bjk", P, P), "sumP": P.sum(1)}


def lang_fwd(V, Wo, PP, sumP, T, eps=EPS, dtype=torch.float64, round_bf16=False):
    """lavt_pwam_lang_fwd(_records): V [B, 32, C], Wo [C, C], PP [B, 32, 32], sumP [B, 32] (the records form: their totals).
    Pbar = sumP * (1 / T), Cov = PP * (1 / T) - Pbar Pbar^T (the kernel multiplies by the rounded reciprocal: where Cov cancels -- one word dominating
    every pixel -- that costs about 5 x the error of a true division, and the floor has to pay it too), VW = V Wo^T, var_w[c] = VW[:, c]^T Cov VW[:, c], rw = rsqrt(max(var_w, 0) + eps), VW' = bf16(VW rw) in
    both layouts, beta = -Pbar VW'.  ("var" is var_w, which the kernel does not store: the dominant-word test prints its range.)"""
    V, Wo, PP, sumP = (t.to(dtype) for t in (V, Wo, PP, sumP))
    invT = (torch.ones((), dtype=dtype) / torch.tensor(float(T), dtype=dtype))
    pbar = sumP * invT
    cov = PP * invT - pbar[:, :, None] * pbar[:, None, :]
    VW = V @ Wo.T
    var = torch.einsum("bjc,bjk,bkc->bc", VW, cov, VW)
    rw = torch.rsqrt(var.clamp(min=0.0) + eps)
    VWs = _r(VW * rw[:, None, :], round_bf16)
    beta = -torch.einsum("bj,bjc->bc", pbar, VWs)
    return {"VWc": VWs.transpose(1, 2).contiguous(), "VWw": VWs, "beta": beta, "rw": rw, "pbar": pbar, "cov": cov, "var": var}


def _what(P, VWc, beta):
    return torch.einsum("btj,bcj->btc", P, VWc) + beta[:, None, :]


def mix0(P, VWc, beta, xbias, X, dtype=torch.float64, round_bf16=False):
    """lavt_pwam_mix mode 0: mm = GELU(X + xbias) * (P VWc^T + beta)"""
    P, VWc, beta, X = (t.to(dtype) for t in (P, VWc, beta, X))
    if xbias is not None:
        X = X + xbias.to(dtype)
    return {"mm": _r(_gelu(X) * _what(P, VWc, beta), round_bf16)}


def mix1(P, VWc, beta, xbias, X, D, dtype=torch.float64, round_bf16=False):
    """lavt_pwam_mix mode 1 / lavt_pwam_mix1: d vpre = D * what * GELU'(X + xbias), d what = D * GELU(X + xbias); with records also
    HT = dwhat^T P [B, C, 32] and s = colsum(dwhat) [B, C] of the d what that was stored."""
    P, VWc, beta, X, D = (t.to(dtype) for t in (P, VWc, beta, X, D))
    if xbias is not None:
        X = X + xbias.to(dtype)
    dvpre = _r(D * _what(P, VWc, beta) * _gelu_grad(X), round_bf16)
    dwhat = _r(D * _gelu(X), round_bf16)
    return {"dvpre": dvpre, "dwhat": dwhat, "HT": torch.einsum("btc,btj->bcj", dwhat, P), "s": dwhat.sum(1)}


def lang_bwd1(HT, s, VWc, rw, pbar, cov, T, dtype=torch.float64, round_bf16=False):
    """lavt_pwam_lang_bwd1(_records): HT [B, C, 32], s [B, C] (records form: totals), VWc [B, C, 32], rw [B, C], pbar [B, 32], cov [B, 32, 32].
    a = s / T, b[c] = VW'[:, c] . (H[:, c] - Pbar s[c]) / T, dVW = rw (H - T Pbar a - T b Cov VW') [B, 32, C] (bf16),
    Q = VW' diag(b) VW'^T [B, 32, 32], u = VW' a [B, 32] (the kernel leaves Q, u as records: compared as their sum).
    "u_scale" = sum_c |VW'[c][j] a[c]| is not an output: u[j] cancels over the channels, so its error is judged against the size of its terms
    (SCALED below) -- against |u[j]| itself a correct fp32 evaluation moves by a factor 6 with the order of the additions."""
    HT, s, VWc, rw, pbar, cov = (t.to(dtype) for t in (HT, s, VWc, rw, pbar, cov))
    a = s / T
    b = (VWc * (HT - pbar[:, None, :] * s[:, :, None])).sum(-1) / T                          # [B, C]
    t = torch.einsum("bjk,bck->bcj", cov, VWc)
    dVW = rw[:, :, None] * (HT - T * pbar[:, None, :] * a[:, :, None] - T * b[:, :, None] * t)
    return {"dVW": _r(dVW.transpose(1, 2).contiguous(), round_bf16), "Q": torch.einsum("bck,bc,bcj->bkj", VWc, b, VWc), "u": torch.einsum("bcj,bc->bj", VWc, a),
            "u_scale": torch.einsum("bcj,bc->bj", VWc.abs(), a.abs())}


def words_bwd_dP(dwhat, VWw, Q, u, pbar, P, dtype=torch.float64, round_bf16=False):
    """(dP, P) of the words backward in `dtype`: dP = dwhat VW'^T - P Q + (Pbar Q - u), Q as the bf16 -Q of the matrix cores when round_bf16"""
    dwhat, VWw, Q, u, pbar, P = (t.to(dtype) for t in (dwhat, VWw, Q, u, pbar, P))
    Qn = _r(-Q, round_bf16)
    vec = -torch.einsum("bi,bij->bj", pbar, Qn) - u
    return torch.einsum("btc,bjc->btj", dwhat, VWw) + torch.einsum("btk,bjk->btj", P, Qn) + vec[:, None, :], P


def words_bwd(dwhat, VWw, Q, u, pbar, P, dtype=torch.float64, round_bf16=False):
    """lavt_pwam_words_bwd: dwhat [B, T, C], VWw [B, 32, C], Q [B, 32, 32] / u [B, 32] (totals of the Qp records), pbar [B, 32], P [B, T, 32].
    dS = P (dP - sum_j P_j dP_j)"""
    dP, P = words_bwd_dP(dwhat, VWw, Q, u, pbar, P, dtype, round_bf16)
    return {"dS": _r(P * (dP - (P * dP).sum(-1, keepdim=True)), round_bf16)}


def lang_bwd2(G, sdS, K, mean, rstd, T, alpha, dtype=torch.float64, round_bf16=False):
    """lavt_pwam_lang_bwd2: G = dS^T q [B, 32, C] (raw q), sdS [B, 32], K [B, 32, C], mean / rstd [B, C].
    Ghat = (G - sdS mu) rstd, dK = alpha Ghat (bf16), K''^T [B, C, 32] = alpha rstd K (bf16), c1 = rstd^2 alpha sum_j K Ghat / T,
    c0 = -rstd alpha sum_j sdS K / T + mu c1"""
    G, sdS, K, mean, rstd = (t.to(dtype) for t in (G, sdS, K, mean, rstd))
    gh = (G - sdS[:, :, None] * mean[:, None, :]) * rstd[:, None, :]
    a2 = alpha * torch.einsum("bj,bjc->bc", sdS, K) / T
    b2 = alpha * (K * gh).sum(1) / T
    c1 = rstd * rstd * b2
    c0 = -rstd * a2 + mean * c1
    K2c = (alpha * rstd[:, None, :] * K).transpose(1, 2).contiguous()
    return {"dK": _r(alpha * gh, round_bf16), "K2c": _r(K2c, round_bf16), "c0": c0, "c1": c1}


def mix2(dS, K2c, c0, c1, q, dtype=torch.float64, round_bf16=False):
    """lavt_pwam_mix mode 2: dq = dS K''  + c0 - q c1"""
    dS, K2c, c0, c1, q = (t.to(dtype) for t in (dS, K2c, c0, c1, q))
    return {"dq": _r(torch.einsum("btj,bcj->btc", dS, K2c) + c0[:, None, :] - q * c1[:, None, :], round_bf16)}


def reference(fn, *a, **k):
    return fn(*a, dtype=torch.float64, round_bf16=False, **k)


def floor(fn, *a, **k):
    return fn(*a, dtype=torch.float32, round_bf16=True, **k)


# ------------------------------------------------------------------------------------------------ the unfused formulation
def _inorm(z):
    mu = z.mean(1, keepdim=True)
    return (z - mu) / torch.sqrt(z.var(1, unbiased=False, keepdim=True) + EPS)


def plain(x, Kl, Vl, maskbias, n_l, Wv, bv, Wq, bq, Wo, bo, Wm, bm, W1, W2):
    """PWAM + language gate as the reference model computes them (lib/backbone.py:1265-1278, 1329-1372, 604-611, 669), differentiable:
    x [B, T, C], Kl / Vl [B, 32, C], maskbias [B, 32] -> (r, xg)"""
    C = x.shape[-1]
    vis = F.gelu(x @ Wv.T + bv)
    q = _inorm(x @ Wq.T + bq)
    S = C ** -0.5 * q @ Kl.transpose(1, 2) + maskbias[:, None, :]
    P = torch.softmax(S[..., :n_l], -1)
    lang = _inorm((P @ Vl[:, :n_l]) @ Wo.T + bo)
    r = F.gelu((vis * lang) @ Wm.T + bm)
    return r, x + torch.tanh(F.relu(r @ W1.T) @ W2.T) * r


# ------------------------------------------------------------------------------------------------ metric and gate
def _rows(t):
    t = t.detach().cpu().to(torch.float64)
    return t.reshape(-1, 1) if t.dim() <= 2 else t.reshape(-1, t.shape[-1])


def row_error(got, ref, scale=None):
    """max over rows of ||got[r] - ref[r]|| / max(d[r], a), d = ||ref[r]|| (or `scale`, one figure per row), a = 1e-3 x the median of the non-zero d.
    NaN / inf in got -> inf."""
    g, r = _rows(got), _rows(ref)
    assert g.shape == r.shape, (g.shape, r.shape)
    if not bool(torch.isfinite(g).all()):
        return math.inf
    rn = r.norm(dim=1) if scale is None else scale.detach().cpu().to(torch.float64).reshape(-1)
    assert rn.shape[0] == r.shape[0]
    nz = rn[rn > 0]
    a = 1e-3 * float(nz.median()) if nz.numel() else 1e-30
    return float(((g - r).norm(dim=1) / rn.clamp(min=a)).max())


def gate(name, got, ref, flo, case="", report=False, scale=None):
    """E(got, ref) <= K_STAGE[name] * E(floor, ref): the one statement of the gate.  Raises AssertionError on a miss and returns (E, F); with report it
    raises nothing and returns (E, F, ok), for a caller that prints every figure of a kernel before it fails.  A floor of exactly 0 (an output the
    kernel's precision reproduces exactly) admits E = 0 only."""
    E, Fl = row_error(got, ref, scale), row_error(flo, ref, scale)
    ok = E <= K_STAGE[name] * Fl
    if report:
        return E, Fl, ok
    assert ok, f"{case} {name}: row error {E:.3e} > {K_STAGE[name]:g} x floor {Fl:.3e} (E / F = {E / Fl if Fl > 0 else math.inf:.2f})"
    return E, Fl


def rejects(name, got, ref, flo, scale=None):
    """the mutation self-test's condition: the gate fails with a factor 2 to spare.  Strict: the mutated tensor differs from the floor and its error is
    above zero -- where reference and floor are identically zero (n_l = 1: what, dS, c1 vanish) a defect that changes nothing cannot count as caught."""
    E = row_error(got, ref, scale)
    differs = got.shape != flo.shape or not torch.equal(got.to(torch.float64), flo.to(torch.float64))
    return differs and E > 0.0 and E >= 2.0 * K_STAGE[name] * row_error(flo, ref, scale)


def k_from_measured(ratio):
    """the rule K_STAGE follows: twice the largest measured E / F, rounded up to two decimals, never under 1"""
    return max(1.0, math.ceil(2.0 * ratio * 100.0 - 1e-9) / 100.0)


# ------------------------------------------------------------------------------------------------ synthetic inputs (shared by the host and GPU tests)
def _gen(seed):
    return torch.Generator("cpu").manual_seed(seed)


def randn(*shape, seed):
    return torch.randn(*shape, generator=_gen(seed))


def make_inputs(B, T, C, n_l, masked_inside=False, open_padding=False, seed=0):
    """The tensors the first kernel receives, bf16 ones already rounded (fp32 tensors holding bf16 values): q = 1.5 randn + 0.3; K / V rows >= n_l and
    masked rows zero, as the projections leave them; Wo = randn C^-0.5; maskbias -1e4 at padding words (0 with open_padding: the kernel's own
    j < n_l bound is then the only thing that keeps them out) and, with masked_inside, at two further words < n_l of sample 0."""
    mb = torch.zeros(B, J)
    if not open_padding:
        mb[:, n_l:] = -1e4
    if masked_inside:
        assert n_l >= 4
        mb[0, 1] = mb[0, n_l - 2] = -1e4
    live = torch.zeros(B, J, 1)
    live[:, :n_l] = 1.0
    live = live * (mb[:, :, None] > -1.0)
    q = bf(randn(B, T, C, seed=seed + 1) * 1.5 + 0.3)
    Kl = bf(randn(B, J, C, seed=seed + 2) * live)
    Vl = bf(randn(B, J, C, seed=seed + 3) * live)
    Wo = bf(randn(C, C, seed=seed + 4) * C ** -0.5)
    qd = q.double()
    mean = qd.mean(1).float()
    rstd = torch.rsqrt(qd.var(1, unbiased=False) + EPS).float()
    return dict(q=q, K=Kl, V=Vl, Wo=Wo, maskbias=mb, mean=mean, rstd=rstd, alpha=float(C ** -0.5), n_l=n_l, B=B, T=T, C=C)


def split_records(total, nrec, seed):
    """fp32 records [B, nrec, ...] that split `total` [B, ...] unevenly (shares between 1 / 2 and 2 x the even one); the caller takes their fp64 sum as
    the total both sides start from"""
    w = 1.0 + torch.rand(total.shape[0], nrec, generator=_gen(seed), dtype=torch.float64)
    w = w / w.sum(1, keepdim=True)
    return (total.double()[:, None] * w.reshape(w.shape + (1,) * (total.dim() - 1))).float()


def sum_records(rec, dtype):
    """total of records [B, n, ...]: exact (fp64) for the reference; for the floor in fp32 and in index order, as the consuming kernels add them"""
    if dtype == torch.float64:
        return rec.double().sum(1)
    tot = torch.zeros_like(rec[:, 0], dtype=torch.float32)
    for r in range(rec.shape[1]):
        tot = tot + rec[:, r].float()
    return tot


def unswap_quads(t):
    """mutation 9: in every 32-wide span of the last axis the 4-element quads land where store_pair16 would put them without its lane exchange"""
    s = t.shape
    v = t.reshape(s[:-1] + (s[-1] // 32, 8, 4))
    return v[..., [0, 4, 2, 6, 1, 5, 3, 7], :].reshape(s)


def tail_rows_from_last(t, T):
    """mutation 1: the rows of the last partial 16-row tile take row T - 1's values ([B, T, n])"""
    t = t.clone()
    t[:, 16 * ((T - 1) // 16):] = t[:, T - 1:T]
    return t


class Case:
    """The inputs of every kernel at one shape, each made from the stage functions before it (fp64 with the bf16 roundings of the contract, fp32 side
    inputs stored as fp32), so that a kernel's test depends on no other kernel and the side inputs are mutually consistent.  Lazy: a test pays for
    the stages in front of its own only."""

    def __init__(self, B, T, C, n_l, masked_inside=False, open_padding=False, seed=0):
        self.B, self.T, self.C, self.n_l, self.seed = B, T, C, n_l, seed
        self.name = f"(B={B}, T={T}, C={C}, n_l={n_l}{', masked inside' if masked_inside else ''}{', open padding' if open_padding else ''})"
        self.i = make_inputs(B, T, C, n_l, masked_inside, open_padding, seed)
        self.alpha = self.i["alpha"]
        self._c = {}

    def _lazy(self, key, fn):
        if key not in self._c:
            self._c[key] = fn()
        return self._c[key]

    @staticmethod
    def _f32(d):
        return {k: v.float() for k, v in d.items()}

    @property
    def words_fwd_args(self):
        i = self.i
        return (i["q"], i["K"], i["mean"], i["rstd"], i["maskbias"], self.n_l, self.alpha)

    @property
    def wf(self):          # P (bf16 values), PP, sumP of that P
        return self._lazy("wf", lambda: self._f32(words_fwd(*self.words_fwd_args, round_bf16=True)))

    @property
    def lang_fwd_args(self):
        return (self.i["V"], self.i["Wo"], self.wf["PP"], self.wf["sumP"], self.T)

    @property
    def lf(self):
        return self._lazy("lf", lambda: self._f32(lang_fwd(*self.lang_fwd_args, round_bf16=True)))

    @property
    def vpre(self):
        return self._lazy("vpre", lambda: bf(randn(self.B, self.T, self.C, seed=self.seed + 5)))

    @property
    def xbias(self):
        return self._lazy("xbias", lambda: 0.2 * randn(self.C, seed=self.seed + 6))

    @property
    def dmm(self):
        return self._lazy("dmm", lambda: bf(1e-2 * randn(self.B, self.T, self.C, seed=self.seed + 7)))

    def mix0_args(self, with_bias=True):
        return (self.wf["P"], self.lf["VWc"], self.lf["beta"], self.xbias if with_bias else None, self.vpre)

    def mix1_args(self, with_bias=True):
        return self.mix0_args(with_bias) + (self.dmm,)

    @property
    def m1(self):
        return self._lazy("m1", lambda: self._f32(mix1(*self.mix1_args(), round_bf16=True)))

    @property
    def lang_bwd1_args(self):
        return (self.m1["HT"], self.m1["s"], self.lf["VWc"], self.lf["rw"], self.lf["pbar"], self.lf["cov"], self.T)

    @property
    def lb1(self):
        return self._lazy("lb1", lambda: self._f32(lang_bwd1(*self.lang_bwd1_args, round_bf16=True)))

    @property
    def words_bwd_args(self):
        return (self.m1["dwhat"], self.lf["VWw"], self.lb1["Q"], self.lb1["u"], self.lf["pbar"], self.wf["P"])

    @property
    def wb(self):
        return self._lazy("wb", lambda: self._f32(words_bwd(*self.words_bwd_args, round_bf16=True)))

    @property
    def lang_bwd2_args(self):
        def gs():
            dS, q = self.wb["dS"].double(), self.i["q"].double()
            return torch.einsum("btj,btc->bjc", dS, q).float(), dS.sum(1).float()
        G, sdS = self._lazy("G", gs)
        return (G, sdS, self.i["K"], self.i["mean"], self.i["rstd"], self.T, self.alpha)

    @property
    def lb2(self):
        return self._lazy("lb2", lambda: self._f32(lang_bwd2(*self.lang_bwd2_args, round_bf16=True)))

    @property
    def mix2_args(self):
        return (self.wb["dS"], self.lb2["K2c"], self.lb2["c0"], self.lb2["c1"], self.i["q"])
