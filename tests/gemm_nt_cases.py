"""The contract of lavt_gemm_nt (include/lavt_hip.h, the comment block above lavt_gemm_nt_t) stated once in fp64, the case table of its per-kernel
parity tests, and a plain-Python restatement of its dispatch.  CPU only, pure torch, nothing imported from the product or from oracle/.

`nt_reference(case)` returns, as a dict, exactly the buffers the kernel owns -- C, C2, Cpre, ln_mean, ln_rstd, those the case has -- with NaN in
every row no m maps to (rows a c_rowmap entry of -1 dropped: the kernel leaves them as they were).  Two switches: `dtype` (float64 / float32: the
precision of every intermediate) and `round_bf16` (rounds what the kernel stores as bf16).  dtype=float64, round_bf16=False is the REFERENCE;
dtype=float32, round_bf16=True is the FLOOR: the same arithmetic at the kernel's precision, evaluated by torch.  The operands are rounded to the
case's dtype when they are made, so both start from the same values.  test_gemm_nt_cases_host.py checks the reference against plain autograd
formulations of the features it restates.

Metric (`nt_error`): the larger of the ROW error, max over rows of ||got[r] - ref[r]|| / max(||ref[r]||, a) with a = 1e-3 x the median norm of
the reference's non-zero rows, and the COLUMN error, the same on the transpose.  A fault confined to one 16-row block, one 4-column fragment, one
wave's column span or one tail tile moves it; a global norm hides such a fault.  A row that must be exactly zero (row_scale 0 without residual) and
is not gives an error of the order 1 / 1e-3; NaN / inf in an owned element is an infinite error.

Gate (`gate`): E(got, ref) <= K_NT[output] * F with F = E(floor, ref) of the same case.

`route(case, tuning)` restates the planner of the family, lavt_gemm_nt_route (csrc/gemm_nt_plan.hip), and its epi_wide rule: which kernel family,
tile, ring depth, K-walk mode, DACT / GD / LNA instantiation, lean level and store form a case takes.  Every row of the table states the route it is
there for; test_gemm_nt_cases_host.py holds `route` to it, and test_gemm_nt_route_host.py holds `route` to the library.  `route` restates the
convolution clauses of the planner too (nt_kwalk, lean level 3, the channel-split clause of nt_pipe_tile, the contract checks of both splits); the
convolution cases themselves, their reference and their table are gemm_nt_conv_cases.py's.  fp8 is restated nowhere."""
import collections
import functools
import math

import torch

BF = torch.bfloat16
NAN = float("nan")
EPS = 1e-5
ACT_NONE, ACT_GELU, ACT_RELU, ACT_TANH, ACT_GELU_D, ACT_STORED = 0, 1, 2, 3, 4, 5

# Gate factors, one per kernel output (".f32": the output is stored as fp32 -- fp32 problems and c_f32): twice the largest E / F measured on MI355X
# over the cases of test_gpu_gemm_nt_cases.py (its MEASURED table), rounded up, and never under 1.
K_NT = {
    "C": 2.0, "C2": 2.0, "Cpre": 2.0,                     # bf16 outputs: the error IS the final rounding
    "C.f32": 3.6, "C2.f32": 2.0, "Cpre.f32": 2.0,         # fp32 outputs: the order of the K sum
    "ln_mean": 4.0, "ln_rstd": 2.6,                       # (ln_mean: the kernel multiplies the row sum by the rounded 1 / K)
}


def k_from_measured(ratio):
    """the rule K_NT follows: twice the largest measured E / F, rounded up to two decimals, never under 1"""
    return max(1.0, math.ceil(2.0 * ratio * 100.0 - 1e-9) / 100.0)


def bf(x):
    """the value a bf16 store leaves, in x's dtype"""
    return x.to(torch.float32).to(BF).to(x.dtype)


def _gelu(z):
    return 0.5 * z * (1.0 + torch.erf(z * 0.7071067811865476))


def _gelu_grad(z):
    return 0.5 * (1.0 + torch.erf(z * 0.7071067811865476)) + z * torch.exp(-0.5 * z * z) * 0.3989422804014327


def _act(a, z):
    return {ACT_NONE: lambda t: t, ACT_GELU: _gelu, ACT_GELU_D: _gelu, ACT_RELU: torch.relu, ACT_TANH: torch.tanh}[a](z)


def _act_grad(a, z):
    if a == ACT_GELU:
        return _gelu_grad(z)
    if a == ACT_RELU:
        return (z > 0).to(z.dtype)
    if a == ACT_TANH:
        return 1.0 - torch.tanh(z) ** 2
    raise ValueError(a)


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ a case
class Case:
    """One launch of lavt_gemm_nt.  `*_x`: elements a leading dimension (or strideC) exceeds its rows by; `a_map` / `c_map`: row gather / scatter;
    `dact`: LAVT_ACT_* of the fused activation gradient (None: no dact_pre); `ln`: the LayerNorm-folded A operand; `exact`: operands kept in fp64
    (the host test's comparison with autograd); `route`: the route the row is in the table for (see `route`); `invalid`: the header refuses it."""
    DEFAULTS = dict(dtype="bf16", batch=1, kmajor=False, lda_x=0, ldb_x=0, ldc_x=0, ldc2_x=0, ldcpre_x=0, stride_x=0, alpha=0.125, bias=False,
                    bias_off=0, row_scale=False, row_scale_div=1, act=ACT_NONE, cpre=False, R=False, mul=False, c_split=0, a_map=False, c_map=False,
                    c_f32=False, dact=None, res_first=False, ln=False, ln_stats=True, ln_sigma=3.0, colstats=False, exact=False, seed=0, route=None,
                    invalid=False, why="")

    def __init__(self, name, M, N, K, **kw):
        self.name, self.M, self.N, self.K = name, M, N, K
        bad = set(kw) - set(self.DEFAULTS)
        assert not bad, bad
        for k, v in self.DEFAULTS.items():
            setattr(self, k, kw.get(k, v))
        self.kw = dict(kw)
        if self.ln:
            self.alpha = kw.get("alpha", 1.0)
            self.bias = kw.get("bias", True)
        self.es = 8 if self.dtype == "bf16" else 4

    def but(self, name, **kw):
        """the same case with some fields changed"""
        return Case(name, kw.pop("M", self.M), kw.pop("N", self.N), kw.pop("K", self.K), **{**self.kw, **kw})

    def __repr__(self):
        return self.name

    # ---- geometry
    @property
    def Ma(self):          # source rows of A
        return self.M // 2 + 3 if self.a_map else self.M

    @property
    def Mo(self):          # rows of the output buffers
        return self.M

    @property
    def Nc(self):          # columns of C
        return self.c_split if self.c_split else self.N

    @property
    def lda(self):
        return self.K + self.lda_x

    @property
    def ldb(self):
        return (self.N if self.kmajor else self.K) + self.ldb_x

    @property
    def ldc(self):
        return self.Nc + self.ldc_x

    @property
    def ldc2(self):
        return self.N - self.c_split + self.ldc2_x

    @property
    def ldcpre(self):
        return self.N + self.ldcpre_x

    @property
    def strideC(self):
        return self.Mo * self.ldc + self.stride_x if self.batch > 1 else 0

    @property
    def ld_side(self):     # leading dimension the tests give R, mul and dact_pre
        return self.N + 8

    @property
    def nrs(self):         # row-scale entries per batch entry
        return cdiv(self.M, self.row_scale_div) if self.row_scale_div > 1 else self.M

    def store_key(self, name):
        f32 = self.dtype == "f32" or (self.c_f32 and name in ("C", "C2"))
        return name + ".f32" if f32 and name in ("C", "C2", "Cpre") else name

    # ---- operands
    def _q(self, x):
        """the case's storage rounding, kept in fp64 (exact) or fp32"""
        if self.exact:
            return x.double()
        return bf(x.float()) if self.dtype == "bf16" else x.float()

    @property
    def inp(self):
        return _inputs(self)


def _gen(seed):
    return torch.Generator("cpu").manual_seed(seed)


def _randn(*shape, seed):
    return torch.randn(*shape, generator=_gen(seed), dtype=torch.float64)


_OPERANDS = collections.OrderedDict()          # (A, W, ln parts) shared by the cases that differ in the epilogue only


def _operands(c):
    key = (c.dtype, c.M, c.N, c.K, c.batch, c.a_map, c.ln, c.ln_sigma, c.alpha, c.exact, c.seed)
    if key in _OPERANDS:
        _OPERANDS.move_to_end(key)
        return _OPERANDS[key]
    s = 1000 * c.seed
    o = {}
    if c.ln:
        # LayerNorm rows: sigma_r in [0.5, 2], mean of ln_sigma sigma_r with either sign; W ~ 1.2 / sqrt(K) so that the pre-activation spreads over [-3, 3]
        sig = 0.5 + 1.5 * torch.rand(c.batch, c.Ma, 1, generator=_gen(s + 11), dtype=torch.float64)
        sign = torch.where(torch.rand(c.batch, c.Ma, 1, generator=_gen(s + 12)) < 0.5, -1.0, 1.0).double()
        o["A"] = c._q(sig * _randn(c.batch, c.Ma, c.K, seed=s + 1) + c.ln_sigma * sig * sign)
        W = (1.2 / math.sqrt(c.K)) * _randn(c.N, c.K, seed=s + 2)
        gamma, beta, b0 = 1.0 + 0.3 * _randn(c.K, seed=s + 13), 0.3 * _randn(c.K, seed=s + 14), _randn(c.N, seed=s + 15)
        if not c.exact:
            W, gamma, beta, b0 = (t.float() for t in (W, gamma, beta, b0))
        # the formula of lavt_ln_fold: Wg = bf16(gamma_k W[n][k]), wsum[n] = sum_k Wg[n][k] of the ROUNDED values, biasp[n] = b_n + sum_k beta_k W[n][k]
        Wg = c._q(W * gamma[None, :])
        o.update(W0=W, gamma=gamma, beta=beta, b0=b0, W=Wg[None], wsum=Wg.double().sum(1), wsum_unfolded=W.double().sum(1),
                 biasp=(b0.double() + W.double() @ beta.double())[None])
        if not c.exact:
            o["wsum"], o["wsum_unfolded"], o["biasp"] = o["wsum"].float(), o["wsum_unfolded"].float(), o["biasp"].float()
    else:
        o["A"] = c._q(_randn(c.batch, c.Ma, c.K, seed=s + 1))
        o["W"] = c._q((1.2 / (abs(c.alpha) * math.sqrt(c.K))) * _randn(c.batch, c.N, c.K, seed=s + 2))          # logical [batch][N][K] in both layouts
    _OPERANDS[key] = o
    while len(_OPERANDS) > 3:
        _OPERANDS.popitem(last=False)
    return o


def _inputs(c):
    """every tensor the launch receives, as CPU tensors holding the values of the case's dtype (fp32 side inputs as fp32)"""
    s = 1000 * c.seed
    i = dict(_operands(c))
    M, N = c.M, c.N
    if c.a_map:          # rows repeated (Ma < M), every fifth row reads zeros
        am = (torch.arange(M) * 7) % c.Ma
        am[torch.arange(M) % 5 == 2] = -1
        i["a_map"] = am.to(torch.int32)
    if c.c_map:          # a permutation, every seventh row dropped
        cm = torch.randperm(M, generator=_gen(s + 20))
        cm[torch.arange(M) % 7 == 3] = -1
        i["c_map"] = cm.to(torch.int32)
    if c.bias and not c.ln:
        i["bias"] = _randn(c.batch, N, seed=s + 3) if c.exact else _randn(c.batch, N, seed=s + 3).float()
    if c.ln and c.bias:
        i["bias"] = i["biasp"]
    if c.row_scale:          # 0, 1 and 1 / 0.7 per row_scale_div block (the DropPath factors of three samples)
        vals = torch.tensor([0.0, 1.0, 1.0 / 0.7], dtype=torch.float64)
        idx = (torch.arange(c.nrs)[None, :] + torch.arange(c.batch)[:, None] + 1) % 3
        i["row_scale"] = vals[idx] if c.exact else vals[idx].float()
    if c.R:
        i["R"] = c._q(_randn(c.Mo, N, seed=s + 4))
    if c.mul:
        i["mul"] = c._q(_randn(c.Mo, N, seed=s + 5))
    if c.dact is not None:
        pre = 1.5 * _randn(c.Mo, N, seed=s + 6)
        i["dact_pre"] = c._q(_gelu_grad(c._q(pre).double()) if c.dact == ACT_STORED else pre)
    return i


# ------------------------------------------------------------------------------------------------ the contract
_ACC = collections.OrderedDict()


def _accumulate(c, i, dtype, drop_k=0):
    """acc[b][m][n] = sum_k A_op[b][m][k] W[b][n][k] and the gathered raw rows (a_rowmap: -1 reads zeros)"""
    key = (c.dtype, c.M, c.N, c.K, c.batch, c.a_map, c.ln, c.ln_sigma, c.alpha, c.exact, c.seed, dtype, drop_k)
    if key in _ACC:
        _ACC.move_to_end(key)
        return _ACC[key]
    A, W = i["A"].to(dtype), i["W"].to(dtype)
    if c.a_map:
        am = i["a_map"].long()
        A = A[:, am.clamp(min=0)] * (am >= 0).to(dtype)[None, :, None]
    Kk = c.K - drop_k
    acc = torch.matmul(A[..., :Kk], W[..., :Kk].transpose(1, 2))
    _ACC[key] = (acc, A)
    while len(_ACC) > 3:
        _ACC.popitem(last=False)
    return acc, A


def nt_reference(case, dtype=torch.float64, round_bf16=False, fault=None):
    """The contract of lavt_gemm_nt for `case`.  `fault` (the host self-test only) plants one defect: "drop_last_k8", "bias_after_scale",
    "mul_after_res", "ignore_res_first", "ignore_row_scale_div", "wsum_unfolded"."""
    c, i = case, case.inp
    rnd = bf if (round_bf16 and c.dtype == "bf16") else (lambda t: t)
    M, N = c.M, c.N
    acc, rows = _accumulate(c, i, dtype, 8 if fault == "drop_last_k8" else 0)
    out = {}
    v = acc
    if c.ln:
        # rstd (acc - mean wsum_n) from the raw rows: mean = sum x / K, var = sum x^2 / K - mean^2 (clamped at 0), as the kernel takes them from its tiles
        mean = rows.sum(-1) / c.K
        rstd = torch.rsqrt(((rows * rows).sum(-1) / c.K - mean * mean).clamp(min=0.0) + EPS)
        wsum = i["wsum_unfolded" if fault == "wsum_unfolded" else "wsum"].to(dtype)
        v = rstd[..., None] * (acc - mean[..., None] * wsum)
        if c.ln_stats:
            out["ln_mean"], out["ln_rstd"] = mean[0], rstd[0]
    bias = i["bias"].to(dtype)[:, None, :] if "bias" in i else None
    rs = None
    if c.row_scale:
        m = torch.arange(M)
        idx = m // c.row_scale_div if c.row_scale_div > 1 else m
        if fault == "ignore_row_scale_div":
            idx = m % c.nrs
        rs = i["row_scale"].to(dtype)[:, idx][..., None]
    v = v * c.alpha
    if fault == "bias_after_scale":
        v = (v * rs if rs is not None else v) + (bias if bias is not None else 0.0)
    else:
        if bias is not None:
            v = v + bias
        if rs is not None:
            v = v * rs
    orow = i["c_map"].long() if c.c_map else torch.arange(M)
    live = orow >= 0
    side = {k: i[k].to(dtype)[orow.clamp(min=0)][None] for k in ("R", "mul", "dact_pre") if k in i}          # indexed by the OUTPUT row
    pre_out = None
    if c.dact is not None:
        first = c.res_first and fault != "ignore_res_first"
        if first:
            v = v + side["R"]
        v = v * (side["dact_pre"] if c.dact == ACT_STORED else _act_grad(c.dact, side["dact_pre"]))
        if c.R and not first:
            v = v + side["R"]
    else:
        if c.cpre:
            pre_out = _gelu_grad(v) if c.act == ACT_GELU_D else v
        v = _act(c.act, v)
        if fault == "mul_after_res":
            v = (v + side["R"]) * side["mul"]
        else:
            if c.mul:
                v = v * side["mul"]
            if c.R:
                v = v + side["R"]

    def scatter(t, keep_f32):
        full = torch.full((t.shape[0], c.Mo, N), NAN, dtype=dtype)
        full[:, orow[live]] = t[:, live]
        return full if keep_f32 else rnd(full)
    full = scatter(v, c.c_f32)
    if c.c_split:
        out["C"], out["C2"] = full[..., :c.c_split].contiguous(), full[0, :, c.c_split:].contiguous()
    else:
        out["C"] = full
    if pre_out is not None:
        out["Cpre"] = scatter(pre_out, False)[0]
    return out


def reference(case):
    return nt_reference(case, torch.float64, False)


def floor(case):
    return nt_reference(case, torch.float32, True)


# ------------------------------------------------------------------------------------------------ metric and gate
def _axis_error(g, r):
    rn = r.norm(dim=1)
    nz = rn[rn > 0]
    a = 1e-3 * float(nz.median()) if nz.numel() else 1e-30
    return float(((g - r).norm(dim=1) / rn.clamp(min=a)).max())


def nt_error(got, ref):
    """max(row error, column error) over the rows the reference owns (its NaN rows are nobody's); NaN / inf in an owned element of got -> inf"""
    g, r = (t.detach().cpu().to(torch.float64) for t in (got, ref))
    assert g.shape == r.shape, (g.shape, r.shape)
    g, r = (t.reshape(-1, 1) if t.dim() == 1 else t.reshape(-1, t.shape[-1]) for t in (g, r))
    own = torch.isfinite(r).all(dim=1)
    g, r = g[own], r[own]
    if not bool(torch.isfinite(g).all()):
        return math.inf
    return max(_axis_error(g, r), _axis_error(g.T, r.T))


def gate(key, got, ref, flo, case="", report=False, factors=None):
    """E(got, ref) <= K[key] * E(floor, ref), K = K_NT or the `factors` of another table of the family.  Raises AssertionError on a miss and returns
    (E, F); with report it raises nothing and returns (E, F, ok).  A floor of exactly 0 admits E = 0 only."""
    K = K_NT if factors is None else factors
    E, Fl = nt_error(got, ref), nt_error(flo, ref)
    ok = E <= K[key] * Fl
    if report:
        return E, Fl, ok
    assert ok, f"{case} {key}: error {E:.3e} > {K[key]:g} x floor {Fl:.3e} (E / F = {E / Fl if Fl > 0 else math.inf:.2f})"
    return E, Fl


def rejects(key, got, ref, flo):
    """the planted-fault condition: the gate fails with a factor 2 to spare, and the mutated tensor differs from the floor"""
    E = nt_error(got, ref)
    same = got.shape == flo.shape and torch.equal(torch.nan_to_num(got.double(), nan=0.0), torch.nan_to_num(flo.double(), nan=0.0))
    return (not same) and E > 0.0 and E >= 2.0 * K_NT[key] * nt_error(flo, ref)


# ------------------------------------------------------------------------------------------------ the launch of a case
def launch_args(c, buf):
    """(args, kwargs) of lavt_hip.ops.gemm_nt / gemm_nt_params for a case.  `buf`: name -> operand, absent or None where the case has none -- A, B, C,
    C2, Cpre, bias (at bias_off already), row_scale, R, mul, dact_pre (rows of c.ld_side elements), a_map, c_map, wsum, ln_mean, ln_rstd.  The GPU test
    passes device tensors, the host route test made-up addresses: one statement of how a case becomes a lavt_gemm_nt_t."""
    g = buf.get
    dt = BF if c.dtype == "bf16" else torch.float32
    strideA, strideB = (c.Ma * c.lda, (c.K if c.kmajor else c.N) * c.ldb) if c.batch > 1 else (0, 0)
    ld_side = c.ld_side
    kw = dict(batch=c.batch, strideA=strideA, strideB=strideB, strideC=c.strideC, a_rowmap=g("a_map"), b_kmajor=c.kmajor, alpha=c.alpha, bias=g("bias"),
              strideBias=c.N if c.batch > 1 else 0, row_scale=g("row_scale"), strideRowScale=c.nrs if c.batch > 1 else 0, row_scale_div=c.row_scale_div, act=c.act,
              Cpre=g("Cpre"), ldcpre=c.ldcpre if c.cpre else 0, R=g("R"), ldr=ld_side if c.R else 0, C2=g("C2"), ldc2=c.ldc2 if c.c_split else 0, c_split=c.c_split,
              c_rowmap=g("c_map"), c_f32=c.c_f32, dact_pre=g("dact_pre"), lddact=ld_side if c.dact is not None else 0, dact=c.dact if c.dact is not None else 0,
              mul=g("mul"), ldmul=ld_side if c.mul else 0, res_first=c.res_first, ln=(g("wsum"), g("ln_mean"), g("ln_rstd"), EPS) if c.ln else None)
    return (dt, c.M, c.N, c.K, buf["A"], c.lda, buf["B"], c.ldb, buf["C"], c.ldc), kw


# ------------------------------------------------------------------------------------------------ the dispatch, restated
# The library decides all of this in ONE place, lavt_gemm_nt_route (csrc/gemm_nt_plan.hip); test_gemm_nt_route_host.py holds `route`, `epi_wide` and
# `colstats_plan` below to its answers, row by row, so a threshold edited there and not here fails on the CPU.
S2_MIN128, GEMM_BIG_LONG = 257, 128          # csrc/gemm_nt_plan.hip
DEFAULT = dict(tile=0, stages=0, pipe=2)      # LAVT_GEMM_TILE / LAVT_GEMM_STAGES / LAVT_GEMM_PIPE as csrc/tuning.hip reads them
INVALID = "invalid"

Route = collections.namedtuple("Route", "family tile stages kmode kind lean forms prefetch")


def route_str(r):
    if r == INVALID:
        return INVALID
    d = lambda x: "-" if x is None else x
    return f"{r.family}/{r.tile}/s{r.stages}/k{d(r.kmode)}/{r.kind or '-'}/L{d(r.lean)}/{'+'.join(sorted(r.forms, reverse=True))}"


def epi_wide(c):
    """lavt_gemm_nt's epi_wide: bit 0 the 16-byte store form (every alignment holds), bit 1 the side inputs requested before the K loop (batch 1).
    (ldr, lddact % 4 and the 16-byte alignment of C, C2, Cpre hold in every case of the table.)"""
    w = (c.dtype == "bf16" and not c.c_f32 and c.ldc % 8 == 0 and (not c.c_split or (c.ldc2 % 8 == 0 and c.c_split % 8 == 0))
         and (not c.cpre or c.ldcpre % 8 == 0) and (not c.bias or ((c.N if c.batch > 1 else 0) % 4 == 0 and c.bias_off % 4 == 0)) and c.strideC % 8 == 0)
    return (1 | (2 if c.batch == 1 else 0)) if w else 0


def _forms(c, span, bf16_kernel=True):
    """the store forms over the wave column spans of width `span`: wide where epi_wide holds and the span is full, narrow otherwise"""
    if not (bf16_kernel and epi_wide(c)):
        return frozenset(["narrow"])
    f = set()
    if c.N // span:
        f.add("wide")
    if c.N % span:
        f.add("narrow")
    return frozenset(f)


WALK_GENERAL, WALK_PLAIN, WALK_TAPS, WALK_PARTIAL = 0, 1, 2, 3          # LAVT_NT_WALK_*


def _cv(c, name, default=0):
    """a convolution field of a case (gemm_nt_conv_cases.ConvCase has them; the plain rows of this file do not)"""
    return getattr(c, name, default)


def fits(c):
    """the 2 GB bound of the pipelined family's 32-bit descriptor offsets, halo margin included (restated for the route comparison only)"""
    lim = (1 << 31) - (1 << 24)
    a_rows = c.M + 2 * ((c.conv_h if c.conv_h > 0 else 1) * c.conv_w + c.conv_w + 1)
    b_rows = c.taps * c.conv_kc if c.kmajor else c.N
    return a_rows * c.lda * 2 < lim and (not c.C2src or a_rows * c.lda2 * 2 < lim) and b_rows * c.ldb * 2 + c.batch * c.strideB * 2 < lim


def kwalk(c, descriptors):
    """the planner's nt_kwalk for bf16 operands; descriptors: the pipelined family (the 2 GB bound, the only home of the partial-block walk)"""
    kc = _cv(c, "conv_kc")
    if kc <= 0:
        return WALK_PLAIN if c.K % 64 == 0 else WALK_GENERAL          # (no row of the plain table has a concat source)
    walkable = (not c.C2src or c.a_split % 64 == 0) and c.taps <= 32 and (not descriptors or fits(c))
    if kc % 64 == 0 and walkable:
        return WALK_TAPS
    if (descriptors and not c.kmajor and kc % 8 == 0 and walkable and c.conv_kc_split <= 0 and c.conv_tap_split <= 0 and c.batch == 1
            and c.K == c.taps * kc and c.ldb >= c.taps * kc):
        return WALK_PARTIAL
    return WALK_GENERAL


def _lean(c, kmode, tile=0):
    """the planner's nt_lean: epilogue instantiations without the features a launch does not use (every K walk but the general decode); 3: the bare
    store with C2 kept, on the 256x256 tile with k-major weights and the tap walk only"""
    if kmode == WALK_GENERAL or c.act != ACT_NONE or c.mul or c.cpre:
        return 0
    bare = not (c.bias or c.R or c.row_scale or c.c_map)
    if not c.c_split:
        return 2 if bare else 1
    return 3 if bare and tile == 256 and c.kmajor and kmode == WALK_TAPS else 0


def _contract_ok(c, t):
    """the argument checks of lavt_gemm_nt itself"""
    if c.K % c.es or (c.kmajor and c.N % c.es) or c.lda % c.es or c.ldb % c.es or c.ldc % 4 or (c.c_split and c.c_split % 4):
        return False
    if _cv(c, "C2src") and (c.a_split % c.es or c.lda2 % c.es):
        return False
    kc = _cv(c, "conv_kc")
    if kc > 0:
        a2_ok = not c.C2src or c.a_split % 64 == 0
        if c.conv_kc_split > 0:
            p = pipe_tile(c, t)
            if not (c.dtype == "bf16" and c.conv_tap_split == 0 and c.conv_kc_split % 64 == 0 and c.batch * c.conv_kc_split == kc and c.K == c.taps * c.conv_kc_split
                    and c.strideB == 0 and c.taps <= 32 and a2_ok and p is not None and p[0] == 128):
                return False
        elif c.conv_tap_split > 0:
            if not (c.dtype == "bf16" and c.K == c.conv_tap_split * kc and c.batch * c.conv_tap_split == c.taps and kc % 64 == 0 and c.taps <= 32 and a2_ok):
                return False
        elif not (c.K == c.taps * kc and kc % c.es == 0 and c.conv_h > 0 and c.conv_w > 0):
            return False
        if c.M % c.vox:
            return False
    if c.act == ACT_GELU_D and not (c.ln and c.cpre and not (c.mul or c.c_split or c.R or c.row_scale or c.c_map)):
        return False
    if c.res_first and not (c.dact is not None and c.R):
        return False
    return True


def _plain_choice(c, t):
    """(big, stages) of the planner's nt_tile_rule with both clauses (forced configuration, long K)"""
    tiles128, tiles64 = cdiv(c.M, 128) * cdiv(c.N, 128) * c.batch, cdiv(c.M, 64) * cdiv(c.N, 64) * c.batch
    big = (t["tile"] == 128) if t["tile"] else ((tiles128 >= 200 or (c.K >= 64 * 64 and tiles128 >= GEMM_BIG_LONG)) and c.N >= 128)
    wgs = tiles128 if big else tiles64
    return big, t["stages"] if t["stages"] else (2 if wgs >= (S2_MIN128 if big else 512) else 4)


def pipe_tile(c, t):
    """the planner's nt_pipe_tile: (tile, stages) of csrc/gemm_nt_pipe.hip, or None"""
    if c.dtype != "bf16" or t["pipe"] < 1 or c.ln or c.dact is not None:
        return None
    if c.lda % 8 or c.ldb % 8 or (_cv(c, "C2src") and c.lda2 % 8):
        return None
    if _cv(c, "conv_kc_split") > 0:          # the channel-split reduction exists in this family's tap-walking mode only
        return 128, 4
    big, stages = _plain_choice(c, t)
    tiles256 = cdiv(c.M, 256) * cdiv(c.N, 256) * c.batch
    rounds = cdiv(tiles256, 256)
    n_fits = c.N % 256 == 0 or (c.N % 8 == 0 and c.N * 16 >= cdiv(c.N, 256) * 256 * 15)
    huge = (t["tile"] == 512) if t["tile"] else (n_fits and c.K >= 1024 and tiles256 >= 128 and tiles256 * 10 >= rounds * 256 * 8)
    if huge:
        return 256, 2
    if big and (t["pipe"] >= 3 or (t["pipe"] == 2 and c.K >= 1024)):
        return 128, 2 if stages == 2 else 4
    return None


def colstats_plan(c, t):
    """lavt_gemm_nt_colstats_plan: row blocks with statistics (0: refused)"""
    if c.batch != 1 or c.bias or c.act or c.R or c.row_scale or c.c_map or c.c_f32 or c.c_split or c.cpre or c.mul or c.N % 4:
        return 0
    p = pipe_tile(c, t)
    return cdiv(c.M, p[0]) * 2 if p else 0


def route(case, tuning=None):
    """-> Route, or INVALID where the launch returns LAVT_ERR_INVALID"""
    c, t = case, dict(DEFAULT, **(tuning or {}))
    if not _contract_ok(c, t) or (c.colstats and not colstats_plan(c, t)):
        return INVALID
    p = pipe_tile(c, t)
    if p:
        kmode = kwalk(c, True)
        return Route("pipe", p[0], p[1], kmode, "", _lean(c, kmode, p[0]), _forms(c, 64 if p[0] == 256 else 32), False)
    kmode = kwalk(c, False)          # plain: no taps, no concat source, K % 64 == 0; taps: the tap walk; else the general decode
    if c.dtype == "bf16":          # csrc/gemm_v2.hip (the zero page is always given; lda, ldb % 8 hold by the contract)
        tiles128, tiles64 = cdiv(c.M, 128) * cdiv(c.N, 128), cdiv(c.M, 64) * cdiv(c.N, 64)
        pick = lambda a, b: (128, 2 if a >= S2_MIN128 else 4) if (a >= 200 and c.N >= 128) else (64, 2 if b >= 512 else 4)          # ignores the forced tile / stages
        if c.ln:          # the LayerNorm-folded operand
            if c.kmajor or c.a_map or c.K % 64 or c.N % 4 or c.batch != 1 or c.dact is not None or not c.bias or c.alpha != 1.0:
                return INVALID
            tile, st = pick(tiles128, tiles64)
            return Route("v2", tile, st, 1, "LNA+GD" if c.act == ACT_GELU_D else "LNA", 0, _forms(c, 32), False)
        if c.dact is not None:          # the fused activation gradient
            if not c.kmajor or c.K % 64 or c.N % 8 or c.c_f32 or c.c_split or c.cpre or c.act or c.mul:
                return INVALID
            tile, st = pick(tiles128 * c.batch, tiles64 * c.batch)
            gd = c.dact == ACT_STORED and not (c.R or c.bias or c.c_map)
            pf = bool(epi_wide(c) & 2) and "wide" in _forms(c, 32) and (tile == 64 or gd)
            return Route("v2", tile, st, 1, "DACT+GD" if gd else "DACT", 0, _forms(c, 32), pf)
        big, stages = _plain_choice(c, t)
        tile, lean = (128 if big else 64), _lean(c, kmode, 128 if big else 64)
        pf = tile == 64 and lean < 2 and bool(epi_wide(c) & 2) and "wide" in _forms(c, 32) and bool(c.R or c.mul)
        return Route("v2", tile, stages, kmode, "", lean, _forms(c, 32), pf)
    if c.ln or c.dact is not None:          # fp32: both exist on the bf16 LDS-DMA path only
        return INVALID
    tiles128 = cdiv(c.M, 128) * cdiv(c.N, 128) * c.batch
    big = (t["tile"] == 128) if t["tile"] else (tiles128 >= 768 and c.N >= 128)
    return Route("classic", 128 if big else 64, 2, None, "", None, _forms(c, 64 if big else 32, False), False)


# ------------------------------------------------------------------------------------------------ the forced configurations
# name -> (LAVT_GEMM_TILE, LAVT_GEMM_STAGES, LAVT_GEMM_PIPE) and the (family, tile, ring depth) a plain bf16 problem takes under it.  The dispatcher
# honours seven distinct ones; the other five of the 3 x 2 x 2 settings fall back onto the 64x64 tile (LAVT_GEMM_TILE=64 has no pipelined form, and
# 512 names the pipelined 256x256 tile only) and are run all the same.
TUNINGS = {
    "t64-s4-p0": ((64, 4, 0), "v2/64/s4"), "t64-s2-p0": ((64, 2, 0), "v2/64/s2"), "t64-s4-p3": ((64, 4, 3), "v2/64/s4"), "t64-s2-p3": ((64, 2, 3), "v2/64/s2"),
    "t128-s4-p0": ((128, 4, 0), "v2/128/s4"), "t128-s2-p0": ((128, 2, 0), "v2/128/s2"), "t128-s4-p3": ((128, 4, 3), "pipe/128/s4"), "t128-s2-p3": ((128, 2, 3), "pipe/128/s2"),
    "t512-s4-p0": ((512, 4, 0), "v2/64/s4"), "t512-s2-p0": ((512, 2, 0), "v2/64/s2"), "t512-s4-p3": ((512, 4, 3), "pipe/256/s2"), "t512-s2-p3": ((512, 2, 3), "pipe/256/s2"),
}
TUNINGS_F32 = {"t64": ((64, 0, 2), "classic/64/s2"), "t128": ((128, 0, 2), "classic/128/s2")}          # the classic kernel: no ring, no K-walk modes, no lean forms


def tuning_dict(name):
    tile, stages, pipe = {**TUNINGS, **TUNINGS_F32}[name][0]
    return dict(tile=tile, stages=stages, pipe=pipe)


def tuning_env(name):
    tile, stages, pipe = {**TUNINGS, **TUNINGS_F32}[name][0]
    return {"LAVT_GEMM_TILE": str(tile), "LAVT_GEMM_STAGES": str(stages), "LAVT_GEMM_PIPE": str(pipe)}


def stated_route(case, tuning_name):
    """the route a row of a forced-configuration group states: (family / tile / ring) of the configuration + the row's own (K walk / kind / lean / forms)"""
    prefix = {**TUNINGS, **TUNINGS_F32}[tuning_name][1]
    return prefix + ("/k-/-/L-/narrow" if prefix.startswith("classic") else "/" + case.route)


# ------------------------------------------------------------------------------------------------ the table
# Rows of the forced-configuration groups state `route` as "K walk / kind / lean / store forms"; the (family, tile, ring) comes from TUNINGS.
# N = 8, 24: below a fragment / a span -> narrow only.  N = 72, 136, 328: full spans and a last span of 8 -> wide + narrow (the same for the 32- and the
# 64-column spans).  N = 128: wide only.  K % 64 != 0 is the general decode (k0), which has no lean form.
def _edge(name, M, N, K, route, **kw):
    return Case("edge-" + name, M, N, K, route=route, **kw)


EDGES = [
    _edge("m5-n8-k8", 5, 8, 8, "k0/-/L0/narrow", why="M < 16, N below a fragment, K below a chunk row of the tile"),
    _edge("m5-n8-k8-km", 5, 8, 8, "k0/-/L0/narrow", kmajor=True),
    _edge("m129-n24-k56", 129, 24, 56, "k0/-/L0/narrow", why="tile + 1 rows, partial first span, K tail only"),
    _edge("m143-n72-k64-km", 143, 72, 64, "k1/-/L2/wide+narrow", kmajor=True, why="tile + 15, exactly one K tile"),
    _edge("m143-n72-k64", 143, 72, 64, "k1/-/L2/wide+narrow"),
    _edge("m145-n136-k72-ld", 145, 136, 72, "k0/-/L0/wide+narrow", lda_x=8, ldb_x=16, ldc_x=8, why="tile + 17, N % 16 == 8, one K tile + tail, lda / ldb / ldc wider than the rows"),
    _edge("m191-n328-k264-km-ld", 191, 328, 264, "k0/-/L0/wide+narrow", kmajor=True, lda_x=24, ldb_x=8, ldc_x=16, why="tile + 63, several column tiles, four K tiles + tail"),
    _edge("m257-n136-k264", 257, 136, 264, "k0/-/L0/wide+narrow", why="256 + 1 rows"),
    _edge("m319-n328-k64", 319, 328, 64, "k1/-/L2/wide+narrow", why="256 + 63 rows, three 128-column tiles"),
    _edge("m271-n72-k72-km", 271, 72, 72, "k0/-/L0/wide+narrow", kmajor=True, why="256 + 15 rows"),
    _edge("m81-n24-k8-km", 81, 24, 8, "k0/-/L0/narrow", kmajor=True, why="64 + 17 rows"),
    _edge("m65-n8-k264-km", 65, 8, 264, "k0/-/L0/narrow", kmajor=True),
    _edge("m129-n132-k64-f32out", 129, 132, 64, "k1/-/L2/narrow", c_f32=True, why="N % 8 == 4 (fp32 output: the narrow form only)"),
    _edge("m273-n328-k56-bias", 273, 328, 56, "k0/-/L0/wide+narrow", bias=True, ldc_x=8, why="256 + 17 rows, bias across the last span"),
]

_W = dict(bias=True)          # the wide twin of the store-form switches: M = 145, N = 128, K = 64, bias
STORE_FORMS = [
    Case("store-wide", 145, 128, 64, route="k1/-/L1/wide", **_W, why="the wide case the switches are compared with"),
    Case("store-ldc+4", 145, 128, 64, route="k1/-/L1/narrow", ldc_x=4, **_W, why="ldc % 8 == 4"),
    Case("store-split68", 145, 128, 64, route="k1/-/L0/narrow", c_split=68, ldc_x=4, ldc2_x=4, **_W, why="c_split % 8 == 4 (ldc = 72, ldc2 = 64)"),
    Case("store-split64", 145, 128, 64, route="k1/-/L0/wide", c_split=64, **_W, why="the wide twin of the split"),
    Case("store-ldcpre+4", 145, 128, 64, route="k1/-/L0/narrow", cpre=True, ldcpre_x=4, act=ACT_RELU, **_W, why="ldcpre % 8 == 4"),
    Case("store-bias+1", 145, 128, 64, route="k1/-/L1/narrow", bias_off=1, **_W, why="bias pointer off 16 bytes by one float"),
    Case("store-batch3-stride+4", 145, 128, 64, route="k1/-/L1/narrow", batch=3, stride_x=4, **_W, why="strideC % 8 == 4"),
    Case("store-batch3", 145, 128, 64, route="k1/-/L1/wide", batch=3, **_W, why="wide without the side prefetch (batch > 1)"),
    Case("store-none-ldc+4", 145, 128, 64, route="k1/-/L2/narrow", ldc_x=4, why="the plain store, narrow in every span"),
]

LEAN = [
    Case("lean-none", 145, 128, 64, route="k1/-/L2/wide", why="no side input at all"),
    Case("lean-bias", 145, 128, 64, route="k1/-/L1/wide", bias=True),
    Case("lean-bias-R-scale-map", 145, 128, 64, route="k1/-/L1/wide", bias=True, R=True, row_scale=True, c_map=True, why="proj forward: residual, DropPath scale, window reverse"),
    Case("lean-C2", 145, 128, 64, route="k1/-/L0/wide", c_split=96, why="C2 alone, the split data gradient of a concat (outside convolutions the full epilogue carries it)"),
    Case("lean-gate", 145, 128, 64, route="k1/-/L0/wide", bias=True, act=ACT_TANH, cpre=True, mul=True, R=True, why="the language-gate form: x + tanh(g) * r"),
    Case("lean-gelu", 145, 136, 64, route="k1/-/L0/wide+narrow", bias=True, act=ACT_GELU, cpre=True, R=True, row_scale=True, why="fc1-like: GELU with its pre-activation, both store forms"),
]

ROWMAPS = [
    Case("map-a", 145, 136, 72, route="k0/-/L0/wide+narrow", a_map=True, bias=True, why="a_rowmap with -1 rows and rows repeated"),
    Case("map-c", 145, 136, 64, route="k1/-/L1/wide+narrow", c_map=True, R=True, why="c_rowmap with -1 rows and a permutation; R by output row"),
    Case("map-both-div", 145, 128, 64, route="k1/-/L1/wide", a_map=True, c_map=True, bias=True, R=True, row_scale=True, row_scale_div=72, why="both, row_scale_div = M // 2 samples"),
    Case("map-both-mul", 81, 72, 56, route="k0/-/L0/wide+narrow", a_map=True, c_map=True, mul=True, R=True, act=ACT_GELU, bias=True, row_scale=True, row_scale_div=27),
]
PLAIN = EDGES + STORE_FORMS + LEAN + ROWMAPS
GROUPS = {"edges": EDGES, "store": STORE_FORMS, "lean": LEAN, "maps": ROWMAPS}


def as_f32(c):
    """the fp32 twin of a plain row (the classic kernel; its narrow form only)"""
    return c.but(c.name + "-f32", dtype="f32")


PLAIN_F32 = [as_f32(c) for c in EDGES + LEAN + ROWMAPS]

# the default rules (no forced configuration): rows state the whole route
DEFAULT_RULES = [
    Case("k1024-pipe128", 3073, 1024, 1024, route="pipe/128/s4/k1/-/L1/wide", bias=True, why="200 tiles of 128x128 with K >= 1024 go to the pipelined kernel at LAVT_GEMM_PIPE=2"),
    Case("k960-v2-128", 3073, 1024, 960, route="v2/128/s4/k1/-/L1/wide", bias=True, why="the same tiles under K = 1024 stay in gemm_v2"),
]

# the four sizes whose tile counts pick the four kernels (tile x ring depth) of the DACT and the LNA kind
SIZES = [(77, 136, "v2/64/s4"), (2053, 1024, "v2/64/s2"), (3190, 1024, "v2/128/s4"), (4217, 1024, "v2/128/s2")]


def _span_forms(N, narrow):
    return "narrow" if narrow else ("wide" if N % 32 == 0 else "wide+narrow")


def _dact_cases():
    rows = []
    for M, N, pre in SIZES:
        for K in (64, 192):
            base = dict(kmajor=True, bias=True, row_scale=True, c_map=True)
            for dact, nm in ((ACT_GELU, "gelu"), (ACT_RELU, "relu"), (ACT_TANH, "tanh")):
                for R, first, tag in ((False, False, ""), (True, False, "-R"), (True, True, "-Rfirst")):
                    rows.append(Case(f"dact-{nm}{tag}-m{M}-k{K}", M, N, K, route=f"{pre}/k1/DACT/L0/{_span_forms(N, False)}", dact=dact, R=R, res_first=first, **base))
            rows.append(Case(f"dact-stored-m{M}-k{K}", M, N, K, route=f"{pre}/k1/DACT+GD/L0/{_span_forms(N, False)}", kmajor=True, row_scale=True, dact=ACT_STORED,
                             why="the stored-derivative instantiation: no side input but the row scale"))
            rows.append(Case(f"dact-stored-R-m{M}-k{K}", M, N, K, route=f"{pre}/k1/DACT/L0/{_span_forms(N, False)}", kmajor=True, dact=ACT_STORED, R=True,
                             why="LAVT_ACT_STORED through the general instantiation"))
        # the narrow form in every span of each of the four kernels, both instantiations
        rows.append(Case(f"dact-gelu-Rfirst-narrow-m{M}", M, N, 64, route=f"{pre}/k1/DACT/L0/narrow", ldc_x=4, dact=ACT_GELU, R=True, res_first=True, **base))
        rows.append(Case(f"dact-stored-narrow-m{M}", M, N, 64, route=f"{pre}/k1/DACT+GD/L0/narrow", ldc_x=4, kmajor=True, dact=ACT_STORED))
    return rows


def _lna_cases():
    rows = []
    for M, N, pre in SIZES:
        for K in (64, 192):
            f = _span_forms(N, False)
            for stats in (True, False):
                s = "" if stats else "-nostats"
                rows.append(Case(f"lna-none{s}-m{M}-k{K}", M, N, K, route=f"{pre}/k1/LNA/L0/{f}", ln=True, ln_stats=stats))
                rows.append(Case(f"lna-gelu{s}-m{M}-k{K}", M, N, K, route=f"{pre}/k1/LNA/L0/{f}", ln=True, ln_stats=stats, act=ACT_GELU, cpre=True))
                rows.append(Case(f"lna-gelud{s}-m{M}-k{K}", M, N, K, route=f"{pre}/k1/LNA+GD/L0/{f}", ln=True, ln_stats=stats, act=ACT_GELU_D, cpre=True))
        rows.append(Case(f"lna-R-scale-map-m{M}", M, N, 64, route=f"{pre}/k1/LNA/L0/{_span_forms(N, False)}", ln=True, act=ACT_GELU, cpre=True, R=True, row_scale=True, c_map=True,
                         why="residual, row scale and row map on the non-GELU_D form"))
        rows.append(Case(f"lna-10sigma-m{M}", M, N, 192, route=f"{pre}/k1/LNA+GD/L0/{_span_forms(N, False)}", ln=True, ln_sigma=10.0, act=ACT_GELU_D, cpre=True,
                         why="rows whose mean is 10 sigma: sum x^2 / K - mean^2 cancels two digits"))
        rows.append(Case(f"lna-none-narrow-m{M}", M, N, 64, route=f"{pre}/k1/LNA/L0/narrow", ln=True, ldc_x=4))
        rows.append(Case(f"lna-gelud-narrow-m{M}", M, N, 64, route=f"{pre}/k1/LNA+GD/L0/narrow", ln=True, act=ACT_GELU_D, cpre=True, ldc_x=4))
    return rows


DACT = _dact_cases()
LNA = _lna_cases()

# combinations the header declares invalid: argument checks in host code, no kernel runs
_R = dict(route=INVALID, invalid=True)
REFUSALS = [
    Case("refuse-gelud-without-ln", 77, 136, 64, act=ACT_GELU_D, cpre=True, bias=True, **_R),
    Case("refuse-resfirst-without-dact", 77, 136, 64, R=True, res_first=True, **_R),
    Case("refuse-dact-k72", 77, 136, 72, kmajor=True, dact=ACT_GELU, **_R),
    Case("refuse-dact-kcontiguous", 77, 136, 64, dact=ACT_GELU, **_R),
    Case("refuse-ln-f32", 77, 136, 64, ln=True, dtype="f32", **_R),
    Case("refuse-ln-alpha", 77, 136, 64, ln=True, alpha=0.125, **_R),
    Case("refuse-ln-nobias", 77, 136, 64, ln=True, bias=False, **_R),
    Case("refuse-colstats", 77, 136, 64, colstats=True, why="64x64 tiles have no statistics epilogue: lavt_gemm_nt_colstats_plan returns 0", **_R),
]

DEFAULT_TABLE = DEFAULT_RULES + DACT + LNA + REFUSALS
BY_NAME = {c.name: c for c in PLAIN + PLAIN_F32 + DEFAULT_TABLE}


def reachable():
    """every (family, tile, ring depth, K walk, DACT / GD / LNA, lean level, store form) the dispatcher can reach outside convolutions and fp8, as
    route_str would print it with one form"""
    out = set()
    walks = [(0, 0), (1, 0), (1, 1), (1, 2)]          # (K walk, lean): the general decode has no lean form
    for form in ("wide", "narrow"):
        for tile, st in ((64, 2), (64, 4), (128, 2), (128, 4)):
            out.update(f"v2/{tile}/s{st}/k{k}/-/L{lean}/{form}" for k, lean in walks)
            out.update(f"v2/{tile}/s{st}/k1/{kind}/L0/{form}" for kind in ("DACT", "DACT+GD", "LNA", "LNA+GD"))
        for tile, st in ((128, 2), (128, 4), (256, 2)):
            out.update(f"pipe/{tile}/s{st}/k{k}/-/L{lean}/{form}" for k, lean in walks)
    out.update(f"classic/{tile}/s2/k-/-/L-/narrow" for tile in (64, 128))
    return out
