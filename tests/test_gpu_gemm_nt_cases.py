"""lavt_gemm_nt alone, one direct launch per case through ops.gemm_nt (the raw launcher), against its fp64 statement in tests/gemm_nt_cases.py.

A test builds the operands on the CPU (bf16 tensors rounded first, so both sides start from the same values), launches the one kernel and holds every
output it owns -- C, C2, Cpre, ln_mean, ln_rstd -- to the gate of gemm_nt_cases: E <= K_NT x F, E the larger of the row and the column error, F the
same error of the fp32 / bf16 floor of the case.  Every figure is printed before the test fails.  Beyond the values:
  * outputs are pre-filled with NaN, and every element the kernel does not own must come back bit-identical: the columns between N and the leading
    dimension, the columns of C at or beyond c_split, the gap between batch entries (strideC), and the rows a c_rowmap entry of -1 dropped;
  * inputs carry NaN wherever the kernel must not read: the columns beyond K / N of A, B, R, mul and dact_pre, the source rows no a_rowmap entry
    names, the rows of R, mul and dact_pre that belong to output rows nobody writes, the float in front of an offset bias -- a read there poisons
    the result;
  * a second run must be bit-identical (this family has no atomics);
  * a case the table says runs and that returns LAVT_ERR_INVALID fails (ops.gemm_nt raises); no case is skipped.

Cases (gemm_nt_cases.py states, per row, the route it is there for; test_gemm_nt_cases_host.py holds `route` to it and shows that the rows reach
every instantiation of the dispatcher outside convolutions -- gemm_nt_conv_cases.py -- and fp8):
  * PLAIN, run under all twelve settings of LAVT_GEMM_TILE 64 / 128 / 512 x LAVT_GEMM_STAGES 2 / 4 x LAVT_GEMM_PIPE 0 / 3 (seven distinct kernels:
    gemm_v2 64x64 and 128x128 with a 2- and a 4-deep ring, the pipelined 128x128 with both rings, the pipelined 256x256):
      edges  M = tile k + {1, 15, 17, 63} and M < 16; N in {8, 24, 72, 136, 328} and 132 with an fp32 output; K in {8, 56, 64, 72, 264}: the general
             decode with a K tail and exactly one tile; both weight layouts; lda, ldb, ldc wider than the rows;
      store  the switches between the 16-byte and the narrow store form, one each, beside the wide case they otherwise equal: ldc = N + 4,
             c_split = 68, ldcpre % 8 == 4, a bias pointer one float off, batch 3 with strideC % 8 == 4, batch 3 aligned (wide, no side prefetch);
      lean   the epilogue instantiations: no side input (LEAN 2), bias only / bias + R + row_scale + c_rowmap (LEAN 1), C2 alone, the language-gate
             form GELU / TANH + Cpre + mul + R (the full epilogue);
      maps   a_rowmap with -1 and repeated rows, c_rowmap with -1 and a permutation, both with row_scale_div = M // 2.
    The edges, lean and maps rows run once more in fp32 through the classic kernel, tiles 64 and 128.
  * DEFAULT_RULES: 200 tiles of 128x128 at K = 1024 (the pipelined kernel at the default LAVT_GEMM_PIPE=2) and at K = 960 (gemm_v2).
  * DACT: dact_pre with GELU / RELU / TANH, each without residual, with it, and with res_first; bias, row_scale and c_rowmap present;
    LAVT_ACT_STORED in its own instantiation and (with R) in the general one; at the four sizes whose tile counts pick the four kernels of
    the planner for dact_pre (77 x 136, 2053 x 1024, 3190 x 1024, 4217 x 1024), K = 64 and 192; plus the narrow form of each kernel (ldc = N + 4).
  * LNA: the LayerNorm-folded operand at the same sizes and K: act NONE / GELU + Cpre / LAVT_ACT_GELU_D + Cpre, statistics requested and NULL, one row
    with R + row_scale + c_rowmap, one whose rows have a mean of 10 sigma, the narrow form of each kernel.
  * REFUSALS: the combinations the header declares invalid return LAVT_ERR_INVALID, set lavt_last_error and leave the outputs untouched.

Elsewhere: the implicit-GEMM convolution modes (tap-walking K walks, LEAN 3, conv_tap_split / conv_kc_split) in test_gpu_gemm_nt_conv_cases.py, the TN
family in test_gpu_gemm_tn_cases.py.  Out of scope: fp8.

Measured E / F on MI355X, the largest over the cases of this file (gemm_nt_cases.K_NT = 2 x that, rounded up, never under 1): MEASURED below.
Every bf16 output sits at 1.000 in every case and under every forced configuration: its error IS the final bf16 rounding, and the kernel rounds the
fp32 value the floor rounds -- the fast GELU / GELU' forms of the bf16 epilogues included.  The fp32 outputs differ from the floor by the order of the
K sum: C.f32 0.525 .. 1.798 through the classic kernel (the largest at M = 65, N = 8, K = 264, the longest fp32 chain of the table), 0.844 for the fp32
output of a bf16 problem.  ln_rstd 0.514 .. 1.298.  ln_mean is exact on both sides at K = 64 (sums of 64 bf16 values are exact in fp32, 1 / 64 is a
power of two: E = F = 0) and stands at 1.45 .. 2.000 at K = 192: the kernel multiplies the row sum by the rounded reciprocal of K where the floor
divides, one more rounding of the same size.  No ratio is above 3.

What the first run of this file found: launch_nt_v2_dact refused dact_pre with a residual unless res_first was set, although the header defines
C * act'(pre) + R and both epilogue forms compute it (the rows dact-*-R-*).  The refusal is gone from the launcher; the header is unchanged there."""
import ctypes
import os

import pytest
import torch

import gemm_nt_cases as G

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
NAN = float("nan")
ENV = ("LAVT_GEMM_TILE", "LAVT_GEMM_STAGES", "LAVT_GEMM_PIPE")

# largest E / F per output over the cases of this file, as measured on MI355X (the table K_NT in gemm_nt_cases.py is derived from)
MEASURED = {"C": 1.000, "C2": 1.000, "Cpre": 1.000, "C.f32": 1.798, "C2.f32": 1.000, "Cpre.f32": 1.000, "ln_mean": 2.000, "ln_rstd": 1.298}


def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m 'not gpu' elsewhere)"
    return torch.device("cuda:0")


def _tuning(monkeypatch, request, env):
    """force (or, with an empty env, clear) the tile switches for one test; the library re-reads them now and again afterwards"""
    from lavt_hip import _capi as K
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    K.lib.lavt_tuning_reload()
    request.addfinalizer(lambda: ([os.environ.pop(k, None) for k in ENV], K.lib.lavt_tuning_reload()))


def bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _padded(t, ld, dtype, dead_rows=None):
    """[..., n] -> device rows [rows, ld] of dtype, NaN in the columns >= n and in `dead_rows`"""
    rows = t.reshape(-1, t.shape[-1])
    buf = torch.full((rows.shape[0], ld), NAN, dtype=dtype)
    buf[:, :rows.shape[1]] = rows.to(dtype)
    if dead_rows is not None:
        buf[dead_rows] = NAN
    return buf.to(dev())


class Launch:
    """the device buffers of one case and its launch"""

    def __init__(self, c):
        self.c, i = c, c.inp
        dt = self.dt = BF if c.dtype == "bf16" else torch.float32
        unused = None
        if c.a_map:
            used = torch.zeros(c.Ma, dtype=torch.bool)
            used[i["a_map"].long()[i["a_map"] >= 0]] = True
            unused = (~used).repeat(c.batch)
        self.A = _padded(i["A"], c.lda, dt, unused)
        self.B = _padded(i["W"].transpose(1, 2) if c.kmajor else i["W"], c.ldb, dt)
        self.written = torch.ones(c.Mo, dtype=torch.bool)
        if c.c_map:
            self.written[:] = False
            self.written[i["c_map"].long()[i["c_map"] >= 0]] = True
        self.bias = None
        if "bias" in i:
            b = torch.full((c.bias_off + c.batch * c.N,), NAN, dtype=torch.float32)
            b[c.bias_off:] = i["bias"].float().reshape(-1)
            self.bias = b.to(dev())[c.bias_off:]
        self.row_scale = i["row_scale"].float().contiguous().to(dev()) if c.row_scale else None
        self.ld_side = c.ld_side
        side = lambda k: _padded(i[k], self.ld_side, dt, ~self.written) if k in i else None
        self.R, self.mul, self.dact_pre = side("R"), side("mul"), side("dact_pre")
        self.a_map = i["a_map"].to(dev()) if c.a_map else None
        self.c_map = i["c_map"].to(dev()) if c.c_map else None
        self.wsum = i["wsum"].float().contiguous().to(dev()) if c.ln else None
        self.out_dt = torch.float32 if (c.c_f32 or c.dtype == "f32") else BF

    def outputs(self):
        c = self.c
        o = {"C": torch.full(((c.batch - 1) * c.strideC + c.Mo * c.ldc,), NAN, dtype=self.out_dt, device=dev())}
        if c.c_split:
            o["C2"] = torch.full((c.Mo, c.ldc2), NAN, dtype=self.out_dt, device=dev())
        if c.cpre:
            o["Cpre"] = torch.full((c.Mo, c.ldcpre), NAN, dtype=self.dt, device=dev())
        if c.ln and c.ln_stats:
            o["ln_mean"], o["ln_rstd"] = (torch.full((c.M,), NAN, dtype=torch.float32, device=dev()) for _ in range(2))
        return o

    def run(self):
        from lavt_hip import ops
        o = self.outputs()
        args, kw = G.launch_args(self.c, dict(o, A=self.A, B=self.B, bias=self.bias, row_scale=self.row_scale, R=self.R, mul=self.mul, dact_pre=self.dact_pre,
                                              a_map=self.a_map, c_map=self.c_map, wsum=self.wsum))
        ops.gemm_nt(*args, **kw)
        torch.cuda.synchronize()
        return o

    def owned(self):
        """name -> bool mask over the flat output buffer: the elements the kernel owns"""
        c = self.c
        m = {"C": torch.zeros((c.batch - 1) * c.strideC + c.Mo * c.ldc, dtype=torch.bool)}
        for b in range(c.batch):
            v = m["C"][b * c.strideC:b * c.strideC + c.Mo * c.ldc].view(c.Mo, c.ldc)
            v[self.written, :c.Nc] = True
        for name, ld, n in (("C2", c.ldc2, c.N - c.c_split), ("Cpre", c.ldcpre, c.N)):
            m[name] = torch.zeros(c.Mo, ld, dtype=torch.bool)
            m[name][self.written, :n] = True
            m[name] = m[name].reshape(-1)
        m["ln_mean"] = m["ln_rstd"] = torch.ones(c.M, dtype=torch.bool)
        return m

    def extract(self, o):
        """the buffers as the reference shapes them (float, CPU)"""
        c = self.c
        got = {"C": torch.stack([o["C"][b * c.strideC:b * c.strideC + c.Mo * c.ldc].view(c.Mo, c.ldc)[:, :c.Nc] for b in range(c.batch)]).float().cpu()}
        if "C2" in o:
            got["C2"] = o["C2"][:, :c.N - c.c_split].float().cpu()
        if "Cpre" in o:
            got["Cpre"] = o["Cpre"][:, :c.N].float().cpu()
        for k in ("ln_mean", "ln_rstd"):
            if k in o:
                got[k] = o[k].float().cpu()
        return got


_REFS = {}


def refs(c):
    """(reference, floor) of a case; kept for the small cases, which run under every forced configuration"""
    if c.name in _REFS:
        return _REFS[c.name]
    r = (G.reference(c), G.floor(c))
    if c.M * c.N * c.batch <= 1 << 18:
        _REFS[c.name] = r
    return r


def check_case(c, tag=""):
    """launch twice, hold the untouched elements and the second run bit-identical, print every figure, then fail on every output that misses the gate"""
    L = Launch(c)
    a = L.run()
    b = L.run()
    ref, flo = refs(c)
    assert set(a) == set(ref), (set(a), set(ref))
    owned = L.owned()
    for k in a:
        assert torch.equal(bits(a[k]), bits(b[k])), f"{c.name} {k}: second run is not bit-identical"
        fresh = bits(torch.full_like(a[k], NAN)).cpu().reshape(-1)
        rest = ~owned[k]
        assert torch.equal(bits(a[k]).cpu().reshape(-1)[rest], fresh[rest]), f"{c.name} {k}: an element the kernel does not own was written"
    got = L.extract(a)
    fails = []
    for k in sorted(ref):
        key = c.store_key(k)
        E, Fl, ok = G.gate(key, got[k].reshape(ref[k].shape), ref[k], flo[k], report=True)
        ratio = E / Fl if Fl > 0 else (0.0 if E == 0 else float("inf"))
        print(f"[gemm-nt] {c.name} {tag} {key}: E {E:.3e} F {Fl:.3e} E/F {ratio:.3f} K {G.K_NT[key]:g}")
        if not ok:
            fails.append((k, E, Fl, ratio))
    assert not fails, (c.name, tag, fails)


# ------------------------------------------------------------------------------------------------ forced configurations
@pytest.mark.parametrize("group", list(G.GROUPS))
@pytest.mark.parametrize("tuning", list(G.TUNINGS))
def test_plain_bf16(tuning, group, monkeypatch, request):
    """the plain rows of the table under one forced (tile, ring depth, pipelined K loop) setting"""
    _tuning(monkeypatch, request, G.tuning_env(tuning))
    for c in G.GROUPS[group]:
        check_case(c, tuning)


@pytest.mark.parametrize("group", ["edges", "lean", "maps"])
@pytest.mark.parametrize("tuning", list(G.TUNINGS_F32))
def test_plain_f32(tuning, group, monkeypatch, request):
    """the same rows in fp32: the classic kernel with tiles 64 and 128"""
    _tuning(monkeypatch, request, G.tuning_env(tuning))
    for c in G.GROUPS[group]:
        check_case(G.BY_NAME[c.name + "-f32"], tuning)


# ------------------------------------------------------------------------------------------------ the dispatcher's own rules
@pytest.mark.parametrize("case", G.DEFAULT_RULES, ids=repr)
def test_default_rules(case, monkeypatch, request):
    _tuning(monkeypatch, request, {})
    check_case(case)


@pytest.mark.parametrize("case", G.DACT, ids=repr)
def test_dact(case, monkeypatch, request):
    """the fused activation gradient; the sizes pick all four kernels of its kind, whose tile rule ignores the forced tile"""
    _tuning(monkeypatch, request, {})
    check_case(case)


@pytest.mark.parametrize("case", G.LNA, ids=repr)
def test_lna(case, monkeypatch, request):
    """the LayerNorm-folded A operand; the sizes pick all four kernels of its kind"""
    _tuning(monkeypatch, request, {})
    check_case(case)


# ------------------------------------------------------------------------------------------------ contract refusals
@pytest.mark.parametrize("case", G.REFUSALS, ids=repr)
def test_refusals(case, monkeypatch, request):
    """argument checks in host code: LAVT_ERR_INVALID, lavt_last_error set, the NaN-filled outputs untouched, nothing launched"""
    from lavt_hip import _capi as K, ops
    _tuning(monkeypatch, request, {})
    L = Launch(case)
    if not case.colstats:
        seen = {}
        orig = L.outputs

        def keep():
            seen.update(orig())
            return seen
        L.outputs = keep
        with pytest.raises(RuntimeError, match=r"rc=-22: \S+"):
            L.run()
        torch.cuda.synchronize()
        outs = seen
    else:
        # ops.gemm_nt asks lavt_gemm_nt_colstats_plan first and leaves colstats NULL where it refuses: set the pointer by hand
        c, outs = case, L.outputs()
        stats = torch.full((2 * 2 * c.N,), NAN, dtype=torch.float32, device=dev())
        outs["colstats"] = stats
        p = K.GemmNT()
        p.dtype, p.M, p.N, p.K, p.batch = K.dt(L.dt), c.M, c.N, c.K, 1
        p.A, p.lda, p.B, p.ldb, p.alpha = K.ptr(L.A), c.lda, K.ptr(L.B), c.ldb, c.alpha
        p.C, p.ldc, p.zeros, p.colstats = K.ptr(outs["C"]), c.ldc, ops._zero_page(dev()), K.ptr(stats)
        rpb = ctypes.c_int32(-1)
        assert int(K.lib.lavt_gemm_nt_colstats_plan(ctypes.byref(p), ctypes.byref(rpb))) == 0 and rpb.value == 0
        rc = int(K.lib.lavt_gemm_nt(ctypes.byref(p), K.stream()))
        torch.cuda.synchronize()
        assert rc == -22 and b"colstats" in K.lib.lavt_last_error()          # LAVT_ERR_INVALID
    assert outs
    for k, t in outs.items():
        assert torch.equal(bits(t), bits(torch.full_like(t, NAN))), f"{case.name}: {k} was written by a refused launch"
