"""The library's NT planner, lavt_gemm_nt_route (csrc/gemm_nt_plan.hip), against its Python restatement (tests/gemm_nt_cases.py), CPU only.

test_gemm_nt_cases_host.py holds every row of the case table to the route it states and shows that the table reaches every instantiation -- Python
against Python.  This file closes the loop: the lavt_gemm_nt_t of a row is filled by the helper the GPU test launches through (gemm_nt_cases.launch_args
-> lavt_hip.ops.gemm_nt_params) with made-up, non-null, 16-byte aligned addresses, and the library's own answer must equal `route()` field by field.
The planner never reads through an address; no struct of this file is ever passed to lavt_gemm_nt.

  * route comparison: PLAIN under every TUNINGS entry and the default tuning, PLAIN_F32 under TUNINGS_F32 and the default, DEFAULT_TABLE under the
    default: family, tile, ring depth, K-walk mode, kind, lean level and epi_wide; LAVT_ERR_INVALID exactly where route() says INVALID.  `forms` and
    `prefetch` of the Python Route are decided inside the kernel (per wave span, from epi_wide and the column range) and stay outside the comparison.
  * refusals: lavt_last_error names the feature the row is refused for.
  * lavt_gemm_nt_colstats_plan equals colstats_plan() for the same rows.
  * the convolution table (tests/gemm_nt_conv_cases.py): every (row, forced configuration) field by field, as for PLAIN; its refusals name the feature.
  * ROWS: fp8 (which route() does not restate), the benchmark's convolutions, the 2 GB descriptor bound and the thresholds' boundaries, written by hand
    from the rules, the route stated per row; every row but the fp8 ones must equal route() too.
  * forced configurations: the LayerNorm-folded and the activation-gradient rows (and gemm_v2's fp8 form) ignore LAVT_GEMM_TILE / LAVT_GEMM_STAGES
    and have no long-K clause; pinned here as today's behaviour."""
import ctypes
import types

import pytest
import torch

import gemm_nt_cases as G
import gemm_nt_conv_cases as V

ENV = ("LAVT_GEMM_TILE", "LAVT_GEMM_STAGES", "LAVT_GEMM_PIPE")
BF, F8 = torch.bfloat16, torch.uint8
FAMILY = {0: "classic", 1: "v2", 2: "pipe"}
GENERAL, PLAIN, TAPS, PARTIAL = 0, 1, 2, 3


def _capi():
    from lavt_hip import _capi as K, ops
    return K, ops


@pytest.fixture
def tuning(monkeypatch, request):
    """set(env): force (or, with {}, clear) the tile switches; the library re-reads them now, and again once the environment is back as it was"""
    K, _ = _capi()

    def set_(env):
        for k in ENV:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, str(v))
        K.lib.lavt_tuning_reload()
    request.addfinalizer(lambda: (monkeypatch.undo(), K.lib.lavt_tuning_reload()))
    return set_


class Addresses:
    """made-up device addresses: non-null, 16-byte aligned, 256 MB apart"""

    def __init__(self):
        self.n = 0

    def __call__(self):
        self.n += 1
        return 0x100000000 + self.n * 0x10000000


def case_params(c):
    """the lavt_gemm_nt_t of a table row, through the helper the GPU test launches with"""
    K, ops = _capi()
    new = Addresses()
    buf = dict(A=new(), B=new(), C=new())
    have = dict(C2=c.c_split, Cpre=c.cpre, row_scale=c.row_scale, R=c.R, mul=c.mul, dact_pre=c.dact is not None, a_map=c.a_map, c_map=c.c_map, wsum=c.ln,
                ln_mean=c.ln and c.ln_stats, ln_rstd=c.ln and c.ln_stats)
    buf.update({k: new() for k, v in have.items() if v})
    if c.bias:
        buf["bias"] = new() + 4 * c.bias_off
    args, kw = G.launch_args(c, buf)
    p = ops.gemm_nt_params(*args, **kw, addr=lambda a: a, zeros=new())
    if c.colstats:
        p.colstats = new()
    return p


def ask(p):
    """-> (rc, route struct, colstats blocks, rows per block)"""
    K, _ = _capi()
    r, rpb = K.GemmNTRoute(), ctypes.c_int32(-1)
    rc = int(K.lib.lavt_gemm_nt_route(ctypes.byref(p), ctypes.byref(r)))
    nblk = int(K.lib.lavt_gemm_nt_colstats_plan(ctypes.byref(p), ctypes.byref(rpb)))
    return rc, r, nblk, rpb.value


def fields(r):
    """the compared fields of a library route, in the vocabulary of gemm_nt_cases.Route"""
    K, _ = _capi()
    fam = FAMILY[r.family]
    kind = "+".join(n for b, n in ((K.NT_DACT, "DACT"), (K.NT_LNA, "LNA"), (K.NT_F8, "F8"), (K.NT_GD, "GD")) if r.kind & b)
    classic = fam == "classic"          # (no K-walk modes, no lean forms: the Python Route says None)
    return fam, r.tile, r.stages, None if classic else r.kwalk, kind, None if classic else r.lean, r.epi_wide


def compare(cases, t):
    bad = []
    for c in cases:
        want = G.route(c, t)
        rc, r, nblk, rpb = ask(case_params(c))
        if want == G.INVALID:
            if rc != -22:
                bad.append((c.name, "INVALID", rc, fields(r)))
            continue
        exp = (want.family, want.tile, want.stages, want.kmode, want.kind, want.lean, G.epi_wide(c))
        waves = 8 if want.family == "pipe" or (want.family == "v2" and want.tile == 128) else 4
        if rc != 0 or fields(r) != exp or r.waves != waves or r.b_kmajor != int(c.kmajor) or r.dtype != (1 if c.dtype == "bf16" else 0):
            bad.append((c.name, exp, rc, fields(r), r.waves, r.b_kmajor))
        pt = G.pipe_tile(c, dict(G.DEFAULT, **t))
        blocks = G.colstats_plan(c, dict(G.DEFAULT, **t))
        if (nblk, rpb) != (blocks, pt[0] // 2 if blocks else 0):
            bad.append((c.name, "colstats", blocks, nblk, rpb))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ the table's rows
@pytest.mark.parametrize("name", [None] + list(G.TUNINGS))
def test_plain_rows_route_as_restated(name, tuning):
    tuning(G.tuning_env(name) if name else {})
    compare(G.PLAIN, G.tuning_dict(name) if name else {})


@pytest.mark.parametrize("name", [None] + list(G.TUNINGS_F32))
def test_plain_f32_rows_route_as_restated(name, tuning):
    tuning(G.tuning_env(name) if name else {})
    compare(G.PLAIN_F32, G.tuning_dict(name) if name else {})


def test_default_table_routes_as_restated(tuning):
    tuning({})
    compare(G.DEFAULT_TABLE, {})


REFUSAL_WORDS = {"refuse-gelud-without-ln": "LAVT_ACT_GELU_D", "refuse-resfirst-without-dact": "res_first", "refuse-dact-k72": "dact_pre", "refuse-dact-kcontiguous": "dact_pre",
                 "refuse-ln-f32": "ln_wsum", "refuse-ln-alpha": "ln_wsum", "refuse-ln-nobias": "ln_wsum", "refuse-colstats": "colstats"}


@pytest.mark.parametrize("case", G.REFUSALS, ids=repr)
def test_refusals_say_why(case, tuning):
    """the GPU refusal tests want rc = -22 with a non-empty message, and "colstats" in the colstats row's; each message names its feature"""
    K, _ = _capi()
    tuning({})
    rc, _, _, _ = ask(case_params(case))          # (the colstats query inside ask() sets no error: the message is the route's)
    msg = K.lib.lavt_last_error().decode()
    assert rc == -22 and msg.startswith("lavt_gemm_nt") and REFUSAL_WORDS[case.name] in msg, (rc, msg)


def test_forced_configurations_do_not_reach_lna_and_dact(tuning):
    """today's behaviour, pinned: under every forced (tile, ring depth, pipe) setting the LayerNorm-folded and the activation-gradient rows take the
    route the table states for the default tuning"""
    for name in G.TUNINGS:
        tuning(G.tuning_env(name))
        for c in G.DACT + G.LNA:
            rc, r, _, _ = ask(case_params(c))
            f = fields(r)
            assert rc == 0 and G.route_str(G.route(c, G.tuning_dict(name))).rsplit("/", 1)[0] == c.route.rsplit("/", 1)[0], (name, c.name)
            assert f"{f[0]}/{f[1]}/s{f[2]}/k{f[3]}/{f[4]}/L{f[5]}" == c.route.rsplit("/", 1)[0], (name, c.name, f, c.route)


# ------------------------------------------------------------------------------------------------ the convolution table
def conv_params(c):
    """the lavt_gemm_nt_t of a convolution row, through the helper the GPU test launches with"""
    K, ops = _capi()
    new = Addresses()
    buf = dict(A_big=new(), B=new(), C=new())
    buf.update({k: new() for k, v in dict(A2=c.C2, C2=c.c_split, Cpre=c.cpre, bias=c.bias).items() if v})
    args, kw = V.launch_args(c, buf)
    p = ops.gemm_nt_params(*args, **kw, addr=lambda a: a, zeros=new())
    if c.colstats:
        p.colstats = new()
    return p


def _conv_tuning(c, name, tuning):
    env = G.tuning_env(name) if name else {}
    tuning(dict(env, **(c.env or {})))
    t = G.tuning_dict(name) if name else {}
    return dict(t, pipe=int(c.env["LAVT_GEMM_PIPE"])) if c.env else t


@pytest.mark.parametrize("name", [None] + sorted({t for _, t in V.launches() if t}))
def test_conv_rows_route_as_restated(name, tuning):
    """every row of the convolution table that runs under this configuration; under the default tuning, every row"""
    rows = [c for c, t in V.launches() if t == name] if name else V.TABLE
    assert rows
    bad = []
    for c in rows:
        t = _conv_tuning(c, name, tuning)
        want = G.route(c, t)
        rc, r, nblk, rpb = ask(conv_params(c))
        if want == G.INVALID:          # (the colstats rows at the default tuning: 64x64 tiles have no statistics epilogue)
            if rc != -22:
                bad.append((c.name, "INVALID", rc, fields(r)))
            continue
        exp = (want.family, want.tile, want.stages, want.kmode, want.kind, want.lean, G.epi_wide(c))
        waves = 8 if want.family == "pipe" or (want.family == "v2" and want.tile == 128) else 4
        if rc != 0 or fields(r) != exp or r.waves != waves or r.b_kmajor != int(c.kmajor) or r.dtype != (1 if c.dtype == "bf16" else 0):
            bad.append((c.name, exp, rc, fields(r), r.waves, r.b_kmajor))
        blocks = G.colstats_plan(c, dict(G.DEFAULT, **t))
        if (nblk, rpb) != (blocks, G.pipe_tile(c, dict(G.DEFAULT, **t))[0] // 2 if blocks else 0):
            bad.append((c.name, "colstats", blocks, nblk, rpb))
        if name and V.route_key(c, want) != V.stated_route(c, name):
            bad.append((c.name, "stated", V.route_key(c, want), V.stated_route(c, name)))
    assert not bad, bad


@pytest.mark.parametrize("case", V.REFUSALS, ids=repr)
def test_conv_refusals_say_why(case, tuning):
    K, _ = _capi()
    t = _conv_tuning(case, None, tuning)
    assert G.route(case, t) == G.INVALID
    rc, _, _, _ = ask(conv_params(case))
    msg = K.lib.lavt_last_error().decode()
    assert rc == -22 and msg.startswith("lavt_gemm_nt") and case.word in msg, (rc, msg)


# ------------------------------------------------------------------------------------------------ rows written by hand
# Written by hand from the rules (the comment block of csrc/gemm_nt_plan.hip); per row the tile counts that decide it.
#   t128 / t64 / t256 = tiles of that size x batch.  128x128 tile: t128 >= 200, or K >= 4096 and t128 >= 128 (N >= 128); ring of 2 from 257 / 512
#   workgroups.  pipe: 256x256 where N fits, K >= 1024, t256 >= 128 and the last round of 256 is >= 80 % full; else the 128x128 tile with K >= 1024.
def conv_fwd(B, H, W, C1, C2, Cout, dtype=BF, **kw):
    """3x3 forward, weight-major [Cout][9][Cin], the concat of two sources as A / A2"""
    Cin = C1 + C2
    k = dict(conv=(H, W, Cin, 0), **kw)
    if C2:
        k.update(A2=True, lda2=C2, a_split=C1)
    return (dtype, B * H * W, Cout, 9 * Cin, C1, 9 * Cin, Cout), k


def conv_dgrad(B, H, W, C1, C2, Cout):
    """3x3 data gradient, the same packed weight read k-major, columns >= C1 into the second source's gradient"""
    Cin = C1 + C2
    return (BF, B * H * W, Cin, 9 * Cout, Cout, 9 * Cin, C1), dict(conv=(H, W, Cout, 1), b_kmajor=True, b_tap_stride=Cin, C2=True, ldc2=C2, c_split=C1)


def plain(M, N, Kd, dtype=BF, **kw):
    return (dtype, M, N, Kd, Kd, Kd, N), kw


def R(family, tile, stages, kwalk, kind="", lean=0, wide=3):
    return family, tile, stages, kwalk, kind, lean, wide


_SPLIT = dict(c_f32=True, strideC=1800 * 512)
ROWS = [
    # ---- the decoder's 3x3 convolutions of the benchmark workload (Swin-B, 480 x 480, batch 2): 1536 -> 512 at 30 x 30, 768 -> 512 at 60 x 60, 640 -> 512 at 120 x 120
    ("fwd-120", conv_fwd(2, 120, 120, 512, 128, 512), {}, R("pipe", 256, 2, TAPS, lean=2)),              # t256 = 113 x 2 = 226: one round, 88 % full
    ("fwd-60", conv_fwd(2, 60, 60, 512, 256, 512), {}, R("pipe", 128, 4, TAPS, lean=2)),                 # t256 = 58; t128 = 57 x 4 = 228 < 257
    ("fwd-30", conv_fwd(2, 30, 30, 1024, 512, 512), {}, R("v2", 64, 4, TAPS, lean=2)),                   # t128 = 60 (< 128 even for K = 13824); t64 = 29 x 8 = 232
    ("dgrad-120", conv_dgrad(2, 120, 120, 512, 128, 512), {}, R("pipe", 128, 2, TAPS)),                  # N = 640 fits no 256-wide tile; t128 = 225 x 5; C2: full epilogue
    ("dgrad-60", conv_dgrad(2, 60, 60, 512, 256, 512), {}, R("pipe", 128, 2, TAPS)),                     # t256 = 29 x 3 = 87; t128 = 57 x 6 = 342
    ("dgrad-30", conv_dgrad(2, 30, 30, 1024, 512, 512), {}, R("pipe", 128, 4, TAPS)),                    # t128 = 15 x 12 = 180 with K = 4608: the long-K clause
    ("dgrad-120-swin-t", conv_dgrad(2, 120, 120, 384, 96, 384), {}, R("pipe", 256, 2, TAPS, lean=3)),    # N = 480 within 1/16 of 512: t256 = 226; the store with C2 kept
    # ---- split reductions (fp32 partial outputs over the batch index: narrow stores)
    ("kc-split", conv_fwd(2, 30, 30, 1024, 512, 512, batch=4, conv_kc_split=384, Kd=9 * 384, **_SPLIT), {}, R("pipe", 128, 4, TAPS, lean=2, wide=0)),
    ("tap-split", conv_fwd(2, 30, 30, 512, 0, 512, batch=3, conv_tap_split=3, Kd=3 * 512, strideB=3 * 512, **_SPLIT), {}, R("v2", 64, 2, TAPS, lean=2, wide=0)),      # t128 = 180, K = 1536; t64 = 696
    # ---- Cin % 64 != 0 (Swin-T's conv1_2: 384 + 96 -> 384): the partial-block walk of the pipelined family; k-major weights and gemm_v2 decode it
    ("partial", conv_fwd(2, 120, 120, 384, 96, 384), {}, R("pipe", 128, 2, PARTIAL, lean=2)),           # N = 384 fits no 256-wide tile; t128 = 225 x 3
    ("partial-v2", conv_fwd(2, 120, 120, 384, 96, 384), dict(pipe=0), R("v2", 128, 2, GENERAL)),
    # ---- an operand beyond the 2 GB descriptor bound (rows of a 32768-element buffer): the pipelined family falls to the general walk, gemm_v2 (64-bit pointers) does not
    ("2gb", conv_fwd(2, 120, 120, 512, 0, 512, lda=32768), {}, R("pipe", 256, 2, GENERAL)),
    ("2gb-v2", conv_fwd(2, 120, 120, 512, 0, 512, lda=32768), dict(pipe=0), R("v2", 128, 2, TAPS, lean=2)),
    # ---- fp8 (K tile of 128 elements).  The pipelined family has the plain and the tap walk only; anything else is gemm_v2's, which has no lean form
    ("f8-pipe-plain", plain(28800, 512, 1024, F8), {}, R("pipe", 256, 2, PLAIN, "F8", 2)),
    ("f8-pipe-taps", conv_fwd(2, 120, 120, 512, 0, 512, F8), {}, R("pipe", 256, 2, TAPS, "F8", 2)),
    ("f8-pipe-bias", plain(7200, 512, 1024, F8, bias=True), {}, R("pipe", 128, 4, PLAIN, "F8", 1)),
    ("f8-general", conv_fwd(2, 120, 120, 576, 0, 512, F8), {}, R("v2", 128, 2, GENERAL, "F8")),          # conv_kc % 128 != 0; t128 = 900
    ("f8-k-tail", plain(28800, 512, 1040, F8), {}, R("v2", 128, 2, GENERAL, "F8")),                      # K % 128 != 0
    ("f8-v2-plain", plain(1800, 512, 1024, F8), {}, R("v2", 64, 4, PLAIN, "F8")),                        # t128 = 60, t64 = 232
    ("f8-v2-taps", conv_fwd(2, 30, 30, 512, 0, 512, F8), {}, R("v2", 64, 4, TAPS, "F8")),
    ("f8-2gb", conv_fwd(2, 120, 120, 512, 0, 512, F8, lda=65536), {}, R("v2", 128, 2, TAPS, "F8")),      # beyond the bound the pipelined family refuses fp8; gemm_v2 walks the taps
    # today's behaviour, pinned: gemm_v2's fp8 form ignores the forced tile / ring and has no long-K clause (bf16: the same shape takes 128 / s4, and 64 / s4 forced)
    ("f8-long-k", plain(1800, 1536, 4608, F8), dict(pipe=0), R("v2", 64, 2, PLAIN, "F8")),               # t128 = 180 < 200; t64 = 29 x 24 = 696
    ("bf16-long-k", plain(1800, 1536, 4608), dict(pipe=0), R("v2", 128, 4, PLAIN, lean=2)),
    ("f8-forced", plain(1800, 1536, 4608, F8), dict(pipe=0, tile=128, stages=4), R("v2", 64, 2, PLAIN, "F8")),
    ("bf16-forced", plain(28800, 512, 1024), dict(pipe=0, tile=64, stages=4), R("v2", 64, 4, PLAIN, lean=2)),
    # ---- the thresholds, one row on either side
    ("t128-199", plain(199 * 128, 128, 64), {}, R("v2", 64, 2, PLAIN, lean=2)),                          # t64 = 796
    ("t128-200", plain(200 * 128, 128, 64), {}, R("v2", 128, 4, PLAIN, lean=2)),
    ("s2-256", plain(256 * 128, 128, 64), {}, R("v2", 128, 4, PLAIN, lean=2)),
    ("s2-257", plain(257 * 128, 128, 64), {}, R("v2", 128, 2, PLAIN, lean=2)),
    ("t64-511", plain(511 * 64, 64, 64), {}, R("v2", 64, 4, PLAIN, lean=2)),
    ("t64-512", plain(512 * 64, 64, 64), {}, R("v2", 64, 2, PLAIN, lean=2)),
    ("pipe-k1016", plain(200 * 128, 128, 1016), {}, R("v2", 128, 4, GENERAL)),
    ("pipe-k1024", plain(200 * 128, 128, 1024), {}, R("pipe", 128, 4, PLAIN, lean=2)),
    ("long-k-127", plain(127 * 128, 128, 4096), {}, R("v2", 64, 4, PLAIN, lean=2)),                      # t64 = 254 x 2 = 508
    ("long-k-128", plain(128 * 128, 128, 4096), {}, R("pipe", 128, 4, PLAIN, lean=2)),
    ("long-k-4032", plain(128 * 128, 128, 4032), {}, R("v2", 64, 2, PLAIN, lean=2)),                     # t64 = 512
    ("t256-204", plain(204 * 256, 256, 1024), {}, R("pipe", 128, 2, PLAIN, lean=2)),                     # 204 of 256: under 80 %
    ("t256-205", plain(205 * 256, 256, 1024), {}, R("pipe", 256, 2, PLAIN, lean=2)),
    ("t256-k1016", plain(205 * 256, 256, 1016), {}, R("v2", 128, 2, GENERAL)),
    ("classic-767", plain(767 * 128, 128, 64, torch.float32), {}, R("classic", 64, 2, None, lean=None, wide=0)),
    ("classic-768", plain(768 * 128, 128, 64, torch.float32), {}, R("classic", 128, 2, None, lean=None, wide=0)),
]


def row_params(args, kw):
    K, ops = _capi()
    new = Addresses()
    dtype, M, N, Kd, lda, ldb, ldc = args
    kw = dict(kw)
    lda, Kd = kw.pop("lda", lda), kw.pop("Kd", Kd)          # (a column block of a wider buffer; the K of one piece of a split reduction)
    for k in ("A2", "C2", "bias"):
        if kw.get(k):
            kw[k] = new()
    if dtype == F8:
        kw["deq"] = (new(), new())
    return ops.gemm_nt_params(dtype, M, N, Kd, new(), lda, new(), ldb, new(), ldc, **kw, addr=lambda a: a, zeros=new())


def row_case(args, kw):
    """a hand-written row as route() reads a case (no fp8)"""
    dtype, M, N, Kd, lda, ldb, ldc = args
    kw = dict(kw)
    lda, Kd = kw.pop("lda", lda), kw.pop("Kd", Kd)
    H, W, kc, flip = kw.get("conv", (0, 0, 0, 0))
    c = types.SimpleNamespace(
        dtype="bf16" if dtype == BF else "f32", es=8 if dtype == BF else 4, M=M, N=N, K=Kd, batch=kw.get("batch", 1), lda=lda, ldb=ldb, ldc=ldc, kmajor=bool(kw.get("b_kmajor")),
        C2src=bool(kw.get("A2")), lda2=kw.get("lda2", 0), a_split=kw.get("a_split", 0), conv_kc=kc, conv_h=H, conv_w=W, taps=9, vox=max(H * W, 1),
        conv_tap_split=kw.get("conv_tap_split", 0), conv_kc_split=kw.get("conv_kc_split", 0), strideB=kw.get("strideB", 0), strideC=kw.get("strideC", 0),
        c_split=kw.get("c_split", 0) if kw.get("C2") else 0, ldc2=kw.get("ldc2", 0), c_f32=bool(kw.get("c_f32")), bias=bool(kw.get("bias")), bias_off=0, act=0, cpre=False,
        ldcpre=0, mul=False, R=False, row_scale=False, c_map=False, a_map=False, ln=False, dact=None, res_first=False, colstats=False, alpha=1.0)
    return c


@pytest.mark.parametrize("name,call,t,want", ROWS, ids=[r[0] for r in ROWS])
def test_hand_written_rows(name, call, t, want, tuning):
    full = dict(G.DEFAULT, **t)
    tuning({} if not t else {"LAVT_GEMM_TILE": full["tile"], "LAVT_GEMM_STAGES": full["stages"], "LAVT_GEMM_PIPE": full["pipe"]})
    rc, r, _, _ = ask(row_params(*call))
    K, _ = _capi()
    assert rc == 0, K.lib.lavt_last_error()
    assert fields(r) == want, (name, fields(r), want)
    if call[0][0] != F8:          # route() restates everything but fp8
        c = row_case(*call)
        got = G.route(c, full)
        assert got != G.INVALID and (got.family, got.tile, got.stages, got.kmode, got.kind, got.lean, G.epi_wide(c)) == want, (name, got, want)
