"""The library's TN planner, lavt_gemm_tn_route / lavt_gemm_tn_group_route (csrc/gemm_tn_plan.hip), against its Python restatement
(tests/gemm_tn_cases.py), CPU only.

test_gemm_tn_cases_host.py holds every row of the case table to the route it states -- Python against Python.  This file closes the loop: the
lavt_gemm_tn_t of a row is filled by the helper the GPU test launches through (gemm_tn_cases.launch_args -> lavt_hip.ops.gemm_tn_params) with made-up,
non-null, 16-byte aligned addresses, and the library's own answer, rendered in the vocabulary of `tn_route`, must equal it.  The planner never reads
through an address; no struct of this file is ever passed to a launching entry.

  * single problems: SINGLES + REFUSALS under the row's own tuning (equal to `tn_route` and to the stated route) and under the default tuning;
    LAVT_ERR_INVALID exactly where `tn_route` says INVALID, lavt_last_error naming lavt_gemm_tn.
  * groups: GROUPS + SK_REFUSED under their tuning: launch, ring depth, per-member pieces, parts, K loop, column-sum form, rider and the stream-K
    workgroups; beyond the route string: the workgroup count, the reducer (against `launches`), the rider's units; lavt_gemm_tn_grouped_sk_ws equals
    the route's scratch floats and `sk_plan`.
  * lavt_gemm_tn_pieces and lavt_gemm_tn_v2_eligible equal Case.pieces_bound and v2_eligible for every member.
  * SINGLE_ROWS / GROUP_ROWS: both sides of every threshold, written by hand from the rules (the comment block of csrc/gemm_tn_plan.hip) with the
    route stated per row; every row must equal `tn_route` too.  Nothing is allocated, so a row is as large as its rule requires."""
import ctypes
import re

import pytest

import gemm_tn_cases as G
from gemm_tn_cases import Case, Group, cdiv, conv

ENV = tuple(G.ENV.values())


def _capi():
    from lavt_hip import _capi as K, ops
    return K, ops


@pytest.fixture
def tuning(monkeypatch, request):
    """set(t): force the planner switches of a tuning dict (gemm_tn_cases.ENV; {}: the defaults); the library re-reads them now, and again once the
    environment is back as it was"""
    K, _ = _capi()

    def set_(t):
        for k in ENV:
            monkeypatch.delenv(k, raising=False)
        for k, v in G.tuning_env(t).items():
            monkeypatch.setenv(k, v)
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


def params(c, new, colsum=None):
    """the lavt_gemm_tn_t of a case, through the helper the GPU test launches with"""
    _, ops = _capi()
    buf = dict(A=new(), B=new(), C=new())
    have = dict(B2=c.b2, a_map=c.a_map, b_map=c.b_map, scale=c.scale, parts=c.partials is not None)
    buf.update({k: new() for k, v in have.items() if v})
    if c.colsum:
        buf["colsum"] = colsum or new()
    args, kw, finish = G.launch_args(c, buf)
    return finish(ops.gemm_tn_params(*args, **kw, addr=lambda a: a, zeros=new()), lambda a: a)


def group_params(g):
    K, _ = _capi()
    new, ps = Addresses(), []
    for c in g.members:
        ps.append(params(c, new, colsum=ps[c.share].colsum if c.share is not None else None))
    return (K.GemmTN * len(ps))(*ps), len(ps)


def last_error():
    K, _ = _capi()
    return K.lib.lavt_last_error().decode()


# ------------------------------------------------------------------------------------------------ single problems
def single_route(c):
    """the library's route of a case in the vocabulary of gemm_tn_cases.route_single"""
    K, _ = _capi()
    r = K.GemmTNRoute()
    rc = int(K.lib.lavt_gemm_tn_route(ctypes.byref(params(c, Addresses())), ctypes.byref(r)))
    if rc != 0:
        assert rc == -22 and last_error().startswith("lavt_gemm_tn"), (c.name, rc, last_error())
        return G.INVALID
    assert r.dtype == (0 if c.dtype == "f32" else 1) and r.pieces * r.kt_per_piece >= cdiv(c.K, 16 if c.dtype == "f32" else 64) > (r.pieces - 1) * r.kt_per_piece, c.name
    if r.family == K.TN_CLASSIC:
        assert (r.waves, r.write, r.maps, r.colsum_form, r.convp) == (4, K.TN_ATOMIC, 0, 0, 0), c.name
        return f"classic/{c.dtype}/{r.tile}/p{r.pieces}"
    assert r.family == K.TN_V2 and r.waves == (8 if r.tile == 128 else 4), c.name
    form = {K.TN_STORE: "store", K.TN_ATOMIC: "atomic", K.TN_PARTS: "parts"}[r.write]
    return f"v2/{r.tile}/{'maps' if r.maps else 'plain'}/cs{r.colsum_form}/{'convp' if r.convp else 'lin'}/p{r.pieces}/{form}"


def compare_singles(rows, tuning, own):
    bad = []
    for c in rows:
        t = c.tuning if own else {}
        tuning(t)
        got, want = single_route(c), G.tn_route(c, t)
        if got != want or (own and got != c.route):
            bad.append((c.name, got, want, c.route))
    assert not bad, bad


@pytest.mark.parametrize("own", [True, False], ids=["own-tuning", "default-tuning"])
def test_single_rows_route_as_restated(own, tuning):
    compare_singles(G.SINGLES + G.REFUSALS, tuning, own)


def test_refusals_name_the_entry(tuning):
    tuning({})
    for c in G.REFUSALS:
        assert single_route(c) == G.INVALID == G.tn_route(c), c.name


# ------------------------------------------------------------------------------------------------ groups
def parse(route, n):
    """a `tn_route` string of a group as the compared fields"""
    base, offered, rider = route.partition("+ln")
    f = dict(rider=("none", 0) if not offered else (("rides", int(rider)) if rider.isdigit() else ("after", 0)))
    p = base.split("/")
    f["launch"] = p[0]
    if p[0] == "sk":
        f.update(maps=p[1] == "maps", cs=int(p[2][2:]), nw=int(p[3][2:]), pieces=[1] * n, parts=False)
    elif p[0] == "group64":
        f.update(maps=p[1] == "maps", cs=int(p[2][2:]), pieces=[int(s) for s in p[3][2:].split(",")], parts=p[-1] == "parts")
    elif p[0] == "pipe":
        f.update(stages=int(p[1][1:]), pieces=[int(s) for s in p[2][4:].split(",")] if p[2].startswith("cut=") else [1] * n)
        f["parts"] = max(f["pieces"]) > 1
    return f


def group_fields(g, t):
    """the library's route of a group as the same fields (None: LAVT_ERR_INVALID), every field `tn_route` does not state checked on the way"""
    K, _ = _capi()
    arr, n = group_params(g)
    ms = g.members
    r = K.GemmTNGroupRoute()
    ln = g.ln if g.entry == "ln" else None
    rc = int(K.lib.lavt_gemm_tn_group_route(arr, n, K.TN_ENTRY_SK if g.entry == "sk" else K.TN_ENTRY_GROUPED, *(ln or (0, 0)), ctypes.byref(r)))
    if rc != 0:
        assert rc == -22 and last_error().startswith("lavt_gemm_tn_grouped_sk" if g.entry == "sk" else "lavt_gemm_tn:"), (g.name, rc, last_error())
        return None
    f = dict(launch={K.TN_EACH: "each", K.TN_GROUP64: "group64", K.TN_PIPE: "pipe", K.TN_SK: "sk"}[r.launch])
    f["rider"] = {K.TN_RIDER_NONE: ("none", 0), K.TN_RIDER_RIDES: ("rides", r.rider_lpr), K.TN_RIDER_AFTER: ("after", 0)}[r.rider]
    pieces, kts = list(r.pieces)[:n], [cdiv(c.K, 64) for c in ms]
    any_maps, any_cs = any(G._maps(c) for c in ms), any(c.colsum for c in ms)
    if f["launch"] == "each":
        assert r.workgroups == 0 and [f"p{p}" in G.route_single(c, t).split("/") for p, c in zip(pieces, ms)] == [True] * min(n, 6), g.name
        return f
    assert all(p * k >= kt > (p - 1) * k for p, k, kt in zip(pieces, list(r.kt_per_piece), kts)), (g.name, pieces, list(r.kt_per_piece))
    assert bool(r.any_parts) == any(list(r.parts)[:n]) and all(p > 1 for p, on in zip(pieces, list(r.parts)) if on), g.name
    f.update(pieces=pieces, parts=bool(r.any_parts))
    kernels = G.launches(g, t)
    reducer = {K.TN_REDUCE_NONE: None, K.TN_REDUCE_GROUP: "tn_reduce_pieces_group", K.TN_REDUCE_PIPE: "tnp_reduce_pieces", K.TN_REDUCE_PIPE_DEEP: "tnp_reduce_pieces_deep"}[r.reducer]
    assert {k for k in kernels if k in ("tn_reduce_pieces_group", "tnp_reduce_pieces", "tnp_reduce_pieces_deep")} == ({reducer} if reducer else set()), (g.name, reducer)
    outs = max([c.I * (8 if c.no_b and f["launch"] == "pipe" else c.J) + c.I for c, on in zip(ms, list(r.parts)) if on], default=0)
    assert r.reducer_grid_x == (cdiv(outs, 1024 if reducer == "tnp_reduce_pieces" else 64) if reducer else 0), (g.name, r.reducer_grid_x, outs)
    blocks = G.ln_geometry(*ln)[0] if f["rider"][0] == "rides" else 0
    if f["launch"] == "sk":
        assert (r.stages, bool(r.maps)) == (2, any_maps) and r.scratch_floats == r.workgroups * 2 * (128 * 128 + 128), g.name
        f.update(maps=any_maps, cs=r.colsum_form, nw=r.workgroups)
    elif f["launch"] == "group64":
        assert r.stages == 2 and r.workgroups == sum(cdiv(c.I, 64) * cdiv(c.J, 64) * p for c, p in zip(ms, pieces)), g.name
        assert (r.rider_blocks, r.rider_wgs) == (blocks, blocks), g.name
        f.update(maps=bool(r.maps), cs=r.colsum_form)
    else:
        assert r.workgroups == sum(cdiv(c.I, 128) * (1 if c.no_b else cdiv(c.J, 128)) * p for c, p in zip(ms, pieces)), g.name
        assert (r.rider_blocks, r.rider_wgs) == (blocks, (blocks + 1) // 2) and (bool(r.maps), r.colsum_form) == (any_maps, 2 if any_cs else 0), g.name
        f["stages"] = r.stages
    return f


def compare_group(g):
    K, _ = _capi()
    t = dict(G.DEFAULT, **g.tuning)
    want, got = G.tn_route(g), group_fields(g, t)
    assert (got is None) == (want == G.INVALID), (g.name, got, want)
    if got is not None:
        assert got == parse(want, len(g.members)), (g.name, got, want)
    # the stream-K scratch query: the route's own answer, whichever entry the row is for
    arr, n = group_params(g)
    r = K.GemmTNGroupRoute()
    rc = int(K.lib.lavt_gemm_tn_group_route(arr, n, K.TN_ENTRY_SK, 0, 0, ctypes.byref(r)))
    plan = G.sk_plan(g.members)
    assert int(K.lib.lavt_gemm_tn_grouped_sk_ws(arr, n)) == (r.scratch_floats if rc == 0 else 0) == (plan[1] if plan else 0), (g.name, rc, plan)


@pytest.mark.parametrize("group", G.GROUPS + G.SK_REFUSED, ids=repr)
def test_group_rows_route_as_restated(group, tuning):
    tuning(group.tuning)
    assert G.tn_route(group) == group.route
    compare_group(group)


def test_pieces_bound_and_eligibility_of_every_member(tuning):
    K, _ = _capi()
    tuning({})
    for c in G.members_of(G.SINGLES + G.REFUSALS + G.GROUPS + G.SK_REFUSED + [r[1] for r in SINGLE_ROWS] + [r[1] for r in GROUP_ROWS]):
        p = params(c, Addresses())
        assert int(K.lib.lavt_gemm_tn_pieces(ctypes.byref(p))) == c.pieces_bound, c.name
        assert int(K.lib.lavt_gemm_tn_v2_eligible(ctypes.byref(p))) == int(G.v2_eligible(c)), c.name


# ------------------------------------------------------------------------------------------------ rows written by hand
# Single problems.  t64 / t128 = output tiles of that size x batch, kt = K tiles of 64 rows.  v2: 128x128 for conv problems with t128 >= 48 and
# kt >= 64; split = (768 + t64 / 2) / t64 (128x128: (384 + t128 / 2) / t128), at least cdiv(kt, 128), at most cdiv(kt, 8) (batch > 1: cdiv(kt, 2)).
_CV = dict(I=6144, conv=conv(1, 64, 64, 8))          # J = 72: one column tile of 128x128, 48 row tiles
SINGLE_ROWS = [
    # TN_BIG_MIN: 48 tiles of 128x128 at 64 K tiles -> split (384 + 24) / 48 = 8; 47 tiles: 94 x 2 tiles of 64x64 -> (768 + 94) / 188 = 4; 63 K tiles: 96 x 2 -> 4 x 16
    ("big-48x64", Case("big-48x64", "v2/128/plain/cs0/convp/p8/atomic", K=4096, **_CV)),
    ("big-47x64", Case("big-47x64", "v2/64/plain/cs0/convp/p4/atomic", K=4096, **dict(_CV, I=6016))),
    ("big-48x63", Case("big-48x63", "v2/64/plain/cs0/convp/p4/atomic", K=4032, **dict(_CV, conv=conv(1, 63, 64, 8)))),
    # K x max(lda, ldb) = 2^20 x 2048 = 2^31 element offsets: the classic kernel (32 tiles: 768 / 32 = 24 pieces of 683 K tiles); ldb = 2040: v2, no
    # workgroup beyond 128 K tiles -> 128 pieces
    ("offsets-2^31", Case("offsets-2^31", "classic/bf16/64/p24", I=8, J=2032, K=1 << 20)),
    ("offsets-below", Case("offsets-below", "v2/64/plain/cs0/lin/p128/atomic", I=8, J=2024, K=1 << 20)),
    # min_kt: 16 K tiles on one tile: 2 pieces of 8; batched (2 tiles): 8 pieces of 2
    ("min-kt-8", Case("min-kt-8", "v2/64/plain/cs0/lin/p2/atomic", I=8, J=8, K=1024)),
    ("min-kt-2", Case("min-kt-2", "v2/64/plain/cs0/lin/p8/atomic", I=8, J=8, K=1024, batch=2)),
    # long_k: 1024 tiles ask for (768 + 512) / 1024 = 1 piece; 129 K tiles make it two
    ("long-k-128", Case("long-k-128", "v2/64/plain/cs0/lin/p1/store", I=2048, J=2048, K=128 * 64)),
    ("long-k-129", Case("long-k-129", "v2/64/plain/cs0/lin/p2/atomic", I=2048, J=2048, K=129 * 64)),
]


@pytest.mark.parametrize("name,case", SINGLE_ROWS, ids=[r[0] for r in SINGLE_ROWS])
def test_hand_written_single_rows(name, case, tuning):
    tuning({})
    assert single_route(case) == case.route == G.tn_route(case, {}), (name, single_route(case), G.tn_route(case, {}))


def _pair(tag, a, b, **kw):
    """two plain members of a x b tiles (of 64x64, or with t=128 of 128x128) each: (rows, columns) per member"""
    t = kw.pop("t", 64)
    per = kw.pop("per", ({}, {}))
    return [Case(f"{tag}/{k}", "", I=t * i, J=t * j, **dict(kw, **per[k])) for k, (i, j) in enumerate((a, b))]


def _src_rows_limit(ld):
    """the first row count a map may name that leaves the 2 GB descriptor: (rows + 1) x ld x 2 + 256 >= 2^31"""
    return cdiv((1 << 31) - 256, 2 * ld) - 1


P0, PU, PC = G.P0, dict(G._PU, stages=4), dict(G._PC, stages=4)
_LD = 58256          # (8192 + 1024) rows x 58256 x 2 bytes = 2^30 + 32768
GROUP_ROWS = [
    # ---- the 64x64 launch (tn_pipe = 0).  uncut: 256 + 255 tiles cut where cutting pays (50 K tiles, zeroed C: cdiv(50, 48) = 2 atomic pieces); 512 stay whole
    ("uncut-511", Group("uncut-511", "group64/plain/cs0/s=2,2", _pair("uncut-511", (16, 16), (15, 17), K=3200, split_k=-1), tuning=P0)),
    ("uncut-512", Group("uncut-512", "group64/plain/cs0/s=1,1", _pair("uncut-512", (16, 16), (16, 16), K=3200, split_k=-1), tuning=P0)),
    # 128 + 127 workgroups are too few to fill the chip
    ("tiles-255", Group("tiles-255", "each", _pair("tiles-255", (8, 16), (127, 1), K=72), tuning=P0)),
    ("tiles-256", Group("tiles-256", "group64/plain/cs0/s=1,1", _pair("tiles-256", (8, 16), (128, 1), K=72), tuning=P0)),
    # a chain of more than 128 K tiles without a scratch keeps the group from forming
    ("chain-128", Group("chain-128", "group64/plain/cs0/s=1,1", _pair("chain-128", (8, 16), (128, 1), K=72, per=({}, dict(K=128 * 64))), tuning=P0)),
    ("chain-129", Group("chain-129", "each", _pair("chain-129", (8, 16), (128, 1), K=72, per=({}, dict(K=129 * 64))), tuning=P0)),
    # ---- the pipelined launch, uncut (min_tiles = min_ktiles = 1).  (K + 1024) x lda x 2 bytes against 2^30; the rows a map may name against 2^31
    ("bytes-below", Group("bytes-below", "pipe/s4/uncut", _pair("bytes-below", (16, 16), (16, 16), K=8192, per=({}, dict(lda=_LD - 8))), tuning=PU)),
    ("bytes-2^30", Group("bytes-2^30", "group64/plain/cs0/s=1,1", _pair("bytes-2^30", (16, 16), (16, 16), K=8192, per=({}, dict(lda=_LD))), tuning=PU)),
    ("a-rows-below", Group("a-rows-below", "pipe/s4/uncut", _pair("a-rows-below", (16, 16), (16, 16), K=512, per=({}, dict(a_map=True, src_rows=(_src_rows_limit(1032) - 1, None)))), tuning=PU)),
    ("a-rows-2^31", Group("a-rows-2^31", "group64/maps/cs0/s=1,1", _pair("a-rows-2^31", (16, 16), (16, 16), K=512, per=({}, dict(a_map=True, src_rows=(_src_rows_limit(1032), None)))), tuning=PU)),
    ("b-rows-below", Group("b-rows-below", "pipe/s4/uncut", _pair("b-rows-below", (16, 16), (16, 16), K=512, per=(dict(b_map=True, src_rows=(None, _src_rows_limit(1040) - 1)), {})), tuning=PU)),
    ("b-rows-2^31", Group("b-rows-2^31", "group64/maps/cs0/s=1,1", _pair("b-rows-2^31", (16, 16), (16, 16), K=512, per=(dict(b_map=True, src_rows=(None, _src_rows_limit(1040))), {})), tuning=PU)),
    # ---- tn_pipe_min_tiles: 64 + 56 tiles of 128x128 at 32 K tiles run uncut from 120 tiles; under 121 they are cut into one round (3840 / 250 -> pieces
    # of 16 K tiles: 240 workgroups).  tn_pipe_min_ktiles: 32 K tiles per tile pass 32, not 33 (480 tiles of 64x64: the 64x64 launch, 32 K tiles uncut)
    ("min-tiles-120", Group("min-tiles-120", "pipe/s4/uncut", _pair("min-tiles-120", (8, 8), (7, 8), t=128, K=2048, partials=2), tuning=dict(min_tiles=120))),
    ("min-tiles-121", Group("min-tiles-121", "pipe/s4/cut=2,2", _pair("min-tiles-121", (8, 8), (7, 8), t=128, K=2048, partials=2), tuning=dict(min_tiles=121))),
    ("min-ktiles-32", Group("min-ktiles-32", "pipe/s4/uncut", _pair("min-ktiles-32", (8, 8), (7, 8), t=128, K=2048, partials=2), tuning=dict(min_tiles=120, min_ktiles=32))),
    ("min-ktiles-33", Group("min-ktiles-33", "group64/plain/cs0/s=1,1", _pair("min-ktiles-33", (8, 8), (7, 8), t=128, K=2048, partials=2), tuning=dict(min_tiles=120, min_ktiles=33))),
    # ---- the cut launch (min_tiles = 4096): one round of 96..256 workgroups, pieces of at most 128 K tiles
    ("cut-95", Group("cut-95", "group64/plain/cs0/s=1,1", _pair("cut-95", (5, 10), (5, 9), t=128, K=512), tuning=PC)),
    ("cut-96", Group("cut-96", "pipe/s4/cut=1,1", _pair("cut-96", (5, 10), (2, 23), t=128, K=512), tuning=PC)),
    ("cut-256", Group("cut-256", "pipe/s4/cut=1,1", _pair("cut-256", (16, 8), (16, 8), t=128, K=512), tuning=PC)),
    ("cut-257", Group("cut-257", "group64/plain/cs0/s=1,1", _pair("cut-257", (16, 8), (3, 43), t=128, K=512), tuning=PC)),
    ("per-128", Group("per-128", "pipe/s4/cut=1,1", _pair("per-128", (16, 8), (16, 8), t=128, K=128 * 64), tuning=PC)),
    ("per-129", Group("per-129", "each", _pair("per-129", (16, 8), (16, 8), t=128, K=129 * 64), tuning=PC)),
    # ---- the rider.  Cost model: 108 tiles at 16 K tiles stay whole under the rider budget and are cut in two without: 0.8 x (16 - 8) us against a
    # LayerNorm of 4 + 6 x rows x 256 / 3e6 + 1 us -- dropped below 2734.4 rows.  Geometry: C = 1024 needs two chunks per lane
    ("rider-cost-kept", Group("rider-cost-kept", "pipe/s4/cut=1,1,1,1+ln32", G._dropped_rider_members("rider-cost-kept"), tuning=PC, entry="ln", ln=(2735, 256))),
    ("rider-cost-dropped", Group("rider-cost-dropped", "pipe/s4/cut=2,2,2,2+ln-after", G._dropped_rider_members("rider-cost-dropped"), tuning=PC, entry="ln", ln=(2733, 256))),
    ("rider-cpl2", Group("rider-cpl2", "pipe/s4/cut=7,7,7,7+ln-after", G._cut_members("rider-cpl2"), tuning=PC, entry="ln", ln=(131, 1024))),
    # ---- stream-K: runs of 6 K-tile iterations, at least 128 of them, at least 32 tiles.  32 tiles x 24 = 768 iterations; 20 x 24 + 13 x 22 = 766;
    # 20 + 11 tiles x 25 = 775 iterations on 31 tiles
    ("sk-nw128", Group("sk-nw128", "sk/plain/cs0/nw128", [Case("sk-nw128/a", "", I=520, J=512, K=1536), Case("sk-nw128/b", "", I=512, J=384, K=1536)], entry="sk")),
    ("sk-nw127", Group("sk-nw127", G.INVALID, [Case("sk-nw127/a", "", I=520, J=512, K=1536), Case("sk-nw127/b", "", I=1664, J=128, K=1408)], entry="sk", invalid=True)),
    ("sk-tiles-32", Group("sk-tiles-32", "sk/plain/cs0/nw133", [Case("sk-tiles-32/a", "", I=520, J=512, K=1600), Case("sk-tiles-32/b", "", I=512, J=384, K=1600)], entry="sk")),
    ("sk-tiles-31", Group("sk-tiles-31", G.INVALID, [Case("sk-tiles-31/a", "", I=520, J=512, K=1600), Case("sk-tiles-31/b", "", I=1408, J=128, K=1600)], entry="sk", invalid=True)),
]


@pytest.mark.parametrize("name,group", GROUP_ROWS, ids=[r[0] for r in GROUP_ROWS])
def test_hand_written_group_rows(name, group, tuning):
    tuning(group.tuning)
    assert G.tn_route(group) == group.route, (name, G.tn_route(group), group.route)
    compare_group(group)


def test_the_rows_stand_on_both_sides_of_every_threshold():
    """the pairs above really differ, and the library's structs are the ones _capi.py declares (a route written past the ctypes struct would corrupt
    the fields compared here)"""
    K, _ = _capi()
    routes = {n: g.route for n, g in GROUP_ROWS}
    routes.update({n: c.route for n, c in SINGLE_ROWS})
    for a, b in re.findall(r"(\S+)\|(\S+)", "big-48x64|big-47x64 big-48x64|big-48x63 offsets-2^31|offsets-below min-kt-8|min-kt-2 long-k-128|long-k-129 uncut-511|uncut-512 "
                           "tiles-255|tiles-256 chain-128|chain-129 bytes-below|bytes-2^30 a-rows-below|a-rows-2^31 b-rows-below|b-rows-2^31 min-tiles-120|min-tiles-121 "
                           "min-ktiles-32|min-ktiles-33 cut-95|cut-96 cut-256|cut-257 per-128|per-129 rider-cost-kept|rider-cost-dropped sk-nw128|sk-nw127 "
                           "sk-tiles-32|sk-tiles-31"):
        assert routes[a] != routes[b], (a, b)
    assert ctypes.sizeof(K.GemmTNRoute) == 40 and ctypes.sizeof(K.GemmTNGroupRoute) == 128 and K.TN_GROUP_MAX == 6
