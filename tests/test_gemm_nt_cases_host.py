"""The fp64 statement of lavt_gemm_nt's contract, its dispatch restatement and its gate (tests/gemm_nt_cases.py) checked themselves, CPU only.

(1) Against autograd: `nt_reference` on operands kept in fp64 reproduces, to 1e-9, plain torch formulations of the features it restates -- F.linear +
    activation + multiplier + residual, index_add for the row scatter, a zero row for the gather's -1, F.layer_norm followed by F.linear for the
    LayerNorm-folded operand (the fold of W, gamma, beta included), and the autograd gradient through GELU, tanh and ReLU for dact_pre, with the
    residual joining after or (res_first) before it.
(2) `route` returns the route every row of the table states, under every forced configuration the row runs in, and the table reaches every
    instantiation the dispatcher can reach outside convolutions and fp8 (gemm_nt_cases.reachable enumerates them; the convolution
    instantiations are gemm_nt_conv_cases.reachable_conv's, held by test_gemm_nt_conv_cases_host.py).
(3) Planted faults: the "kernel" is the floor evaluation (fp32, bf16 roundings of the contract) with one defect injected, at the smallest case of the
    table that has the feature.  The gate, with K_NT as committed, must reject every defect with a factor 2 to spare and pass the unmutated floor."""
import pytest
import torch
import torch.nn.functional as F

import gemm_nt_cases as G

F64 = torch.float64
TOL = 1e-9


def _close(a, b, what):
    own = torch.isfinite(b)
    assert bool(torch.isfinite(a[own]).all()), what
    err = float((a[own] - b[own]).abs().max()) if own.any() else 0.0
    assert err <= TOL * max(1.0, float(b[own].abs().max())), (what, err)


ACTS = {G.ACT_NONE: lambda t: t, G.ACT_GELU: F.gelu, G.ACT_RELU: F.relu, G.ACT_TANH: torch.tanh}


def _plain_forward(c):
    """(pre, y) of the plain formulation, rows in m order, [batch, M, N]"""
    i = c.inp
    A = i["A"]
    if c.a_map:
        Az = torch.cat([A, torch.zeros(c.batch, 1, c.K, dtype=F64)], 1)          # -1 -> the appended zero row
        am = i["a_map"].long()
        A = Az.index_select(1, torch.where(am >= 0, am, torch.full_like(am, c.Ma)))
    v = torch.stack([c.alpha * F.linear(A[b], i["W"][b]) for b in range(c.batch)])
    if c.bias:
        v = v + i["bias"][:, None, :]
    if c.row_scale:
        v = v * i["row_scale"][:, torch.arange(c.M) // max(c.row_scale_div, 1)][..., None]
    return v


def _scatter(c, t):
    """[batch, M, n] rows in m order -> [batch, Mo, n] by index_add over the kept rows; rows nobody writes -> NaN"""
    if not c.c_map:
        return t
    cm = c.inp["c_map"].long()
    keep = cm >= 0
    out = torch.zeros(t.shape[0], c.Mo, t.shape[2], dtype=F64).index_add(1, cm[keep], t[:, keep])
    hit = torch.zeros(c.Mo, dtype=F64).index_add(0, cm[keep], torch.ones(int(keep.sum()), dtype=F64))
    assert float(hit.max()) == 1.0
    out[:, hit == 0] = G.NAN
    return out


def _by_out_row(c, t):
    """a side input [Mo, N] as seen by row m"""
    return t[c.inp["c_map"].long().clamp(min=0)] if c.c_map else t


@pytest.mark.parametrize("act", [G.ACT_NONE, G.ACT_GELU, G.ACT_RELU, G.ACT_TANH])
@pytest.mark.parametrize("kw", [dict(), dict(batch=3), dict(a_map=True, c_map=True, R=True, mul=True, row_scale=True, row_scale_div=13, cpre=True),
                                dict(c_split=24, R=True, c_map=True), dict(row_scale=True, cpre=True, R=True, c_f32=True)], ids=["plain", "batch", "maps", "split", "f32out"])
def test_reference_is_linear_act_residual(act, kw):
    c = G.Case("host", 37, 40, 24, exact=True, bias=True, act=act, **kw)
    ref = G.nt_reference(c)
    pre = _plain_forward(c)
    y = ACTS[act](pre)
    if c.mul:
        y = y * _by_out_row(c, c.inp["mul"])
    if c.R:
        y = y + _by_out_row(c, c.inp["R"])
    y = _scatter(c, y)
    if c.c_split:
        _close(ref["C"], y[..., :c.c_split], "C")
        _close(ref["C2"], y[0, :, c.c_split:], "C2")
        assert ref["C"].shape == (1, 37, 24) and ref["C2"].shape == (37, 16)
    else:
        _close(ref["C"], y, "C")
    assert torch.equal(torch.isnan(ref["C"]), torch.isnan(y[..., :c.Nc]))
    if c.cpre:
        _close(ref["Cpre"], _scatter(c, pre)[0], "Cpre")
    assert set(ref) == {"C"} | ({"C2"} if c.c_split else set()) | ({"Cpre"} if c.cpre else set())


_RSM = dict(R=True, row_scale=True, c_map=True)          # (the header gives LAVT_ACT_GELU_D none of these)


@pytest.mark.parametrize("act,sigma,extra", [(a, s, {}) for a in (G.ACT_NONE, G.ACT_GELU, G.ACT_GELU_D) for s in (3.0, 10.0)] + [(G.ACT_NONE, 3.0, _RSM), (G.ACT_GELU, 3.0, _RSM)])
def test_reference_is_layernorm_then_linear(act, sigma, extra):
    c = G.Case("host-ln", 37, 40, 64, exact=True, ln=True, ln_sigma=sigma, act=act, cpre=act != G.ACT_NONE, **extra)
    i = c.inp
    ref = G.nt_reference(c)
    x = i["A"][0].clone().requires_grad_(False)
    pre = F.linear(F.layer_norm(x, (c.K,), i["gamma"], i["beta"], G.EPS), i["W0"], i["b0"])
    if c.row_scale:
        pre = pre * i["row_scale"][0][:, None]
    p = pre.detach().clone().requires_grad_(True)
    y = F.gelu(p) if act != G.ACT_NONE else p
    (dgelu,) = torch.autograd.grad(y.sum(), p)
    y = y.detach()
    if c.R:
        y = y + _by_out_row(c, i["R"])
    _close(ref["C"], _scatter(c, y[None]), "C")
    if c.cpre:
        _close(ref["Cpre"], _scatter(c, (dgelu if act == G.ACT_GELU_D else pre)[None])[0], "Cpre")
    _close(ref["ln_mean"], x.mean(1), "ln_mean")
    _close(ref["ln_rstd"], torch.rsqrt(x.var(1, unbiased=False) + G.EPS), "ln_rstd")
    assert "ln_mean" not in G.nt_reference(c.but("host-ln-nostats", ln_stats=False))


@pytest.mark.parametrize("dact", [G.ACT_GELU, G.ACT_RELU, G.ACT_TANH, G.ACT_STORED])
@pytest.mark.parametrize("R,first", [(False, False), (True, False), (True, True)], ids=["noR", "R", "Rfirst"])
def test_reference_is_autograd_through_the_activation(dact, R, first):
    """the layer after an activation: y = act(pre), upstream gradient g = the GEMM's value (with res_first: g + R) -> d / d pre by autograd"""
    c = G.Case("host-dact", 37, 40, 64, exact=True, kmajor=True, bias=True, row_scale=True, c_map=True, dact=dact, R=R, res_first=first)
    i = c.inp
    ref = G.nt_reference(c)
    g = _plain_forward(c)[0]
    pre = (1.5 * G._randn(c.Mo, c.N, seed=1000 * c.seed + 6)).requires_grad_(True)          # what _inputs drew dact_pre from
    fn = F.gelu if dact == G.ACT_STORED else ACTS[dact]
    (d,) = torch.autograd.grad(fn(pre).sum(), pre)
    if dact == G.ACT_STORED:
        _close(i["dact_pre"], d, "the stored derivative is GELU'")
    else:
        assert torch.equal(i["dact_pre"], pre.detach())
    d = _by_out_row(c, d)
    Rm = _by_out_row(c, i["R"]) if R else 0.0
    y = (g + Rm) * d if first else g * d + Rm
    _close(ref["C"], _scatter(c, y[None]), "C")


def test_floor_rounds_what_the_kernel_stores():
    c = G.BY_NAME["lean-gelu"]
    flo = G.floor(c)
    for k in ("C", "Cpre"):
        assert flo[k].dtype == torch.float32 and torch.equal(flo[k], G.bf(flo[k]))
    f32 = G.floor(G.BY_NAME["edge-m129-n132-k64-f32out"])["C"]
    assert not torch.equal(f32, G.bf(f32))
    for k, v in c.inp.items():
        if k in ("A", "W", "R"):
            assert torch.equal(v, G.bf(v)), k


# ------------------------------------------------------------------------------------------------ (2) the dispatch
def _rows():
    """(case, tuning name or None, stated route) for every launch of the GPU file"""
    for c in G.PLAIN:
        for t in G.TUNINGS:
            yield c, t, G.stated_route(c, t)
    for c in G.PLAIN_F32:
        for t in G.TUNINGS_F32:
            yield c, t, G.stated_route(c, t)
    for c in G.DEFAULT_TABLE:
        yield c, None, c.route


def test_route_is_the_stated_route_of_every_row():
    names = [c.name for c in G.PLAIN + G.PLAIN_F32 + G.DEFAULT_TABLE]
    assert len(names) == len(set(names))
    for c, t, stated in _rows():
        assert c.route is not None, c
        got = G.route_str(G.route(c, G.tuning_dict(t) if t else None))
        assert got == stated, (c.name, t, got, stated)
        assert (got == G.INVALID) == c.invalid


def test_table_reaches_every_instantiation():
    seen = set()
    for c, t, _ in _rows():
        r = G.route(c, G.tuning_dict(t) if t else None)
        if r != G.INVALID:
            seen.update(G.route_str(r._replace(forms=frozenset([f]))) for f in r.forms)
    missing = G.reachable() - seen
    assert not missing, sorted(missing)
    assert not seen - G.reachable(), sorted(seen - G.reachable())


def test_store_form_switches_and_prefetch():
    t64 = G.tuning_dict("t64-s4-p0")
    wide = G.route(G.BY_NAME["store-wide"], t64)
    assert wide.forms == {"wide"}
    for n in ("store-ldc+4", "store-split68", "store-ldcpre+4", "store-bias+1", "store-batch3-stride+4", "store-none-ldc+4"):
        r = G.route(G.BY_NAME[n], t64)
        assert r.forms == {"narrow"} and r[:4] == wide[:4], n
    assert G.epi_wide(G.BY_NAME["store-batch3"]) == 1 and G.epi_wide(G.BY_NAME["store-wide"]) == 3
    # the side inputs requested before the K loop: 64x64 tiles with a residual / multiplier, and the activation-gradient kernels
    assert G.route(G.BY_NAME["lean-bias-R-scale-map"], t64).prefetch and not G.route(G.BY_NAME["lean-bias-R-scale-map"], G.tuning_dict("t128-s4-p0")).prefetch
    assert G.route(G.BY_NAME["dact-gelu-R-m77-k64"]).prefetch and G.route(G.BY_NAME["dact-stored-m3190-k64"]).prefetch
    assert not G.route(G.BY_NAME["dact-gelu-R-m3190-k64"]).prefetch


def test_dact_and_lna_sizes_pick_all_four_kernels():
    for kind, rows in (("DACT", G.DACT), ("DACT+GD", G.DACT), ("LNA", G.LNA), ("LNA+GD", G.LNA)):
        picked = {(r.tile, r.stages) for r in (G.route(c) for c in rows) if r.kind == kind}
        assert picked == {(64, 4), (64, 2), (128, 4), (128, 2)}, (kind, picked)
        for K in (64, 192):
            assert {(r.tile, r.stages) for r in (G.route(c) for c in rows if c.K == K) if r.kind == kind} == picked, (kind, K)


# ------------------------------------------------------------------------------------------------ (3) planted faults
def _smallest(rows, pred):
    hits = [c for c in rows if pred(c)]
    assert hits
    return min(hits, key=lambda c: c.M * c.N * c.K * c.batch)


def _check(c, mutated, keys=None):
    ref, flo = G.reference(c), G.floor(c)
    for k in keys or mutated:
        key = c.store_key(k)
        E, Fl = G.gate(key, flo[k], ref[k], flo[k])          # the unmutated floor passes
        assert E == Fl
        assert G.rejects(key, mutated[k], ref[k], flo[k]), (c.name, k, G.nt_error(mutated[k], ref[k]), Fl, G.K_NT[key])


@pytest.mark.parametrize("rows", ["bf16", "f32"])
def test_gate_rejects_a_fragment_from_its_neighbour(rows):
    """one 4-column fragment of one 16-row block replaced by its neighbour, in the smallest and in the widest case"""
    table = G.PLAIN if rows == "bf16" else G.PLAIN_F32
    for c in (_smallest(table, lambda c: c.M >= 32 and c.N >= 16 and not c.c_map), max(table, key=lambda c: c.N * c.M)):
        m = G.floor(c)["C"].clone()
        m[0, 16:32, 4:8] = m[0, 16:32, 8:12]
        _check(c, {"C": m})


def test_gate_rejects_a_dropped_k_chunk():
    """the last 8-element K chunk dropped, at the shortest and at the longest reduction of the table"""
    for c in (_smallest(G.PLAIN, lambda c: c.K >= 16), max(G.PLAIN, key=lambda c: c.K), G.BY_NAME["k1024-pipe128"].but("k1024-small", M=129, N=136)):
        _check(c, G.nt_reference(c, torch.float32, True, fault="drop_last_k8"), ["C"])


@pytest.mark.parametrize("fault,pred,keys", [
    ("bias_after_scale", lambda c: c.bias and c.row_scale, ["C"]),
    ("mul_after_res", lambda c: c.mul and c.R, ["C"]),
    ("ignore_row_scale_div", lambda c: c.row_scale and c.row_scale_div > 1, ["C"]),
    ("ignore_res_first", lambda c: c.res_first and not c.invalid, ["C"]),
    ("wsum_unfolded", lambda c: c.ln and c.cpre and not c.invalid, ["C", "Cpre"]),
])
def test_gate_rejects_a_wrong_epilogue(fault, pred, keys):
    c = _smallest(G.PLAIN + G.DEFAULT_TABLE, pred)
    _check(c, G.nt_reference(c, torch.float32, True, fault=fault), keys)


def test_gate_rejects_the_split_boundary_in_the_wrong_buffer():
    c = _smallest(G.PLAIN, lambda c: c.c_split)
    flo = G.floor(c)
    C, C2 = flo["C"].clone(), flo["C2"].clone()
    C[0, :, -4:], C2[:, :4] = flo["C2"][:, :4], flo["C"][0, :, -4:]
    _check(c, {"C": C, "C2": C2})


def test_gate_counts_an_unwritten_element_as_infinite():
    c = G.BY_NAME["map-c"]
    ref, flo = G.reference(c), G.floor(c)
    m = flo["C"].clone()
    own = torch.isfinite(ref["C"][0]).all(1).nonzero()[5, 0]
    m[0, own, 7] = G.NAN
    assert G.nt_error(m, ref["C"]) == float("inf") and G.rejects("C", m, ref["C"], flo["C"])


def test_k_nt_follows_the_measured_ratios():
    from test_gpu_gemm_nt_cases import MEASURED
    assert set(MEASURED) == set(G.K_NT)
    for n, ratio in MEASURED.items():
        assert G.K_NT[n] == G.k_from_measured(ratio), (n, G.K_NT[n], ratio)
