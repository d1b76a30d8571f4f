"""The case table of the convolution parity tests (tests/gemm_nt_conv_cases.py) held to its own claims, CPU only.

  * mode int, per case: every exact output value is representable in the type it is stored in (so the final rounding is the identity), the sum of the
    addends' magnitudes stays under 2^24 (every partial sum in every order is exact in fp32) and fewer than 5 % of the owned outputs are exactly zero
    (a dropped contribution shows) -- counted over the outputs whose reduction is not empty: the dy = -1 tap group of a split has nothing but halo
    for the first image row, a share no choice of operands can lower (2 / 15 of a 5 x 7 image's partial outputs); what the reduce kernels store into
    bf16 after a split is representable too;
  * the two statements of the contract agree exactly: the index form on the physical buffers == F.conv3d / autograd's input gradient in float64;
    no NaN of `build` (guard rows, padding columns, the weights outside the b_off column block) reaches the reference;
  * every row's stated route == gemm_nt_cases.route() per (row, forced configuration), the union of the routes == reachable_conv();
  * every listed fault is rejected by the gate on a case named for it;
  * no two rows share a name or a purpose.

test_gemm_nt_route_host.py holds route() to the library's planner for the same rows.  fp8 convolutions are out of scope."""
import pytest
import torch

import gemm_nt_cases as G
import gemm_nt_conv_cases as V


def tuning_of(c, t):
    d = G.tuning_dict(t) if t else {}
    if c.env:
        d = dict(d, pipe=int(c.env["LAVT_GEMM_PIPE"]))
    return d


def whole(c, out):
    """[M, N]: the outputs of a case put together -- the batch entries of a split summed, C2 beside C"""
    t = out["C"].sum(0)
    return torch.cat([t, out["C2"]], 1) if c.c_split else t


@pytest.mark.parametrize("case", V.INT_TABLE, ids=repr)
def test_int_cases_are_exact(case):
    c = case
    o = V.build(c)
    ref = V.reference(c)
    for k, v in ref.items():
        assert bool(torch.isfinite(v).all()), (c.name, k, "a NaN of build() reached the reference")
        if k != "acc":
            assert V.stored_exactly(c, k, v), (c.name, k, float(v.abs().max()))
    # the sum of the addends' magnitudes: |x| against |w| through the same index form
    mag = {k: (t.double().abs() if torch.is_floating_point(t) else t) for k, t in o.items()}
    bound = float(V.accumulate(c, mag).sum(0).max()) * abs(c.alpha) + (float(mag["bias"].max()) if c.bias else 0.0)
    assert bound < 2 ** 24, (c.name, bound)
    owned = torch.cat([v.reshape(-1) for k, v in ref.items() if k != "acc"])
    # zeros: over the outputs whose reduction is not empty.  A tap group of a split lies wholly in the halo along one image side; the exact 0 the
    # contract demands there is held by the bit comparison like every other value, and counts neither for nor against the operands' density
    ne = V.nonempty(c)
    assert bool((ref["C"][~ne] == 0).all())
    live = torch.cat([ref["C"][ne].reshape(-1)] + [v[ne[0]].reshape(-1) for k, v in ref.items() if k in ("C2", "Cpre")])
    assert live.numel() >= 0.6 * owned.numel()
    zeros = float((live == 0).double().mean())
    if c.batch > 1:          # what the reduce kernels store into bf16: the sum of the entries, and with an integer bias
        total = ref["C"].sum(0)
        assert V.stored_exactly(c.but("x", tap_split=0, kc_split=0), "C", total) and V.stored_exactly(c.but("x", tap_split=0, kc_split=0), "C", total + 3) \
            and V.stored_exactly(c.but("x", tap_split=0, kc_split=0), "C", total - 3), (c.name, float(total.abs().max()))
    print(f"[conv-host] {c.name}: max |value| {float(owned.abs().max()):g}, sum of magnitudes {bound:g}, zero share {zeros:.4f}")
    assert zeros < 0.05, (c.name, zeros)


@pytest.mark.parametrize("case", V.TABLE, ids=repr)
def test_index_form_equals_torch_convolution(case):
    c = case
    a, b = whole(c, V.reference(c)), V.conv_reference(c)
    if c.mode == "int":
        assert torch.equal(a, b), (c.name, float((a - b).abs().max()))
    else:          # real operands: two orders of an fp64 sum
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max())), c.name
    if c.cpre and c.act == G.ACT_NONE:
        assert torch.equal(V.reference(c)["Cpre"], a)


@pytest.mark.parametrize("case", [c for c in V.TABLE if c.batch > 1], ids=repr)
def test_split_entries_contract_their_own_part(case):
    """entry bz alone == the convolution with every other tap / channel of the weight zeroed"""
    c = case
    x, w, b = V.logical(c)
    ref = V.reference(c)["C"]
    for bz in range(c.batch):
        wz = torch.zeros_like(w)
        c0, c1 = c.chans_of(bz)
        taps = list(c.taps_of(bz))
        wz[taps, c0:c1] = w[taps, c0:c1]
        V._LOGICAL[(c.geom, c.kern, c.C1, c.C2, c.Nw, c.mode, c.p, c.dtype, c.seed + 1000, c.M)] = (x, wz, b)
        part = c.but(c.name + "-part", seed=c.seed + 1000, tap_split=0, kc_split=0, stride_x=0)
        assert torch.equal(V.conv_reference(part), ref[bz]), (c.name, bz)
        del V._LOGICAL[(c.geom, c.kern, c.C1, c.C2, c.Nw, c.mode, c.p, c.dtype, c.seed + 1000, c.M)]


def test_stated_routes_and_reachability():
    seen, bad = set(), []
    for c, t in V.launches():
        r = V.route_key(c, G.route(c, tuning_of(c, t)))
        if r != V.stated_route(c, t):
            bad.append((c.name, t, r, V.stated_route(c, t)))
        seen.add(r)
    assert not bad, bad
    assert seen == V.reachable_conv(), (sorted(V.reachable_conv() - seen), sorted(seen - V.reachable_conv()))


@pytest.mark.parametrize("case", V.REFUSALS, ids=repr)
def test_refusals_are_invalid_routes(case):
    assert G.route(case, tuning_of(case, None)) == G.INVALID and case.word


def test_plain_rows_keep_their_routes():
    """the convolution clauses of route() leave every row of the plain table where it was"""
    for c in G.PLAIN:
        for name in G.TUNINGS:
            assert G.route_str(G.route(c, G.tuning_dict(name))) == G.stated_route(c, name), (c.name, name)
    for c in G.DEFAULT_TABLE:
        assert G.route_str(G.route(c)) == c.route, c.name


def _rejected(c, fault):
    ref, bad = V.reference(c), V.index_reference(c, fault=fault)
    if c.mode == "int":
        return any(not V.bit_equal(bad[k], ref[k]) for k in ref if k != "acc")
    flo = V.floor(c)
    return any(G.rejects(c.store_key(k), bad[k], ref[k], flo[k]) for k in ref if k != "acc")


@pytest.mark.parametrize("fault", list(V.FAULTS))
def test_faults_are_rejected(fault):
    names = V.FAULTS[fault]
    assert names and all(n in V.BY_NAME for n in names)
    hit = [n for n in names if _rejected(V.BY_NAME[n], fault)]
    print(f"[conv-host] {fault}: rejected by {hit} of {names}")
    assert hit == names, (fault, names, hit)


def test_rows_are_distinct():
    rows = V.TABLE + V.REFUSALS
    assert len({c.name for c in rows}) == len(rows)

    def purpose(c):
        return tuple(sorted((k, str(v)) for k, v in c.kw.items() if k not in ("why", "seed")) + [("N", str(c.N))])
    seen = {}
    for c in rows:
        assert purpose(c) not in seen, (c.name, seen[purpose(c)])
        seen[purpose(c)] = c.name
    whys = [c.why for c in rows if c.why]
    assert len(set(whys)) == len(whys)
    # the shapes stay small: every GPU case takes a launch of a few microseconds
    assert all(c.M <= 288 and c.K <= 3456 and c.N <= 264 for c in rows)
