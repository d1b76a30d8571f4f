"""CPU checks of tests/gemm_tn_cases.py: the reference against autograd, the exactness conditions of the integer cases, the restated planners against the
route every row states, the coverage of the reachable instantiations, and twelve planted faults the cases must reject."""
import pytest
import torch
import torch.nn.functional as F

import gemm_tn_cases as G

INT_SINGLES = [c for c in G.SINGLE + G.SINGLE_128 + G.CLASSIC + G.TAPS if c.I * c.J * c.K <= 1 << 26]
INT_ALL = [c for c in G.members_of(G.ALL_ROUTED) if c.mode == "int" and not c.invalid]


# ------------------------------------------------------------------------------------------------ the reference against autograd
@pytest.mark.parametrize("scale,div", [("scaled", 25), ("binary", 75), (None, 1)])
def test_reference_is_linear_weight_and_bias_gradient(scale, div):
    """y_k = s_k (W x_k + b): dW = sum_k s_k dy_k x_k^T, db = sum_k s_k dy_k -- what ops._linear_wgrad asks of the family (binary: the value sits in alpha)"""
    c = G.Case(f"host-linear-{scale}", "", mode="real", dtype="f32", I=12, J=20, K=130, scale=scale, div=div, v=1.25, alpha=1.25 if scale == "binary" else 1.0, colsum=True,
               a_map=True)
    i = G.inputs(c)
    lin = torch.nn.Linear(c.J, c.I).double()
    x = i["B"][0][:c.K]
    s = torch.ones(c.K, dtype=torch.float64) if scale is None else i["scale"].double()[torch.arange(c.K) // div]
    m = i["a_map"].long()
    dy = torch.where(m[:, None] >= 0, i["A"][0][m.clamp(min=0)], torch.zeros(1, dtype=torch.float64))
    (lin(x) * s[:, None] * dy).sum().backward()
    r = G.tn_reference(c)
    torch.testing.assert_close(r["C"][0], lin.weight.grad, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(r["colsum"][0], lin.bias.grad, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("geo", [dict(n=3, h=9, w=7), dict(n=1, h=2, w=67), dict(n=2, h=2, w=5, d=3, k=(3, 3, 3)), dict(n=2, h=2, w=5, d=3, k=(3, 1, 1)),
                                 dict(n=2, h=2, w=5, d=3, k=(1, 3, 3))], ids=str)
def test_reference_is_conv_weight_gradient(geo):
    """the tap-shifted form with c_conv_permute is torch.nn.grad.conv2d_weight / conv3d_weight of the NHWC rows (zero padding, sample borders)"""
    cv = G.conv(kc=8, **geo)
    c = G.Case(f"host-conv-{geo}", "", I=16, K=cv["n"] * cv["d"] * cv["h"] * cv["w"], conv=cv, permute=True)
    i = G.inputs(c)
    x = i["B"][0].view(cv["n"], cv["d"], cv["h"], cv["w"], 8).permute(0, 4, 1, 2, 3)
    dy = i["A"][0].view(cv["n"], cv["d"], cv["h"], cv["w"], c.I).permute(0, 4, 1, 2, 3)
    k = (cv["kd"], cv["kh"], cv["kw"])
    if cv["d"] == 1:
        ref = torch.nn.grad.conv2d_weight(x[:, :, 0], (c.I, 8, 3, 3), dy[:, :, 0], padding=1)
    else:
        ref = torch.nn.grad.conv3d_weight(x, (c.I, 8) + k, dy, padding=tuple(t // 2 for t in k))
    got = G.tn_reference(c)["C"][0].reshape(ref.shape)
    assert torch.equal(got, ref.double())
    # and lavt_unpack_conv_grad of the unpermuted result is the permuted one
    packed = G.tn_reference(G.unpermuted(c), inp=i)["C"][0]
    assert torch.equal(G.unpack_reference(c, packed, torch.zeros(c.I, 8, G.taps_of(cv), dtype=torch.float64)).reshape(ref.shape), got)


def test_conv_wgrad_reference_is_autograd_of_concat_conv():
    cc = G.ConvCase("host-cw", "", B=2, H=5, W=6, Cout=128, Cin=88, c1=64, accumulate=True)
    i = G.inputs(cc.tn)
    x = torch.cat([i["B"][0], i["B2"]], dim=1).view(2, 5, 6, 88).permute(0, 3, 1, 2)
    w = torch.zeros(128, 88, 3, 3, dtype=torch.float64, requires_grad=True)
    dy = i["A"][0].view(2, 5, 6, 128).permute(0, 3, 1, 2)
    (F.conv2d(x, w, padding=1) * dy).sum().backward()
    assert torch.equal(G.conv_wgrad_reference(cc), w.grad.reshape(128, 88, 9) + i["C0"][0].reshape(128, 88, 9))


def test_integer_reference_is_an_int64_matmul():
    for c in INT_SINGLES[:12] + [G.BY_NAME["s-batch3-amap"], G.BY_NAME["c-maps-taps"], G.BY_NAME["t-3d-333"]]:
        Ae, Bv = G.effective(c)
        acc = torch.matmul((Ae * 2).long().transpose(1, 2), Bv.long())
        C8 = (G.inputs(c)["C0"] * 8).long() + int(c.alpha * 4) * acc
        if c.permute:
            C8 = C8.reshape(c.batch, c.I, G.taps_of(c.conv), c.conv["kc"]).transpose(2, 3).reshape(c.batch, c.I, c.J)
        r = G.tn_reference(c)["C"]
        assert torch.equal((r * 8).long(), C8) and torch.equal(r * 8, C8.double()), c.name


# ------------------------------------------------------------------------------------------------ exactness: "bit-exact on any route" is a theorem
@pytest.mark.parametrize("case", INT_ALL, ids=repr)
def test_integer_cases_are_exact_in_fp32(case):
    """sum_k |alpha s a b| + |initial value| < 2^20 and every addend a multiple of 2^-3: every partial sum, in any order, is a multiple of 2^-3 below 2^20 and
    so has at most 23 significant bits -- fp32 holds it exactly"""
    m, mult = G.exactness(case)
    assert mult and m < 2.0 ** 20, (case.name, m, mult)
    i = G.inputs(case)
    for k in ("A", "B", "B2"):
        if k in i:
            assert float(i[k].abs().max()) <= 3 and torch.equal(i[k], i[k].round())
            assert torch.equal(i[k].to(torch.float8_e4m3fn).double(), i[k]) and torch.equal(i[k].to(torch.bfloat16).double(), i[k])
    r = G.tn_reference(case)
    for t in r.values():
        assert torch.equal(t.float().double(), t) and torch.equal((t * 8).round(), t * 8)


def test_integers_to_16_survive_e4m3():
    v = torch.arange(-16, 17).double()
    assert torch.equal(v.to(torch.float8_e4m3fn).double(), v)


def test_shuffled_fp32_chunk_sums_equal_int64():
    g = torch.Generator().manual_seed(5)
    a, b = torch.randint(-3, 4, (28800,), generator=g), torch.randint(-3, 4, (28800,), generator=g)
    exact = int((a * b).sum())
    for chunk in (64, 450, 1800):
        perm = torch.randperm(28800, generator=g)
        parts = (a[perm].float() * b[perm].float() * 1.25).split(chunk)
        order = torch.randperm(len(parts), generator=g)
        s = torch.zeros((), dtype=torch.float32)
        for j in order:
            s = s + parts[j].sum(dtype=torch.float32)
        assert float(s) == exact * 1.25


# ------------------------------------------------------------------------------------------------ routes
@pytest.mark.parametrize("row", G.ALL_ROUTED, ids=repr)
def test_route_is_the_stated_one(row):
    assert G.tn_route(row) == row.route, (row.name, G.tn_route(row), row.route)
    assert (row.route == G.INVALID) <= bool(row.invalid)


def test_groups_that_do_not_form_run_valid_members():
    for g in G.GROUPS:
        if g.route.startswith("each"):
            t = dict(G.DEFAULT, **g.tuning)
            assert all(G.route_single(c, t) != G.INVALID for c in g.members), g.name


def test_table_covers_the_reachable_instantiations():
    """per __global__ instantiation as the launchers pick them (gemm_tn_cases.reachable: 53 kernels, and the paths a piece count or a host decision
    selects inside them), over the rows that run -- a refused row launches nothing"""
    seen = set().union(*(G.launches(row) for row in G.ALL_ROUTED))
    assert seen == G.reachable(), (sorted(G.reachable() - seen), sorted(seen - G.reachable()))
    assert len([k for k in G.reachable() if "/" not in k]) == 53
    # every rider kernel runs with an odd row count, and the refused rows really are left out
    assert all(g.ln[0] % 2 for g in G.RIDER) and not any(G.launches(r) for r in G.REFUSALS + G.SK_REFUSED + G.CONVW_REFUSED)


def test_forms_and_features_are_all_present():
    """every write form on every single-problem family, and the contract features the issue lists, appear in the table"""
    forms = {(r.route.split("/")[1], r.route.rsplit("/", 1)[1]) for r in G.SINGLE + G.SINGLE_128 + G.TAPS if r.route.startswith("v2")}
    assert forms >= {(t, f) for t in ("64", "128") for f in ("store", "atomic", "parts")}
    ms = list(G.members_of(G.ALL_ROUTED))
    assert any(c.batch > 1 and c.colsum and c.partials for c in ms) and any(c.no_b for c in ms) and any(c.share is not None for c in ms)
    assert any(c.conv and c.conv["d"] > 1 for c in ms) and any(c.b2 and c.conv for c in ms) and any(c.c_off for c in ms) and any(c.part_off for c in ms)
    assert {c.div for c in ms if c.scale} >= {25, 75, 225}
    assert {c.alpha for c in ms if c.mode == "int" and not isinstance(c, G.ConvCase)} >= {1.0, 1.25, -0.5}


def test_build_puts_nan_where_no_kernel_may_read():
    c = G.BY_NAME["s-batch3-amap"]
    b, i = G.build(c), G.inputs(c)
    A = b["A"]
    for bz in range(3):
        v = A[bz * c.strideA:bz * c.strideA + c.Ra_buf * c.lda].view(c.Ra_buf, c.lda)
        assert torch.isnan(v[:, c.I:].float()).all() and torch.isnan(v[c.Ra:].float()).all()
        used = torch.zeros(c.Ra, dtype=torch.bool)
        used[i["a_map"].long()[i["a_map"] >= 0]] = True
        assert torch.isnan(v[:c.Ra][~used].float()).all() and torch.equal(v[:c.Ra][used][:, :c.I].double(), i["A"][bz][used])
        assert torch.isnan(A[bz * c.strideA + c.Ra_buf * c.lda:(bz + 1) * c.strideA if bz < 2 else None].float()).all()
    assert torch.isnan(b["C"][~b["C_own"]]).all() and not torch.isnan(b["C"][b["C_own"]]).any() and int(b["C_own"].sum()) == 3 * c.I * c.J


# ------------------------------------------------------------------------------------------------ planted faults
@pytest.mark.parametrize("fault", G.FAULTS)
def test_planted_fault_is_rejected(fault):
    """applied to the reference, a fault must change the integer result of at least one case it can show on (most: of every such case), and must miss the
    real-mode gate with a factor 2 to spare on every real case it applies to"""
    changed = []
    pool = INT_SINGLES + ([G.BY_NAME["s-batch3"], G.BY_NAME["c-f32-batch3"]] if "batch" in fault else [])
    for c in pool:
        if not G.applies(fault, c):
            continue
        good, bad = G.tn_reference(c), G.tn_reference(c, fault=fault)
        if any(not torch.equal(good[k], bad[k]) for k in good):
            changed.append(c.name)
    assert changed, fault
    for c in G.REAL:
        if not G.applies(fault, c):
            continue
        ref, flo, bad = G.tn_reference(c), G.tn_reference(c, floor=True), G.tn_reference(c, fault=fault, floor=True)
        hit = False
        for k in ref:
            E, Fl = G.nt_error(bad[k], ref[k]), G.nt_error(flo[k], ref[k])
            hit = hit or E >= 2.0 * G.K_TN[k] * Fl and E > 0
        assert hit, (fault, c.name)


def test_k_tn_follows_the_measured_ratios():
    from test_gpu_gemm_tn_cases import MEASURED
    assert set(MEASURED) == set(G.K_TN)
    for n, ratio in MEASURED.items():
        assert G.K_TN[n] == G.k_from_measured(ratio), (n, G.K_TN[n], ratio)
