"""The TN weight-gradient family, one direct launch per case, against its statement in tests/gemm_tn_cases.py: lavt_gemm_tn, lavt_gemm_tn_grouped,
_grouped_ln, _grouped_sk, lavt_conv3x3_wgrad, lavt_conv3x3_wgrad_f8 and lavt_unpack_conv_grad.

A test builds the operands on the CPU, fills a lavt_gemm_tn_t through gemm_tn_cases.launch_args -> ops.gemm_tn_params (split_k, partials and zeros set on the struct) and
calls the entry point itself.  Integer mode (small-integer operands: every partial sum exact in fp32, see gemm_tn_cases.py) holds C and colsum to the
integer reference with torch.equal -- on every route, whatever the tile, the K pieces, the order atomics land in.  Real mode holds them to
E <= K_TN x F (E: the larger of the row and the column relative error against fp64, F: the same error of the fp32 floor evaluated by torch); every figure
is printed before the test fails.  Beyond the values:
  * A, B and B2 carry NaN in the columns beyond I / J, in source rows no map entry names, in the rows at and beyond K and between batch entries; the
    partials / stream-K / conv scratch is NaN-filled; a read there poisons the result;
  * C and colsum are NaN wherever the kernel does not own them (beyond J up to ldc, between batch entries, in front of an offset C) and must come back
    bit-identical there;
  * a second run is bit-identical: in integer mode on every route, in real mode on the routes without atomics (unsplit stores, partial tiles, stream-K,
    the fused conv gradients);
  * a case the table says runs and that returns an error fails; no case is skipped.

Routes (gemm_tn_cases.py states one per row; test_gemm_tn_cases_host.py holds the restated planners to it and shows that the rows launch each of the 53
__global__ instantiations the launchers can pick, both reducers of the pipelined launch on both of their loops included):
single problems on gemm_tn_v2's 64x64 and 128x128 tiles (plain / mapped K loop, scalar / matrix-core column sums, with and without tap state; stores,
atomics, partial tiles; batch 3), the classic kernel (fp32; bf16 with a non-binary row scale, without a zero page, with maps under taps / B2; tiles 64
and 128), 2-D and 3-D taps with B2 and the permuted store, the grouped 64x64 launch (uncut, cut through atomics, cut through partials, groups that do not
form), the pipelined grouped launch (ring depths 3 and 4, uncut and cut, fall-backs), the LayerNorm rider on both, stream-K, both fused conv gradients,
and the refusals.

Measured E / F on MI355X, the largest over the real-mode cases of this file (gemm_tn_cases.K_TN = 2 x that, rounded up, never under 1): MEASURED below,
per route (C / colsum; the floor of a column sum adds the K rows in sequence, as the kernels do): v2 64x64 store 1.013 / 1.000, atomic 0.505 / 1.000, partial
tiles 0.680 / 9.410 (one element with a near-cancelled value, see K_TN), 128x128 0.773 / 1.000, taps 0.858 / exact; classic fp32 0.570 / 1.398, bf16 with a
non-binary scale 0.708 / 3.885; grouped 64x64 uncut 0.896 / 1.000, through partial tiles 1.134 / 4.518 (K = 3144); pipelined uncut 1.339 / 1.000, cut
1.063 / 1.000; stream-K 1.037 / 0.647; the fused conv gradient 1.127.  The integer cases have no figure: they are equal or they fail.

What the first run of this file found: every integer case was exact on every route except the column sums of the classic kernel (gemm_tn_kernel of
csrc/gemm.hip), which left alpha out -- 16 rows, and 20 % = 1 - 1 / 1.25 missing from the fc2 bias gradient of an MLP node under DropPath in fp32
(test_mlp_bias_gradient_under_droppath).  The kernel now multiplies its column sum by alpha as the LDS-DMA kernels do; the header states the contract.
The rows added for the reducers of the cut pipelined launch found a second one: a column-sum-only side member cut into pieces stores no C pieces, and both
tnp_reduce_pieces and tnp_reduce_pieces_deep added that never-written scratch into its C (NaN here; in the model that C is a discard buffer, so no
gradient was wrong).  Both reducers now leave the C of such a member alone."""
import ctypes
import os

import pytest
import torch

import gemm_tn_cases as G

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
NAN = float("nan")
ENV = tuple(G.ENV.values())
# largest E / F per output over the real-mode cases of this file, as measured on MI355X (the table K_TN in gemm_tn_cases.py is derived from)
MEASURED = {"C": 1.339, "colsum": 9.410}


def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m 'not gpu' elsewhere)"
    return torch.device("cuda:0")


def _tuning(monkeypatch, request, t):
    """force (or, with an empty dict, clear) the planner switches for one test; the library re-reads them now and again afterwards"""
    from lavt_hip import _capi as K
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in G.tuning_env(t).items():
        monkeypatch.setenv(k, v)
    K.lib.lavt_tuning_reload()
    request.addfinalizer(lambda: ([os.environ.pop(k, None) for k in ENV], K.lib.lavt_tuning_reload()))


def bits(t):
    return t.contiguous().view(torch.int32)


def _ratio(E, F):
    """E / F for the report (a floor of exactly zero: 0 when the kernel is exact too, else inf)"""
    return E / F if F > 0 else (0.0 if E == 0 else float("inf"))


class Member:
    """the device buffers of one problem and its struct"""

    def __init__(self, c, colsum_of=None):
        from lavt_hip import ops
        self.c, self.host = c, G.build(c)
        h, d = self.host, dev()
        self.A = h["A"].to(d)
        self.B = h["B"].to(d) if "B" in h else ops._zero_page_tensor(d)
        self.B2 = h["B2"].to(d) if "B2" in h else None
        self.a_map, self.b_map, self.scale = (h[k].to(d) if k in h else None for k in ("a_map", "b_map", "scale"))
        self.colsum_of = colsum_of
        self.parts = torch.full((c.partials_floats + c.part_off,), NAN, device=d) if c.partials is not None else None

    def fresh(self):
        """new output buffers holding the initial values (NaN wherever the kernel owns nothing); the partials scratch is all NaN again before every launch"""
        c, h, d = self.c, self.host, dev()
        if self.parts is not None:
            self.parts.fill_(NAN)
        self.C = torch.cat([torch.full((c.c_off,), NAN), h["C"]]).to(d)
        self.cs = None
        if c.colsum:
            self.cs = self.colsum_of.cs if self.colsum_of is not None else h["colsum"].to(d)
        self.C0, self.cs0 = self.C.clone(), (self.cs.clone() if self.cs is not None else None)

    def struct(self):
        from lavt_hip import _capi as K, ops
        c = self.c
        buf = dict(A=self.A, B=self.B, B2=self.B2, a_map=self.a_map, b_map=self.b_map, scale=self.scale, C=self.C, colsum=self.cs, parts=self.parts)
        args, kw, finish = G.launch_args(c, buf)
        p = finish(ops.gemm_tn_params(*args, **kw), K.ptr)
        assert (p.a_src_rows, p.b_src_rows) == (self.A.numel() // c.lda if c.a_map else 0, self.B.numel() // max(c.ldb, 1) if c.b_map else 0)
        return p

    def owned(self):
        c, h = self.c, self.host
        return torch.cat([torch.zeros(c.c_off, dtype=torch.bool), h["C_own"]]), h["cs_own"]

    def got(self):
        c = self.c
        return G.extract(c, self.C[c.c_off:].cpu(), self.cs.cpu() if self.cs is not None else None)


def _expected(members, floor=False):
    """per member {'C', 'colsum'}; the members that share a bias gradient expect the sum of both contributions in it"""
    refs = [G.tn_reference(m.c, floor=floor) for m in members]
    for k, m in enumerate(members):
        if m.c.share is not None:
            s = m.c.share
            own0, first0 = G.inputs(m.c)["cs0"], G.inputs(members[s].c)["cs0"]
            total = refs[s]["colsum"] + (refs[k]["colsum"] - own0)
            refs[s]["colsum"] = refs[k]["colsum"] = total
            assert first0.shape == own0.shape
    return refs


def _verify(name, route, members, launch, second=True):
    """launch, compare every owned buffer (bit for bit in integer mode, through the gate in real mode), hold everything else untouched, launch again on
    fresh outputs and hold the result bit-identical where the route promises it"""
    def once():
        for m in members:
            m.fresh()
        launch([m.struct() for m in members])
        torch.cuda.synchronize()
        return [(m.C.clone(), m.cs.clone() if m.cs is not None else None) for m in members]
    first = once()
    mode = members[0].c.mode
    ref, flo = _expected(members), (_expected(members, floor=True) if mode == "real" else None)
    fails = []
    for k, m in enumerate(members):
        oc, ocs = m.owned()
        assert torch.equal(bits(m.C).cpu()[~oc], bits(m.C0).cpu()[~oc]), f"{m.c.name}: C was written outside the I x J block the kernel owns"
        if m.cs is not None:
            assert torch.equal(bits(m.cs).cpu()[~ocs], bits(m.cs0).cpu()[~ocs]), f"{m.c.name}: colsum was written between the batch entries"
        C, cs = m.got()
        for key, g in (("C", C), ("colsum", cs)):
            if key not in ref[k]:
                continue
            r = ref[k][key]
            if mode == "int":
                bad = g.double() != r
                if bool(bad.any()) or not bool(torch.isfinite(g).all()):
                    idx = torch.nonzero(bad | ~torch.isfinite(g).reshape(bad.shape))
                    fails.append((m.c.name, key, int(idx.shape[0]), idx[:4].tolist(), g[tuple(idx[0])].item(), r[tuple(idx[0])].item()))
            else:
                E, Fl, ok = G.gate(key, g, r, flo[k][key])
                ratio = _ratio(E, Fl)
                print(f"[gemm-tn] {m.c.name} {route} {key}: E {E:.3e} F {Fl:.3e} E/F {ratio:.3f} K {G.K_TN[key]:g}")
                if not ok:
                    fails.append((m.c.name, key, E, Fl, ratio))
    assert not fails, (name, route, fails)
    if second and (mode == "int" or G.order_free(route)):
        again = once()
        for m, (a, acs), (b, bcs) in zip(members, first, again):
            assert torch.equal(bits(a), bits(b)), f"{m.c.name}: C of a second run is not bit-identical"
            assert acs is None or torch.equal(bits(acs), bits(bcs)), f"{m.c.name}: colsum of a second run is not bit-identical"


def _members(cases):
    ms = []
    for c in cases:
        ms.append(Member(c, colsum_of=ms[c.share] if c.share is not None else None))
    return ms


def _launch_single(structs):
    from lavt_hip import _capi as K
    for p in structs:
        K.check(K.lib.lavt_gemm_tn(ctypes.byref(p), K.stream()))


def check_single(c):
    _verify(c.name, c.route, _members([c]), _launch_single)


# ------------------------------------------------------------------------------------------------ single problems
@pytest.mark.parametrize("case", G.SINGLE + G.SINGLE_128 + G.CLASSIC + G.TAPS, ids=repr)
def test_single_exact(case, monkeypatch, request):
    _tuning(monkeypatch, request, case.tuning)
    check_single(case)


@pytest.mark.parametrize("case", G.REAL, ids=repr)
def test_single_real(case, monkeypatch, request):
    _tuning(monkeypatch, request, case.tuning)
    check_single(case)


@pytest.mark.parametrize("case", G.UNPACK, ids=repr)
def test_unpack_conv_grad_equals_the_permuted_store(case, monkeypatch, request):
    """lavt_unpack_conv_grad of the unpermuted result, added into zeros, is the c_conv_permute result, value for value (the addition into +0 turns the
    -0 a negative alpha stores for an empty sum into +0: the one difference of bits there can be)"""
    from lavt_hip import _capi as K
    _tuning(monkeypatch, request, case.tuning)
    u = G.unpermuted(case)
    G._INPUTS[u.name] = G.inputs(case)          # the same operands
    a, b = _members([case])[0], _members([u])[0]
    for m in (a, b):
        m.fresh()
        _launch_single([m.struct()])
    packed = b.got()[0][0].contiguous().to(dev())
    dw = torch.zeros(case.I, case.conv["kc"], G.taps_of(case.conv), device=dev())
    K.check(K.lib.lavt_unpack_conv_grad(K.ptr(packed), K.ptr(dw), case.I, case.conv["kc"], G.taps_of(case.conv), K.stream()))
    torch.cuda.synchronize()
    want = a.got()[0][0].to(dev())
    assert torch.equal(dw.reshape(case.I, -1), want) and torch.isfinite(dw).all()
    assert torch.equal(dw.reshape(case.I, -1).cpu().double(), G.tn_reference(case)["C"][0])


# ------------------------------------------------------------------------------------------------ groups
def _launch_group(g, ln_args=None):
    from lavt_hip import _capi as K

    def go(structs):
        arr = (K.GemmTN * len(structs))(*structs)
        if g.entry == "sk":
            ws = int(K.lib.lavt_gemm_tn_grouped_sk_ws(arr, len(structs)))
            assert ws > 0 and ws == G.sk_plan(g.members)[1], (ws, G.sk_plan(g.members))
            scratch = torch.full((ws,), NAN, device=dev())
            K.check(K.lib.lavt_gemm_tn_grouped_sk(arr, len(structs), K.ptr(scratch), ws, K.stream()))
        elif g.entry == "ln":
            ln_args(arr, len(structs))
        else:
            K.check(K.lib.lavt_gemm_tn_grouped(arr, len(structs), K.stream()))
    return go


@pytest.mark.parametrize("group", G.GROUP64 + G.PIPE + G.STREAMK + G.REAL_GROUPS, ids=repr)
def test_group(group, monkeypatch, request):
    _tuning(monkeypatch, request, group.tuning)
    _verify(group.name, group.route, _members(group.members), _launch_group(group))


@pytest.mark.parametrize("group", G.RIDER, ids=repr)
def test_rider(group, monkeypatch, request):
    """lavt_gemm_tn_grouped_ln: the weight gradients stay exact, dx and the partial sums of the LayerNorm stay bit-identical to lavt_layernorm_bwd_partial"""
    from lavt_hip import _capi as K
    _tuning(monkeypatch, request, group.tuning)
    rows, Cn = group.ln
    g = torch.Generator().manual_seed(rows * 7 + Cn)
    mk = lambda s=0.5: (torch.randn(rows, Cn, generator=g) * s).to(dev()).to(BF)
    dy, x, dres = mk(), mk(1.0), mk()
    gamma = (1.0 + 0.1 * torch.randn(Cn, generator=g)).to(dev())
    mean, rstd = x.float().mean(1), torch.rsqrt(x.float().var(1, unbiased=False) + 1e-5)
    nblk = int(K.lib.lavt_layernorm_bwd_blocks(K.BF16, rows, Cn))
    assert nblk == G.ln_geometry(rows, Cn)[0]
    out = {}

    def ln_args(arr, n):
        out["dx"], out["ws"] = torch.full((rows, Cn), NAN, dtype=BF, device=dev()), torch.full((nblk * 2 * Cn,), NAN, device=dev())
        K.check(K.lib.lavt_gemm_tn_grouped_ln(arr, n, K.ptr(dy), K.ptr(x), K.ptr(gamma), K.ptr(mean), K.ptr(rstd), K.ptr(out["dx"]), K.ptr(out["ws"]), out["ws"].numel(),
                                              K.ptr(dres), rows, Cn, K.stream()))
    _verify(group.name, group.route, _members(group.members), _launch_group(group, ln_args))
    dx, ws = torch.full((rows, Cn), NAN, dtype=BF, device=dev()), torch.full((nblk * 2 * Cn,), NAN, device=dev())
    K.check(K.lib.lavt_layernorm_bwd_partial(K.BF16, K.ptr(dy), K.ptr(x), None, K.ptr(gamma), K.ptr(mean), K.ptr(rstd), K.ptr(dx), K.ptr(ws), ws.numel(), K.ptr(dres), rows, Cn,
                                             K.stream()))
    torch.cuda.synchronize()
    assert torch.equal(dx.view(torch.int16), out["dx"].view(torch.int16)) and torch.isfinite(dx.float()).all()
    assert torch.equal(bits(ws), bits(out["ws"])) and torch.isfinite(ws).all()


# ------------------------------------------------------------------------------------------------ fused conv weight gradients
def _conv_run(cc, scratch_floats=None):
    from lavt_hip import _capi as K, ops
    c, d = cc.tn, dev()
    h = G.build(c)
    ws = int(K.lib.lavt_conv3x3_wgrad_ws(cc.B, cc.H, cc.W, cc.Cout, cc.Cin, cc.c1 or cc.Cin))
    assert ws == G.cw_ws(cc), (ws, G.cw_ws(cc))
    if cc.f8:
        assert int(K.lib.lavt_conv3x3_wgrad_f8_ok(cc.B, cc.H, cc.W, cc.Cout, cc.Cin, cc.c1 or cc.Cin)) == int(G.cw_supported(cc))
    conv = (lambda t: t.float().to(torch.float8_e4m3fn).view(torch.uint8).to(d)) if cc.f8 else (lambda t: t.to(d))
    dy, x1, x2 = conv(h["A"]), conv(h["B"]), (conv(h["B2"]) if "B2" in h else None)
    n = ws if scratch_floats is None else scratch_floats
    parts = torch.full((max(n, 1),), NAN, device=d)
    dW = h["C"].clone() if cc.accumulate else torch.full_like(h["C"], NAN)          # accumulate == 0 overwrites: nothing of the old content may survive
    dW = dW.to(d)
    before = dW.clone()
    z = ops._zero_page(d)
    if cc.f8:
        am = [torch.tensor([a], device=d) for a in cc.amax]
        rc = K.lib.lavt_conv3x3_wgrad_f8(K.ptr(dy), c.lda, K.ptr(am[0]), K.ptr(x1), c.ldb, K.ptr(x2), c.ldb2, K.ptr(am[1]), cc.c1, cc.B, cc.H, cc.W, cc.Cout, cc.Cin, K.ptr(parts),
                                         n, K.ptr(dW), int(cc.accumulate), z, K.stream())
    else:
        rc = K.lib.lavt_conv3x3_wgrad(K.ptr(dy), c.lda, K.ptr(x1), c.ldb, K.ptr(x2), c.ldb2, cc.c1, cc.B, cc.H, cc.W, cc.Cout, cc.Cin, K.ptr(parts), n, K.ptr(dW),
                                      int(cc.accumulate), z, K.stream())
    torch.cuda.synchronize()
    return int(rc), dW, before


@pytest.mark.parametrize("cc", G.CONVW + G.CONVW8 + G.REAL_CONVW, ids=repr)
def test_conv_wgrad(cc):
    rc, dW, _ = _conv_run(cc)
    assert rc == 0, rc
    ref = G.conv_wgrad_reference(cc)
    got = dW.cpu().reshape(ref.shape)
    if cc.mode == "int":
        bad = torch.nonzero(got.double() != ref)
        assert bad.shape[0] == 0, (cc.name, cc.route, int(bad.shape[0]), bad[:4].tolist(), got[tuple(bad[0])].item(), ref[tuple(bad[0])].item())
    else:
        flo = G.conv_wgrad_reference(cc, floor=True)
        E, Fl, ok = G.gate("C", got.reshape(cc.Cout, -1), ref.reshape(cc.Cout, -1), flo.reshape(cc.Cout, -1))
        print(f"[gemm-tn] {cc.name} {cc.route} C: E {E:.3e} F {Fl:.3e} E/F {_ratio(E, Fl):.3f} K {G.K_TN['C']:g}")
        assert ok, (cc.name, E, Fl)
    rc2, dW2, _ = _conv_run(cc)
    assert rc2 == 0 and torch.equal(bits(dW), bits(dW2)), "a second run is not bit-identical"


# ------------------------------------------------------------------------------------------------ refusals
def _refused(rc, K, word):
    assert rc == -22, rc          # LAVT_ERR_INVALID
    msg = K.lib.lavt_last_error()
    assert msg and word in msg, msg


@pytest.mark.parametrize("case", G.REFUSALS, ids=repr)
def test_refusals(case, monkeypatch, request):
    from lavt_hip import _capi as K
    _tuning(monkeypatch, request, {})
    m = _members([case])[0]
    m.fresh()
    rc = int(K.lib.lavt_gemm_tn(ctypes.byref(m.struct()), K.stream()))
    torch.cuda.synchronize()
    _refused(rc, K, b"lavt_gemm_tn")
    assert torch.equal(bits(m.C), bits(m.C0)) and (m.cs is None or torch.equal(bits(m.cs), bits(m.cs0))), "a refused launch wrote an output"


@pytest.mark.parametrize("group", G.SK_REFUSED, ids=repr)
def test_streamk_refusals(group, monkeypatch, request):
    """a group lavt_gemm_tn_grouped_sk_ws answers 0 for, and a scratch one float short"""
    from lavt_hip import _capi as K
    _tuning(monkeypatch, request, group.tuning)
    ms = _members(group.members)
    for m in ms:
        m.fresh()
    structs = [m.struct() for m in ms]
    arr = (K.GemmTN * len(structs))(*structs)
    ws = int(K.lib.lavt_gemm_tn_grouped_sk_ws(arr, len(structs)))
    plan = G.sk_plan(group.members)
    assert ws == (plan[1] if plan else 0)
    n = ws - 1 if group.scratch == "short" else 1 << 20
    scratch = torch.full((n,), NAN, device=dev())
    rc = int(K.lib.lavt_gemm_tn_grouped_sk(arr, len(structs), K.ptr(scratch), n, K.stream()))
    torch.cuda.synchronize()
    _refused(rc, K, b"lavt_gemm_tn_grouped_sk")
    for m in ms:
        assert torch.equal(bits(m.C), bits(m.C0)), "a refused launch wrote an output"
    assert torch.isnan(scratch).all()


@pytest.mark.parametrize("cc", G.CONVW_REFUSED, ids=repr)
def test_conv_wgrad_refusals(cc):
    from lavt_hip import _capi as K
    short = cc.scratch == "short"
    rc, dW, before = _conv_run(cc, scratch_floats=G.cw_ws(cc) - 1 if short else 1 << 16)
    _refused(rc, K, b"lavt_conv3x3_wgrad")
    assert torch.equal(bits(dW), bits(before)), "a refused launch wrote dW"
    if not short:
        assert G.cw_ws(cc) == 0 or cc.f8


# ------------------------------------------------------------------------------------------------ the colsum contract at the ops level
@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
def test_mlp_bias_gradient_under_droppath(dtype):
    """an MLP node under DropPath (row_scale in {0, 1 / keep}, the value folded into alpha of the fc2 weight-gradient launch): the fc2 bias gradient is
    sum_m s_m dy_m, 1 / keep included, in both compute types (fp32 takes the classic kernel, whose column sum once left alpha out)"""
    from lavt_hip import ops
    g = torch.Generator().manual_seed(9)
    M, Cc, v = 100, 64, 1.25
    x0 = torch.randn(M, Cc, generator=g).to(dtype)
    ws = [torch.randn(2 * Cc, Cc, generator=g) * Cc ** -0.5, torch.randn(2 * Cc, generator=g) * 0.1, torch.randn(Cc, 2 * Cc, generator=g) * (2 * Cc) ** -0.5,
          torch.randn(Cc, generator=g) * 0.1]
    mask = torch.tensor([v, 0.0, v, v])
    dy = torch.randn(M, Cc, generator=g).to(dtype)
    ps = [torch.nn.Parameter(w.clone().to(dev())) for w in ws]
    y = ops.mlp(x0.to(dev()), ps[0], ps[1], ps[2], ps[3], row_scale=mask.to(dev()), row_scale_div=M // 4, row_scale_value=v)
    y.backward(dy.to(dev()))
    torch.cuda.synchronize()
    s = mask[torch.arange(M) // (M // 4)].double()
    rs = [torch.nn.Parameter(w.clone().double()) for w in ws]
    h = torch.nn.functional.gelu(torch.nn.functional.linear(x0.double(), rs[0], rs[1]))
    (torch.nn.functional.linear(h, rs[2], rs[3]) * s[:, None] * dy.double()).sum().backward()
    db2, ref = ps[3].grad.double().cpu(), rs[3].grad
    err = float((db2 - ref).abs().max()) / float(ref.abs().max())
    print(f"[gemm-tn] mlp {dtype} fc2 bias gradient: relative error {err:.3e}")
    assert err <= 1e-5, err          # sums of 75 fp32 / bf16 values times 1.25 in fp32: no rounding of the operands is involved
