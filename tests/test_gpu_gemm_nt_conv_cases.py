"""The implicit-GEMM convolution modes of lavt_gemm_nt, one direct launch per (case, forced configuration) through ops.gemm_nt, against their
statement in tests/gemm_nt_conv_cases.py -- and a short product-level part through ops.conv3x3 / ops.conv3d with integer operands.

Mode int (small-integer operands, see gemm_nt_conv_cases.py): every owned element of C, C2, Cpre and of the fp32 partial outputs of a split must equal
the integer reference BIT FOR BIT (the sign of a zero aside), under every tile, ring depth, K walk and weight layout the row runs under; the per-block
column sums of the statistics epilogue likewise (the centred moments stay with test_gpu_ops.test_conv_epilogue_column_statistics).  After a split
case lavt_splitk_reduce and lavt_splitk_reduce_epi (integer bias + ReLU) run on the partial outputs and are exact into bf16.  Mode real (GELU + Cpre +
bias of the Conv3d forward, one plain forward and one data gradient per kernel family): E <= K_CONV x F, the gate of test_gpu_gemm_nt_cases.py, every figure
printed before the test fails.  Beyond the values:
  * A and A2 carry NaN in two guard rows before their first and after their last row (the operand is passed through a_off) and in the columns beyond
    the channels; the weight carries NaN beyond its rows' K and, k-major, in every column outside the b_off column block: a read there poisons the
    result;
  * outputs are pre-filled with NaN and every element the kernel does not own comes back bit-identical: the columns up to ldc / ldc2 / ldcpre, the gap
    between the batch entries of the partial outputs (strideC = M N + 12);
  * a second run is bit-identical;
  * the refusals return LAVT_ERR_INVALID, name the feature in lavt_last_error and leave the outputs untouched; no case is skipped.

Cases: gemm_nt_conv_cases.py states per row the route it is there for; test_gemm_nt_conv_cases_host.py shows that the rows reach every convolution
instantiation of the planner (reachable_conv) and that each listed fault -- a shifted tap, a halo side or face not zeroed, a sample boundary crossed,
conv_flip ignored, the concat sources swapped for a channel block, the partial block padded from the next tap, a tap group on its neighbour's
weights, a channel piece from channel 0, b_tap_stride taken as conv_kc, C2 from column 0, the kernel axes permuted -- changes an integer of a case
named for it; test_gemm_nt_route_host.py holds the library's planner to the same routes.  fp8 convolutions are out of scope.

Product level (default tuning): ops.conv3x3 and ops.conv3d forward and backward with integer operands against float64 F.conv2d / F.conv3d; y, dx1, dx2,
dW (and db) bit-exact.  Shapes take each branch of _ConvTaps: 512 -> 64 on 2 x 5 x 7 (the reduction cut into tap groups, into two channel pieces, and
into what "auto" picks), 256 + 64 -> 64 (the two-launch data gradient), 64 + 32 -> 64 (one launch with C2), 2 x 3 x 4 x 5 under a 3 x 3 x 3 kernel with
bias.  This holds lavt_pack_conv3x3 and the weight-gradient path (fused taps, or the TN GEMM with lavt_unpack_conv_grad) too.

Measured E / F on MI355X, the largest over the real-mode cases of this file: MEASURED below.  Every bf16 output (C, C2, Cpre, GELU included) sits at
1.000 under every kernel family: its error IS the final rounding; k_from_measured gives 2.0, the entry of gemm_nt_cases.K_NT, which is reused.  The
fp32 output of the classic kernel stands at 2.158 (forward, K = 180) and 2.575 (data gradient, K = 648), above the 1.798 of the plain table: the
floor adds one torch matmul per tap, the kernel one chain over all of K.  gemm_nt_conv_cases.K_CONV carries that one entry of its own (5.15);
test_measured_gives_the_gate_factors holds the table to this one.

What the first run of this file found: nothing to fix.  Every integer case was bit-exact on its first launch under every forced configuration, the
partial outputs of both splits, the column sums and both reduce kernels included, and so was the product-level part."""
import os

import pytest
import torch
import torch.nn.functional as F

import gemm_nt_cases as G
import gemm_nt_conv_cases as V

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
NAN = float("nan")
ENV = ("LAVT_GEMM_TILE", "LAVT_GEMM_STAGES", "LAVT_GEMM_PIPE")

# largest E / F per output over the real-mode cases of this file, as measured on MI355X
MEASURED = {"C": 1.000, "C2": 1.000, "Cpre": 1.000, "C.f32": 2.575}


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


def same_bits(got, ref):
    """bit equality of two tensors of one dtype, the sign of a zero aside"""
    return got.shape == ref.shape and torch.equal(bits(got + 0.0), bits(ref + 0.0))


class Launch:
    """the device buffers of one case and its launch"""

    def __init__(self, c):
        self.c = c
        o = V.build(c)
        self.dt = BF if c.dtype == "bf16" else torch.float32
        self.out_dt = torch.float32 if (c.c_f32 or c.dtype == "f32") else BF
        self.A_big = o["A_big"].to(dev())
        self.A2_big = o["A2_big"].to(dev()) if c.C2 else None
        self.B = o["B"].to(dev())
        self.bias = o["bias"].to(dev()) if c.bias else None
        self.stats = None

    def outputs(self):
        c = self.c
        o = {"C": torch.full(((c.batch - 1) * c.strideC + c.M * c.ldc,), NAN, dtype=self.out_dt, device=dev())}
        if c.c_split:
            o["C2"] = torch.full((c.M, c.ldc2), NAN, dtype=self.out_dt, device=dev())
        if c.cpre:
            o["Cpre"] = torch.full((c.M, c.ldcpre), NAN, dtype=self.dt, device=dev())
        return o

    def run(self):
        from lavt_hip import ops
        c, o = self.c, self.outputs()
        buf = dict(o, A_big=self.A_big, B=self.B, bias=self.bias, A2=self.A2_big[V.GUARD:] if c.C2 else None)
        args, kw = V.launch_args(c, buf)
        self.stats = ops.gemm_nt(*args, want_colstats=c.colstats, **kw)
        torch.cuda.synchronize()
        return o

    def owned(self):
        c = self.c
        m = {"C": torch.zeros((c.batch - 1) * c.strideC + c.M * c.ldc, dtype=torch.bool)}
        for b in range(c.batch):
            m["C"][b * c.strideC:b * c.strideC + c.M * c.ldc].view(c.M, c.ldc)[:, :c.Nc] = True
        for name, ld, n in (("C2", c.ldc2, c.N - c.c_split), ("Cpre", c.ldcpre, c.N)):
            if ld:
                m[name] = torch.zeros(c.M, ld, dtype=torch.bool)
                m[name][:, :n] = True
                m[name] = m[name].reshape(-1)
        return m

    def extract(self, o):
        """the buffers as the reference shapes them, in the dtype they are stored in (CPU)"""
        c = self.c
        got = {"C": torch.stack([o["C"][b * c.strideC:b * c.strideC + c.M * c.ldc].view(c.M, c.ldc)[:, :c.Nc] for b in range(c.batch)]).cpu()}
        if "C2" in o:
            got["C2"] = o["C2"][:, :c.N - c.c_split].cpu()
        if "Cpre" in o:
            got["Cpre"] = o["Cpre"][:, :c.N].cpu()
        return got


_REFS = {}


def refs(c):
    if c.name not in _REFS:
        _REFS[c.name] = (V.reference(c), V.floor(c) if c.mode == "real" else None)
    return _REFS[c.name]


RATIOS = {}          # output -> the largest E / F this run saw (printed by test_measured_stays_within_k_nt)


def check_case(c, tag=""):
    """launch twice; hold the second run and the untouched elements bit-identical; int: every owned element bit-equal; real: print every figure, then gate"""
    L = Launch(c)
    a = L.run()
    stats = L.stats
    b = L.run()
    ref, flo = refs(c)
    assert set(a) == set(ref) - {"acc"}, (set(a), set(ref))
    owned = L.owned()
    for k in a:
        assert torch.equal(bits(a[k]), bits(b[k])), f"{c.name} {tag} {k}: second run is not bit-identical"
        fresh = bits(torch.full_like(a[k], NAN)).cpu().reshape(-1)
        rest = ~owned[k]
        assert torch.equal(bits(a[k]).cpu().reshape(-1)[rest], fresh[rest]), f"{c.name} {tag} {k}: an element the kernel does not own was written"
    got = L.extract(a)
    fails = []
    for k in sorted(got):
        r = ref[k].reshape(got[k].shape)
        if c.mode == "int":
            want = r.to(got[k].dtype)
            ok = same_bits(got[k], want)
            wrong = (got[k].double() != r) | ~torch.isfinite(got[k].double())
            print(f"[gemm-nt-conv] {c.name} {tag} {k}: {int(wrong.sum())} of {wrong.numel()} elements differ" +
                  (f", first at {tuple(int(v) for v in torch.nonzero(wrong)[0])}: got {float(got[k][tuple(torch.nonzero(wrong)[0])])} want {float(r[tuple(torch.nonzero(wrong)[0])])}"
                   if bool(wrong.any()) else ""))
            if not ok:
                fails.append((k, int(wrong.sum())))
        else:
            key = c.store_key(k)
            E, Fl, ok = G.gate(key, got[k].float(), r, flo[k].reshape(r.shape), report=True, factors=V.K_CONV)
            ratio = E / Fl if Fl > 0 else (0.0 if E == 0 else float("inf"))
            RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
            print(f"[gemm-nt-conv] {c.name} {tag} {key}: E {E:.3e} F {Fl:.3e} E/F {ratio:.3f} K {V.K_CONV[key]:g}")
            if not ok:
                fails.append((k, E, Fl, ratio))
    if c.colstats:
        assert stats is not None, f"{c.name} {tag}: the launch left no column statistics"
        parts, nblk, rpb = stats
        sums = parts.view(nblk, 2, c.N)[:, 0].cpu()
        want = V.colsums(c, rpb)
        assert want.shape[0] == nblk, (nblk, rpb)
        wrong = sums.double() != want
        print(f"[gemm-nt-conv] {c.name} {tag} colstats sums: {int(wrong.sum())} of {wrong.numel()} differ ({nblk} blocks of {rpb} rows)")
        if bool(wrong.any()) or not bool(torch.isfinite(parts).all()):
            fails.append(("colstats", int(wrong.sum())))
    if c.batch > 1 and c.mode == "int":
        fails += check_reduce(c, got["C"], tag)
    assert not fails, (c.name, tag, fails)


def check_reduce(c, parts_cpu, tag):
    """lavt_splitk_reduce and lavt_splitk_reduce_epi (integer bias + ReLU) on the partial outputs of a split case: exact into bf16"""
    from lavt_hip import _capi as K
    parts = parts_cpu.contiguous().to(dev())          # [pieces, M, N] fp32, contiguous as the reduce kernels read them
    bias = torch.randint(-3, 4, (c.N,), generator=torch.Generator("cpu").manual_seed(5)).float()
    ld, fails = c.N + 8, []
    for name, b, relu in (("reduce", None, False), ("reduce-epi", bias, True)):
        out = torch.full((c.M, ld), NAN, dtype=BF, device=dev())
        if b is None:
            K.check(K.lib.lavt_splitk_reduce(K.dt(BF), K.ptr(parts), c.batch, c.M, c.N, K.ptr(out), ld, K.stream()))
        else:
            K.check(K.lib.lavt_splitk_reduce_epi(K.dt(BF), K.ptr(parts), c.batch, c.M, c.N, K.ptr(b.to(dev())), G.ACT_RELU, K.ptr(out), ld, K.stream()))
        torch.cuda.synchronize()
        want = V.reduced(c, b, relu)
        got = out[:, :c.N].cpu()
        wrong = got.double() != want
        print(f"[gemm-nt-conv] {c.name} {tag} {name}: {int(wrong.sum())} of {wrong.numel()} elements differ")
        if bool(wrong.any()) or not same_bits(got, want.to(BF)):
            fails.append((name, int(wrong.sum())))
        if not torch.equal(bits(out[:, c.N:]), bits(torch.full_like(out[:, c.N:], NAN))):
            fails.append((name, "wrote beyond N"))
    return fails


# ------------------------------------------------------------------------------------------------ the table
def _id(ct):
    return f"{ct[0].name}-{ct[1] or 'default'}"


@pytest.mark.parametrize("case,tuning", V.launches(V.INT_TABLE), ids=[_id(x) for x in V.launches(V.INT_TABLE)])
def test_int_cases(case, tuning, monkeypatch, request):
    """integer operands: bit-exact under the forced (tile, ring depth, pipelined K loop) setting the row states a route for"""
    _tuning(monkeypatch, request, G.tuning_env(tuning) if tuning else {})
    check_case(case, tuning or "default")


@pytest.mark.parametrize("case,tuning", V.launches(V.REAL), ids=[_id(x) for x in V.launches(V.REAL)])
def test_real_cases(case, tuning, monkeypatch, request):
    _tuning(monkeypatch, request, G.tuning_env(tuning) if tuning else {})
    check_case(case, tuning or "default")


def test_measured_gives_the_gate_factors():
    """K = k_from_measured(MEASURED): within gemm_nt_cases.K_NT the entry of that table is reused, beyond it K_CONV holds exactly the derived factor"""
    for key, ratio in MEASURED.items():
        k = G.k_from_measured(ratio)
        assert V.K_CONV[key] == (G.K_NT[key] if k <= G.K_NT[key] else k), (key, ratio, k, V.K_CONV[key])
    assert set(MEASURED) == {c.store_key(k) for c in V.REAL for k in (["C"] + (["C2"] if c.c_split else []) + (["Cpre"] if c.cpre else []))}
    print(f"[gemm-nt-conv] largest E / F of this run: { {k: round(v, 3) for k, v in sorted(RATIOS.items())} }")


# ------------------------------------------------------------------------------------------------ contract refusals
@pytest.mark.parametrize("case", V.REFUSALS, ids=repr)
def test_refusals(case, monkeypatch, request):
    """argument checks in host code: LAVT_ERR_INVALID, the feature named in lavt_last_error, the NaN-filled outputs untouched, nothing launched"""
    _tuning(monkeypatch, request, case.env or {})
    L = Launch(case)
    seen, orig = {}, L.outputs

    def keep():
        seen.update(orig())
        return seen
    L.outputs = keep
    with pytest.raises(RuntimeError, match=r"rc=-22: lavt_gemm_nt") as e:
        L.run()
    torch.cuda.synchronize()
    assert case.word in str(e.value), str(e.value)
    assert seen
    for k, t in seen.items():
        assert torch.equal(bits(t), bits(torch.full_like(t, NAN))), f"{case.name}: {k} was written by a refused launch"


# ------------------------------------------------------------------------------------------------ product level
def _ints(lo, hi, *shape, seed):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator("cpu").manual_seed(seed)).double()


def _ternary(p, *shape, seed):
    g = torch.Generator("cpu").manual_seed(seed)
    return (torch.randint(0, 2, shape, generator=g).double() * 2 - 1) * (torch.rand(*shape, generator=g) < p).double()


def _product(geom, ks, C1, C2, Cout, bias, p, name):
    """ops.conv3x3 / ops.conv3d forward + backward on integer operands against float64 autograd: y, dx1, dx2, dW, db exact"""
    import lavt_hip
    from lavt_hip import ops
    B, D, H, W = geom
    Cin, M, three_d = C1 + C2, B * D * H * W, len(ks) == 3
    x1, x2 = _ints(-2, 2, M, C1, seed=1), (_ints(-2, 2, M, C2, seed=2) if C2 else None)
    w, b = _ternary(p, Cout, Cin, *ks, seed=3), (_ints(-3, 3, Cout, seed=4) if bias else None)
    dy = _ints(-1, 1, M, Cout, seed=5)
    r1, r2, rw, rb = (t.clone().requires_grad_(True) if t is not None else None for t in (x1, x2, w, b))
    xin = (r1 if r2 is None else torch.cat([r1, r2], 1)).view(B, D, H, W, Cin).permute(0, 4, 1, 2, 3)
    yr = F.conv3d(xin, rw if three_d else rw.unsqueeze(2), rb, padding=tuple(k // 2 for k in (ks if three_d else (1,) + tuple(ks))))
    yr = yr.permute(0, 2, 3, 4, 1).reshape(M, Cout)
    yr.backward(dy)
    d = dev()
    g1 = x1.to(d).to(BF).requires_grad_(True)
    g2 = x2.to(d).to(BF).requires_grad_(True) if C2 else None
    gw = w.float().to(d).requires_grad_(True)
    gb = b.float().to(d).requires_grad_(True) if bias else None
    ops.weights.invalidate()
    with lavt_hip.use_dtype(BF):
        y = ops.conv3d(g1, gw, gb, B, D, H, W) if three_d else ops.conv3x3(g1, g2, gw, B, H, W)
        y.backward(dy.to(d).to(BF))
    torch.cuda.synchronize()
    pairs = [("y", y.detach(), yr.detach()), ("dx1", g1.grad, r1.grad), ("dW", gw.grad, rw.grad)]
    if C2:
        pairs.append(("dx2", g2.grad, r2.grad))
    if bias:
        pairs.append(("db", gb.grad, rb.grad))
    fails = []
    for k, got, ref in pairs:
        assert got is not None, f"{name}: no {k}"
        got = got.cpu()
        assert bool((ref.to(got.dtype).double() == ref).all()), f"{name} {k}: the reference is not representable (max {float(ref.abs().max())})"
        wrong = (got.double() != ref.reshape(got.shape)) | ~torch.isfinite(got.double())
        print(f"[gemm-nt-conv] product {name} {k}: {int(wrong.sum())} of {wrong.numel()} elements differ (max |ref| {float(ref.abs().max()):g})")
        if bool(wrong.any()):
            fails.append((k, int(wrong.sum())))
    assert not fails, (name, fails)


@pytest.mark.parametrize("pieces", ["0", "2", "auto"])
def test_product_conv3x3_split_reduction(pieces, monkeypatch, request):
    """512 -> 64 on 2 x 5 x 7: K = 4608 on 70 rows, the reduction cut into tap groups ("0"), two channel pieces ("2") or what "auto" picks"""
    from lavt_hip import ops
    _tuning(monkeypatch, request, {})
    monkeypatch.setattr(ops, "_CONV_KC_SPLITS", pieces)
    assert ops._conv_split(BF, 70, 64, 512, 512, 0, 9, None, 0) == {"0": (3, False), "2": (2, True), "auto": (8, True)}[pieces]
    _product((2, 1, 5, 7), (3, 3), 512, 0, 64, False, 0.125, f"512->64 pieces={pieces}")


@pytest.mark.parametrize("C1,C2,name", [(256, 64, "two-launch data gradient"), (64, 32, "one launch with C2")])
def test_product_conv3x3_concat(C1, C2, name, monkeypatch, request):
    _tuning(monkeypatch, request, {})
    _product((2, 1, 5, 7), (3, 3), C1, C2, 64, False, 0.25 if C1 > 64 else 0.5, f"{C1}+{C2}->64 {name}")


def test_product_conv3d(monkeypatch, request):
    _tuning(monkeypatch, request, {})
    _product((2, 3, 4, 5), (3, 3, 3), 64, 0, 64, True, 0.25, "3x3x3 64->64 bias")
