"""The implicit-GEMM convolution modes of lavt_gemm_nt (include/lavt_hip.h: conv_kc > 0) stated twice, the case table of their per-kernel parity tests
and the list of convolution instantiations the planner can reach.  CPU only, pure torch, nothing imported from the product or from oracle/; builds on
gemm_nt_cases.py (nt_error, gate, k_from_measured, TUNINGS, Route, route -- which restates the planner for convolutions too).

A case (ConvCase) is ONE launch with conv_kc > 0: a (B, D, H, W) voxel grid, a (kd, kh, kw) kernel, the channel concat C1 + C2 of two sources
(A2 / a_split), N output columns; forward = k-contiguous weights [N][taps][Cin]; data gradient = conv_flip, k-major weights found through b_tap_stride
and b_off inside the packed forward weight [conv_kc][taps][Nw], optionally the second output C2 / c_split; conv_tap_split / conv_kc_split with batch,
strideB, strideC and fp32 partial outputs; bias, act, Cpre, colstats, alpha; bf16 / fp32.

Mode "int": activations uniform integers in [-2, 2], weights in {-1, 0, 1} (non-zero with probability p), integer bias, alpha in {1, 0.5}.  Every
partial sum in every order is exact in fp32 and every stored value is representable in its type (test_gemm_nt_conv_cases_host.py checks that per
case, and that the addends' magnitudes stay under 2^24 and that fewer than 5 % of the outputs are zero), so the kernel must return the reference BIT
FOR BIT: a misplaced tap, pixel, channel block or piece changes an integer.  Mode "real" only for what integers cannot state (GELU): normal operands
rounded to the dtype, fp64 reference, fp32 / bf16 floor by torch, gate E <= K x F as in gemm_nt_cases.py.

Two statements of the contract, held equal by the host test:
  (a) `index_reference`: the index form of the header, evaluated on the PHYSICAL buffers `build` lays out -- k = tap * conv_kc + c,
      tap = ((dz+1) kh + (dy+1)) kw + (dx+1) over the axes of size 3, source row = the neighbour voxel inside its own zero-padded sample (mirrored
      under conv_flip), channels >= a_split from A2, weights at B + n ldb + k or, k-major, B + c ldb + tap b_tap_stride + n; entry bz of a split
      contracts its taps / channels only.  `fault=` plants one defect (FAULTS: the named cases must reject it).
  (b) `conv_reference`: F.conv3d in float64 on the logical tensors for the forward, autograd's input gradient for the flipped form.

`build(case)` puts NaN wherever no kernel may read: the columns between the channels and lda / lda2 / ldb, two guard rows before the first and after
the last row of A and A2 (the operand is passed through a_off into the larger tensor), the weight rows' columns outside the b_off column block, and
(the outputs, pre-filled by the GPU test) the gap between batch entries of the partial outputs.

fp8 convolutions are out of scope."""
import collections
import math

import torch
import torch.nn.functional as F

import gemm_nt_cases as G
from gemm_nt_cases import ACT_GELU, ACT_NONE, BF, INVALID, NAN, TUNINGS, TUNINGS_F32, bf, cdiv

GUARD = 2          # NaN rows before and after A / A2

# Gate factors of the real-mode cases, per output: gemm_nt_cases.K_NT wherever twice the largest E / F measured on MI355X over the convolution rows
# (the MEASURED table of test_gpu_gemm_nt_conv_cases.py) stays within it -- every bf16 output: 1.000, the final rounding -- and one entry of its own:
# "C.f32", the fp32 output of the classic kernel, measured at 2.575 (K = 648 data gradient) and 2.158 (K = 180).  The floor of this file adds one
# torch matmul per tap (blocked sums of conv_kc products, then 9 or 27 partial results), the kernel one sequential chain over all of K: the same
# values, a longer chain, an error of the order of the K sum on both sides (E 5.8e-07, F 2.2e-07).
K_CONV = dict(G.K_NT, **{"C.f32": 5.15})


class ConvCase:
    """One lavt_gemm_nt launch with conv_kc > 0.  geom = (B, D, H, W); kern = (kd, kh, kw); C1 + C2 = conv_kc; N columns; dgrad: the flipped k-major
    form, whose weight is the packed forward weight [conv_kc][taps][Nw] read at column block [b_off, b_off + N); `route`: the route the row is there
    for as "K walk / layout / lean", one per kernel family where they differ ({"pipe": ..., "v2": ...}, a tile-specific key "pipe/256" first);
    `tunings`: the forced configurations it runs under (None: the default tuning, `route` then states the whole route)."""
    DEFAULTS = dict(geom=(2, 1, 5, 7), kern=(1, 3, 3), C1=64, C2=0, dgrad=False, Nw=0, b_off=0, c_split=0, tap_split=0, kc_split=0, stride_x=0, bias=False,
                    act=ACT_NONE, cpre=False, colstats=False, alpha=1.0, dtype="bf16", mode="int", p=None, lda_x=8, lda2_x=16, ldb_x=8, ldc_x=0, ldc2_x=0,
                    ldcpre_x=0, seed=0, route=None, tunings=None, invalid=False, word="", env=None, why="", K=None, batch=None, c_f32=None, M=None)
    # what route() asks of a plain case and no convolution has
    ln = mul = R = row_scale = c_map = a_map = res_first = False
    dact, bias_off = None, 0

    def __init__(self, name, N, **kw):
        bad = set(kw) - set(self.DEFAULTS)
        assert not bad, bad
        self.name, self.N, self.kw = name, N, dict(kw)
        for k, v in self.DEFAULTS.items():
            setattr(self, k, kw.get(k, v))
        self.B_, self.D, self.H, self.W = self.geom
        self.kd, self.kh, self.kw_ = self.kern
        self.taps, self.vox = self.kd * self.kh * self.kw_, self.D * self.H * self.W
        self.M = self.M or self.B_ * self.vox
        self.conv_kc, self.a_split, self.C2src = self.C1 + self.C2, (self.C1 if self.C2 else 0), bool(self.C2)
        self.conv_h, self.conv_w, self.conv_tap_split, self.conv_kc_split = self.H, self.W, self.tap_split, self.kc_split
        self.kmajor = self.dgrad
        self.es = 8 if self.dtype == "bf16" else 4
        split = self.tap_split or self.kc_split
        if self.batch is None:
            self.batch = self.taps // self.tap_split if self.tap_split else (self.conv_kc // self.kc_split if self.kc_split else 1)
        if self.K is None:
            self.K = self.tap_split * self.conv_kc if self.tap_split else (self.taps * self.kc_split if self.kc_split else self.taps * self.conv_kc)
        if self.c_f32 is None:
            self.c_f32 = bool(split)
        self.Nw = self.Nw or self.N
        self.strideB = self.tap_split * self.conv_kc if (self.tap_split and not self.dgrad) else 0
        if self.p is None:          # p * K (whole reduction) stays under ~ 860 / 2: every sum is far inside the bf16-exact range
            kt = self.taps * self.conv_kc
            self.p = 1.0 if kt <= 256 else (0.5 if kt <= 640 else (0.25 if kt <= 1728 else 0.125))

    def but(self, name, **kw):
        return ConvCase(name, kw.pop("N", self.N), **{**self.kw, **kw})

    def __repr__(self):
        return self.name

    # ---- leading dimensions
    Mo = property(lambda s: s.M)
    Nc = property(lambda s: s.c_split if s.c_split else s.N)
    lda = property(lambda s: s.C1 + s.lda_x)
    lda2 = property(lambda s: s.C2 + s.lda2_x if s.C2 else 0)
    ldb = property(lambda s: (s.taps * s.Nw if s.dgrad else s.taps * s.conv_kc) + s.ldb_x)
    b_tap_stride = property(lambda s: s.Nw if s.dgrad else 0)
    ldc = property(lambda s: s.Nc + s.ldc_x)
    ldc2 = property(lambda s: s.N - s.c_split + s.ldc2_x if s.c_split else 0)
    ldcpre = property(lambda s: s.N + s.ldcpre_x)
    strideC = property(lambda s: s.M * s.ldc + s.stride_x if s.batch > 1 else 0)

    def store_key(self, name):
        f32 = self.dtype == "f32" or (self.c_f32 and name in ("C", "C2"))
        return name + ".f32" if f32 else name

    def taps_of(self, bz):
        return range(bz * self.tap_split, (bz + 1) * self.tap_split) if self.tap_split else range(self.taps)

    def chans_of(self, bz):
        return (bz * self.kc_split, (bz + 1) * self.kc_split) if self.kc_split else (0, self.conv_kc)


# ------------------------------------------------------------------------------------------------ operands
def _gen(seed):
    return torch.Generator("cpu").manual_seed(seed)


_LOGICAL = collections.OrderedDict()


def logical(c):
    """x [M, conv_kc] (both sources), w [taps, conv_kc, Nw] (w[tap][c][n] multiplies channel c of the tap's neighbour into column n), bias [N]: float64
    tensors holding values of the case's dtype"""
    key = (c.geom, c.kern, c.C1, c.C2, c.Nw, c.mode, c.p, c.dtype, c.seed, c.M)
    if key in _LOGICAL:
        return _LOGICAL[key]
    s = 7919 * c.seed + 17
    if c.mode == "int":
        x = torch.randint(-2, 3, (c.M, c.conv_kc), generator=_gen(s + 1)).double()
        sign = torch.randint(0, 2, (c.taps, c.conv_kc, c.Nw), generator=_gen(s + 2)).double() * 2 - 1
        w = sign * (torch.rand(c.taps, c.conv_kc, c.Nw, generator=_gen(s + 3)) < c.p).double()
        b = torch.randint(-3, 4, (c.Nw,), generator=_gen(s + 4)).double()
    else:
        q = (lambda t: bf(t.float()).double()) if c.dtype == "bf16" else (lambda t: t.float().double())
        x = q(torch.randn(c.M, c.conv_kc, generator=_gen(s + 1), dtype=torch.float64))
        w = q(torch.randn(c.taps, c.conv_kc, c.Nw, generator=_gen(s + 2), dtype=torch.float64) * (1.2 / math.sqrt(c.taps * c.conv_kc)))
        b = torch.randn(c.Nw, generator=_gen(s + 4), dtype=torch.float64).float().double()
    _LOGICAL[key] = (x, w, b)
    while len(_LOGICAL) > 4:
        _LOGICAL.popitem(last=False)
    return _LOGICAL[key]


def build(c):
    """the operands as the kernel sees them (CPU tensors of the case's dtype, NaN wherever no kernel may read) and where they start:
    A_big / A2_big [GUARD + M + GUARD, ld]; B [rows, ldb]; bias [N] fp32"""
    dt = BF if c.dtype == "bf16" else torch.float32
    x, w, b = logical(c)
    o = {}
    for name, c0, cn, ld in (("A_big", 0, c.C1, c.lda),) + ((("A2_big", c.C1, c.C2, c.lda2),) if c.C2 else ()):
        t = torch.full((c.M + 2 * GUARD, ld), NAN, dtype=dt)
        t[GUARD:GUARD + c.M, :cn] = x[:, c0:c0 + cn].to(dt)
        o[name] = t
    if c.dgrad:          # the packed forward weight [conv_kc][taps][Nw]; only the column block [b_off, b_off + N) of every tap may be read
        Bm = torch.full((c.conv_kc, c.ldb), NAN, dtype=dt)
        v = Bm[:, :c.taps * c.Nw].view(c.conv_kc, c.taps, c.Nw)
        v[:, :, c.b_off:c.b_off + c.N] = w.permute(1, 0, 2)[:, :, c.b_off:c.b_off + c.N].to(dt)
    else:                # [N][taps][conv_kc]
        Bm = torch.full((c.N, c.ldb), NAN, dtype=dt)
        Bm[:, :c.taps * c.conv_kc] = w[:, :, :c.N].permute(2, 0, 1).reshape(c.N, -1).to(dt)
    o["B"] = Bm
    if c.bias:
        o["bias"] = b[c.b_off:c.b_off + c.N].float()
    return o


def launch_args(c, buf):
    """(args, kwargs) of lavt_hip.ops.gemm_nt / gemm_nt_params.  buf: A_big, A2 (the second source's first row), B, C, and C2, Cpre, bias where the case
    has them -- device tensors in the GPU test, made-up addresses in the host route test"""
    g = buf.get
    dt = BF if c.dtype == "bf16" else torch.float32
    kw = dict(batch=c.batch, strideB=c.strideB, strideC=c.strideC, A2=g("A2"), lda2=c.lda2, a_split=c.a_split, conv=(c.H, c.W, c.conv_kc, int(c.dgrad), c.D, c.kd, c.kh, c.kw_),
              b_kmajor=c.kmajor, b_tap_stride=c.b_tap_stride, alpha=c.alpha, bias=g("bias"), act=c.act, Cpre=g("Cpre"), ldcpre=c.ldcpre if c.cpre else 0, C2=g("C2"),
              ldc2=c.ldc2, c_split=c.c_split, c_f32=c.c_f32, a_off=GUARD * c.lda, b_off=c.b_off if c.dgrad else 0, conv_tap_split=c.tap_split, conv_kc_split=c.kc_split)
    return (dt, c.M, c.N, c.K, buf["A_big"], c.lda, buf["B"], c.ldb, buf["C"], c.ldc), kw


# ------------------------------------------------------------------------------------------------ (a) the index form
def tap_offset(c, tap, permuted=False):
    """(dz, dy, dx) of a tap: kw fastest, each axis of size 3 running over -1, 0, 1"""
    if permuted:          # FAULT: the axes decoded in the order kw, kh, kd
        return tap % c.kd - c.kd // 2, (tap // c.kd) % c.kh - c.kh // 2, tap // (c.kd * c.kh) - c.kw_ // 2
    return tap // (c.kw_ * c.kh) - c.kd // 2, (tap // c.kw_) % c.kh - c.kh // 2, tap % c.kw_ - c.kw_ // 2


def source_rows(c, tap, fault=None):
    """row of A the tap reads for every output row m, -1 = zeros (outside the sample's zero-padded volume)"""
    dz, dy, dx = tap_offset(c, tap, fault == "kernel_order_permuted")
    if c.dgrad and fault != "ignore_flip":
        dz, dy, dx = -dz, -dy, -dx
    if fault == "tap_shift" and tap == 0:
        dx += 1
    m = torch.arange(c.M)
    pix = m % c.vox
    z, y, x = pix // (c.H * c.W), (pix // c.W) % c.H, pix % c.W
    okz, oky, okx = (z + dz >= 0) & (z + dz < c.D), (y + dy >= 0) & (y + dy < c.H), (x + dx >= 0) & (x + dx < c.W)
    if fault == "halo_side":          # the right image side is not zeroed: x + 1 == W reads the linear neighbour
        okx = okx | (x + dx == c.W)
    if fault == "halo_face":          # the far volume face is not zeroed
        okz = okz | (z + dz == c.D)
    if fault == "sample_wrap":        # the last row of a sample reads the first row of the next sample
        last = (y == c.H - 1) & (z == c.D - 1)
        oky = oky | (last & (y + dy == c.H))
        okz = okz | (last & (y + dy == c.H))
    src = m + (dz * c.H + dy) * c.W + dx
    return torch.where(okz & oky & okx & (src >= 0) & (src < c.M), src, torch.full_like(src, -1))


def _gather(c, o, src, dtype, fault=None):
    """[M, conv_kc]: the channels of the source rows, from A and (c >= a_split) A2, through a_off"""
    A = o["A_big"].to(dtype)[GUARD:]
    parts = [A[src.clamp(min=0), :c.C1]]
    if c.C2:
        parts.append(o["A2_big"].to(dtype)[GUARD:][src.clamp(min=0), :c.C2])
    X = torch.cat(parts, 1) * (src >= 0).to(dtype)[:, None]
    if fault == "swap_sources_block" and c.C2 >= 64:          # the first 64-channel block of either source read from the other
        X = X.clone()
        X[:, :64], X[:, c.C1:c.C1 + 64] = X[:, c.C1:c.C1 + 64].clone(), X[:, :64].clone()
    return X


def _weights(c, o, tap, dtype, fault=None):
    """[conv_kc, N]: the weights of one tap, by the header's address"""
    Bf = o["B"].to(dtype).reshape(-1)
    ch, n = torch.arange(c.conv_kc)[:, None], torch.arange(c.N)[None, :]
    if c.kmajor:
        ts = c.conv_kc if fault == "tap_stride_as_kc" else c.b_tap_stride
        idx = ch * c.ldb + tap * ts + c.b_off + n
    else:
        idx = n * c.ldb + tap * c.conv_kc + ch
    return Bf[idx % Bf.numel()]


def accumulate(c, o=None, dtype=torch.float64, fault=None):
    """acc [batch, M, N]: entry bz contracts its taps / channels only"""
    o = o or build(c)
    acc = torch.zeros(c.batch, c.M, c.N, dtype=dtype)
    for bz in range(c.batch):
        c0, c1 = c.chans_of(bz)
        for tap in c.taps_of(bz):
            X = _gather(c, o, source_rows(c, tap, fault), dtype, fault)
            wt = tap
            if fault == "tap_group_next_weights" and c.tap_split and bz == 0:
                wt = tap + c.tap_split
            Wt = _weights(c, o, wt, dtype, fault)
            a0, a1 = (0, c1 - c0) if (fault == "kc_piece_from_zero" and bz == 1) else (c0, c1)
            acc[bz] += X[:, a0:a1] @ Wt[a0:a1]
            pad = (-c.conv_kc) % 64
            if fault == "partial_pad_next_tap" and pad and tap + 1 < c.taps:          # the lanes past the last channel block run on into the next tap's k
                acc[bz] += X[:, :pad] @ _weights(c, o, tap + 1, dtype)[:pad]
    return acc


def index_reference(c, dtype=torch.float64, round_bf16=False, fault=None, o=None):
    """the buffers the launch owns -- C [batch, M, Nc], C2 [M, N - c_split], Cpre [M, N] -- and "acc" (alpha applied, before bias: what colstats sums)"""
    o = o or build(c)
    rnd = bf if (round_bf16 and c.dtype == "bf16") else (lambda t: t)
    v = accumulate(c, o, dtype, fault) * c.alpha
    out = {"acc": v[0]}
    if c.bias:
        v = v + o["bias"].to(dtype)[None, None, :]
    pre = v
    v = G._act(c.act, v)
    full = v if c.c_f32 else rnd(v)
    if c.c_split:
        first = 0 if fault == "c2_from_col0" else c.c_split
        out["C"], out["C2"] = full[..., :c.c_split].contiguous(), full[0, :, first:first + c.N - c.c_split].contiguous()
    else:
        out["C"] = full
    if c.cpre:
        out["Cpre"] = rnd(pre[0])
    return out


def reference(c):
    return index_reference(c, torch.float64, False)


def floor(c):
    return index_reference(c, torch.float32, True)


def nonempty(c):
    """[batch, M] bool: the rows of an entry whose reduction has at least one tap inside the sample.  A tap group of a split lies wholly in the halo for
    the pixels of one image side (the dy = -1 group for the first image row): there the contract demands an exact 0, whatever the operands"""
    return torch.stack([torch.stack([source_rows(c, t) >= 0 for t in c.taps_of(bz)]).any(0) for bz in range(c.batch)])


def colsums(c, rows_per_block):
    """[blocks, N]: the per-row-block column sums of the accumulator (alpha applied) the statistics epilogue stores; exact integers in mode int"""
    acc = reference(c)["acc"]
    nblk = cdiv(c.M, 2 * rows_per_block) * 2
    out = torch.zeros(nblk, c.N, dtype=torch.float64)
    for b in range(nblk):
        out[b] = acc[b * rows_per_block:(b + 1) * rows_per_block].sum(0)
    return out


def reduced(c, bias=None, relu=False):
    """what lavt_splitk_reduce (/ _epi with an integer bias and ReLU) leaves from the partial outputs of a split case, in fp64"""
    v = reference(c)["C"].sum(0)
    if bias is not None:
        v = v + bias.double()[None, :]
    return torch.relu(v) if relu else v


# ------------------------------------------------------------------------------------------------ (b) torch's convolution
def conv_reference(c):
    """[M, N] in float64: the whole reduction (all batch entries of a split summed), alpha, bias and activation applied -- F.conv3d on the logical
    tensors for the forward, autograd's input gradient for the data gradient"""
    x, w, b = logical(c)
    vol = lambda t, ch: t.reshape(c.B_, c.D, c.H, c.W, ch).permute(0, 4, 1, 2, 3).contiguous()
    rows = lambda t: t.permute(0, 2, 3, 4, 1).reshape(c.M, -1)
    pad = (c.kd // 2, c.kh // 2, c.kw_ // 2)
    if not c.dgrad:
        wt = w[:, :, :c.N].permute(2, 1, 0).reshape(c.N, c.conv_kc, c.kd, c.kh, c.kw_)
        y = rows(F.conv3d(vol(x, c.conv_kc), wt, padding=pad))
    else:
        wt = w[:, :, c.b_off:c.b_off + c.N].permute(1, 2, 0).reshape(c.conv_kc, c.N, c.kd, c.kh, c.kw_)          # forward weight [Cout = conv_kc][Cin = N][taps]
        x0 = torch.zeros(c.B_, c.N, c.D, c.H, c.W, dtype=torch.float64, requires_grad=True)
        F.conv3d(x0, wt, padding=pad).backward(vol(x, c.conv_kc))
        y = rows(x0.grad)
    y = y * c.alpha
    if c.bias:
        y = y + b[c.b_off:c.b_off + c.N][None, :]
    return G._act(c.act, y)


# ------------------------------------------------------------------------------------------------ gates
def bit_equal(got, ref):
    """mode int: every element equal as a number (the reference holds exactly representable values, so this IS bit equality, -0 aside)"""
    g, r = got.double(), ref.double()
    return g.shape == r.shape and bool(torch.isfinite(g).all()) and bool((g == r).all())


def stored_exactly(c, name, t):
    """does every value survive the store into the output's type"""
    f32 = c.dtype == "f32" or (c.c_f32 and name in ("C", "C2"))
    return bool((t.float().double() == t).all()) if f32 else bool((bf(t.float()).double() == t).all())


# ------------------------------------------------------------------------------------------------ routes
ALL7 = ["t64-s4-p0", "t64-s2-p0", "t128-s4-p0", "t128-s2-p0", "t128-s4-p3", "t128-s2-p3", "t512-s4-p3"]          # the seven distinct forced configurations
PIPE3 = ALL7[4:]
F32_2 = list(TUNINGS_F32)


def route_key(c, r):
    """a convolution instantiation: family / tile / ring / K walk / weight layout / lean"""
    if r == INVALID:
        return INVALID
    d = lambda x: "-" if x is None else x
    return f"{r.family}/{r.tile}/s{r.stages}/k{d(r.kmode)}/{'km' if c.kmajor else 'nk'}/L{d(r.lean)}"


def stated_route(c, tuning):
    """the route a row states for a forced configuration (None: the default tuning, the row states the whole route)"""
    if c.invalid:
        return INVALID
    if tuning is None:
        return c.route
    prefix = {**TUNINGS, **TUNINGS_F32}[tuning][1]
    if c.kc_split:          # the channel split has one home whatever the forced tile
        prefix = "pipe/128/s4"
    r = c.route
    if isinstance(r, dict):
        fam_tile = "/".join(prefix.split("/")[:2])
        r = r.get(fam_tile) or r[prefix.split("/")[0]]
    return f"{prefix}/{r}"


def reachable_conv():
    """every convolution instantiation the planner can reach for bf16 and fp32 operands (fp8 aside)"""
    out = set()
    for fam, tiles in (("pipe", ((128, 2), (128, 4), (256, 2))), ("v2", ((64, 2), (64, 4), (128, 2), (128, 4)))):
        for tile, st in tiles:
            for lay in ("nk", "km"):
                out.add(f"{fam}/{tile}/s{st}/k0/{lay}/L0")          # the general decode: the full epilogue only
                out.update(f"{fam}/{tile}/s{st}/k2/{lay}/L{lean}" for lean in (0, 1, 2))
            if fam == "pipe":          # the partial-block walk: pipelined family, k-contiguous weights
                out.update(f"pipe/{tile}/s{st}/k3/nk/L{lean}" for lean in (0, 1, 2))
    out.add("pipe/256/s2/k2/km/L3")          # the bare store with the second output kept
    out.update(f"classic/{tile}/s2/k-/{lay}/L-" for tile in (64, 128) for lay in ("nk", "km"))
    return out


# ------------------------------------------------------------------------------------------------ the table
# the default geometry (2, 5, 7): M = 70 crosses a 64-row tile, the sample boundary lies inside a 16-row block; (2, 9, 15): M = 270 crosses 128 and 256
G2b = (2, 1, 9, 15)
def _pv(pipe, v2):
    return {"pipe": pipe, "v2": v2}


_PRE = dict(cpre=True, bias=True)          # an exact full epilogue: integer bias, the pre-activation kept beside the output (ReLU would zero half of it)
CORE = [          # one row per K walk x layout x lean: under all seven forced configurations
    ConvCase("taps-nk-bare", 72, geom=G2b, route="k2/nk/L2", tunings=ALL7, why="tap walk, k-contiguous weights, bare store; M = 270"),
    ConvCase("taps-nk-bias", 24, C1=128, bias=True, alpha=0.5, route="k2/nk/L1", tunings=ALL7, why="two channel blocks per tap, bias, alpha 1/2"),
    ConvCase("taps-nk-cat-pre", 136, C2=64, **_PRE, route="k2/nk/L0", tunings=ALL7, why="the source switch in the middle of the walk; the full epilogue"),
    ConvCase("taps-km-bare", 64, geom=G2b, dgrad=True, route="k2/km/L2", tunings=ALL7, why="data gradient: mirrored neighbour, k-major weights"),
    ConvCase("taps-km-bias", 136, C1=128, dgrad=True, bias=True, route="k2/km/L1", tunings=ALL7, why="N = 136: a last column span of 8"),
    ConvCase("taps-km-C2", 136, dgrad=True, c_split=64, route={"pipe/256": "k2/km/L3", "pipe": "k2/km/L0", "v2": "k2/km/L0"}, tunings=ALL7,
             why="c_split 64 (+72): the full epilogue on 128x128, the bare store with C2 kept on the forced 256x256 tile"),
    ConvCase("taps-km-C2-bias", 136, C1=128, C2=64, dgrad=True, c_split=128, bias=True, route="k2/km/L0", tunings=ALL7, why="c_split 128 (+8), two sources of dy"),
    ConvCase("general-nk-cat", 24, C1=96, C2=32, route="k0/nk/L0", tunings=ALL7, why="a_split % 64 != 0: decoded per K tile"),
    ConvCase("general-km-72", 64, C1=72, dgrad=True, route="k0/km/L0", tunings=ALL7, why="data gradient with conv_kc = Cout = 72"),
    ConvCase("partial-nk-72", 72, C1=72, route=_pv("k3/nk/L2", "k0/nk/L0"), tunings=ALL7, why="one channel block + 8: partial on the pipelined tiles, general in gemm_v2"),
    ConvCase("partial-nk-cat-bias", 24, C1=64, C2=32, bias=True, route=_pv("k3/nk/L1", "k0/nk/L0"), tunings=ALL7, why="the partial block lies in the second source"),
    ConvCase("partial-nk-cat-pre", 264, C1=128, C2=40, **_PRE, route=_pv("k3/nk/L0", "k0/nk/L0"), tunings=ALL7, why="128 + 40, Cout = 264"),
]
_TS = dict(stride_x=12)          # strideC = M * N + 12
SPLITS = [          # the reduction cut at tap groups: both layouts, a concat source, on every tile
    ConvCase("tapsplit3-nk", 72, tap_split=3, **_TS, route="k2/nk/L2", tunings=ALL7, why="three tap groups, strideB = 3 conv_kc"),
    ConvCase("tapsplit1-nk-cat", 24, C2=64, tap_split=1, p=1.0, **_TS, route="k2/nk/L2", tunings=ALL7, why="nine single taps over two sources"),
    ConvCase("tapsplit3-km", 64, dgrad=True, tap_split=3, **_TS, route="k2/km/L2", tunings=ALL7, why="k-major: strideB = 0, the group found through b_tap_stride"),
]
G3a, G3b, G3c = (2, 3, 4, 5), (2, 4, 6, 6), (2, 1, 4, 5)
K333 = (3, 3, 3)
_ONE = ["t128-s4-p3"]
_THREE = ["t64-s4-p0", "t128-s4-p3", "t512-s4-p3"]          # one tile of each size: gemm_v2 64x64, pipelined 128x128 and 256x256
REST = [          # geometry, channels and epilogues: under the configuration that reaches the instantiation, the geometries on one tile of each size
    ConvCase("geom-h1", 24, geom=(3, 1, 1, 11), route="k2/nk/L2", tunings=_THREE, why="every vertical tap is halo"),
    ConvCase("geom-w1", 24, geom=(3, 1, 6, 1), dgrad=True, Nw=24, route="k2/km/L2", tunings=_THREE, why="every horizontal tap is halo"),
    ConvCase("geom-m4", 24, geom=(1, 1, 2, 2), route="k2/nk/L2", tunings=_THREE, why="M < 16"),
    ConvCase("geom-3d-333", 24, geom=G3a, kern=K333, route="k2/nk/L2", tunings=_THREE, why="27 taps over a volume"),
    ConvCase("geom-3d-311", 24, geom=G3a, kern=(3, 1, 1), bias=True, route="k2/nk/L1", tunings=_THREE, why="the depth axis alone"),
    ConvCase("geom-3d-133", 64, geom=G3a, kern=(1, 3, 3), dgrad=True, route="k2/km/L2", tunings=_THREE, why="nine taps inside a volume"),
    ConvCase("geom-3d-333-m288", 72, geom=G3b, kern=K333, C1=128, dgrad=True, Nw=72, route="k2/km/L2", tunings=_THREE, why="M = 288, K = 3456, mirrored 3-D neighbour"),
    ConvCase("geom-3d-d1", 24, geom=G3c, kern=K333, route="k2/nk/L2", tunings=_THREE, why="every dz != 0 tap is halo"),
    ConvCase("geom-3d-partial", 24, geom=G3a, kern=K333, C1=72, bias=True, route=_pv("k3/nk/L1", "k0/nk/L0"), tunings=_THREE, why="the partial block over 27 taps"),
    ConvCase("partial-8", 24, geom=G2b, C1=8, route="k3/nk/L2", tunings=_ONE, why="a channel block of 8"),
    ConvCase("partial-96", 136, C1=96, route="k3/nk/L2", tunings=["t512-s4-p3"], why="64 + 32 of one source"),
    ConvCase("taps-cat-128-64", 24, geom=G2b, C1=128, C2=64, route="k2/nk/L2", tunings=["t128-s4-p0"], why="128 + 64"),
    ConvCase("taps-n264", 264, geom=G2b, C1=128, route="k2/nk/L2", tunings=["t128-s2-p3", "t512-s4-p3"], why="Cout = 264: three column tiles of 128, two of 256; M = 270"),
    ConvCase("taps-km-n264-boff", 64, geom=G2b, dgrad=True, Nw=264, b_off=200, route="k2/km/L2", tunings=["t512-s4-p3"],
             why="b_off: the second source's column block alone, inside rows of 264"),
    ConvCase("taps-km-n264", 264, geom=G2b, dgrad=True, c_split=128, ldc2_x=8, route={"pipe/256": "k2/km/L3", "pipe": "k2/km/L0", "v2": "k2/km/L0"}, tunings=_THREE,
             why="N = 264 with c_split 128 (+136): the split inside the first 256-column tile, C2 across two"),
    ConvCase("colstats-taps", 72, geom=G2b, colstats=True, route="k2/nk/L2", tunings=PIPE3, why="the statistics epilogue: per-block column sums are exact integers"),
    ConvCase("colstats-partial", 24, C1=72, colstats=True, route="k3/nk/L2", tunings=PIPE3, why="the same through the partial-block walk"),
]
KCSPLIT_T = ["t128-s4-p3", "t512-s4-p3", "t64-s4-p3"]          # (the channel split takes the pipelined 128x128 tile with a 4-deep ring under each)
KCSPLITS = [
    ConvCase("kcsplit-128", 72, C1=128, kc_split=64, **_TS, route="k2/nk/L2", tunings=KCSPLIT_T, why="128 in two pieces of 64"),
    ConvCase("kcsplit-64+128", 24, C1=64, C2=128, kc_split=64, **_TS, route="k2/nk/L2", tunings=KCSPLIT_T, why="three pieces of 64: two start in the second source"),
    ConvCase("kcsplit-64+192", 24, C1=64, C2=192, kc_split=128, **_TS, route="k2/nk/L2", tunings=KCSPLIT_T, why="two pieces of 128: piece 0 crosses the boundary"),
    ConvCase("kcsplit-km", 136, C1=128, dgrad=True, kc_split=64, **_TS, route="k2/km/L2", tunings=KCSPLIT_T, why="k-major: the piece's rows of the weight"),
    ConvCase("kcsplit-3d", 24, geom=G3a, kern=K333, C1=128, kc_split=64, **_TS, route="k2/nk/L2", tunings=KCSPLIT_T, why="27 taps"),
]
TAPSPLITS_3D = [
    ConvCase("tapsplit9-3d", 24, geom=G3a, kern=K333, tap_split=9, **_TS, route="k2/nk/L2", tunings=_ONE, why="27 taps in three planes"),
    ConvCase("tapsplit3-3d-km", 64, geom=G3a, kern=K333, dgrad=True, tap_split=3, p=0.5, **_TS, route="k2/km/L2", tunings=["t64-s4-p0"], why="27 taps in nine rows, k-major"),
]
F32 = [          # the fp32 twins of the general rows: the classic kernel, both tiles
    ConvCase("f32-nk-cat", 24, C1=96, C2=32, dtype="f32", lda_x=4, lda2_x=4, ldb_x=4, route="k-/nk/L-", tunings=F32_2),
    ConvCase("f32-km-72", 64, C1=72, dgrad=True, dtype="f32", lda_x=4, ldb_x=4, route="k-/km/L-", tunings=F32_2),
    ConvCase("f32-nk-20", 24, geom=G2b, C1=20, bias=True, dtype="f32", lda_x=4, ldb_x=4, route="k-/nk/L-", tunings=F32_2, why="Cin = 20"),
]
_GELU = dict(mode="real", act=ACT_GELU, cpre=True, bias=True)
REAL = [          # what integers cannot state
    ConvCase("real-3d-gelu", 72, geom=G3a, kern=K333, **_GELU, route="k2/nk/L0", tunings=_ONE, why="Conv3d forward of SepTPWAM: GELU + Cpre + bias"),
    ConvCase("real-3d-gelu-v2", 72, geom=G3a, kern=K333, **_GELU, route="v2/64/s4/k2/nk/L0", tunings=None, why="the same at the default tuning"),
    ConvCase("real-fwd-pipe", 72, geom=G2b, C2=64, mode="real", route="k2/nk/L2", tunings=["t512-s4-p3"]),
    ConvCase("real-dgrad-pipe", 136, geom=G2b, dgrad=True, c_split=64, mode="real", route="k2/km/L3", tunings=["t512-s4-p3"]),
    ConvCase("real-fwd-v2", 72, geom=G2b, C2=64, mode="real", route="k2/nk/L2", tunings=["t128-s2-p0"]),
    ConvCase("real-dgrad-v2", 136, geom=G2b, dgrad=True, c_split=64, mode="real", route="k2/km/L0", tunings=["t64-s4-p0"]),
    ConvCase("real-fwd-f32", 24, C1=20, mode="real", dtype="f32", lda_x=4, ldb_x=4, route="k-/nk/L-", tunings=["t64"]),
    ConvCase("real-dgrad-f32", 64, C1=72, dgrad=True, mode="real", dtype="f32", lda_x=4, ldb_x=4, route="k-/km/L-", tunings=["t128"]),
]
_R = dict(invalid=True, tunings=[None])
REFUSALS = [
    ConvCase("refuse-kcsplit-pipe0", 72, C1=128, kc_split=64, word="conv_kc_split", env={"LAVT_GEMM_PIPE": "0"}, **_R),
    ConvCase("refuse-kcsplit-batch", 72, C1=128, kc_split=64, batch=3, word="conv_kc_split", **_R, why="batch * conv_kc_split != conv_kc"),
    ConvCase("refuse-tapsplit-batch", 72, tap_split=3, batch=2, word="conv_tap_split", **_R, why="batch * conv_tap_split != taps"),
    ConvCase("refuse-tapsplit-kc72", 72, C1=72, tap_split=3, word="conv_tap_split", **_R, why="a tap split with conv_kc % 64 != 0"),
    ConvCase("refuse-k", 72, K=8 * 64, word="conv geometry", **_R, why="K != taps * conv_kc"),
    ConvCase("refuse-m", 72, M=64, word="D*H*W", **_R, why="M % (D*H*W) != 0"),
]
INT_TABLE = CORE + SPLITS + REST + KCSPLITS + TAPSPLITS_3D + F32
TABLE = INT_TABLE + REAL
BY_NAME = {c.name: c for c in TABLE + REFUSALS}


def launches(cases=None):
    """every (case, forced configuration) of the table"""
    return [(c, t) for c in (TABLE if cases is None else cases) for t in (c.tunings or [None])]


# fault -> the cases named for it: the gate must fail on each of them
FAULTS = {
    "tap_shift": ["taps-nk-bare", "geom-m4"],
    "halo_side": ["taps-nk-bare", "taps-km-bare"],
    "halo_face": ["geom-3d-333", "geom-3d-311"],
    "sample_wrap": ["taps-nk-bias", "geom-h1"],
    "ignore_flip": ["taps-km-bare", "geom-3d-333-m288"],
    "swap_sources_block": ["taps-nk-cat-pre", "kcsplit-64+128"],
    "partial_pad_next_tap": ["partial-nk-72", "partial-8"],
    "tap_group_next_weights": ["tapsplit3-nk", "tapsplit3-km"],
    "kc_piece_from_zero": ["kcsplit-128", "kcsplit-km"],
    "tap_stride_as_kc": ["taps-km-n264-boff", "taps-km-bias"],
    "c2_from_col0": ["taps-km-C2", "taps-km-n264"],
    "kernel_order_permuted": ["geom-3d-133", "geom-3d-333"],
}
