"""The contract of the TN weight-gradient family (include/lavt_hip.h: lavt_gemm_tn_t, lavt_gemm_tn_grouped*, lavt_conv3x3_wgrad*) stated once, the case
table of its per-kernel parity tests, and a plain-Python restatement of its host planners.  CPU only, pure torch, nothing imported from the product.

    C[b][i][j]  (+)= alpha * sum_k s_k * A[b][map_a[k]][i] * Bv[b][k][j]
    colsum[b][i] (+)= alpha * sum_k s_k * A[b][map_a[k]][i]

map_a[k] = a_rowmap[k] (k without a map; -1: a zero row), s_k = a_rowscale[k / a_rowscale_div] (1 without; a_rowscale_binary: 1 where the entry is
non-zero -- the caller folded the one non-zero value into alpha), Bv[k][j] = B[map_b[k]][j] for a plain problem (columns >= b_split from B2) and, with
conv taps, column j = tap * kc + c reads channel c of the (dz, dy, dx) neighbour of voxel row map_b[k] inside its own zero-padded sample.
c_conv_permute stores column (tap, c) at c * taps + tap.  The row map, the row scale and B2 are shared by the batch entries; A, B, C and colsum move by
their strides.  accumulate == 0 promises zeros in C and colsum, so "(+)=" is "=" there.

TWO MODES.  mode "int": A and B hold integers in [-3, 3], row scales come from {0, 0.5, 1, 2} (binary: {0, v}), alpha from {1, 1.25, -0.5}, the initial
C and colsum are integers.  Every addend alpha * s * a * b is then a multiple of 2^-3 and the sum of their magnitudes stays under 2^20
(test_gemm_tn_cases_host.py checks both per case), so every partial sum in every order is exact in fp32: whatever the route -- tile, K pieces, atomics in
any order, partial tiles, stream-K runs -- the kernel must return the exact value BIT FOR BIT.  `tn_reference` evaluates it in integers (scaled by 8,
through float64 products, which are exact far beyond that range; the host test holds it to a true int64 matmul).  A row that is dropped, doubled,
mis-paired, mis-masked or mis-shifted changes an integer.  mode "real": normal operands rounded to the case's dtype, reference in fp64, FLOOR in fp32 by
torch (exact products of the rounded operands, fp32 sums -- the column sum row after row, as every K loop adds --, alpha last) -- the scheme of gemm_nt_cases.py with its row / column metric `nt_error`:
E(got, ref) <= K_TN x E(floor, ref).  The classic kernel rounds s * A to the operand type before the MFMA; the non-binary scales of this table are
powers of two (or 0), so that rounding is exact and the floor needs no model of it.

`build(case)` lays the operands out as the kernel sees them, with NaN wherever no kernel may read: the columns between I and lda, J and ldb / ldb2, the
source rows no map entry names, the rows at and beyond K, the gap between batch entries; C and colsum carry NaN in everything the kernel does not own.
Rows masked by a zero row scale hold finite values (a kernel may read and multiply them).

`tn_route(case_or_group, tuning)` restates the family's planner, csrc/gemm_tn_plan.hip: lavt_gemm_tn_route (the contract checks, tn_v2_eligible, both
tile and split rules) and lavt_gemm_tn_group_route (tn_route_pipe, tn_route_group64, tn_route_sk), and cw_supported / cw_pieces and the fp8 launcher's
piece rounding (csrc/conv_wgrad.hip).  Every row of the table states the route it is there for; test_gemm_tn_cases_host.py holds `tn_route` to it and
test_gemm_tn_route_host.py holds it to the library's own answer.  `launch_args(case, buf)` is the one way both the GPU test and that host test fill
a lavt_gemm_tn_t from a row."""
import collections
import math
import re
import zlib

import torch

from gemm_nt_cases import nt_error

BF = torch.bfloat16
NAN = float("nan")
INVALID = "invalid"

# Gate factor of the real-mode cases per output: twice the largest E / F measured on MI355X over test_gpu_gemm_tn_cases.py (its MEASURED table), rounded
# up, never under 1.  C: 1.339 (the uncut pipelined launch; every route lies between 0.5 and 1.4 -- the order of the fp32 K sum).  colsum: 9.410.  The
# floor of a column sum adds the K rows in sequence, as the kernels do (against torch's pairwise sum the 64x64 group cut into pieces at K = 3144 stood at
# 11.5; now 4.5), and all routes but three stand at or under 1.4 -- most at 1.000, both sums exact to the last bit.  The 9.41 is ONE element of
# r-v2-64-parts: the column metric of a vector is the relative error of its single elements, that row accumulates alpha = -0.5 times the sum into an
# initial value, element 28 comes out at 0.41 where the median is 6.1, the kernel's three pieces land 4.8e-7 from it and the floor, by luck, 7e-9.  Summing
# the three pieces one after the other in fp32 on the CPU gives the same 9.410 to the last digit: it is the order of the sum, not a fault.
K_TN = {"C": 2.68, "colsum": 18.82}


def k_from_measured(ratio):
    return max(1.0, math.ceil(2.0 * ratio * 100.0 - 1e-9) / 100.0)


def cdiv(a, b):
    return -(-a // b)


def taps_of(cv):
    return cv["kd"] * cv["kh"] * cv["kw"]


def conv(n, h, w, kc, d=1, k=(1, 3, 3)):
    return dict(n=n, d=d, h=h, w=w, kd=k[0], kh=k[1], kw=k[2], kc=kc)


class Case:
    """one lavt_gemm_tn_t problem (also a member of a group, and the TN form of a fused conv weight gradient)"""

    def __init__(self, name, route, *, I, K, J=0, mode="int", dtype="bf16", batch=1, a_map=False, b_map=False, scale=None, div=1, v=1.0, alpha=1.0,
                 accumulate=False, colsum=False, colsum_atomic=False, split_k=0, partials=None, zeros=True, conv=None, b_split=0, permute=False,
                 tuning=None, no_b=False, c_off=0, part_off=0, ld_pad=(8, 16, 4), lda=None, invalid=False, share=None, src_rows=(None, None)):
        self.name, self.route, self.mode, self.dtype, self.I, self.K, self.batch = name, route, mode, dtype, I, K, batch
        self.a_map, self.b_map, self.scale, self.div, self.v, self.alpha = a_map, b_map, scale, div, v, alpha
        self.accumulate, self.colsum, self.colsum_atomic, self.split_k, self.partials, self.zeros = accumulate, colsum, colsum_atomic, split_k, partials, zeros
        self.conv, self.b_split, self.permute, self.tuning, self.no_b = conv, b_split, permute, dict(tuning or {}), no_b
        self.c_off, self.part_off, self.invalid, self.share, self.src_rows = c_off, part_off, invalid, share, src_rows
        self.J = taps_of(conv) * conv["kc"] if conv else ((J or 8) if no_b else J)
        self.bcols = conv["kc"] if conv else self.J                      # logical columns of the B source (channels under taps)
        self.b1 = b_split if b_split else self.bcols                     # columns held by B (the rest by B2)
        self.b2 = self.bcols - self.b1
        self.lda = lda if lda is not None else I + ld_pad[0]
        self.ldb = 0 if no_b else self.b1 + ld_pad[1]
        self.ldb2 = self.b2 + ld_pad[1] if self.b2 else 0
        self.ldc = self.J + ld_pad[2]
        self.vox = conv["d"] * conv["h"] * conv["w"] if conv else 0
        self.Ra = K + 5 if a_map else K                                  # source rows of A
        self.Rb = (conv["n"] * self.vox if conv else (K + 7 if b_map else K))
        self.Ra_buf, self.Rb_buf = self.Ra + 2, self.Rb + 2              # two NaN rows beyond the last one
        self.strideA = self.Ra_buf * self.lda + 16 if batch > 1 else 0
        self.strideB = self.Rb_buf * self.ldb + 16 if batch > 1 else 0
        self.strideC = I * self.ldc + 12 if batch > 1 else 0
        self.strideColsum = I + 4 if batch > 1 else 0
        self.nrs = cdiv(K, div) if scale else 0
        if conv and not b_map:
            assert K == self.Rb, (name, K, self.Rb)

    def __repr__(self):
        return self.name

    @property
    def epc(self):
        return 4 if self.dtype == "f32" else 8

    @property
    def tdtype(self):
        return torch.float32 if self.dtype == "f32" else BF

    @property
    def a_src_rows(self):
        """lavt_gemm_tn_t.a_src_rows: the rows of the A buffer `build` lays out (what a_rowmap may name), or the row's own statement; 0 without a map"""
        rows = ((self.batch - 1) * self.strideA + self.Ra_buf * self.lda + 8) // self.lda
        return 0 if not self.a_map else (rows if self.src_rows[0] is None else self.src_rows[0])

    @property
    def b_src_rows(self):
        rows = ((self.batch - 1) * self.strideB + self.Rb_buf * self.ldb + 8) // max(self.ldb, 1)
        return 0 if not self.b_map else (rows if self.src_rows[1] is None else self.src_rows[1])

    @property
    def pieces_bound(self):
        """lavt_gemm_tn_pieces"""
        kt = cdiv(self.K, 64)
        return max(1, min(kt, cdiv(kt, 2 if self.batch > 1 else 8)))

    @property
    def partials_floats(self):
        """the scratch the case lends: 'exact' = batch * lavt_gemm_tn_pieces * (I*J + I); an int: that many pieces"""
        if self.partials is None:
            return 0
        n = self.pieces_bound if self.partials == "exact" else int(self.partials)
        return self.batch * n * (self.I * self.J + self.I)


class Group:
    """n problems through lavt_gemm_tn_grouped (entry 'grouped'), _grouped_sk ('sk') or _grouped_ln ('ln': ln = (rows, C) of the rider)"""

    def __init__(self, name, route, members, *, tuning=None, entry="grouped", ln=None, invalid=False, scratch="ws"):
        self.name, self.route, self.members, self.tuning, self.entry, self.ln, self.invalid, self.scratch = name, route, members, dict(tuning or {}), entry, ln, invalid, scratch
        self.mode = members[0].mode

    def __repr__(self):
        return self.name


# ------------------------------------------------------------------------------------------------ operands
def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


_INPUTS = collections.OrderedDict()
SCALES = (0.5, 0.0, 2.0, 1.0, 2.0, 0.0, 0.5)          # non-binary row scales, cyclic
MASK = (1, 0, 1, 1, 0)                                  # binary masks alternate between neighbouring samples, cyclic


def inputs(c):
    """the logical operands of a case as float64 CPU tensors (values exact in the case's dtype): A [batch][Ra][I], B [batch][Rb][b1], B2 [Rb][b2],
    a_map / b_map int32 [K], scale fp32 [nrs], C0 [batch][I][J], cs0 [batch][I]"""
    if c.name in _INPUTS:
        return _INPUTS[c.name]
    g, i = _gen(c.name), {}
    if c.mode == "int":
        mk = lambda *s: torch.randint(-3, 4, s, generator=g).double()
        init = lambda *s: torch.randint(-5, 6, s, generator=g).double()
    else:
        mk = lambda *s: (torch.randn(*s, generator=g) * 0.5).to(c.tdtype).double()
        init = lambda *s: torch.randn(*s, generator=g).float().double()
    i["A"] = mk(c.batch, c.Ra, c.I)
    if not c.no_b:
        i["B"] = mk(c.batch, c.Rb, c.b1)
        if c.b2:
            i["B2"] = mk(c.Rb, c.b2)
    if c.a_map:
        m = torch.randint(-1, c.Ra, (c.K,), generator=g, dtype=torch.int32)
        m[c.K // 2] = -1
        if c.K > 2:
            m[c.K - 1] = m[0] if m[0] >= 0 else 1          # a repeated row, and a live last row
        i["a_map"] = m
    if c.b_map:
        m = torch.randint(0, c.Rb, (c.K,), generator=g, dtype=torch.int32)
        if c.K > 3:
            m[c.K // 3] = -1
        i["b_map"] = m
    if c.scale == "binary":
        i["scale"] = torch.tensor([MASK[r % len(MASK)] * c.v for r in range(c.nrs)], dtype=torch.float32)
    elif c.scale == "scaled":
        i["scale"] = torch.tensor([SCALES[r % len(SCALES)] for r in range(c.nrs)], dtype=torch.float32)
    zero = lambda *s: torch.zeros(*s, dtype=torch.float64)
    i["C0"] = init(c.batch, c.I, c.J) if c.accumulate else zero(c.batch, c.I, c.J)
    i["cs0"] = init(c.batch, c.I) if c.accumulate else zero(c.batch, c.I)          # (a shared bias gradient starts from zeros: two atomic addends, any order)
    if c.I * c.J * c.batch <= 1 << 19:
        _INPUTS[c.name] = i
    return i


def build(c, inp=None):
    """the operands as flat buffers of the case's dtype with NaN wherever no kernel may read, the outputs as flat fp32 buffers holding the initial
    values where the kernel owns them and NaN elsewhere; 'C_own' / 'cs_own': bool masks of the owned elements"""
    i = inp or inputs(c)
    dt, o = c.tdtype, {}

    def rows(t, ld, used_rows, nbuf, stride):
        nb = t.shape[0]
        buf = torch.full(((nb - 1) * stride + nbuf * ld + 8,), NAN, dtype=dt)
        for b in range(nb):
            v = buf[b * stride:b * stride + nbuf * ld].view(nbuf, ld)
            v[:t.shape[1], :t.shape[2]] = t[b].to(dt)
            if used_rows is not None:
                v[:t.shape[1]][~used_rows] = NAN
        return buf

    def used(m, n):
        if m is None:
            return None
        u = torch.zeros(n, dtype=torch.bool)
        u[m.long()[m >= 0]] = True
        return u

    ua = used(i.get("a_map"), c.Ra)
    ub = None
    if c.b_map and not c.conv:
        ub = used(i["b_map"], c.Rb)
    o["A"] = rows(i["A"], c.lda, ua, c.Ra_buf, c.strideA)
    if not c.no_b:
        o["B"] = rows(i["B"], c.ldb, ub, c.Rb_buf, c.strideB)
        if c.b2:
            o["B2"] = rows(i["B2"][None], c.ldb2, ub, c.Rb_buf, 0)
    for k in ("a_map", "b_map", "scale"):
        if k in i:
            o[k] = i[k].clone()
    n = (c.batch - 1) * c.strideC + c.I * c.ldc
    o["C"], o["C_own"] = torch.full((n,), NAN, dtype=torch.float32), torch.zeros(n, dtype=torch.bool)
    n = (c.batch - 1) * c.strideColsum + c.I
    o["colsum"], o["cs_own"] = torch.full((n,), NAN, dtype=torch.float32), torch.zeros(n, dtype=torch.bool)
    for b in range(c.batch):
        v = o["C"][b * c.strideC:b * c.strideC + c.I * c.ldc].view(c.I, c.ldc)
        v[:, :c.J] = i["C0"][b].float()
        o["C_own"][b * c.strideC:b * c.strideC + c.I * c.ldc].view(c.I, c.ldc)[:, :c.J] = True
        o["colsum"][b * c.strideColsum:b * c.strideColsum + c.I] = i["cs0"][b].float()
        o["cs_own"][b * c.strideColsum:b * c.strideColsum + c.I] = True
    return o


def extract(c, Cflat, csflat):
    """the owned parts of the flat output buffers in the shape of the reference"""
    C = torch.stack([Cflat[b * c.strideC:b * c.strideC + c.I * c.ldc].view(c.I, c.ldc)[:, :c.J] for b in range(c.batch)])
    cs = torch.stack([csflat[b * c.strideColsum:b * c.strideColsum + c.I] for b in range(c.batch)]) if csflat is not None else None
    return C, cs


def launch_args(c, buf):
    """-> (args, kw, finish): lavt_hip.ops.gemm_tn_params(*args, **kw) fills the lavt_gemm_tn_t of a case and finish(p, addr) sets what the tests decide
    per row on the filled struct: split_k, the lent partials scratch (at its offset) and a missing zero page.  buf: the operands A, B (the zero page for
    a column-sum-only member), C and, where the case has them, B2, a_map, b_map, scale, colsum, parts -- device tensors (GPU test, addr = the tensor's
    address) or made-up addresses (host test, addr = identity)"""
    cv = None
    if c.conv:
        v = c.conv
        cv = (v["h"], v["w"], v["kc"]) + ((v["d"], v["kd"], v["kh"], v["kw"]) if (v["d"], v["kd"], v["kh"], v["kw"]) != (1, 1, 3, 3) else ())
    args = (c.tdtype, c.I, c.J, c.K, buf["A"], c.lda, buf["B"], c.ldb, buf["C"], c.ldc)
    kw = dict(batch=c.batch, strideA=c.strideA, strideB=c.strideB, strideC=c.strideC, a_rowmap=buf.get("a_map"), a_rowscale=buf.get("scale"), a_rowscale_div=c.div,
              a_rowscale_binary=c.scale == "binary", accumulate=c.accumulate, B2=buf.get("B2"), ldb2=c.ldb2, b_split=c.b_split if c.b2 else 0, b_rowmap=buf.get("b_map"),
              conv=cv, alpha=c.alpha, c_conv_permute=c.permute, colsum=buf.get("colsum"), strideColsum=c.strideColsum, c_off=c.c_off, colsum_atomic=c.colsum_atomic,
              a_src_rows=c.a_src_rows, b_src_rows=c.b_src_rows)

    def finish(p, addr):
        p.split_k = c.split_k
        p.partials, p.partials_floats = (addr(buf["parts"]) + 4 * c.part_off, c.partials_floats) if buf.get("parts") is not None else (None, 0)
        if not c.zeros:
            p.zeros = None
        return p
    return args, kw, finish


# ------------------------------------------------------------------------------------------------ the contract
FAULTS = ("k_last_dropped", "piece_first_doubled", "scale_index_plus1", "map_minus1_as_row0", "tap_dx_mirrored", "border_wrap", "sample_border_ignored",
          "b_split_off8", "permute_transposed", "colsum_without_alpha", "colsum_batch_stride_ignored", "piece_omitted")


def _piece_rows(c):
    """rows [lo, hi) of the second K piece: of the p<n> pieces the case's stated route names, else of a cut in two (None: a single K tile)"""
    bk = 16 if c.dtype == "f32" else 64
    kt, n = cdiv(c.K, bk), 2
    for part in c.route.split("/"):
        if re.fullmatch(r"p\d+", part) and int(part[1:]) > 1:
            n = int(part[1:])
    if kt < 2:
        return None
    lo = cdiv(kt, n) * bk
    return (lo, min(c.K, 2 * lo)) if lo < c.K else None


def applies(fault, c):
    """whether a planted fault can show on this case at all"""
    return {"k_last_dropped": True, "piece_first_doubled": _piece_rows(c) is not None, "piece_omitted": _piece_rows(c) is not None,
            "scale_index_plus1": c.scale is not None, "map_minus1_as_row0": c.a_map or c.b_map,
            "tap_dx_mirrored": c.conv is not None and c.conv["kw"] > 1, "border_wrap": c.conv is not None and c.conv["kw"] > 1,
            "sample_border_ignored": c.conv is not None and c.conv["n"] > 1 and (c.conv["kh"] > 1 or c.conv["kd"] > 1),
            "b_split_off8": c.b2 > 0 and c.b1 >= 8, "permute_transposed": c.permute, "colsum_without_alpha": c.colsum and c.alpha != 1.0,
            "colsum_batch_stride_ignored": c.colsum and c.batch > 1}[fault]


def _gather(t, m, fault):
    """rows m of t [batch][R][n]; -1: a zero row"""
    if m is None:
        return t
    ml = m.long()
    out = t[:, ml.clamp(min=0)]
    if fault != "map_minus1_as_row0":
        out = out * (ml >= 0).to(t.dtype)[None, :, None]
    return out


def _neighbours(c, src, tap, fault):
    """voxel row of the tap's neighbour of every row in src (int64; -1 stays -1), -1 outside the zero-padded sample"""
    cv = c.conv
    dx, dy, dz = tap % cv["kw"] - cv["kw"] // 2, (tap // cv["kw"]) % cv["kh"] - cv["kh"] // 2, tap // (cv["kw"] * cv["kh"]) - cv["kd"] // 2
    if fault == "tap_dx_mirrored":
        dx = -dx
    s = src.clamp(min=0)
    pix = s % c.vox
    z, rem = pix // (cv["h"] * cv["w"]), pix % (cv["h"] * cv["w"])
    y, x = rem // cv["w"], rem % cv["w"]
    ok = src >= 0
    if fault != "border_wrap":
        ok = ok & (x + dx >= 0) & (x + dx < cv["w"])
    if fault != "sample_border_ignored":
        ok = ok & (y + dy >= 0) & (y + dy < cv["h"]) & (z + dz >= 0) & (z + dz < cv["d"])
    nb = s + (dz * cv["h"] + dy) * cv["w"] + dx
    ok = ok & (nb >= 0) & (nb < c.Rb)
    return torch.where(ok, nb, torch.full_like(nb, -1))


def effective(c, inp=None, fault=None):
    """Ae [batch][K][I] = s_k A[map_a[k]] and Bv [batch][K][J] (None for the column-sum-only member), float64"""
    i = inp or inputs(c)
    Ae = _gather(i["A"], i.get("a_map"), fault)[:, :c.K]
    if c.scale:
        idx = torch.arange(c.K)
        if fault == "scale_index_plus1":
            idx = idx + 1
        s = i["scale"].double()[(idx // c.div).clamp(max=c.nrs - 1)]
        if c.scale == "binary":
            s = (s != 0).double()
        Ae = Ae * s[None, :, None]
    if fault == "k_last_dropped":
        Ae = Ae.clone()
        Ae[:, c.K - 1] = 0
    pr = _piece_rows(c)
    if fault == "piece_first_doubled" and pr:
        Ae = Ae.clone()
        Ae[:, pr[0]] *= 2
    if fault == "piece_omitted" and pr:
        Ae = Ae.clone()
        Ae[:, pr[0]:pr[1]] = 0
    if c.no_b:
        return Ae, None
    src = i["B"]
    if c.b2:
        b1 = c.b1
        if fault == "b_split_off8" and c.b1 >= 8:
            b1 = c.b1 - 8
            cols = [(ch, 0) if ch < b1 else ((ch - b1) % c.b2, 1) for ch in range(c.bcols)]
            src = torch.stack([(i["B"][:, :, k] if w == 0 else i["B2"][None, :, k].expand(c.batch, -1)) for k, w in cols], dim=2)
        else:
            src = torch.cat([i["B"], i["B2"][None].expand(c.batch, -1, -1)], dim=2)
    if c.conv is None:
        return Ae, _gather(src, i.get("b_map"), fault)[:, :c.K]
    rowsrc = i["b_map"].long() if c.b_map else torch.arange(c.K)
    if c.b_map and fault == "map_minus1_as_row0":
        rowsrc = rowsrc.clamp(min=0)
    Bv = torch.cat([_gather(src, _neighbours(c, rowsrc, t, fault), None) for t in range(taps_of(c.conv))], dim=2)
    return Ae, Bv


def tn_reference(c, inp=None, fault=None, floor=False):
    """{'C': [batch][I][J], 'colsum': [batch][I]} as float64: the exact value in mode 'int', the fp64 value in mode 'real' -- or, with floor, the fp32
    evaluation by torch.  colsum only where the case has one."""
    i = inp or inputs(c)
    Ae, Bv = effective(c, i, fault)

    def stored(acc):          # column (tap, c) of the contraction lands at c * taps + tap
        if c.permute and fault != "permute_transposed":
            return acc.reshape(c.batch, c.I, taps_of(c.conv), c.conv["kc"]).transpose(2, 3).reshape(c.batch, c.I, c.J)
        return acc
    if c.mode == "int" and not floor:
        # integers scaled by 8: 2 s and 4 alpha are integers
        A2 = (Ae * 2.0).round()
        assert torch.equal(A2, Ae * 2.0)
        a4 = round(c.alpha * 4.0)
        assert a4 == c.alpha * 4.0
        acc = torch.zeros(c.batch, c.I, c.J, dtype=torch.float64) if Bv is None else torch.matmul(A2.transpose(1, 2), Bv)
        cs = A2.sum(1)
        C8, cs8 = i["C0"] * 8.0 + a4 * stored(acc), i["cs0"] * 8.0 + (4 if fault == "colsum_without_alpha" else a4) * cs
        assert float(C8.abs().max()) < 2.0 ** 50
        C, cs = C8.round().to(torch.int64).double() / 8.0, cs8.round().to(torch.int64).double() / 8.0
    else:
        dt = torch.float32 if floor else torch.float64
        Ad = Ae.to(dt)
        acc = torch.zeros(c.batch, c.I, c.J, dtype=dt) if Bv is None else torch.matmul(Ad.transpose(1, 2), Bv.to(dt))
        al = torch.tensor(c.alpha, dtype=dt)
        C = (i["C0"].to(dt) + al * stored(acc)).double()
        if floor:          # row after row, as every K loop of the family adds them (torch's own sum is pairwise: a floor no sequential kernel can reach)
            tot = torch.zeros(c.batch, c.I, dtype=dt)
            for k in range(c.K):
                tot += Ad[:, k]
        else:
            tot = Ad.sum(1)
        cs = (i["cs0"].to(dt) + (1.0 if fault == "colsum_without_alpha" else al) * tot).double()
    if fault == "colsum_batch_stride_ignored" and c.batch > 1:
        tot = cs - i["cs0"]
        cs = i["cs0"].clone()
        cs[0] = cs[0] + tot.sum(0)
    out = {"C": C}
    if c.colsum:
        out["colsum"] = cs
    return out


def unpack_reference(c, packed, dw0):
    """lavt_unpack_conv_grad: dw [Cout][Cin][taps] += packed [Cout][taps][Cin]"""
    t = taps_of(c.conv)
    return dw0 + packed.reshape(c.I, t, c.conv["kc"]).transpose(1, 2)


def exactness(c, inp=None):
    """(largest sum over k of |addend| plus |initial value| over C and colsum, whether every addend is a multiple of 2^-3) of an integer case"""
    i = inp or inputs(c)
    Ae, Bv = effective(c, i)
    a = abs(c.alpha)
    m = float((a * Ae.abs().sum(1) + i["cs0"].abs()).max())
    ok = bool(torch.equal((Ae * c.alpha * 8.0).round(), Ae * c.alpha * 8.0))
    if Bv is not None:
        m = max(m, float((a * torch.matmul(Ae.abs().transpose(1, 2), Bv.abs()) + i["C0"].abs()).max()))
    return m, ok


def gate(key, got, ref, flo):
    E, F = nt_error(got, ref), nt_error(flo, ref)
    return E, F, E <= K_TN[key] * F


# ------------------------------------------------------------------------------------------------ the fused conv weight gradient
class ConvCase:
    """lavt_conv3x3_wgrad (f8=False) / lavt_conv3x3_wgrad_f8: dW [Cout][Cin][9] over B images of H x W, X = concat(x1 [c1], x2 [Cin - c1])"""

    def __init__(self, name, route, *, B, H, W, Cout=128, Cin, c1=0, accumulate=False, f8=False, amax=(448.0, 448.0), mode="int", invalid=False, scratch="ws"):
        self.scratch, self.tuning = scratch, {}
        self.name, self.route, self.B, self.H, self.W, self.Cout, self.Cin, self.c1 = name, route, B, H, W, Cout, Cin, c1
        self.accumulate, self.f8, self.amax, self.mode, self.invalid = accumulate, f8, amax, mode, invalid
        pad = 16 if f8 else 8
        self.tn = Case(name + "/tn", "", I=Cout, K=B * H * W, conv=conv(B, H, W, Cin), b_split=c1, permute=True, accumulate=accumulate, mode=mode,
                       alpha=(amax[0] / 448.0) * (amax[1] / 448.0), ld_pad=(pad, pad, 0))

    def __repr__(self):
        return self.name


def conv_wgrad_reference(cc, floor=False):
    """dW [Cout][Cin][9] float64: the TN contract with taps, two concat sources and the permuted store (alpha = the de-quantisation factor of the fp8 form)"""
    return tn_reference(cc.tn, floor=floor)["C"][0].reshape(cc.Cout, cc.Cin, 9)


# ------------------------------------------------------------------------------------------------ the planners, restated
DEFAULT = dict(tile=0, tn_pipe=2, min_tiles=128, min_ktiles=12, stages=4)      # csrc/tuning.hip
ENV = {"tile": "LAVT_GEMM_TILE", "tn_pipe": "LAVT_TN_PIPE", "min_tiles": "LAVT_TN_PIPE_MIN_TILES", "min_ktiles": "LAVT_TN_PIPE_MIN_KTILES", "stages": "LAVT_TN_PIPE_STAGES"}


def tuning_env(t):
    return {ENV[k]: str(v) for k, v in t.items()}


def _maps(c):
    return bool(c.a_map or c.scale or c.b_map)


def contract_ok(c):
    """the argument checks of lavt_gemm_tn_route"""
    e = c.epc
    if c.I % e or c.J % e or c.lda % e or c.ldb % e:
        return False
    if c.b2 and (c.b1 % e or c.ldb2 % e):
        return False
    if c.conv and (c.conv["kc"] % e or c.J != taps_of(c.conv) * c.conv["kc"]):
        return False
    return True


def v2_eligible(c):
    if c.dtype != "bf16" or not c.zeros:
        return False
    if c.lda % 8 or c.ldb % 8 or (c.b2 and c.ldb2 % 8):
        return False
    if c.scale == "scaled":
        return False
    if _maps(c) and (c.conv or c.b2):
        return False
    return c.K * max(c.lda, c.ldb) < 1 << 31


def route_single(c, t):
    """lavt_gemm_tn -> 'v2/<tile>/<maps|plain>/cs<0|1|2>/<convp|lin>/p<pieces>/<store|atomic|parts>' or 'classic/<type>/<tile>/p<pieces>'"""
    if not contract_ok(c):
        return INVALID
    force = t["tile"]
    if v2_eligible(c):
        kt = cdiv(c.K, 64)
        t64, t128 = cdiv(c.I, 64) * cdiv(c.J, 64) * c.batch, cdiv(c.I, 128) * cdiv(c.J, 128) * c.batch
        big = force == 128 if force else (c.conv is not None and t128 >= 48 and kt >= 64)
        tiles = t128 if big else t64
        split = c.split_k
        if split <= 0:
            split = (384 + tiles // 2) // tiles if big else (768 + tiles // 2) // tiles
            split = max(split, (kt + 127) // 128)
            min_kt = 2 if c.batch > 1 else 8
            split = max(1, min(split, (kt + min_kt - 1) // min_kt))
        split = min(split, kt)
        tile = 128 if big else 64
        maps = _maps(c)
        cs = 0 if not c.colsum else (2 if tile == 64 and cdiv(c.J, 64) >= 4 else 1)
        convp = (not maps) and (c.conv is not None or c.permute)
        per = cdiv(kt, split)
        pieces = cdiv(kt, per)
        parts = pieces > 1 and c.partials is not None and not c.permute and c.partials_floats >= c.batch * pieces * (c.I * c.J + c.I)
        form = "parts" if parts else ("atomic" if pieces > 1 or c.accumulate else "store")
        return f"v2/{tile}/{'maps' if maps else 'plain'}/cs{cs}/{'convp' if convp else 'lin'}/p{pieces}/{form}"
    if c.colsum_atomic:
        return INVALID
    bk = 16 if c.dtype == "f32" else 64
    big = force == 128 if force else (c.I >= 256 and c.J >= 1024 and c.K >= 8192)
    tb = 128 if big else 64
    tiles, kt = cdiv(c.I, tb) * cdiv(c.J, tb), cdiv(c.K, bk)
    split = c.split_k
    if split <= 0:
        split = max(1, 768 // (tiles * c.batch))
        split = max(1, min(split, (kt + 3) // 4))
    split = min(split, kt)
    per = cdiv(kt, split)
    return f"classic/{c.dtype}/{tb}/p{cdiv(kt, per)}"


def ln_geometry(rows, C):
    """ln_bwd_geometry (csrc/norm.hip), bf16: (blocks, lanes per row, chunks per lane)"""
    nch = C // 8
    lpr = 16 if nch <= 16 else 32 if nch <= 32 else 64
    rpb = 4 * (64 // lpr)
    blocks = cdiv(rows, rpb)
    if blocks > 1280:
        blocks = cdiv(rows, 2 * rpb)
    return max(1, min(blocks, 2048)), lpr, cdiv(nch, lpr)


def _route_pipe(ms, t, ln):
    """tn_route_pipe: None when the group does not qualify"""
    if t["tn_pipe"] == 0 or not 2 <= len(ms) <= 6:
        return None
    base, work, geo = 0, 0, []
    for c in ms:
        if c.dtype != "bf16" or c.batch != 1 or c.conv or c.b2 or c.permute:
            return None
        if c.I % 8 or c.J % 4 or c.lda % 8 or c.ldb % 8 or c.K < 8:
            return None
        if (c.K + 1024) * c.lda * 2 >= 1 << 30 or (c.K + 1024) * c.ldb * 2 >= 1 << 30:
            return None
        if (c.a_src_rows > 0 and (c.a_src_rows + 1) * c.lda * 2 + 256 >= 1 << 31) or (c.b_src_rows > 0 and (c.b_src_rows + 1) * c.ldb * 2 + 256 >= 1 << 31):
            return None          # the rows a map may name stay inside the 2 GB descriptor
        if c.scale and (c.scale != "binary" or c.div < 64 or cdiv(c.K, c.div) > 64):
            return None
        if (c.no_b and not c.colsum) or (not c.no_b and c.J % 8):
            return None
        tl = cdiv(c.I, 128) * (1 if c.no_b else cdiv(c.J, 128))
        geo.append(tl)
        base += tl
        work += tl * cdiv(c.K, 64)
    rider = ""
    if ln is not None:
        _, lpr, cpl = ln_geometry(*ln)
        rider = f"+ln{lpr}" if cpl == 1 else "+ln-after"
    if base >= t["min_tiles"]:
        if work < base * t["min_ktiles"] or any(cdiv(c.K, 64) > 128 for c in ms):
            return None
        return f"pipe/s{3 if t['stages'] == 3 else 4}/uncut{rider}"
    if t["tn_pipe"] < 2:
        return None

    def piece_len(budget):
        l = max(8, cdiv(work, budget))
        while sum(tl * cdiv(cdiv(c.K, 64), l) for tl, c in zip(geo, ms)) > budget and l < 128:
            l += 1
        return l
    ln_len = piece_len(208 if ln is not None else 250)
    if ln is not None:
        free = piece_len(250)
        if 0.8 * ln_len > 0.8 * free + 4.0 + 6.0 * ln[0] * ln[1] / 3.0e6 + 1.0:
            ln_len, rider = free, "+ln-after"
    tiles, cut = 0, []
    for tl, c in zip(geo, ms):
        kt = cdiv(c.K, 64)
        per = cdiv(kt, cdiv(kt, ln_len))
        ns = cdiv(kt, per)
        if per > 128:
            return None
        if ns > 1 and c.partials_floats < ns * (c.I * c.J + c.I):
            return None
        cut.append(ns)
        tiles += tl * ns
    if tiles < 96 or tiles > 256:
        return None
    return f"pipe/s{3 if t['stages'] == 3 else 4}/cut={','.join(map(str, cut))}{rider}"


def _route_group64(ms, t, ln):
    """tn_route_group64, asked after the pipelined launch declined: None when the group does not form"""
    if not 2 <= len(ms) <= 6:
        return None
    uncut = sum(cdiv(c.I, 64) * cdiv(c.J, 64) for c in ms)
    cut_pays = uncut < 512
    per_piece = 8
    while True:
        tiles, splits, any_parts = 0, [], False
        for c in ms:
            if not v2_eligible(c) or c.batch != 1 or c.conv or c.b2 or c.I % 8 or c.J % 8:
                return None
            kt = cdiv(c.K, 64)
            want = cdiv(kt, per_piece)
            parts = c.partials is not None and not c.permute and kt > 48 and (cut_pays or kt > 128) and want > 1 and c.partials_floats >= want * (c.I * c.J + c.I)
            if parts:
                ns = want
            else:
                if kt > 128:
                    return None
                ns = min(4, cdiv(kt, 48) if (c.split_k < 0 and cut_pays) else 1)
            ns = cdiv(kt, cdiv(kt, ns))
            any_parts = any_parts or (parts and ns > 1)
            splits.append(ns)
            tiles += cdiv(c.I, 64) * cdiv(c.J, 64) * ns
        if tiles <= 2048 or not any_parts or per_piece >= 64:
            break
        per_piece *= 2
    if tiles < 256:
        return None
    maps, cs = any(_maps(c) for c in ms), any(c.colsum for c in ms)
    rider = ""
    if ln is not None:
        _, lpr, cpl = ln_geometry(*ln)
        rider = f"+ln{lpr}" if (cs and cpl == 1 and 3 * lpr * cpl * 8 * 4 <= 32768 + (2560 if maps else 0)) else "+ln-after"
    return f"group64/{'maps' if maps else 'plain'}/cs{2 if cs else 0}/s={','.join(map(str, splits))}{'/parts' if any_parts else ''}{rider}"


def sk_plan(ms):
    """tn_route_sk: (workgroups, scratch floats) or None"""
    if not 2 <= len(ms) <= 6:
        return None
    its = tiles = 0
    for c in ms:
        if not v2_eligible(c) or c.batch != 1 or c.conv or c.b2 or c.I % 8 or c.J % 8 or c.permute:
            return None
        tl = cdiv(c.I, 128) * cdiv(c.J, 128)
        its, tiles = its + tl * cdiv(c.K, 64), tiles + tl
    nw = 512 if its // 512 >= 6 else its // 6
    if nw < 128 or tiles < 32:
        return None
    return nw, nw * 2 * (128 * 128 + 128)


def cw_pieces(B, H, Cout, Cin, f8=False, W=0):
    tiles, rows = (Cout // 128) * cdiv(Cin, 64), B * H
    p = max(1, min(max(1, 256 // tiles), max(1, rows // 8)))
    rpp = cdiv(rows, p)
    if f8:
        rpk = 1 if W > 64 else 2
        rpp = cdiv(rpp, rpk) * rpk
    return cdiv(rows, rpp), rpp


def cw_supported(cc, f8=None):
    B, H, W, Cout, Cin, c1 = cc.B, cc.H, cc.W, cc.Cout, cc.Cin, cc.c1 or cc.Cin
    ok = B > 0 and H > 0 and 0 < W <= 128 and Cout % 128 == 0 and Cin % 8 == 0 and c1 % 64 == 0 and c1 <= Cin and B * H * W < 1 << 24
    if cc.f8 if f8 is None else f8:
        ok = ok and W > 32 and Cin % 16 == 0 and (W > 64 or H % 2 == 0)
    return ok


def cw_ws(cc):
    """lavt_conv3x3_wgrad_ws: floats of scratch (0: the bf16 kernel does not cover the shape)"""
    if not cw_supported(cc, f8=False):
        return 0
    tiles_j = cdiv(cc.Cin, 64)
    p = max(1, min(max(1, 256 // ((cc.Cout // 128) * tiles_j)), max(1, cc.B * cc.H // 8)))
    return p * cc.Cout * 9 * tiles_j * 64


def tn_route(x, tuning=None):
    t = dict(DEFAULT)
    t.update(x.tuning if tuning is None else tuning)
    if isinstance(x, ConvCase):
        if not cw_supported(x):
            return INVALID
        p, rpp = cw_pieces(x.B, x.H, x.Cout, x.Cin, x.f8, x.W)
        return f"{'cw8/rpk' + str(1 if x.W > 64 else 2) if x.f8 else 'cw'}/p{p}x{rpp}"
    if isinstance(x, Case):
        return route_single(x, t)
    ms = x.members
    if x.entry == "sk":
        plan = sk_plan(ms)
        if plan is None:
            return INVALID
        return f"sk/{'maps' if any(_maps(c) for c in ms) else 'plain'}/cs{1 if any(c.colsum for c in ms) else 0}/nw{plan[0]}"
    ln = x.ln if x.entry == "ln" else None
    r = _route_pipe(ms, t, ln) or _route_group64(ms, t, ln)
    if r is not None:
        return r
    each = [route_single(c, t) for c in ms]
    return INVALID if INVALID in each else "each" + ("+ln-after" if ln is not None else "")


# ------------------------------------------------------------------------------------------------ the table: single problems
T64, T128 = dict(tile=64), dict(tile=128)
_cs = dict(colsum=True)
SINGLE = [
    # v2 64x64: edges of I, J, K; the K tail; column sums scalar (cs1) and on the matrix cores (cs2: J = 264, four column tiles)
    Case("s-8x8x1", "v2/64/plain/cs0/lin/p1/store", I=8, J=8, K=1),
    Case("s-72x72x7-cs", "v2/64/plain/cs1/lin/p1/store", I=72, J=72, K=7, alpha=1.25, **_cs),
    Case("s-136x264x63-cs", "v2/64/plain/cs2/lin/p1/store", I=136, J=264, K=63, alpha=-0.5, **_cs),
    Case("s-72x8x64", "v2/64/plain/cs0/lin/p1/store", I=72, J=8, K=64),
    Case("s-8x72x65-acc", "v2/64/plain/cs1/lin/p1/atomic", I=8, J=72, K=65, accumulate=True, alpha=1.25, **_cs),
    Case("s-136x72x129", "v2/64/plain/cs1/lin/p1/store", I=136, J=72, K=129, **_cs),
    Case("s-72x264x1032-auto", "v2/64/plain/cs2/lin/p3/atomic", I=72, J=264, K=1032, alpha=-0.5, **_cs),
    Case("s-72x264x1032-auto-parts", "v2/64/plain/cs2/lin/p3/parts", I=72, J=264, K=1032, alpha=-0.5, partials="exact", **_cs),
    # explicit splits on 17 K tiles: 1, 2, 3 (6 + 6 + 5), ktiles, ktiles + 5; atomics and partial tiles (ktiles pieces exceed the lent bound: atomics)
    Case("s-split1", "v2/64/plain/cs1/lin/p1/store", I=72, J=72, K=1032, split_k=1, alpha=-0.5, **_cs),
    Case("s-split2", "v2/64/plain/cs1/lin/p2/atomic", I=72, J=72, K=1032, split_k=2, alpha=1.25, **_cs),
    Case("s-split3", "v2/64/plain/cs1/lin/p3/atomic", I=72, J=72, K=1032, split_k=3, **_cs),
    Case("s-split3-parts", "v2/64/plain/cs1/lin/p3/parts", I=72, J=72, K=1032, split_k=3, partials="exact", accumulate=True, alpha=-0.5, **_cs),
    Case("s-split17", "v2/64/plain/cs1/lin/p17/atomic", I=72, J=72, K=1032, split_k=17, **_cs),
    Case("s-split17-parts-small", "v2/64/plain/cs1/lin/p17/atomic", I=72, J=72, K=1032, split_k=17, partials="exact", **_cs),
    Case("s-split17-parts", "v2/64/plain/cs1/lin/p17/parts", I=72, J=72, K=1032, split_k=17, partials=17, alpha=1.25, **_cs),
    Case("s-split22", "v2/64/plain/cs0/lin/p17/atomic", I=136, J=8, K=1032, split_k=22),
    Case("s-split2-parts-nocs", "v2/64/plain/cs0/lin/p2/parts", I=8, J=264, K=129, split_k=2, partials=2),
    # maps: a_rowmap with -1 and repeats, b_rowmap, both, the binary mask (div 25: boundaries inside a K tile)
    Case("s-amap", "v2/64/maps/cs1/lin/p1/store", I=72, J=72, K=129, a_map=True, alpha=1.25, **_cs),
    Case("s-bmap", "v2/64/maps/cs0/lin/p1/store", I=136, J=72, K=65, b_map=True),
    Case("s-abmap-split", "v2/64/maps/cs2/lin/p3/atomic", I=72, J=264, K=1029, a_map=True, b_map=True, split_k=3, alpha=-0.5, **_cs),
    Case("s-abmap-parts", "v2/64/maps/cs1/lin/p3/parts", I=72, J=72, K=1029, a_map=True, b_map=True, split_k=3, partials="exact", accumulate=True, **_cs),
    Case("s-mask25", "v2/64/maps/cs1/lin/p1/store", I=72, J=72, K=450, scale="binary", div=25, v=1.25, alpha=1.25, **_cs),
    Case("s-mask75-amap-auto", "v2/64/maps/cs2/lin/p3/atomic", I=136, J=264, K=1050, scale="binary", div=75, a_map=True, v=2.0, alpha=-0.5, **_cs),
    Case("s-mask225-parts", "v2/64/maps/cs1/lin/p4/parts", I=8, J=72, K=1800, scale="binary", div=225, split_k=4, partials="exact", alpha=1.25, **_cs),
    # batch 3, all four strides wider than the matrices
    Case("s-batch3", "v2/64/plain/cs1/lin/p1/store", I=72, J=72, K=65, batch=3, alpha=1.25, **_cs),
    Case("s-batch3-split", "v2/64/plain/cs1/lin/p5/atomic", I=72, J=72, K=577, batch=3, alpha=-0.5, **_cs),
    Case("s-batch3-parts", "v2/64/plain/cs1/lin/p5/parts", I=72, J=72, K=577, batch=3, partials="exact", accumulate=True, **_cs),
    Case("s-batch3-amap", "v2/64/maps/cs0/lin/p3/atomic", I=8, J=136, K=321, batch=3, a_map=True, split_k=3),
]
SINGLE_128 = [
    Case("b-136x264x129-cs", "v2/128/plain/cs1/lin/p1/store", I=136, J=264, K=129, alpha=1.25, tuning=T128, **_cs),
    Case("b-72x8x1032-split3", "v2/128/plain/cs1/lin/p3/atomic", I=72, J=8, K=1032, split_k=3, alpha=-0.5, tuning=T128, **_cs),
    Case("b-abmap-parts", "v2/128/maps/cs1/lin/p3/parts", I=136, J=136, K=1029, a_map=True, b_map=True, split_k=3, partials="exact", accumulate=True, tuning=T128, **_cs),
    Case("b-mask75", "v2/128/maps/cs0/lin/p1/store", I=264, J=72, K=450, scale="binary", div=75, v=0.5, tuning=T128),
    Case("b-264x136x65", "v2/128/plain/cs0/lin/p1/atomic", I=264, J=136, K=65, accumulate=True, alpha=-0.5, tuning=T128),
    Case("b-conv-1x2x67-cs", "v2/128/plain/cs1/convp/p1/store", I=136, K=134, conv=conv(1, 2, 67, 72), b_split=8, alpha=1.25, tuning=T128, **_cs),
    Case("b-conv-3x9x7", "v2/128/plain/cs0/convp/p1/store", I=136, K=189, conv=conv(3, 9, 7, 72), permute=True, tuning=T128),
    # the default rule: a conv problem with 56 tiles of 128x128 and 64 K tiles (split = (384 + 28) / 56 = 7 -> 10 K tiles per piece, 7 pieces)
    Case("b-conv-default", "v2/128/plain/cs0/convp/p7/atomic", I=1024, K=4096, conv=conv(1, 64, 64, 96)),
]
CLASSIC = [
    # fp32: I = 12, J = 20 and the edge list; BK = 16
    Case("c-f32-12x20x7", "classic/f32/64/p1", dtype="f32", I=12, J=20, K=7, alpha=1.25, ld_pad=(4, 8, 4), **_cs),
    Case("c-f32-72x72x65", "classic/f32/64/p2", dtype="f32", I=72, J=72, K=65, alpha=-0.5, accumulate=True, ld_pad=(4, 8, 4), **_cs),
    Case("c-f32-136x264x129-maps", "classic/f32/64/p3", dtype="f32", I=136, J=264, K=129, a_map=True, b_map=True, alpha=1.25, ld_pad=(4, 8, 4), **_cs),
    Case("c-f32-mask25", "classic/f32/64/p8", dtype="f32", I=72, J=8, K=450, scale="binary", div=25, v=1.25, alpha=1.25, ld_pad=(4, 8, 4), **_cs),
    Case("c-f32-12x20x1032-split3", "classic/f32/64/p3", dtype="f32", I=12, J=20, K=1032, split_k=3, alpha=-0.5, ld_pad=(4, 8, 4), **_cs),
    Case("c-f32-batch3", "classic/f32/64/p2", dtype="f32", I=12, J=72, K=65, batch=3, alpha=1.25, ld_pad=(4, 8, 4), **_cs),
    Case("c-f32-12x20x63-128", "classic/f32/128/p1", dtype="f32", I=12, J=20, K=63, alpha=1.25, tuning=T128, ld_pad=(4, 8, 4), **_cs),
    Case("c-f32-136x264x129-128", "classic/f32/128/p3", dtype="f32", I=136, J=264, K=129, alpha=-0.5, scale="scaled", div=25, tuning=T128, ld_pad=(4, 8, 4), **_cs),
    # bf16 problems the LDS-DMA kernels decline: a non-binary row scale, no zero page, maps under taps, maps with a second source
    Case("c-scaled", "classic/bf16/64/p2", I=72, J=72, K=450, scale="scaled", div=25, alpha=1.25, **_cs),
    Case("c-scaled-amap-128", "classic/bf16/128/p3", I=136, J=264, K=1032, scale="scaled", div=75, a_map=True, alpha=-0.5, split_k=3, tuning=T128, **_cs),
    Case("c-nozeros", "classic/bf16/64/p1", I=72, J=72, K=129, zeros=False, alpha=1.25, accumulate=True, **_cs),
    Case("c-nozeros-mask", "classic/bf16/64/p2", I=8, J=264, K=450, zeros=False, scale="binary", div=225, v=2.0, alpha=-0.5, **_cs),
    Case("c-maps-taps", "classic/bf16/64/p1", I=72, K=150, conv=conv(3, 9, 7, 8), b_map=True, a_map=True, alpha=1.25, permute=True, **_cs),
    Case("c-maps-b2", "classic/bf16/64/p1", I=72, J=72, K=129, b_split=8, a_map=True, alpha=-0.5, **_cs),
    Case("c-mask-taps-b2", "classic/bf16/64/p1", I=8, K=189, conv=conv(3, 9, 7, 72), b_split=64, scale="binary", div=63, v=1.25, alpha=1.25, **_cs),
    # the default big rule of the classic family: I >= 256, J >= 1024, K >= 8192
    Case("c-big-default", "classic/bf16/128/p32", I=256, J=1024, K=8192, zeros=False, alpha=1.25, **_cs),
]
TAPS = [
    Case(f"t-{n}x{h}x{w}-kc{kc}" + ("-b2" if bs else "") + ("-perm" if pm else ""), r, I=72, K=n * h * w, conv=conv(n, h, w, kc), b_split=bs, permute=pm, alpha=al,
         accumulate=acc, colsum=cs)
    for n, h, w, kc, bs, pm, al, acc, cs, r in [
        (1, 3, 5, 8, 0, False, 1.0, False, True, "v2/64/plain/cs1/convp/p1/store"),
        (3, 3, 5, 72, 8, True, 1.25, False, False, "v2/64/plain/cs0/convp/p1/store"),
        (1, 9, 7, 72, 64, False, -0.5, True, True, "v2/64/plain/cs2/convp/p1/atomic"),
        (3, 9, 7, 8, 0, True, 1.0, False, True, "v2/64/plain/cs1/convp/p1/store"),
        (3, 2, 67, 8, 0, False, 1.25, False, True, "v2/64/plain/cs1/convp/p1/store"),
        (1, 2, 67, 72, 8, True, -0.5, False, False, "v2/64/plain/cs0/convp/p1/store"),
    ]
] + [
    Case("t-3x9x7-kc72-split", "v2/64/plain/cs0/convp/p3/atomic", I=136, K=189, conv=conv(3, 9, 7, 72), b_split=64, permute=True, split_k=3, alpha=1.25),
    Case("t-3d-333", "v2/64/plain/cs2/convp/p1/store", I=72, K=60, conv=conv(2, 2, 5, 8, d=3, k=(3, 3, 3)), alpha=1.25, permute=True, **_cs),
    Case("t-3d-311", "v2/64/plain/cs0/convp/p1/store", I=8, K=60, conv=conv(2, 2, 5, 72, d=3, k=(3, 1, 1)), alpha=-0.5),
    Case("t-3d-133", "v2/64/plain/cs2/convp/p1/atomic", I=72, K=60, conv=conv(2, 2, 5, 72, d=3, k=(1, 3, 3)), b_split=8, accumulate=True, **_cs),
]
# the unpermuted twin of every permuted row: lavt_unpack_conv_grad of its result must equal the permuted result bit for bit
UNPACK = [c for c in TAPS if c.permute and not c.accumulate]


def unpermuted(c):
    return Case(c.name + "-packed", "", I=c.I, K=c.K, conv=c.conv, b_split=c.b_split, permute=False, alpha=c.alpha, colsum=c.colsum, split_k=c.split_k)


# ------------------------------------------------------------------------------------------------ the table: groups
def six(K, tag, *, split_k=0, partials=None, div=75, side_j4=False, unaligned=True, mode="int"):
    """the six member kinds of a Swin block's launch: plain, masked, both maps + accumulate, the column-sum-only side member and the member it shares a
    bias gradient with (colsum_atomic), C at a 12-byte offset; 72 + 45 + 24 + 7 + 35 + 81 = 264 tiles of 64x64, every one with overhang"""
    kw = dict(K=K, partials=partials, mode=mode)
    return [
        Case(f"{tag}/plain", "", I=520, J=504, split_k=split_k, alpha=1.25, colsum=True, **kw),
        Case(f"{tag}/masked", "", I=264, J=520, scale="binary", div=div, v=1.25, alpha=1.25, split_k=split_k, colsum=True, **kw),
        Case(f"{tag}/maps-acc", "", I=200, J=328, a_map=True, b_map=True, accumulate=True, alpha=-0.5, colsum=True, **kw),
        Case(f"{tag}/side", "", I=392, no_b=True, J=4 if side_j4 else 0, a_map=True, colsum=True, colsum_atomic=True, split_k=split_k, ld_pad=(8, 16, 0), **kw),
        Case(f"{tag}/shared", "", I=392, J=264, a_map=True, colsum=True, colsum_atomic=True, share=3, split_k=split_k, **kw),
        Case(f"{tag}/unaligned", "", I=520, J=520, c_off=3 if unaligned else 0, part_off=3 if (unaligned and partials) else 0, split_k=split_k, colsum=True, ld_pad=(8, 16, 0), **kw),
    ]


P0 = dict(tn_pipe=0)
GROUP64 = [
    Group("g64-k72", "group64/maps/cs2/s=1,1,1,1,1,1", six(72, "g64-k72"), tuning=P0),
    Group("g64-k3144-atomic", "group64/maps/cs2/s=2,2,1,2,2,2", six(3144, "g64-k3144-atomic", split_k=-1), tuning=P0),
    Group("g64-k3144-parts", "group64/maps/cs2/s=7,7,7,7,7,7/parts", six(3144, "g64-k3144-parts", partials=7), tuning=P0),
    Group("g64-mixed", "group64/maps/cs2/s=1,1,1,1", [
        Case("g64-mixed/a", "", I=520, J=504, K=129, alpha=1.25, colsum=True), Case("g64-mixed/b", "", I=520, J=520, K=65, a_map=True, colsum=True),
        Case("g64-mixed/c", "", I=520, J=392, K=130), Case("g64-mixed/d", "", I=264, J=520, K=72, b_map=True, accumulate=True, alpha=-0.5, colsum=True)], tuning=P0),
    Group("g64-nocolsum", "group64/plain/cs0/s=1,1,1,1", [Case(f"g64-nocolsum/{k}", "", I=520, J=504, K=72 + k, alpha=1.25) for k in range(4)], tuning=P0),
    Group("g64-maps-nocolsum", "group64/maps/cs0/s=1,1,1,1", [Case(f"g64-maps-nocolsum/{k}", "", I=520, J=504, K=65 + k, a_map=k == 1, b_map=k == 2, scale="binary" if k == 3 else None,
                                                                   div=25, v=2.0, alpha=-0.5) for k in range(4)], tuning=P0),
    # groups that must not form and run one by one with the same result
    Group("g64-n1", "each", [Case("g64-n1/a", "", I=520, J=504, K=129, alpha=1.25, colsum=True)], tuning=P0),
    Group("g64-few-tiles", "each", [Case(f"g64-few-tiles/{k}", "", I=136, J=264, K=129, a_map=k == 1, alpha=1.25, colsum=True) for k in range(3)], tuning=P0),
    Group("g64-batched", "each", [Case("g64-batched/a", "", I=520, J=1032, K=72, colsum=True), Case("g64-batched/b", "", I=520, J=1032, K=72, alpha=-0.5),
                                  Case("g64-batched/c", "", I=72, J=72, K=65, batch=3, colsum=True)], tuning=P0),
    Group("g64-conv", "each", [Case("g64-conv/a", "", I=520, J=1032, K=72, colsum=True), Case("g64-conv/b", "", I=520, J=1032, K=72, alpha=1.25),
                               Case("g64-conv/c", "", I=72, K=63, conv=conv(1, 9, 7, 8), permute=True)], tuning=P0),
]
_PU = dict(tn_pipe=2, min_ktiles=1, min_tiles=1)
_PC = dict(tn_pipe=2, min_ktiles=1, min_tiles=4096)


def _cut_members(tag, K=3080, pieces=7, div=75, ragged=0, **kw):
    """four 256x256 members (16 tiles of 128x128) the pipelined launch cuts into `pieces` pieces each: masked, accumulate, no column sum (C and partials
    off the 16-byte grid when `unaligned`), both maps (`ragged`: its reduction ends that many rows earlier, inside a group of eight map entries)"""
    ms = [Case(f"{tag}/{k}", "", I=256, J=256, K=K - (ragged if k == 3 else 0), partials=pieces, colsum=k != 2, alpha=(1.25, 1.0, -0.5, 1.0)[k], accumulate=k == 1,
               a_map=k == 3, b_map=k == 3, part_off=3 if (k == 2 and kw.get("unaligned")) else 0, c_off=3 if (k == 2 and kw.get("unaligned")) else 0,
               ld_pad=(8, 16, 0), scale="binary" if k == 0 else None, div=div if k == 0 else 1, v=1.25) for k in range(4)]
    if kw.get("side"):          # + the column-sum-only side member (its C stays as it was) and the member it shares a bias gradient with
        ms += [Case(f"{tag}/side", "", I=256, no_b=True, K=K, partials=pieces, a_map=True, colsum=True, colsum_atomic=True, ld_pad=(8, 16, 0)),
               Case(f"{tag}/shared", "", I=256, J=256, K=K, partials=pieces, a_map=True, colsum=True, colsum_atomic=True, share=4, ld_pad=(8, 16, 0))]
    return ms


def _deep_members(tag, K, pieces):
    """six 128x128 members (one tile each) on a long reduction -- the shape of stage 0, cut into ~20 pieces each: plain, masked, both maps + accumulate on a
    ragged reduction, the column-sum-only side member and the member it shares a bias gradient with, C and partials off the 16-byte grid"""
    kw = dict(K=K, partials=pieces, ld_pad=(8, 16, 0))
    return [
        Case(f"{tag}/plain", "", I=128, J=128, alpha=1.25, colsum=True, **kw),
        Case(f"{tag}/masked", "", I=128, J=128, scale="binary", div=225, v=1.25, alpha=1.25, colsum=True, **kw),
        Case(f"{tag}/maps-acc", "", I=128, J=128, a_map=True, b_map=True, accumulate=True, alpha=-0.5, colsum=True, **dict(kw, K=K - 3)),
        Case(f"{tag}/side", "", I=128, no_b=True, a_map=True, colsum=True, colsum_atomic=True, **kw),
        Case(f"{tag}/shared", "", I=128, J=128, a_map=True, colsum=True, colsum_atomic=True, share=3, **kw),
        Case(f"{tag}/unaligned", "", I=128, J=128, c_off=3, part_off=3, **kw),
    ]


PIPE = [Group(f"p{s}-k{K}", r.format(s=s), six(K, f"p{s}-k{K}", partials=pt), tuning=dict(_PU, stages=s))
        for s in (3, 4) for K, pt, r in [(8, None, "pipe/s{s}/uncut"), (72, None, "pipe/s{s}/uncut"), (450, None, "pipe/s{s}/uncut")]] + [
    # 129 K tiles: the pipelined launch declines; with a scratch the 64x64 launch cuts every member -- pieces of 8 and 16 K tiles give 4488 and 2376
    # workgroups (> 2048), pieces of 32 give cdiv(129, 32) = 5 each
    Group("p4-k8200", "group64/maps/cs2/s=5,5,5,5,5,5/parts", six(8200, "p4-k8200", partials=17, div=225), tuning=dict(_PU, stages=4)),
    Group("p3-cut", "pipe/s3/cut=7,7,7,7", _cut_members("p3-cut", unaligned=True), tuning=dict(_PC, stages=3)),
    Group("p4-cut", "pipe/s4/cut=7,7,7,7", _cut_members("p4-cut", unaligned=False), tuning=dict(_PC, stages=4)),
    # the two reducers of the cut launch.  tnp_reduce_pieces adds eight pieces at a time and then the rest: 7 pieces (above) take only the rest, 8 pieces
    # (64 K tiles) only the eights.  More than 8 pieces go to tnp_reduce_pieces_deep, four piece lanes per output: 12 pieces (96 K tiles, 192
    # workgroups) take its one-by-one loop alone, 20 pieces (six one-tile members at 160 K tiles) its four-way unrolled one.  The mapped member of each
    # ends its reduction 3 rows short of a multiple of 8: the ragged map tail inside the LAST piece of a cut member
    Group("p3-cut8", "pipe/s3/cut=8,8,8,8,8,8", _cut_members("p3-cut8", K=4040, pieces=8, ragged=3, side=True), tuning=dict(_PC, stages=3)),
    Group("p4-cut12", "pipe/s4/cut=12,12,12,12", _cut_members("p4-cut12", K=6088, pieces=12, div=225, ragged=3, unaligned=True), tuning=dict(_PC, stages=4)),
    Group("p4-cut20", "pipe/s4/cut=20,20,20,20,20,20", _deep_members("p4-cut20", 10200, 20), tuning=dict(_PC, stages=4)),
    Group("p3-cut20", "pipe/s3/cut=20,20,20,20,20,20", _deep_members("p3-cut20", 10200, 20), tuning=dict(_PC, stages=3)),
    # a mask whose samples are shorter than a K tile: the pipelined launch keeps one keep bit per sample of >= 64 rows and declines
    Group("p4-div25", "group64/maps/cs2/s=1,1,1,1,1,1", six(450, "p4-div25", div=25), tuning=dict(_PU, stages=4)),
    # J % 8 == 4 on the column-sum-only member (its C is four columns wide and stays as it was)
    Group("p4-j4", "pipe/s4/uncut", six(72, "p4-j4", side_j4=True), tuning=dict(_PU, stages=4)),
]


def _rider_members(tag, C, T, maps=False):
    """the four weight gradients of a Swin block; `maps`: under DropPath and window partition -- fc2 masked per sample, proj and qkv through row maps"""
    fc2 = dict(scale="binary", div=75, v=1.25) if maps else {}
    return [Case(f"{tag}/fc2", "", I=C, J=4 * C, K=T, colsum=True, alpha=1.25, **fc2), Case(f"{tag}/fc1", "", I=4 * C, J=C, K=T, colsum=True),
            Case(f"{tag}/proj", "", I=C, J=C, K=T, colsum=True, alpha=-0.5, a_map=maps), Case(f"{tag}/qkv", "", I=3 * C, J=C, K=T, colsum=True, b_map=maps)]


def _dropped_rider_members(tag):
    """108 tiles of 128x128 at 16 K tiles: with a fifth of the chip kept for riders (208 workgroups) the members stay whole, without (250) they are cut in
    two -- 0.8 us x (16 - 8) K tiles is more than the LayerNorm's own launch, so the pipelined launch drops the rider it was offered"""
    return [Case(f"{tag}/{k}", "", I=384, J=1152, K=1000 - (3 if k == 3 else 0), partials=2, colsum=k != 2, alpha=(1.25, 1.0, -0.5, 1.0)[k], accumulate=k == 1,
                 a_map=k == 3, b_map=k == 3, ld_pad=(8, 16, 0)) for k in range(4)]


# rider: the LayerNorm's geometry follows ITS (rows, C); the four members (block width 512: 768 tiles of 64x64, 1024: 3072) only carry it.  A block of width
# 128 (48 tiles) does not form a group on the 64x64 launch: one by one, the LayerNorm after them
RIDER = [
    Group("r64-each", "each+ln-after", _rider_members("r64-each", 128, 451), tuning=P0, entry="ln", ln=(451, 128)),
    Group("r64-128", "group64/plain/cs2/s=1,1,1,1+ln16", _rider_members("r64-128", 512, 451), tuning=P0, entry="ln", ln=(451, 128)),
    Group("r64-256", "group64/plain/cs2/s=1,1,1,1+ln32", _rider_members("r64-256", 512, 451), tuning=P0, entry="ln", ln=(451, 256)),
    Group("r64-512", "group64/plain/cs2/s=1,1,1,1+ln64", _rider_members("r64-512", 512, 451), tuning=P0, entry="ln", ln=(451, 512)),
    Group("r64-1024", "group64/plain/cs2/s=1,1,1,1+ln-after", _rider_members("r64-1024", 1024, 131), tuning=P0, entry="ln", ln=(131, 1024)),
    Group("rp-128", "pipe/s4/uncut+ln16", _rider_members("rp-128", 128, 451), tuning=dict(_PU, stages=4), entry="ln", ln=(451, 128)),
    Group("rp-256", "pipe/s3/uncut+ln32", _rider_members("rp-256", 256, 451), tuning=dict(_PU, stages=3), entry="ln", ln=(451, 256)),
    Group("rp-512", "pipe/s4/uncut+ln64", _rider_members("rp-512", 512, 451), tuning=dict(_PU, stages=4), entry="ln", ln=(451, 512)),
    Group("rp-1024", "pipe/s4/uncut+ln-after", _rider_members("rp-1024", 1024, 131), tuning=dict(_PU, stages=4), entry="ln", ln=(131, 1024)),
    # a block under DropPath and window partition on the 64x64 launch: the rider kernels of the MAPPED K loop, one per LayerNorm width
    Group("r64m-128", "group64/maps/cs2/s=1,1,1,1+ln16", _rider_members("r64m-128", 512, 451, maps=True), tuning=P0, entry="ln", ln=(451, 128)),
    Group("r64m-256", "group64/maps/cs2/s=1,1,1,1+ln32", _rider_members("r64m-256", 512, 451, maps=True), tuning=P0, entry="ln", ln=(451, 256)),
    Group("r64m-512", "group64/maps/cs2/s=1,1,1,1+ln64", _rider_members("r64m-512", 512, 451, maps=True), tuning=P0, entry="ln", ln=(451, 512)),
    # the other ring depth of every rider width of the pipelined launch (mapped members: the kernel is one per (stages, lanes), whatever the members)
    Group("rpm-128", "pipe/s3/uncut+ln16", _rider_members("rpm-128", 128, 451, maps=True), tuning=dict(_PU, stages=3), entry="ln", ln=(451, 128)),
    Group("rpm-256", "pipe/s4/uncut+ln32", _rider_members("rpm-256", 256, 451, maps=True), tuning=dict(_PU, stages=4), entry="ln", ln=(451, 256)),
    Group("rpm-512", "pipe/s3/uncut+ln64", _rider_members("rpm-512", 512, 451, maps=True), tuning=dict(_PU, stages=3), entry="ln", ln=(451, 512)),
    # the CUT pipelined launch offered a rider: pieces sized for 208 workgroups; kept (the piece length is the same 8 K tiles either way) and dropped
    # (return code 3: the entry point launches the LayerNorm itself)
    Group("rp-cut", "pipe/s4/cut=7,7,7,7+ln32", _cut_members("rp-cut"), tuning=dict(_PC, stages=4), entry="ln", ln=(451, 256)),
    Group("rp-cut-dropped", "pipe/s4/cut=2,2,2,2+ln-after", _dropped_rider_members("rp-cut-dropped"), tuning=dict(_PC, stages=4), entry="ln", ln=(451, 256)),
]
STREAMK = [
    Group("sk-maps-nocs", "sk/maps/cs0/nw133", [Case("sk-maps-nocs/a", "", I=520, J=512, K=1544, a_map=True, b_map=True, alpha=1.25), Case("sk-maps-nocs/b", "", I=512, J=384, K=1544, accumulate=True)],
          entry="sk"),
    # 20 + 12 = 32 tiles of 128x128 at 25 K tiles: 800 iterations, 133 runs of ~6
    Group("sk-2", "sk/plain/cs1/nw133", [Case("sk-2/a", "", I=520, J=512, K=1544, alpha=1.25, colsum=True), Case("sk-2/b", "", I=512, J=384, K=1544, accumulate=True, alpha=-0.5, colsum=True)],
          entry="sk"),
    Group("sk-nocs", "sk/plain/cs0/nw133", [Case("sk-nocs/a", "", I=520, J=512, K=1544, alpha=1.25), Case("sk-nocs/b", "", I=512, J=384, K=1544)], entry="sk"),
    Group("sk-pair", "sk/maps/cs1/nw200", [
        Case("sk-pair/a", "", I=520, J=512, K=1544, scale="binary", div=75, v=1.25, alpha=1.25, colsum=True), Case("sk-pair/b", "", I=512, J=384, K=1544, accumulate=True, colsum=True),
        Case("sk-pair/side", "", I=392, no_b=True, K=1544, a_map=True, colsum=True, colsum_atomic=True, ld_pad=(8, 16, 0)),
        Case("sk-pair/shared", "", I=392, J=264, K=1544, a_map=True, colsum=True, colsum_atomic=True, share=2)], entry="sk"),
]
SK_REFUSED = [
    Group("sk-small", INVALID, [Case("sk-small/a", "", I=520, J=512, K=72), Case("sk-small/b", "", I=512, J=384, K=72)], entry="sk", invalid=True),
    Group("sk-short-scratch", "sk/plain/cs0/nw133", [Case("sk-short-scratch/a", "", I=520, J=512, K=1544), Case("sk-short-scratch/b", "", I=512, J=384, K=1544)], entry="sk",
          invalid=True, scratch="short"),
]

# ------------------------------------------------------------------------------------------------ the table: fused conv weight gradients
CONVW = [ConvCase(f"cw-{B}x{H}x{W}-ci{Cin}" + ("-acc" if acc else ""), r, B=B, H=H, W=W, Cin=Cin, c1=c1, accumulate=acc)
         for B, H, W, Cin, c1, acc, r in [
             (1, 3, 5, 64, 0, False, "cw/p1x3"), (3, 7, 32, 88, 64, True, "cw/p2x11"), (2, 9, 33, 128, 0, False, "cw/p2x9"), (3, 7, 64, 64, 0, True, "cw/p2x11"),
             (2, 9, 65, 88, 64, False, "cw/p2x9"), (1, 3, 96, 128, 64, True, "cw/p1x3"), (3, 7, 97, 64, 0, False, "cw/p2x11"), (2, 9, 128, 88, 64, True, "cw/p2x9"),
             (3, 7, 5, 128, 64, False, "cw/p2x11")]]
CONVW8 = [ConvCase(f"cw8-{B}x{H}x{W}-ci{Cin}-{int(am[0])}" + ("-acc" if acc else ""), r, B=B, H=H, W=W, Cin=Cin, c1=c1, accumulate=acc, f8=True, amax=am)
          for B, H, W, Cin, c1, acc, am, r in [
              (3, 6, 33, 64, 0, False, (448.0, 448.0), "cw8/rpk2/p2x10"), (3, 6, 64, 80, 64, True, (224.0, 448.0), "cw8/rpk2/p2x10"),
              (3, 7, 65, 64, 0, True, (448.0, 448.0), "cw8/rpk1/p2x11"), (2, 9, 128, 80, 64, False, (224.0, 448.0), "cw8/rpk1/p2x9")]]
CONVW_REFUSED = [ConvCase("cw-w129", INVALID, B=1, H=3, W=129, Cin=64, invalid=True), ConvCase("cw-cout64", INVALID, B=1, H=3, W=5, Cout=64, Cin=64, invalid=True),
                 ConvCase("cw-c1-8", INVALID, B=1, H=3, W=5, Cin=64, c1=8, invalid=True), ConvCase("cw8-w32", INVALID, B=1, H=4, W=32, Cin=64, f8=True, invalid=True),
                 ConvCase("cw8-h-odd", INVALID, B=1, H=3, W=64, Cin=64, f8=True, invalid=True),
                 ConvCase("cw-short-scratch", "cw/p1x3", B=1, H=3, W=5, Cin=64, invalid=True, scratch="short")]

# ------------------------------------------------------------------------------------------------ refusals of lavt_gemm_tn
REFUSALS = [
    Case("x-i-mod8", INVALID, I=12, J=72, K=65, invalid=True),
    Case("x-lda-mod8", INVALID, I=72, J=72, K=65, lda=76, invalid=True),
    Case("x-j-not-taps-kc", INVALID, I=72, K=15, conv=conv(1, 3, 5, 8), invalid=True),
    Case("x-colsum-atomic-f32", INVALID, dtype="f32", I=12, J=20, K=7, colsum=True, colsum_atomic=True, ld_pad=(4, 8, 4), invalid=True),
]
REFUSALS[2].J = 64          # J != taps * kc

# ------------------------------------------------------------------------------------------------ real mode: one row per route
REAL = [
    Case("r-v2-64", "v2/64/plain/cs2/lin/p1/store", mode="real", I=136, J=264, K=1032, split_k=1, alpha=1.25, **_cs),
    Case("r-v2-64-parts", "v2/64/plain/cs1/lin/p3/parts", mode="real", I=72, J=72, K=1032, split_k=3, partials="exact", accumulate=True, alpha=-0.5, **_cs),
    Case("r-v2-64-atomic", "v2/64/maps/cs2/lin/p3/atomic", mode="real", I=72, J=264, K=1029, a_map=True, b_map=True, split_k=3, alpha=-0.5, **_cs),
    Case("r-v2-64-mask", "v2/64/maps/cs1/lin/p1/store", mode="real", I=72, J=72, K=450, scale="binary", div=25, v=1.25, alpha=1.25, **_cs),
    Case("r-v2-128", "v2/128/plain/cs1/lin/p1/store", mode="real", I=136, J=264, K=129, alpha=1.25, tuning=T128, **_cs),
    Case("r-v2-taps", "v2/64/plain/cs1/convp/p1/store", mode="real", I=72, K=189, conv=conv(3, 9, 7, 8), permute=True, **_cs),
    Case("r-classic-f32", "classic/f32/64/p3", mode="real", dtype="f32", I=136, J=264, K=129, a_map=True, b_map=True, alpha=1.25, ld_pad=(4, 8, 4), **_cs),
    Case("r-classic-scaled", "classic/bf16/64/p2", mode="real", I=72, J=72, K=450, scale="scaled", div=25, alpha=1.25, **_cs),
]
REAL_GROUPS = [
    Group("r-g64", "group64/maps/cs2/s=1,1,1,1,1,1", six(72, "r-g64", mode="real"), tuning=P0),
    Group("r-g64-parts", "group64/maps/cs2/s=7,7,7,7,7,7/parts", six(3144, "r-g64-parts", partials=7, mode="real"), tuning=P0),
    Group("r-pipe", "pipe/s4/uncut", six(450, "r-pipe", mode="real"), tuning=dict(_PU, stages=4)),
    Group("r-pipe-cut", "pipe/s4/cut=7,7,7,7", [Case(f"r-pipe-cut/{k}", "", mode="real", I=256, J=256, K=3080, partials=7, colsum=True, ld_pad=(8, 16, 0)) for k in range(4)],
          tuning=dict(_PC, stages=4)),
    Group("r-sk", "sk/plain/cs1/nw133", [Case("r-sk/a", "", mode="real", I=520, J=512, K=1544, alpha=1.25, colsum=True),
                                           Case("r-sk/b", "", mode="real", I=512, J=384, K=1544, accumulate=True, colsum=True)], entry="sk"),
]
REAL_CONVW = [ConvCase("r-cw", "cw/p2x11", B=3, H=7, W=33, Cin=88, c1=64, accumulate=True, mode="real")]


def order_free(route):
    """routes whose result does not depend on the order atomics land in (a second run must be bit-identical in real mode too): unsplit stores and partial
    tiles of a single problem, uncut groups (one writer per element; a shared bias gradient takes two addends into zeros), groups cut through partial
    tiles, stream-K, the fused conv gradients"""
    r = route.split("+ln")[0]
    p = r.split("/")
    if p[0] == "v2":
        return p[-1] in ("store", "parts")
    if p[0] == "group64":
        return p[-1] == "parts" or set(p[3][2:].split(",")) == {"1"}
    return p[0] in ("pipe", "sk", "cw", "cw8")

SINGLES = SINGLE + SINGLE_128 + CLASSIC + TAPS + REAL
GROUPS = GROUP64 + PIPE + RIDER + STREAMK + REAL_GROUPS
BY_NAME = {c.name: c for c in SINGLES + REFUSALS}
ALL_ROUTED = SINGLES + REFUSALS + GROUPS + SK_REFUSED + CONVW + CONVW8 + CONVW_REFUSED + REAL_CONVW


def members_of(rows):
    for r in rows:
        if isinstance(r, Group):
            yield from r.members
        elif isinstance(r, ConvCase):
            yield r.tn
        else:
            yield r


def reachable():
    """every __global__ instantiation the launchers of the family can pick, named after the kernel with the template arguments that vary, plus (names with
    a '/') the paths inside a kernel that a host decision or a piece count selects: what the host test requires the rows that run to cover"""
    v2 = {f"gemm_tn_v2_kernel<{t},{m},{cs},{cv}>" for t in (64, 128) for m in ("maps", "plain") for cs in ("cs0", "cs1", "cs2") for cv in ("lin", "convp")
          if not (t == 128 and cs == "cs2") and not (m == "maps" and cv == "convp")}
    classic = {f"gemm_tn_kernel<{d},{t}>" for d in ("f32", "bf16") for t in (64, 128)}
    group = {f"gemm_tn_v2_grouped_kernel<{m},{cs}>" for m in ("maps", "plain") for cs in ("cs0", "cs2")}
    group |= {f"gemm_tn_v2_grouped_ln_kernel<{m},{l}>" for m in ("maps", "plain") for l in (16, 32, 64)}
    pipe = {f"gemm_tn_pipe_kernel<{s},{l}>" for s in (3, 4) for l in (0, 16, 32, 64)}
    pipe |= {f"gemm_tn_pipe_kernel<{s},*>/tile{m}/{k}" for s in (3, 4) for m in (0, 1, 2) for k in ("whole", "cut")}
    reducers = {"tn_reduce_pieces", "tn_reduce_pieces_group", "tnp_reduce_pieces", "tnp_reduce_pieces/eights", "tnp_reduce_pieces/rest", "tnp_reduce_pieces_deep",
                "tnp_reduce_pieces_deep/one-by-one", "tnp_reduce_pieces_deep/unrolled", "gemm_tn_pipe_kernel/cut+rider", "gemm_tn_pipe_kernel/cut-rider-dropped"}
    sk = {f"gemm_tn_v2_streamk_kernel<{m},{cs}>" for m in ("maps", "plain") for cs in ("cs0", "cs1")} | {"tn_streamk_fixup"}
    cw = {f"conv_wgrad3x3_kernel<{ks}>" for ks in (1, 2, 3, 4)} | {f"conv_wgrad3x3_f8_kernel<{r}>" for r in (1, 2)} | {"conv_wgrad3x3_reduce"}
    return v2 | classic | group | pipe | reducers | sk | cw


def _single_launches(route):
    p = route.split("/")
    if p[0] == "classic":
        return {f"gemm_tn_kernel<{p[1]},{p[2]}>"}
    return {f"gemm_tn_v2_kernel<{p[1]},{p[2]},{p[3]},{p[4]}>"} | ({"tn_reduce_pieces"} if p[6] == "parts" else set())


def launches(x, tuning=None):
    """what a row launches, in the names of `reachable` (empty for a row that is refused)"""
    t = dict(DEFAULT)
    t.update(x.tuning if tuning is None else tuning)
    r = tn_route(x, tuning)
    if r == INVALID or x.invalid:
        return set()
    if isinstance(x, ConvCase):
        return {f"conv_wgrad3x3_f8_kernel<{1 if x.W > 64 else 2}>" if x.f8 else f"conv_wgrad3x3_kernel<{cdiv(x.W, 32)}>", "conv_wgrad3x3_reduce"}
    if isinstance(x, Case):
        return _single_launches(r)
    if r.startswith("each"):
        return set().union(*(_single_launches(route_single(c, t)) for c in x.members))
    base, _, rider = r.partition("+ln")
    lanes = int(rider) if rider.isdigit() else 0
    p = base.split("/")
    if p[0] == "sk":
        return {f"gemm_tn_v2_streamk_kernel<{p[1]},{p[2]}>", "tn_streamk_fixup"}
    if p[0] == "group64":
        out = {f"gemm_tn_v2_grouped_ln_kernel<{p[1]},{lanes}>" if lanes else f"gemm_tn_v2_grouped_kernel<{p[1]},{p[2]}>"}
        return out | ({"tn_reduce_pieces_group"} if p[-1] == "parts" else set())
    s = p[1][1:]
    out = {f"gemm_tn_pipe_kernel<{s},{lanes}>"}
    cut = [int(n) for n in p[2][4:].split(",")] if p[2].startswith("cut=") else [1] * len(x.members)
    for c, ns in zip(x.members, cut):
        mode = 2 if (c.a_map or c.b_map) and c.K & 7 else 1 if _maps(c) else 0
        out.add(f"gemm_tn_pipe_kernel<{s},*>/tile{mode}/{'cut' if ns > 1 else 'whole'}")
    if max(cut) > 8:
        out |= {"tnp_reduce_pieces_deep", "tnp_reduce_pieces_deep/unrolled" if max(cut) > 12 else "tnp_reduce_pieces_deep/one-by-one"}
    elif max(cut) > 1:
        out |= {"tnp_reduce_pieces"} | {"tnp_reduce_pieces/eights" for n in cut if n >= 8} | {"tnp_reduce_pieces/rest" for n in cut if n > 1 and n % 8}
    if max(cut) > 1 and rider:
        out.add("gemm_tn_pipe_kernel/cut+rider" if lanes else "gemm_tn_pipe_kernel/cut-rider-dropped")
    return out
