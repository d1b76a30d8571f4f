"""Pairwise-sensitive references and gates for the window-attention kernels (csrc/attention_mfma.hip, attention.hip, attention_stream.hip, wmsa_fused.hip,
dtable_body.h).  CPU only: fp64 statements of the op built from the oracle's index and mask functions, the selecting probe, the per-entry table-gradient
metric, and the gate functions shared by the mutation self-test (test_attention_gates_host.py) and the GPU tests (test_gpu_attention_pairs.py).

Why these gates: with randn inputs the softmax is near-uniform, so a fault on a few (query, key) pairs -- a wrong table index at the corner offsets, one
mask bit, one padding column -- moves the output and the gradients by 1-3 % of their maximum, inside every bf16 max-norm gate.  The probe makes one pair
per query row carry the whole row; the per-entry metric weighs a table entry by the number of pairs it sums instead of by the largest entry."""
import itertools
from types import SimpleNamespace

import torch

from oracle import lavt_oracle as O
from oracle import lavt_video_oracle as OV

HD = 32                     # head dimension of every Swin / Video-Swin stage
PROBE = 30.0                # the probe's table value: exp(-30) * 1152 keys = 1e-10 of the row's mass stays on the other keys
FWD_BF16, FWD_L2 = 3e-2, 2e-2            # test_stream_parity's forward gates for the same arithmetic
BWD_BF16, BWD_L2 = 4.5e-2, 3e-2
FWD_F32, BWD_F32 = 2e-4, 1e-3
ENTRY_F32 = 1e-3
# bf16 per-entry gate = ENTRY_K[route] x the rounding floor F of the same case (reference with P, the stored output and dS rounded to bf16): twice the
# worst E / F measured on MI355X over that route's cases (test_gpu_attention_pairs.test_backward_per_entry lists them), and not under the floor itself
ENTRY_K = {"_WindowAttnBackward": 2 * 1.52, "_WindowAttnComposedBackward": 2 * 2.66, "_WindowAttnStreamBackward": 1.0}


def make_case(dims, window, shifted, batch=2):
    """dims: feature (D, H, W) (2-D: (1, H, W)); window: the layer's full window (2-D: (1, ws, ws)).  The window is clipped to the feature per axis as
    lib/video_swin_transformer.py:137-168 does; the bias is the top-left N x N block of the FULL window's index matrix."""
    dims, window = tuple(dims), tuple(window)
    win, shift = OV.clip_window(dims, window, tuple(w // 2 for w in window) if shifted else (0, 0, 0))
    assert all(d % w == 0 for d, w in zip(dims, win)), "op-level cases take features that are whole windows"
    N = win[0] * win[1] * win[2]
    nW = (dims[0] // win[0]) * (dims[1] // win[1]) * (dims[2] // win[2])
    two_d = window[0] == 1
    if two_d:
        idx = O.rel_pos_index(window[1])
        mask = O.shift_mask(dims[1], dims[2], window[1], shift[1]) if any(shift) else None
    else:
        idx = OV.rel_pos_index_3d(*window)[:N, :N]
        mask = OV.shift_mask_3d(*dims, win, shift) if any(shift) else None
    R = (2 * window[0] - 1) * (2 * window[1] - 1) * (2 * window[2] - 1)
    return SimpleNamespace(dims=dims, window=window, win=win, shift=shift, N=N, nW=nW, Bw=batch * nW, R=R, idx=idx.contiguous(), mask=mask, two_d=two_d)


def _bf(x):
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def _chunks(case, heads):
    step = max(1, (1 << 24) // (heads * case.N * case.N))
    return [(a, min(case.Bw, a + step)) for a in range(0, case.Bw, step)]


def _probs(case, q, k, table, idx, mask, a, b, pad_key):
    """P [b - a, heads, N, N (+1 with pad_key)] of windows a..b in fp64"""
    heads = table.shape[1]
    s = (q[a:b] * HD ** -0.5) @ k[a:b].transpose(-1, -2) + table[idx.reshape(-1)].view(case.N, case.N, heads).permute(2, 0, 1)[None]
    if mask is not None:
        s = s + mask.to(torch.float64)[torch.arange(a, b) % case.nW][:, None]
    if pad_key:          # a padded key column whose bias is 0 instead of -1e30: k = 0 gives the score 0, no mask reaches it, v = 0
        s = torch.cat([s, torch.zeros_like(s[..., :1])], -1)
    return s.softmax(-1)


def _split(case, qkv, heads):
    return qkv.to(torch.float64).view(case.Bw, case.N, 3, heads, HD).permute(2, 0, 3, 1, 4)


def reference(case, qkv, table, go=None, round_bf16=False, idx=None, mask=None, bin_idx=None, pad_key=False, with_dbias=False, with_top=False):
    """fp64 window attention: qkv [Bw * N, 3 * heads * 32] windowed rows, table [R, heads] -> y [Bw * N, heads * 32]; with go also (dqkv, dtable).
    round_bf16: P, the stored output (the one delta is formed from) and dS go through bf16, everything else stays fp64 -- the rounding floor of a
    bf16 kernel that keeps fp32 accumulators.  idx / mask replace the case's index matrix / mask (mutations); bin_idx replaces the index matrix of
    the table-gradient binning alone; pad_key appends one visible zero key (a padding column with bias 0); with_dbias also returns the dense bias
    gradient [heads, N, N] that `rebin` turns into a table gradient under another index matrix; with_top (forward only) returns (y, selection)
    from the same pass."""
    heads = table.shape[1]
    idx = case.idx if idx is None else idx
    mask = case.mask if mask is None else mask
    bin_idx = idx if bin_idx is None else bin_idx
    table = table.to(torch.float64)
    q, k, v = _split(case, qkv, heads)
    y = torch.empty(case.Bw, heads, case.N, HD, dtype=torch.float64)
    if go is not None:
        g = go.to(torch.float64).view(case.Bw, case.N, heads, HD).permute(0, 2, 1, 3)
        dq, dk, dv = torch.empty_like(y), torch.empty_like(y), torch.empty_like(y)
        dbias = torch.zeros(heads, case.N, case.N, dtype=torch.float64)
    tops = []
    for a, b in _chunks(case, heads):
        p = _probs(case, q, k, table, idx, mask, a, b, pad_key)[..., :case.N]
        if with_top:
            tops.append(p.max(-1))
        if round_bf16:
            p = _bf(p)
        y[a:b] = p @ v[a:b]
        if go is None:
            continue
        delta = (g[a:b] * (_bf(y[a:b]) if round_bf16 else y[a:b])).sum(-1, keepdim=True)
        ds = p * (g[a:b] @ v[a:b].transpose(-1, -2) - delta)
        if round_bf16:
            ds = _bf(ds)
        dv[a:b] = p.transpose(-1, -2) @ g[a:b]
        dq[a:b] = (ds @ k[a:b]) * HD ** -0.5
        dk[a:b] = (ds.transpose(-1, -2) @ q[a:b]) * HD ** -0.5
        dbias += ds.sum(0)
    y = y.permute(0, 2, 1, 3).reshape(case.Bw * case.N, heads * HD)
    if go is None:
        return (y, (torch.cat([t.values for t in tops]), torch.cat([t.indices for t in tops]))) if with_top else y
    dqkv = torch.stack([dq, dk, dv]).permute(1, 3, 0, 2, 4).reshape(case.Bw * case.N, 3 * heads * HD)
    dtable = rebin(case, dbias, bin_idx)
    return (y, dqkv, dtable, dbias) if with_dbias else (y, dqkv, dtable)


def rebin(case, dbias, bin_idx):
    """dense bias gradient [heads, N, N] -> table gradient [R, heads] through the index matrix bin_idx"""
    heads = dbias.shape[0]
    return torch.zeros(case.R, heads, dtype=torch.float64).index_add_(0, bin_idx.reshape(-1), dbias.permute(1, 2, 0).reshape(case.N * case.N, heads))


def corner_rows(case):
    """table rows of the offset box's corners (the first entries of probe_offsets)"""
    return probe_offsets(case, 1)[:2 ** sum(w > 1 for w in case.win)]


def idx_corners_to_neighbour(case):
    """mutation: every corner offset reads / bins into the neighbouring table entry"""
    idx = case.idx.clone()
    for r in corner_rows(case):
        idx[case.idx == r] = r + 1 if r + 1 < case.R and (r + 1) % (2 * case.window[2] - 1) != 0 else r - 1
    return idx


def idx_one_pair_shifted(case):
    """mutation: one (i, j) pair uses table row r + 1.  The pair is (first token, last token), the only pair of its offset.  One misplaced pair is
    1 / count[r] of its entry's terms: at the centre offset (count N) that is under the bf16 floor of any metric, so the self-test places the fault
    where a single pair is the whole entry."""
    idx = case.idx.clone()
    idx[0, case.N - 1] += 1
    return idx


def padding_table(case, heads):
    """-30 at every table row: softmax is invariant to the shift, so the reference is the zero table's (uniform attention over the visible keys) -- but a
    key column whose bias does not come from the table, such as a padding column left at 0 instead of -1e30, takes the whole row (e^30 against N keys)"""
    return torch.full((case.R, heads), -PROBE)


def masked_candidates(case, rows):
    """[nW, len(rows)]: pairs per window at each probed table row that the shift mask removes (zeros for an unshifted case)"""
    at = torch.stack([case.idx == r for r in rows])
    if case.mask is None:
        return torch.zeros(case.nW, len(rows), dtype=torch.long)
    return (at[None] & (case.mask < -1)[:, None]).flatten(2).sum(-1)


def assert_probe_bites(case, rows, sel, name=""):
    """the two conditions that keep a probe run from being vacuous: (1) every probe head selects (reference top probability >= 0.99) in every window
    whose mask leaves it a pair at its offset, and in at least one window of every image; (2) in a shifted case the mask removes a candidate pair of at
    least one probe offset"""
    top = sel[0]
    at = torch.stack([case.idx == r for r in rows])
    open_ = at[None] & ((case.mask > -1)[:, None] if case.mask is not None else torch.ones(case.nW, 1, case.N, case.N, dtype=torch.bool))
    has = open_.flatten(2).any(-1)                                              # [nW, heads]
    got = (top >= 0.99).any(-1).view(-1, case.nW, len(rows))
    assert bool((got == has[None]).all()), f"{name}: selecting rows do not match the windows that keep a pair at the probed offset"
    assert bool(has.any(0).all()), f"{name}: a probe head selects in no window"
    if case.mask is not None:
        assert int(masked_candidates(case, rows).sum()) > 0, f"{name}: the mask removes no candidate pair of any probe offset"


def selection(case, qkv, table, idx=None, mask=None):
    """(top probability, its key) of every query row, [Bw, heads, N] each, from the fp64 reference"""
    return reference(case, qkv, table, idx=idx, mask=mask, with_top=True)[1]


def selection_misses(case, y, qkv, heads, sel):
    """number of selecting rows (reference top probability >= 0.99) whose output row has a V row of its window and head strictly nearer (l2) than
    the selected key's.  Equal V rows tie (the padded tokens of a Swin block all carry the bias row) and are no miss."""
    top, key = sel
    v = _split(case, qkv, heads)[2]
    yh = y.detach().cpu().to(torch.float64).view(case.Bw, case.N, heads, HD).permute(0, 2, 1, 3)
    misses = 0
    for a, b in _chunks(case, heads):
        d = yh[a:b].square().sum(-1, keepdim=True) + v[a:b].square().sum(-1)[..., None, :] - 2 * yh[a:b] @ v[a:b].transpose(-1, -2)
        picked = d.gather(-1, key[a:b, ..., None])[..., 0]
        misses += int(((picked > d.min(-1).values + 1e-9 * d.abs().max()) & (top[a:b] >= 0.99)).sum())
    return misses, int((top >= 0.99).sum())


def probe_offsets(case, count):
    """table rows of the probed relative offsets: every corner of the offset box over the axes whose (clipped) window extent is > 1, the centre, the
    centre +-1 along each such axis, then seeded random reachable offsets up to `count`"""
    axes = [a for a in range(3) if case.win[a] > 1]
    strides = ((2 * case.window[1] - 1) * (2 * case.window[2] - 1), 2 * case.window[2] - 1, 1)

    def row(off):
        return sum((off[a] + case.window[a] - 1) * strides[a] for a in range(3))
    offs = []
    for signs in itertools.product((-1, 1), repeat=len(axes)):
        o = [0, 0, 0]
        for a, s in zip(axes, signs):
            o[a] = s * (case.win[a] - 1)
        offs.append(tuple(o))
    offs.append((0, 0, 0))
    for a in axes:
        for s in (-1, 1):
            offs.append(tuple(s if b == a else 0 for b in range(3)))
    rows = [row(o) for o in offs]
    reachable = torch.unique(case.idx).tolist()
    assert all(r in reachable for r in rows)
    rest = [r for r in reachable if r not in rows]
    perm = torch.randperm(len(rest), generator=torch.Generator("cpu").manual_seed(1234)).tolist()
    need = -(-len(rows) // count) * count - len(rows)
    return rows + [rest[i] for i in perm[:need]]


def probe_tables(case, heads):
    """tables [R, heads] of zeros with +30 at one offset per head; together they cover probe_offsets (more than one table when there are more offsets
    than heads).  Returns (tables, the offsets' table rows per table)."""
    rows = probe_offsets(case, heads)
    tables, per = [], []
    for a in range(0, len(rows), heads):
        t = torch.zeros(case.R, heads)
        t[rows[a:a + heads], torch.arange(heads)] = PROBE
        tables.append(t)
        per.append(rows[a:a + heads])
    return tables, per


def probe_qkv(case, heads, seed=1):
    """randn rows with the q and k thirds scaled by 0.25 (|score| well under 1: the table decides), on bf16-representable values"""
    x = torch.randn(case.Bw * case.N, 3, heads * HD, generator=torch.Generator("cpu").manual_seed(seed))
    x[:, :2] *= 0.25
    return x.view(case.Bw * case.N, 3 * heads * HD).to(torch.bfloat16).float()


def pair_counts(case):
    """[R]: (i, j) pairs of one window at every table row (the clipped index matrix's histogram)"""
    return torch.bincount(case.idx.reshape(-1), minlength=case.R)


def per_entry_error(got, ref, counts):
    """max-norm error of a table gradient [R, heads] after both sides are divided by sqrt(count[r]): an entry is the sum of count[r] pairs per window, so
    its size grows like sqrt(count) and a corner entry (one pair) is 1 / sqrt(N) of the centre entry -- 100 % wrong inside a gate relative to the largest
    entry.  Rows no pair reaches keep the divisor 1: the kernel must leave them zero."""
    w = counts.clamp(min=1).to(torch.float64).rsqrt()[:, None]
    got, ref = got.detach().cpu().to(torch.float64) * w, ref.detach().cpu().to(torch.float64) * w
    return float((got - ref).abs().max()) / float(ref.abs().max())


# ------------------------------------------------------------------------------------------------ gates (raise AssertionError)
def _assert_close(*a, **k):
    from test_gpu_ops import assert_close
    return assert_close(*a, **k)


def gate_forward(y, y_ref, dtype, name):
    _assert_close(y, y_ref, dtype, name + " forward", f32=FWD_F32, bf16=FWD_BF16, l2=FWD_L2 if dtype == torch.bfloat16 else None)


def gate_selection(case, y, qkv, heads, sel, name):
    """no tolerance: wherever the reference puts >= 0.99 of a row on one key, the kernel's output row is nearer to that key's V row than to any other"""
    wrong, rows = selection_misses(case, y, qkv, heads, sel)
    assert rows > 0 and wrong == 0, f"{name}: {wrong} of {rows} selecting rows land on another key"


def gate_backward(dqkv, dtable, ref, dtype, name):
    _assert_close(dqkv, ref[1], dtype, name + " dqkv", f32=BWD_F32, bf16=BWD_BF16, l2=BWD_L2 if dtype == torch.bfloat16 else None)
    _assert_close(dtable, ref[2], dtype, name + " dtable", f32=BWD_F32, bf16=BWD_BF16, l2=BWD_L2 if dtype == torch.bfloat16 else None)


def gate_per_entry(dtable, dtable_ref, counts, dtype, floor, k, name):
    """floor: per_entry_error of the bf16-rounded reference of the same case, k: the route's ENTRY_K (both ignored for fp32).  Returns (error, gate)."""
    err = per_entry_error(dtable, dtable_ref, counts)
    gate = ENTRY_F32 if dtype == torch.float32 else k * floor
    assert err <= gate, f"{name}: per-entry table-gradient error {err:.3e} > {gate:.3e}" + ("" if dtype == torch.float32 else f" = {k} x floor {floor:.3e}")
    return err, gate
