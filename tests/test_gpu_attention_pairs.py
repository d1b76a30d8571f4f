"""Pairwise-sensitive GPU parity of window attention on every route (csrc/attention_mfma.hip, attention.hip, attention_stream.hip, wmsa_fused.hip,
dtable_body.h) against the fp64 statement of tests/attn_pairs.py: the selecting probe for the bias gather, the shift mask and the padding columns, the
per-entry gate for the table-gradient binning, and the launch geometries of the MFMA backward that no other op-level test reaches.  That each gate fails
on a subtly wrong kernel is shown on the CPU by test_attention_gates_host.py."""
import functools

import pytest
import torch

import attn_pairs as AP
from test_gpu_ops import dev, rnd

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
FUSED, COMPOSED, STREAM = "_WindowAttnBackward", "_WindowAttnComposedBackward", "_WindowAttnStreamBackward"
W7, W12, V7, V12 = (1, 7, 7), (1, 12, 12), (8, 7, 7), (8, 12, 12)

# id: (dims, window, shifted, batch, dtype, route, how)   how: None = ops.window_attention as routed; "env" = LAVT_ATTN_COMPOSED=1; "direct" =
# ops._WindowAttnComposed itself (window_attention sends every N <= 160 to the fused kernels, the composed route's Np = 152 padding is reached this way)
SHAPES = {
    "mfma4-s0": ((1, 14, 14), W7, 0, 2, BF, FUSED, None),                  # N = 49: 4 key tiles, 15 padded keys
    "mfma4-s3": ((1, 14, 14), W7, 1, 2, BF, FUSED, None),
    "mfma9-s6": ((1, 24, 24), W12, 1, 2, BF, FUSED, None),                 # N = 144: 9 tiles, none padded
    "mfma10-clipped": ((3, 14, 14), V7, 1, 2, BF, FUSED, None),            # N = 147 of a clipped (3, 7, 7) window: 10 tiles, 13 padded keys
    "mfma25": ((8, 14, 7), V7, 1, 2, BF, FUSED, None),                     # N = 392: 25 tiles, 8 padded keys
    "fp32-w7-s0": ((1, 14, 14), W7, 0, 2, F32, FUSED, None),
    "fp32-w7-s3": ((1, 14, 14), W7, 1, 2, F32, FUSED, None),
    "fp32-w12-s6": ((1, 24, 24), W12, 1, 2, F32, FUSED, None),
    "composed147-bf16": ((3, 14, 14), V7, 1, 2, BF, COMPOSED, "direct"),   # Np = 152
    "composed147-fp32": ((3, 14, 14), V7, 1, 2, F32, COMPOSED, "direct"),
    "composed392-bf16": ((8, 14, 7), V7, 1, 2, BF, COMPOSED, "env"),
    "composed392-fp32": ((8, 14, 7), V7, 1, 2, F32, COMPOSED, None),
    "stream-s0": ((8, 12, 12), V12, 0, 1, BF, STREAM, None),
    "stream-shifted": ((8, 24, 24), V12, 1, 1, BF, STREAM, None),
}
# MFMA backward launch geometries (bf16; lavt_window_attn_bwd_mfma, dtable_geometry): id: (dims, window, shifted, batch, heads)
GEOMETRY = {
    "units288": ((1, 42, 56), W7, 0, 2, 3),          # 96 x 3: 32 extra units cut into 8 pieces of one task; units >= 256 on the rotated slot; 3 binning groups of 32
    "units384": ((1, 56, 56), W7, 0, 2, 3),          # 128 x 3: 128 extra units cut into 2 pieces
    "units385": ((1, 49, 77), W7, 0, 1, 5),          # 77 x 5: 129 extra units, not split: a second round; binning groups 26 / 26 / 25
    "groups17+16": ((1, 21, 77), W7, 0, 1, 2),       # 33 windows: binning groups 17 + 16
    "w12-units288": ((1, 72, 72), W12, 1, 2, 4),     # 72 x 4, shifted: 8 waves, 18 tasks over 8 pieces (uneven cuts)
    "two-windows": ((1, 35, 287), W7, 0, 5, 2),      # 1025 x 2 = 2050 units: win_per_block = 2, the last chunk holds one window
    "video-units288": ((8, 56, 63), V7, 0, 2, 2),    # 144 x 2: the 25-tile kernel with split units
}
PROBE_HEADS, DIFFUSE_HEADS = 16, 4


@functools.lru_cache(maxsize=None)
def _case(dims, window, shifted, batch):
    return AP.make_case(dims, window, bool(shifted), batch)


def _region(cs):
    from lavt_hip import rowmaps
    if not any(cs.shift):
        return None
    ids = rowmaps.region_ids_np(cs.dims[1], cs.dims[2], cs.window[1], cs.shift[1]) if cs.two_d else rowmaps.region_ids3d_np(*cs.dims, cs.win, cs.shift)
    return torch.from_numpy(ids).to(dev())


def _attend(cs, qkv, table, dtype, route, how, monkeypatch, go=None):
    """one forward (and backward) of the op on the GPU from CPU fp32 tensors; asserts the route taken"""
    from lavt_hip import ops
    ops.weights.invalidate()
    monkeypatch.delenv("LAVT_ATTN_COMPOSED", raising=False)
    if how == "env":
        monkeypatch.setenv("LAVT_ATTN_COMPOSED", "1")
    heads = table.shape[1]
    q = qkv.to(dev()).to(dtype).requires_grad_(True)
    t = table.to(dev()).requires_grad_(True)
    win = cs.window[1] if cs.two_d else cs.window
    if how == "direct":
        y = ops._WindowAttnComposed.apply(q, t, _region(cs), ops._win3(win), heads, cs.N)
    else:
        y = ops.window_attention(q, t, _region(cs), win, heads, N=cs.N)
    assert type(y.grad_fn).__name__ == route, (type(y.grad_fn).__name__, route)
    if go is None:
        torch.cuda.synchronize()
        return y.detach()
    y.backward(go.to(dev()).to(dtype))
    torch.cuda.synchronize()
    return y.detach(), q.grad, t.grad


@functools.lru_cache(maxsize=None)
def _probe(key):
    """probe inputs and their fp64 references, shared by the routes and dtypes that run the same shape"""
    cs = _case(*key)
    qkv = AP.probe_qkv(cs, PROBE_HEADS)
    tables, rows = AP.probe_tables(cs, PROBE_HEADS)
    runs = []
    for table, r in zip(tables, rows):
        y_ref, sel = AP.reference(cs, qkv, table, with_top=True)
        AP.assert_probe_bites(cs, r, sel, str(key))
        runs.append((table, sel, y_ref))
    pad = AP.padding_table(cs, PROBE_HEADS)
    return qkv, runs, pad, AP.reference(cs, qkv, pad)


@functools.lru_cache(maxsize=None)
def _diffuse(key, heads):
    """diffuse inputs on bf16-representable values, the fp64 reference (with the dense bias gradient) and the bf16 rounding floor of the per-entry metric"""
    cs = _case(*key)
    qkv = rnd(cs.Bw * cs.N, 3 * heads * 32, seed=1).to(BF).float()
    table = rnd(cs.R, heads, seed=2, scale=0.5).to(BF).float()
    go = rnd(cs.Bw * cs.N, heads * 32, seed=99).to(BF).float()
    ref = AP.reference(cs, qkv, table, go, with_dbias=True)
    counts = AP.pair_counts(cs)
    floor = AP.per_entry_error(AP.reference(cs, qkv, table, go, round_bf16=True)[2], ref[2], counts)
    # the smallest per-entry error of the binning faults of the self-test on THIS case: the corner offsets / the one corner pair binned next door
    faults = min(AP.per_entry_error(AP.rebin(cs, ref[3], idx), ref[2], counts) for idx in (AP.idx_corners_to_neighbour(cs), AP.idx_one_pair_shifted(cs)))
    return qkv, table, go, ref, counts, floor, faults


@pytest.mark.parametrize("name", list(SHAPES))
def test_probe_forward(name, monkeypatch):
    """Selecting probe: q and k small, the table zero but +30 at one relative offset per head (corners of the offset box, centre, centre +-1 per axis,
    seeded others).  A query row then IS the V row of the key at that offset, if its window and region hold one: a wrong table index, mask bit or
    padding column on that pair moves the row by ~1 x max|ref|.  Gates: the forward gates of test_stream_parity; every selecting row nearest to its
    selected key's V row (no tolerance); and the padding probe (table -30 everywhere: only a key column whose bias is not the table's can win)."""
    dims, window, shifted, batch, dtype, route, how = SHAPES[name]
    key = (dims, window, shifted, batch)
    cs = _case(*key)
    qkv, runs, pad, y_pad = _probe(key)
    for n, (table, sel, y_ref) in enumerate(runs):
        y = _attend(cs, qkv, table, dtype, route, how, monkeypatch)
        AP.gate_forward(y, y_ref, dtype, f"{name} probe table {n}")
        AP.gate_selection(cs, y, qkv, PROBE_HEADS, sel, f"{name} probe table {n}")
    AP.gate_forward(_attend(cs, qkv, pad, dtype, route, how, monkeypatch), y_pad, dtype, f"{name} padding probe")


def _backward_case(name, key, heads, dtype, route, how, monkeypatch):
    cs = _case(*key)
    qkv, table, go, ref, counts, floor, faults = _diffuse(key, heads)
    y, dqkv, dtable = _attend(cs, qkv, table, dtype, route, how, monkeypatch, go=go)
    err = AP.per_entry_error(dtable, ref[2], counts)
    print(f"\n[{name}] per-entry dtable error E = {err:.3e}, bf16 floor F = {floor:.3e}, E/F = {err / floor:.2f}, smallest binning fault {faults:.3e}")
    AP.gate_forward(y, ref[0], dtype, name)
    AP.gate_backward(dqkv, dtable, ref, dtype, name)
    _, gate = AP.gate_per_entry(dtable, ref[2], counts, dtype, floor, AP.ENTRY_K[route], name)
    assert gate <= faults / 3, f"{name}: per-entry gate {gate:.3e} above a third of the smallest binning fault {faults:.3e}"


@pytest.mark.parametrize("name", [n for n in SHAPES if n != "stream-shifted"])
def test_backward_per_entry(name, monkeypatch):
    """Diffuse inputs (randn qkv, table std 0.5: the gradient of a saturated softmax vanishes), fp64 reference.  Gates: forward and dqkv / dtable at the
    gates of test_stream_parity, and the per-entry table-gradient error E (attn_pairs.per_entry_error) <= k x F, F = the same metric of the reference
    with P, the stored output and dS rounded to bf16 (fp32 routes: 1e-3).  k x F must stay under a third of the smallest per-entry error of the
    binning faults (corner offsets, or the one corner pair, binned next door) on the same case.

    E / F measured on MI355X (E, F in units of 1e-3; the fp32 routes measure E = 1.4e-7 .. 4.5e-7):
      MFMA bf16      mfma4-s0 1.72 / 1.82 = 0.94   mfma4-s3 1.13 / 1.52 = 0.75   mfma9-s6 1.32 / 1.55 = 0.85   mfma10-clipped 1.67 / 2.59 = 0.64
                     mfma25 2.52 / 2.97 = 0.85   units288 2.45 / 2.68 = 0.92   units384 2.23 / 2.74 = 0.82   units385 2.38 / 2.15 = 1.11
                     groups17+16 3.07 / 2.02 = 1.52   w12-units288 2.51 / 2.65 = 0.95   two-windows 1.61 / 4.09 = 0.39   video-units288 1.61 / 3.68 = 0.44
      composed bf16  composed147 3.05 / 2.59 = 1.18   composed392 7.92 / 2.97 = 2.66 (S is stored in bf16 before the softmax: one more rounding than F models)
      stream bf16    stream-s0 0.32 / 3.35 = 0.10 (dS reaches the bias gradient without a bf16 slab)
    k = twice the worst ratio of the route: 3.04 (MFMA), 5.32 (composed); the streaming route gets 1.0, the floor itself, not 0.2.  One k for all
    routes (5.32) would put the streaming case's gate at 1.78e-2, above a third of its smallest binning fault (4.5e-2 / 3); per route every case
    keeps the condition, the tightest being mfma10-clipped (7.9e-3 against 1.78e-2) and composed147 (1.38e-2 against 1.78e-2)."""
    dims, window, shifted, batch, dtype, route, how = SHAPES[name]
    _backward_case(name, (dims, window, shifted, batch), DIFFUSE_HEADS, dtype, route, how, monkeypatch)


@pytest.mark.parametrize("name", list(GEOMETRY))
def test_backward_launch_geometry(name, monkeypatch):
    """the MFMA backward's unit splitting, rotated slot, two windows per workgroup and multiple binning groups, at the gates of test_backward_per_entry"""
    dims, window, shifted, batch, heads = GEOMETRY[name]
    _backward_case(name, (dims, window, shifted, batch), heads, BF, FUSED, None, monkeypatch)


def _block_qkv(sd, x, H, W, ws, shifted):
    """fp64 qkv rows in window order of a Swin block (norm1 -> pad -> shift -> partition -> qkv; lib/backbone.py:201-217), as oracle.lavt_oracle.swin_block"""
    import torch.nn.functional as F
    B, _, C = x.shape
    s = ws // 2 if shifted else 0
    u = F.layer_norm(x.double(), (C,), sd["norm1.weight"].double(), sd["norm1.bias"].double(), 1e-5).view(B, H, W, C)
    Hp, Wp = -(-H // ws) * ws, -(-W // ws) * ws
    u = torch.roll(F.pad(u, (0, 0, 0, Wp - W, 0, Hp - H)), (-s, -s), (1, 2))
    win = u.view(B, Hp // ws, ws, Wp // ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, C)
    return F.linear(win, sd["attn.qkv.weight"].double(), sd["attn.qkv.bias"].double())


@pytest.mark.parametrize("C,ws,H,W", [(128, 12, 15, 15), (64, 7, 10, 9)])
def test_probe_wmsa_block(C, ws, H, W, monkeypatch):
    """The probe through a shifted Swin block with padded windows, on the one-kernel W-MSA forward (csrc/wmsa_fused.hip: its own gather and mask, after
    padding and shifting through the row map) and on the unfused sequence: the q and k rows of the qkv projection are zero, so the scores ARE bias + mask.
    Gates: the block output within 3 % relative l2 of oracle.lavt_oracle.swin_block (fp32, same bf16-rounded input).  A corner-offset fault moves that
    figure by 0.3 % (ws 12) to 1.2 % (ws 7) -- one row of a window per head, behind the residual -- so the attention core's output, captured in
    window order, also goes through the forward and selection gates of test_probe_forward against the fp64 core on the block's fp64 qkv rows."""
    import lavt_hip
    from lavt_hip import ops
    from lavt_hip.detweights import fill_state_dict_
    from lib.backbone import SwinTransformerBlock
    from oracle import lavt_oracle as O
    B, nH = 2, C // 32
    blk = SwinTransformerBlock(C, nH, ws, shift_size=ws // 2).eval()
    fill_state_dict_(blk)
    with torch.no_grad():
        blk.attn.qkv.weight[:2 * C] = 0
        blk.attn.qkv.bias[:2 * C] = 0
    blk.to(dev())
    blk.H, blk.W = H, W
    x0 = rnd(B, H * W, C, seed=21).to(BF).float()
    cs = _case((1, -(-H // ws) * ws, -(-W // ws) * ws), (1, ws, ws), 1, B)
    tables, rows = AP.probe_tables(cs, nH)
    assert len(tables) * nH >= 9
    core = []
    plain_fused, plain_attn = ops.wmsa_fused, ops.window_attention

    def fused(*a, **k):
        out = plain_fused(*a, **k)
        core.append(out[0].detach())
        return out

    def attn(*a, **k):
        out = plain_attn(*a, **k)
        core.append(out.detach())
        return out
    monkeypatch.setattr(ops, "wmsa_fused", fused)
    monkeypatch.setattr(ops, "window_attention", attn)
    lavt_hip.set_compute_dtype(BF)
    try:
        for n, (table, r) in enumerate(zip(tables + [AP.padding_table(cs, nH)], rows + [None])):
            with torch.no_grad():
                blk.attn.relative_position_bias_table.copy_(table)
            sd = {k: v.detach().float().cpu() for k, v in blk.state_dict().items()}
            y_ref = O.swin_block({"blk." + k: v for k, v in sd.items()}, "blk", x0, H, W, nH, ws, shifted=True)
            qkv_ref = _block_qkv(sd, x0, H, W, ws, True)
            o_ref, sel = AP.reference(cs, qkv_ref, table, with_top=True)
            if r is not None:
                AP.assert_probe_bites(cs, r, sel, f"wmsa table {n}")
            for on in ("1", "0"):
                monkeypatch.setenv("LAVT_WMSA_FUSED", on)
                ops.weights.invalidate()
                x = x0.to(dev()).to(BF)
                assert ops.wmsa_fused_ok(x.reshape(B * H * W, C), ws, nH, True) == (on == "1")
                core.clear()
                with torch.no_grad():
                    y = blk(x)
                torch.cuda.synchronize()
                name = f"wmsa C={C} ws={ws} fused={on} table {n}"
                rel = float((y.float().cpu() - y_ref).norm()) / float(y_ref.norm())
                assert rel <= 3e-2, f"{name}: block output relative l2 {rel:.3e}"
                assert len(core) == 1 and core[0].shape == o_ref.shape, name
                AP.gate_forward(core[0], o_ref, BF, name + " core")
                if r is not None:
                    AP.gate_selection(cs, core[0], qkv_ref, nH, sel, name + " core")
    finally:
        lavt_hip.set_compute_dtype(F32)
