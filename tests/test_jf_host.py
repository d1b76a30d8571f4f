"""Host checks of the J&F measure (DAVIS 2017 db_eval_iou / db_eval_boundary / _seg2bmap without void pixels): hand cases as literals against the
yardstick tests/jf_ref.py and against the library's restatement lavt_hip.metrics, the yardstick against a brute-force loop, the host meter's
grouping, the host form of the device block, and the C ABI's new symbols.  No GPU."""
import numpy as np
import pytest
import torch

import jf_ref
from lavt_hip import metrics as M


def _pix(shape, *at):
    m = np.zeros(shape, dtype=np.uint8)
    for y, x in at:
        m[y, x] = 1
    return m


def _square(x0):
    m = np.zeros((32, 32), dtype=np.uint8)
    m[8:20, x0:x0 + 12] = 1
    return m


S32 = (32, 32)
# (name, P, G, r, [I, U, n_fg, n_gt, m_fg, m_gt], J, F)
HAND = [
    ("same pixel", _pix(S32, (10, 10)), _pix(S32, (10, 10)), 2, [1, 1, 4, 4, 4, 4], 1.0, 1.0),
    ("2 apart", _pix(S32, (10, 10)), _pix(S32, (10, 12)), 2, [0, 2, 4, 4, 4, 4], 0.0, 1.0),
    ("3 apart", _pix(S32, (10, 10)), _pix(S32, (10, 13)), 2, [0, 2, 4, 4, 2, 2], 0.0, 0.5),
    ("4 apart", _pix(S32, (10, 10)), _pix(S32, (10, 14)), 2, [0, 2, 4, 4, 0, 0], 0.0, 0.0),
    ("(3,4) r5", _pix(S32, (10, 10)), _pix(S32, (13, 14)), 5, [0, 2, 4, 4, 4, 4], 0.0, 1.0),
    ("(4,4) r5", _pix(S32, (10, 10)), _pix(S32, (14, 14)), 5, [0, 2, 4, 4, 3, 3], 0.0, 0.75),
    ("corner 31,31", _pix(S32, (31, 31)), _pix(S32, (31, 31)), 1, [1, 1, 3, 3, 3, 3], 1.0, 1.0),
    ("corner 0,0", _pix(S32, (0, 0)), _pix(S32, (0, 0)), 1, [1, 1, 1, 1, 1, 1], 1.0, 1.0),
    ("last row", _pix(S32, (31, 5)), _pix(S32, (31, 5)), 1, [1, 1, 4, 4, 4, 4], 1.0, 1.0),
    ("last column", _pix(S32, (5, 31)), _pix(S32, (5, 31)), 1, [1, 1, 4, 4, 4, 4], 1.0, 1.0),
    ("all ones", np.ones((8, 9), np.uint8), np.ones((8, 9), np.uint8), 1, [72, 72, 0, 0, 0, 0], 1.0, 1.0),
    ("empty", np.zeros((8, 9), np.uint8), np.zeros((8, 9), np.uint8), 1, [0, 0, 0, 0, 0, 0], 1.0, 1.0),
    ("empty vs full", np.zeros((8, 9), np.uint8), np.ones((8, 9), np.uint8), 1, [0, 72, 0, 0, 0, 0], 0.0, 1.0),
    ("pixel vs empty", _pix((8, 9), (3, 3)), np.zeros((8, 9), np.uint8), 1, [0, 1, 4, 0, 0, 0], 0.0, 0.0),
    ("squares r1", _square(8), _square(11), 1, [108, 180, 48, 48, 24, 24], 0.6, 0.5),
    ("squares r2", _square(8), _square(11), 2, [108, 180, 48, 48, 28, 28], 0.6, 28.0 / 48.0),
    ("squares r3", _square(8), _square(11), 3, [108, 180, 48, 48, 48, 48], 0.6, 1.0),
]


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_hand_cases(case):
    _, P, G, r, row, J, F = case
    assert jf_ref.counts(P, G, r) == row
    got = M.boundary_counts_numpy(P, G, r)
    assert got.dtype == np.int32 and got.shape == (1, 8)
    assert got[0].tolist() == row + [0, 0]
    assert jf_ref.jf(row) == (J, F)
    j, f = M.jf_from_counts(np.array([row]))
    assert j.dtype == np.float64 and (float(j[0]), float(f[0])) == (J, F)
    j8, f8 = M.jf_from_counts(got)
    assert (float(j8[0]), float(f8[0])) == (J, F)


def test_one_sided_boundaries():
    """the precision / recall edge rules, on bare count rows"""
    assert jf_ref.jf([0, 5, 0, 7, 0, 0]) == (0.0, 0.0)          # precision 1, recall 0
    assert jf_ref.jf([0, 5, 7, 0, 0, 0]) == (0.0, 0.0)          # precision 0, recall 1
    assert jf_ref.jf([0, 0, 0, 0, 0, 0]) == (1.0, 1.0)
    rows = np.array([[0, 5, 0, 7, 0, 0], [0, 5, 7, 0, 0, 0], [0, 0, 0, 0, 0, 0], [3, 7, 10, 20, 5, 4]])
    j, f = M.jf_from_counts(rows)
    for k, row in enumerate(rows.tolist()):
        assert (float(j[k]), float(f[k])) == jf_ref.jf(row)
    p, r = 5 / 10, 4 / 20
    assert float(f[3]) == ((2.0 * p) * r) / (p + r) and float(j[3]) == 3 / 7


def test_davis_bound_pix():
    sizes = {(480, 854): 8, (720, 1280): 12, (384, 384): 5, (75, 100): 1, (300, 400): 4, (2160, 3840): 36}
    for (H, W), r in sizes.items():
        assert M.davis_bound_pix(H, W) == r == jf_ref.bound_pix(H, W)


def test_ref_against_brute_force_and_numpy():
    rng = np.random.default_rng(20171)
    for k in range(20):
        H, W, r = int(rng.integers(3, 41)), int(rng.integers(3, 41)), int(rng.integers(1, 7))
        d = (0.05, 0.3, 0.5, 0.95)[k % 4]
        P, G = rng.random((H, W)) < d, rng.random((H, W)) < d
        want = jf_ref.counts_brute(P, G, r)
        assert jf_ref.counts(P, G, r) == want, (H, W, r, d)
        assert M.boundary_counts_numpy(P, G, r)[0, :6].tolist() == want, (H, W, r, d)
    # batches, any nonzero value is foreground, radii up to the largest the library takes
    P, G = (rng.random((3, 50, 70)) < 0.1) * 255, (rng.random((3, 50, 70)) < 0.1).astype(np.int64) << 32
    for r in (12, M.BOUNDARY_MAX_RADIUS):
        batch = jf_ref.counts_batch(P, G, r)
        assert batch.tolist() == [jf_ref.counts(p, g, r) for p, g in zip(P, G)]          # the stacked dilation is the per-frame one
        assert np.array_equal(M.boundary_counts_numpy(P, G, r)[:, :6], batch)


def test_symbols_bound_under_abi_7():
    from lavt_hip import _capi as K
    assert K.lib.lavt_abi_version() == K.EXPECTED_ABI == 7
    for name in ("lavt_boundary_counts", "lavt_boundary_counts_ws", "lavt_jf_meter_bytes", "lavt_jf_meter_append"):
        assert name in K.EXPORTED and name in K._PROTOTYPES
        getattr(K.lib, name)
    assert M.BOUNDARY_MAX_RADIUS >= 40
    for cap in (1, 3, 4096):
        assert K.lib.lavt_jf_meter_bytes(cap) == M.jf_meter_bytes(cap) == 8 * 16 + 32 * cap
    assert K.lib.lavt_jf_meter_bytes(0) == 0 and K.lib.lavt_jf_meter_bytes(-3) == 0
    assert K.lib.lavt_boundary_counts_ws(36, 720, 1280) == 2 * 36 * 720 * 20
    assert K.lib.lavt_boundary_counts_ws(1, 1, 65) == 4 and K.lib.lavt_boundary_counts_ws(0, 5, 5) == 0
    # bad arguments are refused on the host, before anything touches a device
    assert K.lib.lavt_boundary_counts(None, None, None, 1, 4, 4, 1, None, 0, None, None) == -22
    assert K.lib.lavt_jf_meter_append(None, None, 4, 2, None, 3, None) == -22


def _rows(rng, n):
    rows = np.zeros((n, 8), dtype=np.int32)
    rows[:, 1] = rng.integers(0, 50, n)
    rows[:, 0] = (rows[:, 1] * rng.random(n)).astype(np.int32)
    rows[:, 2], rows[:, 3] = rng.integers(0, 30, n), rng.integers(0, 30, n)
    rows[:, 4], rows[:, 5] = (rows[:, 2] * rng.random(n)).astype(np.int32), (rows[:, 3] * rng.random(n)).astype(np.int32)
    rows[::7, 1] = 0
    rows[::7, 0] = 0
    rows[::5, 2] = 0
    rows[::5, 4] = 0
    return rows


def test_jfmeter_grouping():
    # unequal lengths: sequence "a" has one perfect frame, "b" three frames of J = F = 0
    good, bad = [4, 4, 4, 4, 4, 4, 0, 0], [0, 2, 4, 4, 0, 0, 0, 0]
    m = M.JFMeter()
    m.update(np.array([good]), "a")
    m.update(np.array([bad, bad, bad]), ["b", "b", "b"])
    s = m.summary()
    assert s == {"J": 50.0, "F": 50.0, "J&F": 50.0, "sequences": 2, "frames": 4}          # the frame mean would be 25
    # interleaved ids over two updates equal the grouped order
    rng = np.random.default_rng(3)
    rows = _rows(rng, 12)
    ids = [0, 1, 0, 2, 1, 0, 2, 2, 1, 0, 1, 2]
    a = M.JFMeter()
    a.update(rows[:5], ids[:5])
    a.update(torch.from_numpy(rows[5:]), np.array(ids[5:]))
    j, f = M.jf_from_counts(rows)
    want_j = want_f = 0.0
    for q in (0, 1, 2):
        js = fs = 0.0
        sel = [k for k, v in enumerate(ids) if v == q]
        for k in sel:
            js += float(j[k])
            fs += float(f[k])
        want_j += js / len(sel)
        want_f += fs / len(sel)
    s = a.summary()
    assert s["J"] == want_j / 3 * 100.0 and s["F"] == want_f / 3 * 100.0 and s["J&F"] == (s["J"] + s["F"]) / 2.0
    assert s["sequences"] == 3 and s["frames"] == 12
    with pytest.raises(ValueError):
        a.update(rows[:3], [0, 1])
    with pytest.raises(RuntimeError):
        M.JFMeter().summary()


def _block_by_hand(rows, T, capacity, live=None):
    """the block from jf_ref's arithmetic alone -> (header list, records list)"""
    h = [0.0] * 16
    h[0] = float(capacity)
    ring = [None] * capacity
    for q in range(len(rows) // T):
        js = fs = 0.0
        cnt = 0
        for k in range(q * T, q * T + T):
            if live is not None and not live[k]:
                continue
            J, F = jf_ref.jf(rows[k])
            js, fs, cnt = js + J, fs + F, cnt + 1
            h[6] += 1.0
            h[7] += J
            h[8] += F
        if cnt:
            seq = int(h[2])
            ring[seq % capacity] = (cnt, 0, js / cnt, fs / cnt, seq)
            h[2] += 1.0
            h[3] += 1.0
            h[4] += js / cnt
            h[5] += fs / cnt
    return h, ring


def test_reference_jf_block_ring_wrap_live_hold_and_state():
    rng = np.random.default_rng(11)
    rows = _rows(rng, 15)
    # ring wrap: capacity 3, 5 sequences of 3 frames
    snap = M.reference_jf_block(rows, 3, 3)
    h, ring = _block_by_hand(rows.tolist(), 3, 3)
    assert snap.header.tolist() == h and snap.n == 5 and snap.sequences == 5 and snap.frames == 15
    assert [tuple(r) for r in snap.ring.tolist()] == ring
    assert [int(r["sequence"]) for r in snap.records()] == [2, 3, 4]
    assert snap.ring.view(np.uint8).size == 3 * 32 and M.jf_meter_bytes(3) == 16 * 8 + 96
    # live: frames left out, and one sequence without a live frame stores nothing
    live = [1, 0, 1, 0, 0, 0, 1, 1, 1, 0, 0, 1, 1, 1, 0]
    snap_l = M.reference_jf_block(rows, 3, 8, live=live)
    h, ring = _block_by_hand(rows.tolist(), 3, 8, live=live)
    assert snap_l.header.tolist() == h and snap_l.sequences == 4 and snap_l.frames == 8
    assert [tuple(r) for r in snap_l.ring.tolist()[:4]] == ring[:4]
    # two appends equal one; hold stores nothing
    two = M.reference_jf_block(rows[9:], 3, 3, block=M.reference_jf_block(rows[:9], 3, 3))
    assert two.header.tobytes() == snap.header.tobytes() and two.ring.tobytes() == snap.ring.tobytes()
    held = M.reference_jf_block(rows[9:], 3, 3, block=M.reference_jf_block(rows[:9], 3, 3), hold=True)
    first = M.reference_jf_block(rows[:9], 3, 3)
    assert held.header.tobytes() == first.header.tobytes() and held.ring.tobytes() == first.ring.tobytes()
    # summary and the state-dict round trip
    s = snap.summary()
    assert s["J"] == h_mean(snap, 4) and s["F"] == h_mean(snap, 5) and s["J&F"] == (s["J"] + s["F"]) / 2.0 and s["sequences"] == 5 and s["frames"] == 15
    state = snap.state_dict()
    assert state["format"] == 1 and state["capacity"] == 3 and state["header"].dtype == torch.float64 and state["ring"].dtype == torch.uint8
    back = M.jf_snapshot_from_state(state)
    assert back.header.tobytes() == snap.header.tobytes() and back.ring.tobytes() == snap.ring.tobytes()
    with pytest.raises(ValueError):
        M.reference_jf_block(rows[:7], 3, 3)


def h_mean(snap, word):
    return float(snap.header[word]) / snap.sequences * 100.0
