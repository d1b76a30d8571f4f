"""The J&F measure of the DAVIS 2017 evaluation (db_eval_iou, db_eval_boundary, _seg2bmap, no void pixels), written out with numpy and
scipy.ndimage.binary_dilation.  The yardstick of tests/test_jf_host.py and tests/test_gpu_jf.py: it imports nothing from lavt_hip.

A frame is a predicted mask P and a ground truth G, both H x W, nonzero = foreground.
  counts(P, G, r) -> [I, U, n_fg, n_gt, m_fg, m_gt]
  jf(row)         -> (J, F) of one frame
"""
import math

import numpy as np
from scipy.ndimage import binary_dilation


def bound_pix(H, W):
    return int(math.ceil(0.008 * math.sqrt(float(H) * float(H) + float(W) * float(W))))


def bmap(S):
    S = np.asarray(S) != 0
    H, W = S.shape
    e = np.zeros_like(S)
    s = np.zeros_like(S)
    se = np.zeros_like(S)
    e[:, :-1] = S[:, 1:]
    s[:-1, :] = S[1:, :]
    se[:-1, :-1] = S[1:, 1:]
    b = (S ^ e) | (S ^ s) | (S ^ se)
    b[-1, :] = S[-1, :] ^ e[-1, :]
    b[:, -1] = S[:, -1] ^ s[:, -1]
    b[-1, -1] = False
    return b


def disk(r):
    d = np.arange(-r, r + 1)
    return (d[:, None] * d[:, None] + d[None, :] * d[None, :]) <= r * r


def dilate(b, r):
    """b (H, W), or a stack (n, H, W) whose frames are dilated independently in one call (the structure is one frame thick: scipy's set-up of a
    large structure is paid once per stack)"""
    return binary_dilation(b, structure=disk(r) if b.ndim == 2 else disk(r)[None], border_value=0)


def counts(P, G, r):
    P, G = np.asarray(P) != 0, np.asarray(G) != 0
    bp, bg = bmap(P), bmap(G)
    return [int((P & G).sum()), int((P | G).sum()), int(bp.sum()), int(bg.sum()), int((bp & dilate(bg, r)).sum()), int((bg & dilate(bp, r)).sum())]


def counts_batch(P, G, r):
    """P, G: (n, H, W) -> int64 (n, 6)"""
    P, G = np.asarray(P) != 0, np.asarray(G) != 0
    if P.shape[0] == 0:
        return np.zeros((0, 6), dtype=np.int64)
    bp, bg = np.stack([bmap(p) for p in P]), np.stack([bmap(g) for g in G])
    n = P.shape[0]
    both = np.concatenate([bp, bg])          # each distinct boundary map is dilated once
    uniq, inv = np.unique(both.reshape(2 * n, -1), axis=0, return_inverse=True)
    d = dilate(uniq.reshape((-1,) + P.shape[1:]), r)[np.asarray(inv).reshape(-1)]
    dp, dg = d[:n], d[n:]
    cols = [(P & G), (P | G), bp, bg, bp & dg, bg & dp]
    return np.stack([c.reshape(c.shape[0], -1).sum(axis=1) for c in cols], axis=1).astype(np.int64)


def jf(row):
    I, U, n_fg, n_gt, m_fg, m_gt = (int(v) for v in row[:6])
    J = 1.0 if U == 0 else I / U
    if n_fg == 0 and n_gt > 0:
        p, r = 1.0, 0.0
    elif n_fg > 0 and n_gt == 0:
        p, r = 0.0, 1.0
    elif n_fg == 0 and n_gt == 0:
        p, r = 1.0, 1.0
    else:
        p, r = m_fg / n_fg, m_gt / n_gt
    F = 0.0 if p + r == 0 else ((2.0 * p) * r) / (p + r)
    return J, F


def dilate_brute(b, r):
    """the definition, pixel by pixel"""
    H, W = b.shape
    out = np.zeros_like(b)
    for y in range(H):
        for x in range(W):
            hit = False
            for dy in range(-r, r + 1):
                for dx in range(-r, r + 1):
                    yy, xx = y + dy, x + dx
                    if dy * dy + dx * dx <= r * r and 0 <= yy < H and 0 <= xx < W and b[yy, xx]:
                        hit = True
            out[y, x] = hit
    return out


def bmap_brute(S):
    S = np.asarray(S) != 0
    H, W = S.shape
    at = lambda y, x: bool(S[y, x]) if (y < H and x < W) else False          # noqa: E731
    b = np.zeros_like(S)
    for y in range(H):
        for x in range(W):
            v = bool(S[y, x])
            if y == H - 1 and x == W - 1:
                b[y, x] = False
            elif y == H - 1:
                b[y, x] = v ^ at(y, x + 1)
            elif x == W - 1:
                b[y, x] = v ^ at(y + 1, x)
            else:
                b[y, x] = (v ^ at(y, x + 1)) | (v ^ at(y + 1, x)) | (v ^ at(y + 1, x + 1))
    return b


def counts_brute(P, G, r):
    P, G = np.asarray(P) != 0, np.asarray(G) != 0
    bp, bg = bmap_brute(P), bmap_brute(G)
    return [int((P & G).sum()), int((P | G).sum()), int(bp.sum()), int(bg.sum()), int((bp & dilate_brute(bg, r)).sum()), int((bg & dilate_brute(bp, r)).sum())]
