"""Test helper (not a test): the Dice+Boundary criterion of the reference (losses.py:142-244 behind the align_corners upsample of lib/_utils.py:21)
restated with plain torch ops, pinned against the fixtures tests/golden/dice_boundary_<tag>.npz by test_dice_boundary_host.py -- the GPU tests use it
for inputs that have no fixture (bf16-rounded logits, selected frames, full-resolution logits, model outputs)."""
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TAGS = ("a", "b", "same", "sat", "blob", "fg", "blob_bonly")


def load(tag):
    """-> dict: x fp32 [B*h*w, 2], target int64 (B, H, W), dims (B, h, w, H, W), rates (dice_rate, boundary_rate), loss, dice, boundary, dy"""
    z = np.load(os.path.join(GOLDEN, f"dice_boundary_{tag}.npz"), allow_pickle=False)
    return {"x": torch.from_numpy(z["x"]), "target": torch.from_numpy(z["target"].astype(np.int64)), "dims": tuple(int(v) for v in z["dims"]),
            "rates": tuple(float(v) for v in z["rates"]), "loss": float(z["loss"]), "dice": float(z["dice"]), "boundary": float(z["boundary"]),
            "dy": torch.from_numpy(z["dy"]), "seed": int(z["seed"]), "scale": float(z["scale"])}


def _edge(m):
    """what a 3x3 dilation adds to m (stride 1, windows clipped at the border)"""
    return F.max_pool2d(m, 3, 1, 1) - m


def criterion(logits, target, dice_rate=1.0, boundary_rate=0.05):
    """logits (n, 2, H, W), target int64 (n, H, W) in {0, 1} -> (loss, dice part, boundary part)"""
    p = torch.softmax(logits, dim=1)
    g = torch.stack([target == 0, target == 1], dim=1).to(p.dtype)
    hw = (2, 3)
    score = 2.0 * (p * g).sum(hw) / ((p * p + g).sum(hw) + 1e-6)
    dice = (1.0 - score).mean(0).sum() / 2
    pred_b, gt_b = _edge(1 - p), _edge(1 - g)
    pred_ext, gt_ext = F.max_pool2d(pred_b, 5, 1, 2), F.max_pool2d(gt_b, 5, 1, 2)
    prec = (pred_b * gt_ext).sum(hw) / (pred_b.sum(hw) + 1e-7)
    rec = (pred_ext * gt_b).sum(hw) / (gt_b.sum(hw) + 1e-7)
    boundary = (1 - 2 * prec * rec / (prec + rec + 1e-7)).mean()
    return dice * dice_rate + boundary * boundary_rate, dice, boundary


def lowres(x, target, dims, dice_rate=1.0, boundary_rate=0.05, sel=None):
    """x [B*h*w, 2] low-resolution NHWC rows -> (loss, dice, boundary, d loss / d x) in x's precision on the CPU; sel: index_select in front of the criterion"""
    B, h, w, H, W = dims
    xr = x.detach().clone().requires_grad_(True)
    up = F.interpolate(xr.view(B, h, w, 2).permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=True)
    if sel is not None:
        up = torch.index_select(up, 0, torch.as_tensor(sel, dtype=torch.int64))
    loss, dice, bnd = criterion(up, target, dice_rate, boundary_rate)
    loss.backward()
    return float(loss.detach()), float(dice.detach()), float(bnd.detach()), xr.grad.detach()
