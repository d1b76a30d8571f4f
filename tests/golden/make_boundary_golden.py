"""Generator of tests/golden/dice_boundary_<tag>.npz: what the reference's own `DiceBoundaryLoss` (losses.py:142-244) gives on the CPU, in fp32, for
small seeded inputs behind `F.interpolate(..., mode="bilinear", align_corners=True)` (lib/_utils.py:21), so that the tests of the fused criterion
need neither the reference nor its environment.

    python tests/golden/make_boundary_golden.py /path/to/the/reference/checkout

Per file: `dims` (B, h, w, H, W), `seed`, `scale` (logits = randn(seed) * scale, NHWC rows [B*h*w, 2]), `x` (those logits), `target` uint8 (B, H, W),
`rates` (dice_rate, boundary_rate), `loss`, `dice`, `boundary` (the two parts, unweighted) and `dy` = d loss / d x.  It also prints, per file, how far
the reference's fp32 gradient lies from its own fp64 gradient: the rounding spread the GPU gate (1e-4 of max |dy|) is derived from."""
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

#        tag      B   h   w    H    W  scale  target       (dice_rate, boundary_rate)
CASES = (("a", 3, 13, 11, 52, 44, 2.0, "random_last_bg", (1.0, 0.05)),          # last sample all background: S4 = 0, R = 0
         ("b", 2, 30, 30, 120, 120, 2.0, "random", (1.0, 0.05)),               # several tiles per side, interior halos
         ("same", 2, 9, 7, 9, 7, 2.0, "random", (1.0, 0.05)),                  # identity upsample, image smaller than a tile plus its halo
         ("sat", 2, 13, 11, 52, 44, 40.0, "random", (1.0, 0.05)),              # the softmax saturates: whole windows tie at a = 0
         ("blob", 2, 16, 16, 64, 64, 2.0, "blob", (1.0, 0.05)),                # a disc and an ellipse: flat interiors, real contours
         ("fg", 1, 8, 8, 32, 32, 2.0, "fg", (1.0, 0.05)),                      # all foreground: no boundary anywhere
         ("blob_bonly", 2, 16, 16, 64, 64, 2.0, "blob", (0.0, 1.0)))           # the boundary part alone carries the comparison


def make_target(kind, B, H, W, g):
    if kind == "fg":
        return torch.ones(B, H, W, dtype=torch.int64)
    if kind == "blob":
        yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
        disc = (yy - 0.45 * H) ** 2 + (xx - 0.55 * W) ** 2 <= (0.27 * min(H, W)) ** 2
        ell = ((yy - 0.6 * H) / (0.18 * H)) ** 2 + ((xx - 0.4 * W) / (0.33 * W)) ** 2 <= 1.0
        return torch.stack([disc, ell]).to(torch.int64)
    t = torch.randint(0, 2, (B, H, W), generator=g)
    if kind == "random_last_bg":
        t[B - 1] = 0
    return t


def run(ref, x, tgt, dims, rates, dtype):
    B, h, w, H, W = dims
    xr = x.to(dtype).clone().requires_grad_(True)
    up = F.interpolate(xr.view(B, h, w, 2).permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=True)
    loss = ref.DiceBoundaryLoss(boundary_rate=rates[1], dice_rate=rates[0])(up, tgt)
    loss.backward()
    with torch.no_grad():
        dice = ref.MultiClassDiceLoss()(up, tgt)
        bnd = ref.BoundaryLoss()(F.softmax(up, dim=1), ref.one_hot(tgt, num_classes=2, dtype=dtype))
    return float(loss.detach()), float(dice.detach()), float(bnd.detach()), xr.grad.detach()


def main():
    spec = importlib.util.spec_from_file_location("reference_losses", os.path.join(sys.argv[1], "losses.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    here = os.path.dirname(os.path.abspath(__file__))
    for i, (tag, B, h, w, H, W, scale, kind, rates) in enumerate(CASES):
        seed = 4100 + (4 if tag == "blob_bonly" else i)          # (blob_bonly: blob's inputs under other rates)
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(B * h * w, 2, generator=g) * scale
        tgt = make_target(kind, B, H, W, g)
        dims = (B, h, w, H, W)
        loss, dice, bnd, dy = run(ref, x, tgt, dims, rates, torch.float32)
        loss64, _, _, dy64 = run(ref, x, tgt, dims, rates, torch.float64)
        peak = float(dy64.abs().max())
        spread = float((dy.double() - dy64).abs().max()) / peak if peak > 0 else 0.0
        path = os.path.join(here, f"dice_boundary_{tag}.npz")
        np.savez_compressed(path, dims=np.array(dims), seed=np.array(seed), scale=np.array(scale, dtype=np.float32), x=x.numpy(),
                            target=tgt.numpy().astype(np.uint8), rates=np.array(rates, dtype=np.float32), loss=np.array(loss, dtype=np.float32),
                            dice=np.array(dice, dtype=np.float32), boundary=np.array(bnd, dtype=np.float32), dy=dy.numpy())
        print(f"{tag:10s} loss {loss:.7f} (fp64 {loss64:.7f}) dice {dice:.7f} boundary {bnd:.7f}  max|dy| {peak:.3e}  "
              f"fp32 vs fp64 gradient spread {spread:.2e} of max|dy|  {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
