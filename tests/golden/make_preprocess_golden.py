"""Generator of tests/golden/preprocess_cases.npz: what PIL (the library the reference's `F.resize` runs on a PIL image) gives for small seeded
inputs, so that the GPU tests of lavt_hip.preprocess need neither PIL nor the reference.

    python tests/golden/make_preprocess_golden.py

Per case `k`: `k_src` uint8 (N, Hs, Ws, 3) seeded random frames, `k_pil` uint8 (N, Ho, Wo, 3) = Image.resize((Wo, Ho), BILINEAR) of each,
`k_msrc` uint8 (N, Hs, Ws) with values 0 / 1 / 2 and `k_mpil` uint8 (N, Ho, Wo) = Image.resize((Wo, Ho), NEAREST).  `pillow` = the version used."""
import os

import numpy as np
import PIL
from PIL import Image

#        name  N  source H, W  output H, W
CASES = (("a", 1, (37, 53), (32, 32)),          # downscale on both axes, ksize 5 / 5
         ("b", 1, (17, 96), (32, 32)),          # upscale y, downscale x by 3, ksize 3 / 7
         ("c", 1, (32, 45), (32, 32)),          # identity axis
         ("d", 1, (90, 134), (20, 20)),         # ksize 11 / 15: many taps, clamped edges
         ("e", 1, (5, 7), (32, 32)),            # strong upscale: every row touches a border
         ("f", 1, (1, 1), (8, 8)),              # degenerate source
         ("g", 1, (50, 200), (33, 130)),        # more than one tile on both axes, ragged last tile in x (130 = 2 * 64 + 2) and y
         ("h", 3, (24, 40), (16, 16)))          # three frames (the test cuts them from a larger buffer), distinct content per frame


def main():
    out = {"pillow": np.array(PIL.__version__)}
    for i, (name, n, (hs, ws), (ho, wo)) in enumerate(CASES):
        rng = np.random.default_rng(20240 + i)
        src = rng.integers(0, 256, (n, hs, ws, 3), dtype=np.uint8)
        msrc = rng.integers(0, 3, (n, hs, ws), dtype=np.uint8)
        out[name + "_src"], out[name + "_msrc"] = src, msrc
        out[name + "_pil"] = np.stack([np.asarray(Image.fromarray(f, "RGB").resize((wo, ho), Image.BILINEAR)) for f in src])
        out[name + "_mpil"] = np.stack([np.asarray(Image.fromarray(m, "L").resize((wo, ho), Image.NEAREST)) for m in msrc])
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "preprocess_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
