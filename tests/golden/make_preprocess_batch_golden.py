"""Generator of tests/golden/preprocess_batch_cases.npz: batches whose sources all have their own size, and what PIL gives for each of them, so that
the tests of the batched input stage (lavt_hip.preprocess.pack_batch / BatchPreprocessor) need neither PIL nor the reference.

    python tests/golden/make_preprocess_batch_golden.py

Per batch `b` with sources i = 0 ..: `b_out` = (Ho, Wo); `b{i}_src` uint8 (Hs, Ws, 3) seeded random, `b{i}_pil` uint8 (Ho, Wo, 3) =
Image.resize((Wo, Ho), BILINEAR); `b{i}_msrc` uint8 (Hs, Ws) with values 0 / 1 / 2, `b{i}_mpil` uint8 (Ho, Wo) = Image.resize((Wo, Ho), NEAREST).
`b_count` = the number of sources, `pillow` = the version used."""
import os

import numpy as np
import PIL
from PIL import Image

#          name  source (H, W) ...                                      output (H, W)
BATCHES = (("m", ((50, 200), (71, 64), (33, 130), (9, 300)), (33, 130)),          # ksize_x 5/3/3/7 and ksize_y 5/7/3/3 in one launch; three x tiles, the last of 2 pixels; ragged last y tile; one identity item
           ("n", ((48, 64), (64, 48), (43, 64), (30, 30), (1, 5)), (32, 32)),     # five items, up- and downscale mixed, a one-row source
           ("v", ((24, 40), (40, 24)), (16, 16)))                                 # clip layout: the tests repeat every source into 3 frames


def main():
    out = {"pillow": np.array(PIL.__version__)}
    for bi, (name, sizes, (ho, wo)) in enumerate(BATCHES):
        out[f"{name}_out"], out[f"{name}_count"] = np.array([ho, wo]), np.array(len(sizes))
        for i, (hs, ws) in enumerate(sizes):
            rng = np.random.default_rng(30500 + 16 * bi + i)
            src = rng.integers(0, 256, (hs, ws, 3), dtype=np.uint8)
            msrc = rng.integers(0, 3, (hs, ws), dtype=np.uint8)
            out[f"{name}{i}_src"], out[f"{name}{i}_msrc"] = src, msrc
            out[f"{name}{i}_pil"] = np.asarray(Image.fromarray(src, "RGB").resize((wo, ho), Image.BILINEAR))
            out[f"{name}{i}_mpil"] = np.asarray(Image.fromarray(msrc, "L").resize((wo, ho), Image.NEAREST))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "preprocess_batch_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
