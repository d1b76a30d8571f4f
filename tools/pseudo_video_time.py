"""Timing of the pseudo-video augmentation in the batched input stage (lavt_hip.preprocess.BatchPreprocessor with warps=; PseudoVideoAugment).

    python tools/pseudo_video_time.py [--iters 200] [--warmup 20] [--out profiles/pseudo_video_time.txt]

B = 2 still images of 480 x 640 with masks -> clips of T = 8 frames at 480^2, into static clip buffers.  Variants, ALTERNATED inside one loop
(iteration k runs every variant once, so drift hits all alike), `--iters` timed calls per variant after `--warmup`:

  repeat     stage(repeat=8), then commit: `--pseudo_video_aug vanilla`, the input stage as it was before the augmentation existed
  repeat_2   the same variant a second time in the same loop: the spread of the measurement
  augment    stage(repeat=8, warps=, target_warps=) with a fresh draw of PseudoVideoAugment() at its defaults, then commit

Timed: commit() alone, between two device events, after a synchronise behind stage() (the upload has landed; what is measured is the kernels the
consuming stream runs in front of a replay), and stage() alone on the host clock with a synchronise behind it (pack + upload).  For each variant:
median / p10 / p90 ms, the bytes uploaded per batch, and the C-ABI launches of one commit with their device time (in-process profiler, one
separate call).

One JSON line per figure on stdout; --out appends them to a text file."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "lavt-rs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = "cuda:0"
B, T, SRC, OUT = 2, 8, (480, 640), (480, 480)


def _stats(ts):
    ts = sorted(ts)
    return dict(ms_median=round(statistics.median(ts), 4), ms_p10=round(ts[len(ts) // 10], 4), ms_p90=round(ts[(len(ts) * 9) // 10], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pseudo_video_time: needs a GPU (a timing on the CPU says nothing)")
    from lavt_hip import _capi as K
    from lavt_hip import preprocess as P

    rng = np.random.default_rng(1)
    images = [rng.integers(0, 256, SRC + (3,), dtype=np.uint8) for _ in range(B)]
    masks = [rng.integers(0, 2, SRC, dtype=np.uint8) for _ in range(B)]
    x = torch.zeros(B, T, 3, *OUT, device=DEV)
    t = torch.zeros(B * T, *OUT, dtype=torch.int64, device=DEV)
    pp, aug = P.BatchPreprocessor(OUT), P.PseudoVideoAugment(seed=0)

    def stage_repeat():
        return pp.stage(images, masks, repeat=T)

    def stage_augment():
        warps = [w for clip in aug.draw([SRC] * B, T) for w in clip]
        return pp.stage(images, masks, repeat=T, warps=warps, target_warps=warps)

    variants = [("repeat", stage_repeat), ("repeat_2", stage_repeat), ("augment", stage_augment)]
    commit_ms, stage_ms, nbytes = {n: [] for n, _ in variants}, {n: [] for n, _ in variants}, {}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for it in range(a.warmup + a.iters):
        for name, stage in variants:
            torch.cuda.synchronize()
            h0 = time.perf_counter()
            nbytes[name] = stage().nbytes
            torch.cuda.synchronize()
            h1 = time.perf_counter()
            e0.record()
            pp.commit(x, t)
            e1.record()
            torch.cuda.synchronize()
            if it >= a.warmup:
                commit_ms[name].append(e0.elapsed_time(e1))
                stage_ms[name].append((h1 - h0) * 1e3)

    lines = []
    for name, stage in variants:
        stage()
        torch.cuda.synchronize()
        K.prof.start()
        try:
            pp.commit(x, t)
        finally:
            rec = K.prof.stop()
        lines.append(dict(part="pseudo_video_commit", variant=name, clips=B, frames=T, source=list(SRC), out=list(OUT), iters=a.iters, h2d_bytes=nbytes[name],
                          launches={r[0]: round(r[3], 1) for r in rec}, kernel_us=round(sum(r[3] for r in rec), 1), **_stats(commit_ms[name])))
        lines.append(dict(part="pseudo_video_stage_host", variant=name, iters=a.iters, **_stats(stage_ms[name])))
    for line in lines:
        print(json.dumps(line))
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
