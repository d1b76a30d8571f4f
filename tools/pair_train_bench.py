"""Pair-list train step against the plain step on the same pixels (DESIGN.md "Pair-list training").

    python tools/pair_train_bench.py [--slots 6] [--images 2] [--steps 20] [--warmup 10] [--reps 0] [--input-iters 50]

Swin-B w12 LAVT at 480^2, bf16, as bench.py builds it (captured step, no optimizer, DropPath 0.3).  A batch of N = --slots (image, expression) pairs
over B = --images distinct images, slot j on image j * B // N (every image named, multiplicities as equal as they come):

  plain   TrainStep at batch N on the gathered images x[image_of]: what a trainer runs today, N x patch embedding and stage 0
  pair    TrainStep(image_of=) on the B images: patch embedding and stage 0 once per image, lavt_gather_samples / lavt_gather_samples_bwd around them

Both live in ONE process, each with its own model copy (same weights) and its own ops.StepContext.  The timed region is bench.py's: `--steps` replays
between two device synchronisations, host clock.  The two variants ALTERNATE, region by region, and the regions are repeated as `bench.py --full`
repeats its own -- until 2 s have been timed per variant, at most 15 (or exactly --reps of them) -- so drift and other tenants' work hit both alike.
Reported: the median ms per step of each variant, every repetition, and the spread (max - min of the repetitions) that a difference has to exceed.

The backward gather alone: one step of an eager twin of the pair step under the in-process profiler gives the device time of the lavt_gather_samples_bwd launch and its
bandwidth (nsel + B) * sample bytes / time (every dy element read once, every dx element written once); the forward gather next to it.

The input stage for the same batch, the way tools/input_stage_time.py measures it: load_batch of B mixed-size sources + N masks against load_batch of
N sources + N masks, alternated, device-synchronised host clock, median over --input-iters calls; and the host-to-device bytes of each.

One JSON line on stdout."""
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
SIZES_HW = [(480, 640), (640, 480), (427, 640), (375, 500)]          # COCO-like sources, as tools/input_stage_time.py


def pair_list(n, b):
    return [j * b // n for j in range(n)]


def _region(step, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step.step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def _sources(seed, n_images, n_masks):
    rng = np.random.default_rng(seed)
    sizes = [SIZES_HW[i % len(SIZES_HW)] for i in range(max(n_images, n_masks))]
    return ([rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes[:n_images]], [rng.integers(0, 2, (h, w), dtype=np.uint8) for h, w in sizes[:n_masks]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=6, help="N: (image, expression) pairs per batch")
    ap.add_argument("--images", type=int, default=2, help="B: distinct images per batch")
    ap.add_argument("--steps", type=int, default=20, help="replays per timed region")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=0, help="timed regions per variant; 0 = until 2 s are timed per variant, at most 15")
    ap.add_argument("--input-iters", type=int, default=50)
    ap.add_argument("--drop-path", type=float, default=0.3)
    a = ap.parse_args()
    N, B = a.slots, a.images
    if not 1 <= B <= N:
        ap.error("1 <= --images <= --slots")
    if not torch.cuda.is_available():
        raise SystemExit("pair_train_bench: needs a GPU (there is no CPU path to time)")

    import bench
    import lavt_hip
    from lavt_hip import _capi as K
    from lavt_hip import ops
    from lavt_hip.detweights import det_inputs
    from lavt_hip.engine import TrainStep
    from lavt_hip.preprocess import pack_batch
    cfg = dict(bench.WORKLOADS["swin_b_w12_480_b2"], name="swin_b_w12_480_b2")
    lavt_hip.set_compute_dtype("bf16")
    pairs = pair_list(N, B)
    x = det_inputs(B, cfg["size"], 20, seed=1234)[0].to(DEV)
    _, l, m, tgt = det_inputs(N, cfg["size"], 20, seed=1235)
    l, m, tgt = l.to(DEV), m.to(DEV), tgt.to(DEV)
    image_of = torch.tensor(pairs, dtype=torch.int32, device=DEV)

    def build(**kw):
        torch.manual_seed(1234)
        model = bench.build_model(cfg, torch.device(DEV), a.drop_path).train()
        step = TrainStep(model, kw.pop("image"), l, m, tgt.clone(), context=ops.StepContext(), **kw)
        step.warmup_and_capture()
        return step
    plain = build(image=x[pairs].contiguous())
    pair = build(image=x, image_of=image_of)
    variants = (("plain", plain), ("pair", pair))
    for _, step in variants:
        for _ in range(a.warmup):
            step.step()
    times = {"plain": [], "pair": []}
    while True:
        for name, step in variants:
            times[name].append(_region(step, a.steps))
        done = len(times["pair"])
        if (a.reps and done >= a.reps) or (not a.reps and (done >= 15 or min(sum(times[n]) for n in times) * a.steps >= 2000.0)):
            break
    med = {n: statistics.median(ts) for n, ts in times.items()}
    spread = {n: max(ts) - min(ts) for n, ts in times.items()}
    gain = med["plain"] - med["pair"]

    # the two gather launches of one eager pair step, timed by the in-process profiler (device events around each C-ABI launch)
    eager = build(image=x, image_of=image_of, use_graph=False)          # (a third copy: the profiler brackets launches, and a replay issues none)
    K.prof.start()
    try:
        eager.step()
    finally:
        rec = K.prof.stop()
    del eager
    per = (cfg["size"] // 4) ** 2 * 128          # one image's stage-0 rows: 14 400 tokens x 128 channels
    kernels = {}
    for entry, moved in (("lavt_gather_samples", 2 * N), ("lavt_gather_samples_bwd", N + B)):
        us = [r[3] for r in rec if r[0] == entry]
        if len(us) != 1:
            raise SystemExit(f"pair_train_bench: expected one {entry} launch in a pair step, saw {len(us)}")
        nbytes = moved * per * 2
        kernels[entry] = dict(us=round(us[0], 2), bytes=nbytes, tb_per_s=round(nbytes / (us[0] * 1e-6) / 1e12, 3))

    # the input stage: B sources + N masks against N sources + N masks
    few, many = _sources(7, B, N), _sources(7, N, N)
    stage = {"pair": (pair, few), "plain": (plain, many)}
    for step, batch in stage.values():
        for _ in range(3):
            step.load_batch(*batch)
    in_times = {"pair": [], "plain": []}
    for _ in range(a.input_iters):
        for name, (step, batch) in stage.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step.load_batch(*batch)
            torch.cuda.synchronize()
            in_times[name].append((time.perf_counter() - t0) * 1e3)
    h2d = {name: int(pack_batch(*batch, out_size=(cfg["size"], cfg["size"]))[1].nbytes) for name, (_, batch) in stage.items()}

    print(json.dumps({
        "tool": "pair_train_bench", "workload": "swin_b_w12_480", "dtype": "bf16", "slots": N, "images": B, "image_of": pairs, "captured": [bool(plain.captured), bool(pair.captured)],
        "steps_per_region": a.steps, "regions": len(times["pair"]), "drop_path": a.drop_path,
        "plain_ms_per_step": round(med["plain"], 3), "pair_ms_per_step": round(med["pair"], 3), "gain_ms": round(gain, 3), "gain_frac_of_plain": round(gain / med["plain"], 4),
        "spread_ms": {n: round(v, 3) for n, v in spread.items()}, "gain_exceeds_spread": bool(gain > max(spread.values())),
        "ms_per_step_all_regions": {n: [round(t, 3) for t in ts] for n, ts in times.items()},
        "loss": {"plain": round(float(plain.loss), 5), "pair": round(float(pair.loss), 5)},
        "gather_kernels": kernels,
        "input_stage": {"iters": a.input_iters, "sources": {"pair": B, "plain": N}, "masks": N, "h2d_bytes": h2d,
                        "ms_median": {n: round(statistics.median(ts), 4) for n, ts in in_times.items()},
                        "ms_p10_p90": {n: [round(sorted(ts)[len(ts) // 10], 4), round(sorted(ts)[(len(ts) * 9) // 10], 4)] for n, ts in in_times.items()}},
    }), flush=True)


if __name__ == "__main__":
    main()
