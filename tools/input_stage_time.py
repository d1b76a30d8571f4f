"""Timing of the batched input stage (lavt_hip.preprocess.BatchPreprocessor, TrainStep.load_batch / stage_batch / commit_batch).

    python tools/input_stage_time.py [--iters 200] [--warmup 20] [--no-train] [--out profiles/input_stage_time.txt]

Part 1, the input stage alone.  A batch of 8 COCO-like sources (640x480, 480x640, 640x427, 500x375 as W x H, each twice) with masks -> 480^2, into
static output buffers.  Variants, ALTERNATED inside one loop (iteration k runs every variant once, so drift hits all alike), each call bracketed by
a device synchronise on both sides (host wall clock), `--iters` (>= 200) timed calls per variant after `--warmup`:

  per_image    the per-image loop over FramePreprocessor.images / .targets with pinned staging: the only device route for mixed sizes without the
               batched stage (one pixel upload, one mask upload and two launches per image)
  per_image_2  the same variant a second time in the same loop: the spread of the measurement
  batch        BatchPreprocessor.batch: one pack, one upload, two launches
  host_pil     transforms.get_transform per image on the host + one fp32 image upload and one int64 target upload, for scale

For each: median / p10 / p90 ms per batch, C-ABI launches per batch and their summed device time (in-process profiler, one separate call) and
host-to-device bytes per batch.

Part 2, the train iteration on `swin_b_w12_480_b2` as bench.py builds and runs it (bf16, captured step, no optimizer), B = 2 mixed-size sources per
iteration, variants alternated in blocks of `--block` iterations, ms per iteration = block time / block length, median over the blocks:

  static          step() on static inputs: what bench.py times
  static_2        the same a second time: the spread
  load_batch      load_batch(images, masks) then step(), every iteration
  stage_commit    commit_batch(); step(); stage_batch(next): the next batch is packed and uploaded while the replay runs
  eager_kernel    one one-element eager kernel in front of step(): what ANY eager launch between two replays costs, whatever it computes

and the host time of one call of step(), stage_batch(), commit_batch() and load_batch() (host clock without a synchronise: what the calling thread is
busy for), which says whether the loop is bound by the device or by the thread that feeds it.

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

SIZES_HW = [(480, 640), (640, 480), (427, 640), (375, 500)]
DEV = "cuda:0"


def _sources(seed, sizes):
    rng = np.random.default_rng(seed)
    return ([rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes], [rng.integers(0, 2, (h, w), dtype=np.uint8) for h, w in sizes])


def _stats(ts):
    ts = sorted(ts)
    return dict(ms_median=round(statistics.median(ts), 4), ms_p10=round(ts[len(ts) // 10], 4), ms_p90=round(ts[(len(ts) * 9) // 10], 4))


def _launches(fn):
    from lavt_hip import _capi as K
    K.prof.start()
    try:
        fn()
    finally:
        rec = K.prof.stop()
    return len(rec), round(sum(r[3] for r in rec), 1)


def input_stage(a, report):
    from lavt_hip import preprocess as P
    out = (480, 480)
    images, masks = _sources(1, SIZES_HW * 2)
    n = len(images)
    x = torch.zeros(n, 3, *out, device=DEV)
    t = torch.zeros(n, *out, dtype=torch.int64, device=DEV)

    fp = P.FramePreprocessor(out)
    for im, mk in zip(images, masks):
        fp.reserve_staging(im.shape)
        fp.reserve_staging(mk.shape)

    def per_image():
        for i in range(n):
            fp.images(images[i], out=x[i:i + 1])
            fp.targets(masks[i], out=t[i:i + 1])

    bp = P.BatchPreprocessor(out)

    def batch():
        bp.batch(images, masks, out_images=x, out_targets=t)

    variants = [("per_image", per_image), ("per_image_2", per_image), ("batch", batch)]
    h2d = {"per_image": sum(im.size + mk.size for im, mk in zip(images, masks)), "batch": P.pack_batch(images, masks, out_size=out)[1].nbytes,
           "host_pil": n * 3 * out[0] * out[1] * 4 + n * out[0] * out[1] * 8}
    h2d["per_image_2"] = h2d["per_image"]
    try:
        from PIL import Image
        import transforms
        tf = transforms.get_transform(out[0])
        pil = [(Image.fromarray(im, "RGB"), Image.fromarray(mk, "L")) for im, mk in zip(images, masks)]

        def host_pil():
            pairs = [tf(i, m) for i, m in pil]
            x.copy_(torch.stack([p[0] for p in pairs]), non_blocking=True)
            t.copy_(torch.stack([p[1] for p in pairs]), non_blocking=True)
        variants.append(("host_pil", host_pil))
    except ImportError as e:
        print(f"[input_stage_time] host_pil left out: {e}", file=sys.stderr)

    per_image()
    ref = (x.clone(), t.clone())
    batch()
    torch.cuda.synchronize()
    same = bool(torch.equal(x, ref[0]) and torch.equal(t, ref[1]))
    times = {name: [] for name, _ in variants}
    for it in range(a.warmup + a.iters):
        for name, fn in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if it >= a.warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
    for name, fn in variants:
        launches, kernel_us = _launches(fn)
        report(part="input_stage", variant=name, batch=n, out=list(out), iters=a.iters, launches=launches, kernel_us=kernel_us, h2d_bytes=int(h2d[name]),
               batch_equals_per_image=same, **_stats(times[name]))


def train_iteration(a, report):
    import bench
    import lavt_hip
    from lavt_hip.detweights import det_inputs
    from lavt_hip.engine import TrainStep
    cfg = dict(bench.WORKLOADS["swin_b_w12_480_b2"], name="swin_b_w12_480_b2")
    lavt_hip.set_compute_dtype("bf16")
    torch.manual_seed(1234)
    model = bench.build_model(cfg, torch.device(DEV), 0.3).train()
    x, l, m, tgt = det_inputs(cfg["batch"], cfg["size"], 20, seed=1234)
    step = TrainStep(model, x.to(DEV), l.to(DEV), m.to(DEV), tgt.to(DEV))
    step.warmup_and_capture()
    batches = [_sources(2, SIZES_HW[:2]), _sources(3, SIZES_HW[2:])]
    for b in batches:          # slots allocated, tables cached
        step.load_batch(*b)
    for _ in range(a.warmup):
        step.step()
    k = [0]

    def static():
        step.step()

    def load_batch():
        k[0] += 1
        step.load_batch(*batches[k[0] & 1])
        step.step()

    def stage_commit():
        k[0] += 1
        step.commit_batch()
        step.step()
        step.stage_batch(*batches[k[0] & 1])

    def eager_kernel():
        one.add_(0)
        step.step()
    one = torch.zeros(1, device=DEV)

    variants = [("static", static), ("static_2", static), ("load_batch", load_batch), ("stage_commit", stage_commit), ("eager_kernel", eager_kernel)]
    blocks = max(a.iters // a.block, 1)
    times = {name: [] for name, _ in variants}
    for r in range(blocks + 1):          # the first round warms every variant
        for name, fn in variants:
            if name == "stage_commit":
                step.stage_batch(*batches[0])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.block):
                fn()
            torch.cuda.synchronize()
            el = (time.perf_counter() - t0) * 1e3 / a.block
            if name == "stage_commit":
                step.commit_batch()          # (the batch staged by the last iteration of the block)
            if r:
                times[name].append(el)
    for name, _ in variants:
        report(part="train_iteration", workload="swin_b_w12_480_b2", variant=name, captured=bool(step.captured), block=a.block, blocks=blocks, loss=float(step.loss),
               **_stats(times[name]))
    # where the host's time goes in one iteration: each call timed on the host clock WITHOUT a synchronise (what the calling thread is busy for),
    # the device drained before every iteration so that no call waits for a full queue
    host = {"step": [], "stage_batch": [], "commit_batch": [], "load_batch": []}

    def clocked(name, fn, *args):
        t0 = time.perf_counter()
        fn(*args)
        host[name].append((time.perf_counter() - t0) * 1e3)
    for i in range(a.block * 3):
        torch.cuda.synchronize()
        clocked("stage_batch", step.stage_batch, *batches[i & 1])
        clocked("commit_batch", step.commit_batch)
        clocked("step", step.step)
        torch.cuda.synchronize()
        clocked("load_batch", step.load_batch, *batches[i & 1])
    for name, ts in host.items():
        report(part="host_time_of_one_call", call=name, calls=len(ts), **_stats(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--block", type=int, default=20, help="part 2: iterations per timed block")
    ap.add_argument("--no-train", action="store_true", help="part 1 only")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    if a.iters < 200:
        ap.error("--iters must be at least 200")
    lines = []

    def report(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)
    input_stage(a, report)
    if not a.no_train:
        train_iteration(a, report)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
