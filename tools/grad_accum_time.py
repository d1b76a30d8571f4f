#!/usr/bin/env python3
"""What gradient accumulation costs per MICRO-step of bench.py's flagship workload (swin_b_w12_480_b2: Swin-B LAVT, window 12, 2 x 480^2, bf16):

    (a) owned_guarded  TrainStep(accumulate=1), make_optimizer(max_grad_norm=1.0, skip_nonfinite=True): one replay = one whole iteration
    (b) accumulate4    TrainStep(accumulate=4), the same optimizer: one replay = one micro-step; 3 of 4 replays only fold, the 4th also updates
    (c) fold           lavt_grad_accumulate alone over route (b)'s flat gradient and accumulation buffers (GB/s: 3 x 4 bytes per element -- g and
                       acc read, acc written; the selecting first micro-step of a cycle moves 2 x 4)
    (d) torch_add      acc.add_(flat, alpha=0.25) over the same buffers: the outside yardstick for (c)

One process, two models in private contexts; the routes are timed ALTERNATELY (a, b, c, d, a, b, ...) so that whatever else the host is doing hits all
of them alike.  Every repetition is a window of `--steps` iterations (a multiple of 4: whole cycles) between two device events, ended by a
synchronise; reported per route: median / min / max over the repetitions (the spread of (a) is the unit any difference between (a) and (b) has to be
read against).  lr = 0 as in tools/train_iter_time.py: same memory traffic, weights left alone.  Prints one JSON line per route and appends them to
profiles/grad_accum_time.jsonl; the last line compares (b) - (a) with (c).

    python tools/grad_accum_time.py [--steps 20] [--reps 7] [--warmup 8]
"""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "lavt-rs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
K_ACC = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="iterations (micro-steps) per timed window: a multiple of 4")
    ap.add_argument("--reps", type=int, default=7, help="timed windows per route")
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_accum_time.jsonl"))
    a = ap.parse_args()
    if a.steps < K_ACC or a.steps % K_ACC or a.warmup % K_ACC:
        sys.exit(f"grad_accum_time.py: --steps and --warmup must be multiples of {K_ACC} (whole accumulation cycles)")

    import torch
    import lavt_hip
    from lavt_hip import ops, _capi as K
    from lavt_hip.detweights import det_inputs, fill_state_dict_
    from lavt_hip.engine import TrainStep
    from lib import segmentation
    if not torch.cuda.is_available():
        sys.exit("grad_accum_time.py measures on the GPU only")
    dev = torch.device("cuda:0")
    lavt_hip.set_compute_dtype(torch.bfloat16)
    x, l, m, t = [v.to(dev) for v in det_inputs(2, 480, 20, seed=1234)]
    okw = dict(lr=0.0, weight_decay=1e-2, total_steps=1000, max_grad_norm=1.0, skip_nonfinite=True)

    def harness(accumulate):
        torch.manual_seed(1234)
        model = segmentation.lavt("", SimpleNamespace(swin_type="base", window12=True, drop_path_rate=0.3, bert_random_init=True))
        fill_state_dict_(model)
        model = model.to(dev).train()
        step = TrainStep(model, x, l, m, t, use_graph=True, context=ops.StepContext(), accumulate=accumulate)
        opt = step.make_optimizer(**okw)
        step.warmup_and_capture()
        if not step.captured:
            sys.exit("grad_accum_time.py: the step was not captured; an eager step is launch-bound and says nothing about these routes")
        return step, opt

    sa, oa = harness(1)
    sb, ob = harness(K_ACC)
    flat, acc = sb.buckets.flat, sb.acc
    n = flat.numel()
    ctl = torch.tensor([0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]).to(dev)          # m = 1 and no tick behind it: every call folds (reads acc), none selects
    acc2 = torch.zeros_like(acc)                                                     # (c) and (d) write a buffer of their own: route (b)'s cycle is not disturbed

    routes = [("owned_guarded", sa.step, a.steps), ("accumulate4", sb.step, a.steps),
              ("fold", lambda: K.check(K.lib.lavt_grad_accumulate(K.ptr(flat), K.ptr(acc2), n, K_ACC, K.ptr(ctl), K.stream())), 25 * a.steps),
              ("torch_add", lambda: acc2.add_(flat, alpha=0.25), 25 * a.steps)]
    for _, fn, _n in routes:
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in routes}
    for _ in range(a.reps):
        for name, fn, cnt in routes:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(cnt):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / cnt)
    extra = {"owned_guarded": {"optimizer_steps": oa.steps_taken(), "skipped_steps": oa.skipped_steps(), "grad_norm": oa.last_grad_norm()},
             "accumulate4": {"accumulate": K_ACC, "optimizer_steps": ob.steps_taken(), "skipped_steps": ob.skipped_steps(), "grad_norm": ob.last_grad_norm(),
                             "micro_step": sb.micro_step()},
             "fold": {"elements": n, "bytes": 12 * n}, "torch_add": {"elements": n, "bytes": 12 * n}}
    lines, med = [], {}
    for name, _, cnt in routes:
        ts = times[name]
        med[name] = statistics.median(ts)
        rec = {"tool": "grad_accum_time", "workload": "swin_b_w12_480_b2", "route": name, "ms_median": round(med[name], 4), "ms_min": round(min(ts), 4),
               "ms_max": round(max(ts), 4), "reps": len(ts), "iterations_per_rep": cnt, "ms_all": [round(v, 4) for v in ts], "device": torch.cuda.get_device_name(0)}
        rec.update(extra[name])
        if "bytes" in rec:
            rec["gb_per_s_median"] = round(rec["bytes"] / rec["ms_median"] / 1e6, 1)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    spread = max(times["owned_guarded"]) - min(times["owned_guarded"])
    lines.append(json.dumps({"tool": "grad_accum_time", "workload": "swin_b_w12_480_b2", "route": "comparison", "b_minus_a_ms": round(med["accumulate4"] - med["owned_guarded"], 4),
                             "c_ms": round(med["fold"], 4), "d_ms": round(med["torch_add"], 4), "spread_of_a_ms": round(spread, 4),
                             "b_minus_a_minus_c_ms": round(med["accumulate4"] - med["owned_guarded"] - med["fold"], 4)}))
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
