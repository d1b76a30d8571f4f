#!/usr/bin/env python3
"""What the training criterion costs inside a captured TrainStep replay of bench.py's flagship workload (swin_b_w12_480_b2: Swin-B LAVT, window 12,
2 x 480^2, bf16), per route:

    mc_dice                 TrainStep(loss="mc_dice"): the fused upsample + MultiClassDiceLoss pair
    dice_boundary           TrainStep(loss="dice_boundary"): the fused upsample + Dice + boundary-F1 stencil (boundary_loss.hip)
    dice_boundary_unfused   the same criterion with fused_loss=False: logits upsampled to (B, 2, 480, 480), then losses.DiceBoundaryLoss

dice_boundary - mc_dice is the cost of the boundary part; dice_boundary_unfused - dice_boundary is what fusing the upsample buys.  One process, one
model per route in a private context; the routes are timed ALTERNATELY so that whatever else the host is doing hits all of them alike.  Every
repetition is a window of `--steps` replays between two device events, ended by a synchronise; reported per route: median / min / max over the
repetitions (the spread is the unit any difference between routes has to be read against).  `--routes mc_dice` runs on a tree that predates the
Dice+Boundary criterion (the before / after comparison of the untouched route).  Prints one JSON line per route and appends them to --out.

    python tools/loss_step_time.py [--steps 20] [--reps 7] [--warmup 5] [--routes mc_dice,dice_boundary,dice_boundary_unfused]
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

ROUTES = {"mc_dice": dict(loss="mc_dice"), "dice_boundary": dict(loss="dice_boundary"), "dice_boundary_unfused": dict(loss="dice_boundary", fused_loss=False)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="replays per timed window")
    ap.add_argument("--reps", type=int, default=7, help="timed windows per route")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--routes", default=",".join(ROUTES))
    ap.add_argument("--tag", default="", help="free text copied into every record (e.g. the commit measured)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_step_time.jsonl"))
    a = ap.parse_args()

    import torch
    import lavt_hip
    from lavt_hip import ops
    from lavt_hip.detweights import det_inputs, fill_state_dict_
    from lavt_hip.engine import TrainStep
    from lib import segmentation
    if not torch.cuda.is_available():
        sys.exit("loss_step_time.py measures on the GPU only")
    dev = torch.device("cuda:0")
    lavt_hip.set_compute_dtype(torch.bfloat16)
    x, l, m, t = [v.to(dev) for v in det_inputs(2, 480, 20, seed=1234)]

    def harness(**kw):
        torch.manual_seed(1234)
        model = segmentation.lavt("", SimpleNamespace(swin_type="base", window12=True, drop_path_rate=0.3, bert_random_init=True))
        fill_state_dict_(model)
        model = model.to(dev).train()
        step = TrainStep(model, x, l, m, t, use_graph=True, context=ops.StepContext(), **kw)
        step.warmup_and_capture()
        if not step.captured:
            sys.exit(f"loss_step_time.py: the step {kw} was not captured; an eager step is launch-bound and says nothing about these routes")
        return step

    names = [n for n in a.routes.split(",") if n]
    steps = {n: harness(**ROUTES[n]) for n in names}
    for n in names:
        for _ in range(a.warmup):
            steps[n].step()
    torch.cuda.synchronize()
    times = {n: [] for n in names}
    for _ in range(a.reps):
        for n in names:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.steps):
                steps[n].step()
            e1.record()
            torch.cuda.synchronize()
            times[n].append(e0.elapsed_time(e1) / a.steps)
    lines = []
    for n in names:
        ts = times[n]
        lines.append(json.dumps({"tool": "loss_step_time", "workload": "swin_b_w12_480_b2", "route": n, "tag": a.tag, "ms_median": round(statistics.median(ts), 4),
                                 "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4), "reps": len(ts), "replays_per_rep": a.steps,
                                 "ms_all": [round(v, 4) for v in ts], "loss": float(steps[n].loss), "device": torch.cuda.get_device_name(0)}))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
