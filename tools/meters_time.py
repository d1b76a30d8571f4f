#!/usr/bin/env python3
"""What the training meters (TrainStep(meters=...), FusedAdamW(tensor_norms=True); DESIGN.md "Training meters") cost on bench.py's flagship workload
(swin_b_w12_480_b2: Swin-B LAVT, window 12, 2 x 480^2, bf16), and what they save:

    (a) replay_plain     one replay of a captured training iteration, owned optimizer with max_grad_norm=1.0, skip_nonfinite=True; no meters
    (b) replay_meters    the same with meters and tensor norms: two launches more per replay, and meters.poll() every 10th step
    (b') replay_append   meters without tensor norms and without polling: the append launch alone (attribution of (b) - (a))
    (c) replay_item      (a)'s step followed by float(step.stats[0]) after EVERY replay -- the reference's habit (train.py:231-235: loss.item())

One process, three models in private contexts; the routes are timed ALTERNATELY so that whatever else the host is doing hits all of them alike.  Every
repetition is a window of iterations between two device events, ended by a synchronise; reported per route: median / min / max over the repetitions, and
the host's wall time per iteration next to the device's (route (c) is bound by the host's wait, not by the device).  lr = 0 as in bench.py's separate
optimizer timing: same memory traffic, weights left alone.  Prints one JSON line per route and appends them to profiles/meters_time.jsonl.

--loss {ce,mc_dice,dice_boundary} chooses the criterion of all three steps (default ce).  Under the Dice criteria a metered step also runs the hard-mask
I / U pass (lavt_upsample_iu: two launches behind the criterion's forward), so (b') - (a) is the append plus that pass; every JSON line names the criterion.

    python tools/meters_time.py [--steps 20] [--reps 7] [--warmup 5] [--loss ce]
"""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "lavt-rs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="iterations per timed window")
    ap.add_argument("--reps", type=int, default=7, help="timed windows per route")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--poll-every", type=int, default=10)
    ap.add_argument("--loss", choices=("ce", "mc_dice", "dice_boundary"), default="ce", help="the criterion of the timed steps")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meters_time.jsonl"))
    a = ap.parse_args()

    import torch
    import lavt_hip
    from lavt_hip import ops
    from lavt_hip.detweights import det_inputs, fill_state_dict_
    from lavt_hip.engine import TrainStep
    from lib import segmentation
    if not torch.cuda.is_available():
        sys.exit("meters_time.py measures on the GPU only")
    dev = torch.device("cuda:0")
    lavt_hip.set_compute_dtype(torch.bfloat16)
    x, l, m, t = [v.to(dev) for v in det_inputs(2, 480, 20, seed=1234)]
    okw = dict(lr=0.0, weight_decay=1e-2, total_steps=1000, max_grad_norm=1.0, skip_nonfinite=True)

    def harness(metered, tensor_norms=None):
        torch.manual_seed(1234)
        model = segmentation.lavt("", SimpleNamespace(swin_type="base", window12=True, drop_path_rate=0.3, bert_random_init=True))
        fill_state_dict_(model)
        model = model.to(dev).train()
        step = TrainStep(model, x, l, m, t, use_graph=True, context=ops.StepContext(), loss=a.loss)
        opt = step.make_optimizer(tensor_norms=metered if tensor_norms is None else tensor_norms, **okw)
        meters = step.make_meters() if metered else None
        step.warmup_and_capture()
        if not step.captured:
            sys.exit("meters_time.py: the step was not captured; an eager step is launch-bound and says nothing about these routes")
        return step, opt, meters

    s_plain, o_plain, _ = harness(False)
    s_met, o_met, meters = harness(True)
    s_app, _, _ = harness(True, tensor_norms=False)
    count = [0]
    seen = []

    def metered():
        s_met.step()
        count[0] += 1
        if count[0] % a.poll_every == 0:
            snap = meters.poll()
            if snap is not None:
                seen.append(snap.n)

    def item():
        s_plain.step()
        seen.append(float(s_plain.stats[0]))

    routes = [("replay_plain", s_plain.step), ("replay_meters", metered), ("replay_append", s_app.step), ("replay_item", item)]
    for _, fn in routes:
        for _ in range(2 * a.warmup):
            fn()
    torch.cuda.synchronize()
    dev_ms, host_ms = {name: [] for name, _ in routes}, {name: [] for name, _ in routes}
    for _ in range(a.reps):
        for name, fn in routes:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            for _ in range(a.steps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            host_ms[name].append((time.perf_counter() - t0) * 1e3 / a.steps)
            dev_ms[name].append(e0.elapsed_time(e1) / a.steps)
    snap = meters.read()
    lines = []
    for name, _ in routes:
        ts, hs = dev_ms[name], host_ms[name]
        rec = {"tool": "meters_time", "workload": "swin_b_w12_480_b2", "loss": a.loss, "route": name, "ms_median": round(statistics.median(ts), 4), "ms_min": round(min(ts), 4),
               "ms_max": round(max(ts), 4), "host_ms_median": round(statistics.median(hs), 4), "reps": len(ts), "iterations_per_rep": a.steps,
               "ms_all": [round(v, 4) for v in ts], "device": torch.cuda.get_device_name(0)}
        if name == "replay_meters":
            rec.update(records=snap.n, iterations=snap.iterations, poll_every=a.poll_every, tensors=len(o_met.grad_norms()), log=str(snap))
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    med = {name: statistics.median(ts) for name, ts in dev_ms.items()}
    lines.append(json.dumps({"tool": "meters_time", "workload": "swin_b_w12_480_b2", "loss": a.loss, "route": "comparison",
                             "meters_minus_plain_us": round((med["replay_meters"] - med["replay_plain"]) * 1e3, 2),
                             "append_minus_plain_us": round((med["replay_append"] - med["replay_plain"]) * 1e3, 2),
                             "item_minus_plain_us": round((med["replay_item"] - med["replay_plain"]) * 1e3, 2),
                             "spread_of_replay_plain_us": round((max(dev_ms["replay_plain"]) - min(dev_ms["replay_plain"])) * 1e3, 2)}))
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
