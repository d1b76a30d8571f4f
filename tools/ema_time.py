#!/usr/bin/env python3
"""What the weight EMA (FusedAdamW(ema_decay=d), DESIGN.md "Weight EMA") costs on bench.py's flagship workload (swin_b_w12_480_b2: Swin-B LAVT, window 12,
2 x 480^2, bf16):

    (a) replay_off     one replay of a captured training iteration, owned optimizer with max_grad_norm=1.0, skip_nonfinite=True, ema_decay=None
    (b) replay_ema     the same with ema_decay=0.999
    (c) update_off     the guarded update alone (lavt_adamw_step_chunks_guarded, the kernel an optimizer without the average launches) over (a)'s tables
    (d) update_ema     lavt_adamw_step_chunks_ema with a control block over (b)'s tables
    (e) swap           lavt_ema_swap over (b)'s tables (an even number of calls per window: the weights end where they started)

One process, two models in private contexts; the routes are timed ALTERNATELY so that whatever else the host is doing hits all of them alike.  Every
repetition is a window of iterations between two device events, ended by a synchronise; reported per route: median / min / max over the repetitions.
lr = 0 as in bench.py's separate optimizer timing: same memory traffic, weights left alone.  Prints one JSON line per route and appends them to
profiles/ema_time.jsonl.

    python tools/ema_time.py [--steps 20] [--reps 7] [--warmup 5]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="iterations per timed window")
    ap.add_argument("--reps", type=int, default=7, help="timed windows per route")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_time.jsonl"))
    a = ap.parse_args()

    import torch
    import lavt_hip
    from lavt_hip import ops, _capi as K
    from lavt_hip.detweights import det_inputs, fill_state_dict_
    from lavt_hip.engine import TrainStep
    from lib import segmentation
    if not torch.cuda.is_available():
        sys.exit("ema_time.py measures on the GPU only")
    dev = torch.device("cuda:0")
    lavt_hip.set_compute_dtype(torch.bfloat16)
    x, l, m, t = [v.to(dev) for v in det_inputs(2, 480, 20, seed=1234)]
    okw = dict(lr=0.0, weight_decay=1e-2, total_steps=1000, max_grad_norm=1.0, skip_nonfinite=True)

    def harness(**kw):
        torch.manual_seed(1234)
        model = segmentation.lavt("", SimpleNamespace(swin_type="base", window12=True, drop_path_rate=0.3, bert_random_init=True))
        fill_state_dict_(model)
        model = model.to(dev).train()
        step = TrainStep(model, x, l, m, t, use_graph=True, context=ops.StepContext())
        opt = step.make_optimizer(**okw, **kw)
        step.warmup_and_capture()
        if not step.captured:
            sys.exit("ema_time.py: the step was not captured; an eager step is launch-bound and says nothing about these routes")
        return step, opt

    s_off, o_off = harness()
    s_ema, o_ema = harness(ema_decay=0.999)
    assert o_off._tables.ema is None and o_ema._tables.ema is not None

    def update_off():
        T = o_off._tables
        K.check(K.lib.lavt_adamw_step_chunks_guarded(K.ptr(T.desc), K.ptr(T.hyper), K.ptr(T.chunks), T.nchunks, K.ptr(o_off._step), o_off.total_steps, o_off.power,
                                                     K.ptr(o_off.guard), K.stream()))

    def update_ema():
        T = o_ema._tables
        K.check(K.lib.lavt_adamw_step_chunks_ema(K.ptr(T.desc), None, K.ptr(T.ema), K.ptr(T.hyper), K.ptr(T.chunks), T.nchunks, K.ptr(o_ema._step),
                                                 o_ema.total_steps, o_ema.power, o_ema.ema_decay, K.ptr(o_ema.guard), K.stream()))

    def swap():
        T = o_ema._tables
        K.check(K.lib.lavt_ema_swap(K.ptr(T.desc), K.ptr(T.ema), K.ptr(T.chunks), T.nchunks, K.stream()))

    k = 10 * a.steps
    routes = [("replay_off", s_off.step, a.steps), ("replay_ema", s_ema.step, a.steps), ("update_off", update_off, k), ("update_ema", update_ema, k),
              ("swap", swap, k)]
    for _, fn, _n in routes:
        for _ in range(2 * a.warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in routes}
    for _ in range(a.reps):
        for name, fn, n in routes:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / n)
    elems = sum(p.numel() for g in o_ema.param_groups for p in g["params"] if p.requires_grad)
    copies = sum(s_ema.context.weights.store[key][1].numel() for key in o_ema._tables.fused)          # the bf16 copies the update writes itself
    nbytes = {"update_off": 28 * elems + 2 * copies, "update_ema": 36 * elems + 2 * copies, "swap": 16 * elems + 2 * copies}
    lines = []
    for name, _, n in routes:
        ts = times[name]
        rec = {"tool": "ema_time", "workload": "swin_b_w12_480_b2", "route": name, "ms_median": round(statistics.median(ts), 4), "ms_min": round(min(ts), 4),
               "ms_max": round(max(ts), 4), "reps": len(ts), "iterations_per_rep": n, "ms_all": [round(v, 4) for v in ts], "device": torch.cuda.get_device_name(0)}
        if name in nbytes:
            rec.update(elements=elems, bytes=nbytes[name], gb_per_s_median=round(nbytes[name] / rec["ms_median"] / 1e6, 1))
        else:
            opt = o_off if name == "replay_off" else o_ema
            rec.update(optimizer_steps=opt.steps_taken(), skipped_steps=opt.skipped_steps())
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    med = {name: statistics.median(ts) for name, ts in times.items()}
    lines.append(json.dumps({"tool": "ema_time", "workload": "swin_b_w12_480_b2", "route": "comparison",
                             "update_ema_over_off": round(med["update_ema"] / med["update_off"], 4), "bytes_ema_over_off": round(nbytes["update_ema"] / nbytes["update_off"], 4),
                             "replay_ema_minus_off_ms": round(med["replay_ema"] - med["replay_off"], 4),
                             "spread_of_replay_off_ms": round(max(times["replay_off"]) - min(times["replay_off"]), 4)}))
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
