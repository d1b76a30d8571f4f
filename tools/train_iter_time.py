#!/usr/bin/env python3
"""What a WHOLE training iteration of bench.py's flagship workload (swin_b_w12_480_b2: Swin-B LAVT, window 12, 2 x 480^2, bf16) costs on each route:

    (a) parent_route   captured step replay, then FusedAdamW.step(check_tables=False) issued from Python
    (b) owned          TrainStep.make_optimizer(): the update is part of the captured graph, one replay per iteration
    (c) owned_guarded  the same with max_grad_norm=1.0, skip_nonfinite=True (lavt_grad_norm + the guarded update in the graph)
    (d) grad_norm      lavt_grad_norm alone over route (c)'s descriptor tables
    (e) torch_norm     torch.linalg.vector_norm over the same flat gradient buffer: the outside yardstick for (d)
    (f) owned_guarded_ema   route (c) with ema_decay=D -- only with --ema-decay D (a fourth model)

One process, three models in private contexts; the routes are timed ALTERNATELY (a, b, c, d, e, a, b, ...) so that whatever else the host is doing
hits all of them alike.  Every repetition is a window of `--steps` iterations between two device events, ended by a synchronise; reported per route:
median / min / max over the repetitions (the spread is the unit any difference between routes has to be read against).  lr = 0 as in bench.py's
separate optimizer timing: same memory traffic, weights left alone.  Prints one JSON line per route and appends them to profiles/train_iter_time.jsonl.

    python tools/train_iter_time.py [--steps 20] [--reps 7] [--warmup 5] [--ema-decay D]
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
    ap.add_argument("--ema-decay", type=float, default=None, help="add route (f): the guarded owned optimizer with this weight-EMA decay")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_iter_time.jsonl"))
    a = ap.parse_args()

    import torch
    import lavt_hip
    from lavt_hip import ops, _capi as K
    from lavt_hip.detweights import det_inputs, fill_state_dict_
    from lavt_hip.engine import TrainStep
    from lavt_hip.optim import FusedAdamW, initial_control_block, lavt_param_groups
    from lib import segmentation
    if not torch.cuda.is_available():
        sys.exit("train_iter_time.py measures on the GPU only")
    dev = torch.device("cuda:0")
    lavt_hip.set_compute_dtype(torch.bfloat16)
    x, l, m, t = [v.to(dev) for v in det_inputs(2, 480, 20, seed=1234)]
    okw = dict(lr=0.0, weight_decay=1e-2, total_steps=1000)

    def harness(owned, **guard):
        torch.manual_seed(1234)
        model = segmentation.lavt("", SimpleNamespace(swin_type="base", window12=True, drop_path_rate=0.3, bert_random_init=True))
        fill_state_dict_(model)
        model = model.to(dev).train()
        ctx = ops.StepContext()
        step = TrainStep(model, x, l, m, t, use_graph=True, context=ctx)
        opt = step.make_optimizer(**okw, **guard) if owned else None
        step.warmup_and_capture()
        if not step.captured:
            sys.exit("train_iter_time.py: the step was not captured; an eager step is launch-bound and says nothing about these routes")
        if not owned:
            opt = FusedAdamW(lavt_param_groups(model), context=ctx, **okw)
            step.step()
            opt.step()                               # builds the tables
        return step, opt

    sa, oa = harness(False)
    sb, ob = harness(True)
    sc, oc = harness(True, max_grad_norm=1.0, skip_nonfinite=True)
    desc, chunks, nchunks = oc._tables.desc, oc._tables.chunks, oc._tables.nchunks
    ctl = initial_control_block().to(dev)
    ws = torch.empty(int(K.lib.lavt_grad_norm_ws(nchunks)), dtype=torch.float32, device=dev)
    flat = sc.buckets.flat
    norm_elems = sum(p.numel() for g in oc.param_groups for p in g["params"] if p.requires_grad)

    def it_a():
        sa.step()
        oa.step(check_tables=False)
    routes = [("parent_route", it_a, a.steps), ("owned", sb.step, a.steps), ("owned_guarded", sc.step, a.steps),
              ("grad_norm", lambda: K.check(K.lib.lavt_grad_norm(K.ptr(desc), K.ptr(chunks), nchunks, K.ptr(ws), K.ptr(ctl), 1.0, 1, K.stream())), 25 * a.steps),
              ("torch_norm", lambda: torch.linalg.vector_norm(flat), 25 * a.steps)]
    if a.ema_decay is not None:
        sf, of = harness(True, max_grad_norm=1.0, skip_nonfinite=True, ema_decay=a.ema_decay)
        routes.append(("owned_guarded_ema", sf.step, a.steps))
    # route (a)'s descriptor tables were built before the later harnesses laid out their flat gradient buffers (ddp.layout_generation is process-wide):
    # one step with the host-side check rebuilds them, outside the timed windows
    sa.step()
    oa.step()
    for _, fn, _n in routes:
        for _ in range(a.warmup):
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
    extra = {"parent_route": {"optimizer_steps": oa.steps_taken()}, "owned": {"optimizer_steps": ob.steps_taken()},
             "owned_guarded": {"optimizer_steps": oc.steps_taken(), "skipped_steps": oc.skipped_steps(), "grad_norm": oc.last_grad_norm()},
             "grad_norm": {"elements": norm_elems, "bytes": 4 * norm_elems, "norm": float(ctl[0])},
             "torch_norm": {"elements": flat.numel(), "bytes": 4 * flat.numel(), "norm": float(torch.linalg.vector_norm(flat))}}
    if a.ema_decay is not None:
        extra["owned_guarded_ema"] = {"optimizer_steps": of.steps_taken(), "skipped_steps": of.skipped_steps(), "ema_decay": a.ema_decay}
    lines = []
    for name, _, n in routes:
        ts = times[name]
        rec = {"tool": "train_iter_time", "workload": "swin_b_w12_480_b2", "route": name, "ms_median": round(statistics.median(ts), 4), "ms_min": round(min(ts), 4),
               "ms_max": round(max(ts), 4), "reps": len(ts), "iterations_per_rep": n, "ms_all": [round(v, 4) for v in ts], "device": torch.cuda.get_device_name(0)}
        rec.update(extra[name])
        if "bytes" in rec:
            rec["gb_per_s_median"] = round(rec["bytes"] / rec["ms_median"] / 1e6, 1)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
