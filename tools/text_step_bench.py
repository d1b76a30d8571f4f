"""The text encoder inside the captured step: what it costs, and what the fused attention core saves (DESIGN.md "Text encoder in the step").

    python tools/text_step_bench.py [--steps 20] [--warmup 10] [--reps 0] [--tokens 20] [--time-limit 900] [--count-limit 600]

Swin-B w12 LAVT at 480^2, bf16, batch 2, as bench.py builds it (captured step, no optimizer, DropPath 0.3), 20 tokens per sentence, a randomly
initialised bert-base (12 layers, 12 heads of 64, dropout 0.1, training mode).  Three steps:

  plain      TrainStep on precomputed language features: the step bench.py measures, a frozen language encoder
  composed   TrainStep(text_encoder=) with fused_attention=False: the attention core of every layer is ops.masked_self_attention, the composed route
  fused      the same with fused_attention=True: ops.sentence_attention, one kernel per direction and layer

Two measurements, each in a fresh child process under its own time limit; the first failure ends the tool with that child's status:

  time    all three steps live in ONE process, each with its own model copy (same weights), encoder copy and ops.StepContext.  The timed region is
          bench.py's: `--steps` replays between two device synchronisations, host clock.  The three ALTERNATE, region by region, until 2 s have been
          timed per variant, at most 15 regions (or exactly --reps): drift and other tenants' work hit all alike.  Reported: the median ms per replay
          of each, every region, and the spread (max - min of the regions) a difference has to exceed.
  count   kernel launches per replay: one replay of each captured step under torch.profiler, counting the device kernel events (library kernels and
          torch's own alike; copies and fills issued as memcpy / memset nodes are not kernels and are listed beside).  Where the tracer reports no
          kernels for a graph launch, the captured step's body is issued eagerly once instead -- the launches the capture recorded -- and the result
          says which it was (`launches_counted_on`).  A run of its own: tracing slows the host.  A count of zero is an error, not a result.

One JSON line on stdout; if a measurement fails, the line holds what was measured before it and an `incomplete` entry, and the exit status is non-zero."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "lavt-rs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

DEV = "cuda:0"
VARIANTS = ("plain", "composed", "fused")


def _build_steps(a):
    """the three captured steps -> {name: TrainStep}"""
    import torch
    import bench
    import lavt_hip
    from bert.modeling_bert import BertConfig, BertModel
    from lavt_hip import ops
    from lavt_hip.detweights import det_inputs, fill_state_dict_
    from lavt_hip.engine import TrainStep
    if not torch.cuda.is_available():
        raise SystemExit("text_step_bench: needs a GPU (there is no CPU path to time)")
    cfg = dict(bench.WORKLOADS["swin_b_w12_480_b2"], name="swin_b_w12_480_b2")
    lavt_hip.set_compute_dtype("bf16")
    x, l, m, tgt = (t.to(DEV) for t in det_inputs(cfg["batch"], cfg["size"], a.tokens, seed=1234))
    mask = m.squeeze(-1).long()
    ids = (torch.randint(1, 30522, mask.shape, generator=torch.Generator().manual_seed(7)).to(DEV) * mask).contiguous()
    steps = {}
    for name in VARIANTS:
        torch.manual_seed(1234)
        model = bench.build_model(cfg, torch.device(DEV), a.drop_path).train()
        if name == "plain":
            step = TrainStep(model, x.clone(), l.clone(), m.clone(), tgt.clone(), context=ops.StepContext())
        else:
            enc = BertModel(BertConfig(), fused_attention=(name == "fused"))
            fill_state_dict_(enc, salt=11)
            enc.pooler = None                    # train.py:602
            step = TrainStep(model, x.clone(), ids.clone(), mask.clone(), tgt.clone(), context=ops.StepContext(), text_encoder=enc.to(DEV).train())
        step.warmup_and_capture()
        if not step.captured:
            raise SystemExit(f"text_step_bench: the {name} step was not captured")
        steps[name] = step
    return steps


def _region(step, n):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        step.step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def measure_time(a):
    steps = _build_steps(a)
    for step in steps.values():
        for _ in range(a.warmup):
            step.step()
    times = {n: [] for n in VARIANTS}
    while True:
        for name in VARIANTS:
            times[name].append(_region(steps[name], a.steps))
        done = len(times["fused"])
        if (a.reps and done >= a.reps) or (not a.reps and (done >= 15 or min(sum(ts) for ts in times.values()) * a.steps >= 2000.0)):
            break
    med = {n: statistics.median(ts) for n, ts in times.items()}
    spread = {n: max(ts) - min(ts) for n, ts in times.items()}
    return {"steps_per_region": a.steps, "regions": len(times["fused"]), "ms_per_replay": {n: round(v, 3) for n, v in med.items()},
            "spread_ms": {n: round(v, 3) for n, v in spread.items()},
            "text_stage_ms": {"composed": round(med["composed"] - med["plain"], 3), "fused": round(med["fused"] - med["plain"], 3)},
            "fused_minus_composed_ms": round(med["fused"] - med["composed"], 3),
            "fused_not_slower_than_composed_by_more_than_the_spread": bool(med["fused"] - med["composed"] <= max(spread["fused"], spread["composed"])),
            "ms_per_replay_all_regions": {n: [round(t, 3) for t in ts] for n, ts in times.items()},
            "loss": {n: round(float(s.loss), 5) for n, s in steps.items()}}


def measure_count(a):
    import torch
    from torch.profiler import ProfilerActivity, profile
    steps = _build_steps(a)

    def traced(fn):
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        dev = [e for e in prof.events() if str(e.device_type).endswith("CUDA")]
        other = [e for e in dev if e.name.lower().startswith(("memcpy", "memset"))]
        return len(dev) - len(other), len(other), len(prof.events())
    out, how = {}, None
    for name, step in steps.items():
        for _ in range(3):
            step.step()
        torch.cuda.synchronize()
        # a replay first; where the tracer does not report the kernels of a graph launch, the step's body issued eagerly: the capture recorded exactly
        # these launches (the same Python, the same static buffers)
        for method, fn in (("replay", step.step), ("eager body", step._body)):
            if how not in (None, method):
                continue
            kernels, other, seen = traced(fn)
            print(f"text_step_bench: {name} / {method}: {kernels} kernel events, {other} memcpy / memset, {seen} events in all", file=sys.stderr)
            if kernels > 0:
                how = method
                break
        else:
            raise SystemExit(f"text_step_bench: the profiler saw no kernel in the {name} step, neither replayed nor issued eagerly: no count")
        out[name] = {"kernels": kernels, "memcpy_memset": other}
    layers = 12
    return {"launches_counted_on": how, "launches_per_replay": out,
            "text_stage_launches": {n: out[n]["kernels"] - out["plain"]["kernels"] for n in ("composed", "fused")},
            "fewer_launches_per_layer_fused": round((out["composed"]["kernels"] - out["fused"]["kernels"]) / layers, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="replays per timed region")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=0, help="timed regions per variant; 0 = until 2 s are timed per variant, at most 15")
    ap.add_argument("--tokens", type=int, default=20)
    ap.add_argument("--drop-path", type=float, default=0.3)
    ap.add_argument("--time-limit", type=float, default=900.0, help="seconds for the timing child")
    ap.add_argument("--count-limit", type=float, default=600.0, help="seconds for the launch-count child")
    ap.add_argument("--child", choices=("time", "count"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps((measure_time if a.child == "time" else measure_count)(a)), flush=True)
        return
    # the parent never touches the GPU: every measurement is a fresh process with a time limit of its own; the first that fails ends the tool
    result = {"tool": "text_step_bench", "workload": "swin_b_w12_480_b2", "dtype": "bf16", "tokens": a.tokens, "bert": "bert-base, random init, dropout 0.1",
              "drop_path": a.drop_path}
    passed = [f"--{k.replace('_', '-')}={getattr(a, k)}" for k in ("steps", "warmup", "reps", "tokens", "drop_path")]
    for child, limit in (("time", a.time_limit), ("count", a.count_limit)):
        failed = None
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", child] + passed, stdout=subprocess.PIPE, timeout=limit)
            if r.returncode != 0:
                failed = f"ended with status {r.returncode}"
        except subprocess.TimeoutExpired:
            failed = f"ran into its time limit of {limit:.0f} s"
        if failed:          # what was measured before it is kept on stdout, marked incomplete; the exit status says so too
            print(json.dumps(dict(result, incomplete=f"the {child} measurement {failed}")), flush=True)
            raise SystemExit(f"text_step_bench: the {child} measurement {failed}; nothing further is started")
        result.update(json.loads(r.stdout.decode().strip().splitlines()[-1]))
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
