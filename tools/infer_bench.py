"""Inference timing: today's eval path against lavt_hip.engine.Predictor (Swin-B w12, 480^2, bf16, batch 1 as the reference's test.py runs it).

    python tools/infer_bench.py [--calls 30] [--warmup 5] [--size 480] [--variant base] [--out profiles/infer_bench.jsonl]

Every figure is the MEDIAN milliseconds per call over `--calls` (>= 20) timed calls after `--warmup`, each call bracketed by a device synchronise
on both sides (host wall clock: what an evaluation loop sees per sample).  Paths:

  eval_host        model.eval() forward under no_grad + argmax + I / U on the host, as test.py:73-83 does (output.cpu().argmax(1), numpy counts);
                   this code path is unchanged by the inference work: the baseline
  predictor_eager  Predictor(use_graph=False).step() + reading the two counts
  predictor_replay Predictor.step() replaying the captured graph + reading the two counts
  3 expressions    three batch-1 replays (one per sentence) against ONE replay of Predictor(expressions_per_image=3)

and the decoder's launch count per call (profiler records in the "decoder" scope) before and after folding.  One JSON line per figure.

    --frames-u8 HxW   (opt-in) also time the input stage for one uint8 frame of that size, same frame on both paths, next to the replay time:
  frames_cpu_pipeline   transforms.get_transform on the PIL image (resize, to-tensor, normalise on the host) + the fp32 upload into the predictor's image buffer
  frames_load_frames    Predictor.load_frames: the uint8 upload (pinned staging) + the resize / normalise kernel into the same buffer"""
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

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", type=int, default=480)
    ap.add_argument("--variant", default="base", choices=["base", "tiny"])
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--frames-u8", default=None, metavar="HxW", help="also time the input stage for a uint8 frame of this size: CPU pipeline vs Predictor.load_frames")
    a = ap.parse_args()
    if a.calls < 20:
        ap.error("--calls must be at least 20")
    import lavt_hip
    from lavt_hip import _capi as K
    from lavt_hip import ops
    from lavt_hip.detweights import det_inputs, fill_state_dict_
    from lavt_hip.engine import Predictor
    from lib import segmentation
    dev = "cuda:0"
    lavt_hip.set_compute_dtype(torch.bfloat16 if a.dtype == "bf16" else torch.float32)
    model = segmentation.lavt("", SimpleNamespace(swin_type=a.variant, window12=a.variant == "base", drop_path_rate=0.3))
    fill_state_dict_(model)
    model.to(dev).eval()
    S = 3
    x, _, _, tgt = det_inputs(1, a.size, 20, seed=1234)
    _, l3, m3, _ = det_inputs(S, a.size, 20, seed=77)
    x, tgt, l3, m3 = x.to(dev), tgt.to(dev), l3.to(dev), m3.to(dev)
    l1, m1 = l3[:1].contiguous(), m3[:1].contiguous()
    tgt_np = tgt.cpu().numpy()
    lines = []

    def report(**kw):
        kw.update(variant=a.variant, size=a.size, dtype=a.dtype, calls=a.calls)
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    # ---- today's path (test.py:73-83)
    def eval_host(l=l1, m=m1):
        with torch.no_grad():
            output = model(x, l, m)
        output = output.cpu()
        mask = output.argmax(1).data.numpy()
        return np.sum(np.logical_and(mask, tgt_np)), np.sum(np.logical_or(mask, tgt_np))
    med, lo, hi = timed(eval_host, a.calls, a.warmup)
    report(path="eval_host", batch=1, ms_median=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3))
    base_iu = eval_host()

    def eval_host_3():
        for j in range(S):
            eval_host(l3[j:j + 1], m3[j:j + 1])
    med3, lo3, hi3 = timed(eval_host_3, a.calls, a.warmup)
    report(path="eval_host", batch=1, expressions=S, note="three forward passes", ms_median=round(med3, 3), ms_min=round(lo3, 3), ms_max=round(hi3, 3))

    # ---- Predictor, one expression
    figures = {}
    for name, use_graph in (("predictor_eager", False), ("predictor_replay", True)):
        p = Predictor(model, x, l1, m1, target=tgt, use_graph=use_graph, context=ops.StepContext())
        p.warmup_and_capture()

        def step(p=p):
            p.step()
            return p.iu.tolist()
        med, lo, hi = timed(step, a.calls, a.warmup)
        figures[name] = med
        iu = step()[0]
        report(path=name, batch=1, captured=p.captured, ms_median=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3), iu=iu,
               iu_eval_host=[int(base_iu[0]), int(base_iu[1])])
        single = p

    # ---- input stage (opt-in): the parent's PIL path against load_frames, same frame, into the replay predictor's image buffer
    if a.frames_u8:
        from PIL import Image
        import transforms
        fh, fw = (int(v) for v in a.frames_u8.lower().split("x"))
        frame = np.random.default_rng(7).integers(0, 256, (1, fh, fw, 3), dtype=np.uint8)
        pil = Image.fromarray(frame[0], "RGB")
        tf = transforms.get_transform(a.size)

        def cpu_pipeline():
            image, _ = tf(pil, None)
            single.x.copy_(image.unsqueeze(0))
        single.load_frames(frame)          # tables uploaded, preprocessor made
        single.preprocessor.reserve_staging(frame.shape)

        def load_frames():
            single.load_frames(frame)
        med_c, lo_c, hi_c = timed(cpu_pipeline, a.calls, a.warmup)
        ref = single.x.clone()
        med_d, lo_d, hi_d = timed(load_frames, a.calls, a.warmup)
        err = float((single.x - ref).abs().max())
        report(path="frames_cpu_pipeline", batch=1, frame=[fh, fw], ms_median=round(med_c, 3), ms_min=round(lo_c, 3), ms_max=round(hi_c, 3),
               predictor_replay_ms=round(figures["predictor_replay"], 3))
        report(path="frames_load_frames", batch=1, frame=[fh, fw], ms_median=round(med_d, 3), ms_min=round(lo_d, 3), ms_max=round(hi_d, 3),
               predictor_replay_ms=round(figures["predictor_replay"], 3), max_abs_diff_vs_cpu_pipeline=err)

    # ---- three expressions of one image
    def three_replays():
        for j in range(S):
            single.l.copy_(l3[j:j + 1])
            single.m.copy_(m3[j:j + 1])
            single.step()
            single.iu.tolist()
    med, lo, hi = timed(three_replays, a.calls, a.warmup)
    report(path="predictor_replay", batch=1, expressions=S, note="three batch-1 replays", ms_median=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3))
    p3 = Predictor(model, x, l3, m3, target=tgt.expand(S, -1, -1).contiguous(), expressions_per_image=S, context=ops.StepContext())
    p3.warmup_and_capture()

    def one_replay():
        p3.step()
        return p3.iu.tolist()
    med, lo, hi = timed(one_replay, a.calls, a.warmup)
    report(path="predictor_replay", batch=1, expressions=S, note="one expressions_per_image=3 replay", captured=p3.captured, ms_median=round(med, 3), ms_min=round(lo, 3),
           ms_max=round(hi, 3))

    # ---- decoder launches per call, before / after folding
    with torch.no_grad():
        feats = model.backbone(x, l1, m1)

        def count(fn):
            K.prof.start()
            try:
                fn()
            finally:
                rec = K.prof.stop()
            names = [r[0] for r in rec if r[1] == "decoder"]
            return len(names), sum(r[3] for r in rec if r[1] == "decoder")
        n0, us0 = count(lambda: model.classifier(feats[3], feats[2], feats[1], feats[0]))
        n1, us1 = count(lambda: model.classifier.forward_folded(feats[3], feats[2], feats[1], feats[0]))
    report(path="decoder_launches", batch=1, unfolded=n0, folded=n1, unfolded_kernel_us=round(us0, 1), folded_kernel_us=round(us1, 1))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
