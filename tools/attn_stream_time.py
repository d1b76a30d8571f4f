"""Times the window-attention core of the four Video-Swin-B --window12 layer shapes (T = 8, 384^2, batch 1, window (8, 12, 12) = 1152 tokens) on the
streaming route (csrc/attention_stream.hip) and on the composed route (GEMM -> softmax -> GEMM, LAVT_ATTN_COMPOSED=1), bf16, unshifted and shifted.
Forward and forward + backward, HIP events around `--iters` calls after `--warmup`; one JSON line per (stage, shift): microseconds, algorithmic TFLOP/s
(4 N^2 32 forward, 10 N^2 32 backward per window-head) and the torch.cuda.max_memory_allocated rise of one forward + backward over the inputs.

    python tools/attn_stream_time.py [--iters 20] [--warmup 5]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "lavt-rs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

# (stage, windows, heads): Video-Swin-B at T = 8, 384^2 -> 96^2 / 48^2 / 24^2 / 12^2 tokens per frame, 8 frames
STAGES = [(0, 64, 4), (1, 16, 8), (2, 4, 16), (3, 1, 32)]
W12, N = (8, 12, 12), 1152


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    from lavt_hip import ops, rowmaps
    dev = torch.device("cuda:0")
    for stage, nwin, heads in STAGES:
        C = 32 * heads
        side = 12 * int(round(nwin ** 0.5))
        for shifted in (0, 1):
            region = None
            if shifted and side > 12:
                region = torch.from_numpy(rowmaps.region_ids3d_np(8, side, side, W12, (0, 6, 6))).to(dev)
            qkv = (torch.randn(nwin * N, 3 * C, device=dev) * 0.5).to(torch.bfloat16).requires_grad_(True)
            table = (torch.randn(15 * 23 * 23, heads, device=dev) * 0.5).requires_grad_(True)
            go = torch.randn(nwin * N, C, device=dev).to(torch.bfloat16)
            rec = {"stage": stage, "windows": nwin, "heads": heads, "N": N, "shifted": bool(region is not None)}
            for route in ("stream", "composed"):
                if route == "composed":
                    os.environ["LAVT_ATTN_COMPOSED"] = "1"
                else:
                    os.environ.pop("LAVT_ATTN_COMPOSED", None)

                def fwd():
                    with torch.no_grad():
                        ops.window_attention(qkv, table, region, W12, heads, N=N)

                def fwdbwd():
                    y = ops.window_attention(qkv, table, region, W12, heads, N=N)
                    torch.autograd.grad(y, (qkv, table), go)
                tf = timed(fwd, a.iters, a.warmup)
                tb = timed(fwdbwd, a.iters, a.warmup)
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                fwdbwd()
                torch.cuda.synchronize()
                peak = torch.cuda.max_memory_allocated() - base
                wh = nwin * heads
                rec[route] = {"fwd_us": round(tf, 1), "fwd_bwd_us": round(tb, 1),
                              "fwd_tflops": round(4.0 * wh * N * N * 32 / tf / 1e6, 2),
                              "fwd_bwd_tflops": round(14.0 * wh * N * N * 32 / tb / 1e6, 2),
                              "peak_mem_mb": round(peak / 2 ** 20, 1)}
            os.environ.pop("LAVT_ATTN_COMPOSED", None)
            rec["fwd_bwd_speedup"] = round(rec["composed"]["fwd_bwd_us"] / rec["stream"]["fwd_bwd_us"], 2)
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
