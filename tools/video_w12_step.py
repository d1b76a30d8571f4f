"""The Video-Swin-B LAVT training step of bench.py's `video_swin_b_t8_384` workload (one clip of T = 8 frames at 384^2, PWAM, decoder, weighted CE),
but with window (8, 12, 12) (`lavt_video(..., window12=True)`): its 1152-token windows run on the streaming attention kernels, or with
LAVT_ATTN_COMPOSED=1 on the composed route.  Times the captured TrainStep on both routes (each in a fresh child process) and prints one bench-style
JSON line per route: ms/clip, frames/s, peak memory.

    python tools/video_w12_step.py [--steps 10] [--warmup 3]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "lavt-rs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)




def build(device):
    import torch
    from types import SimpleNamespace
    from lavt_hip.detweights import fill_state_dict_
    from lib.mask_predictor import SimpleDecoding
    from lib.video_swin_transformer import MultiModalSwinTransformer3D

    class VideoStep(torch.nn.Module):
        def __init__(self, backbone, classifier):
            super().__init__()
            self.backbone, self.classifier = backbone, classifier

        def forward_lowres(self, x, l, m):
            f = self.backbone(x.permute(0, 2, 1, 3, 4), l, m)
            return self.classifier(f[3], f[2], f[1], f[0])

        def forward(self, x, l, m):
            from lib._utils import _upsample_logits
            return _upsample_logits(self.forward_lowres(x, l, m), x.shape[-2:])
    a = SimpleNamespace()
    bb = MultiModalSwinTransformer3D(patch_size=(1, 4, 4), embed_dim=128, depths=[2, 2, 18, 2], num_heads=[4, 8, 16, 32], window_size=(8, 12, 12),
                                     drop_path_rate=0.3, patch_norm=True, out_indices=(0, 1, 2, 3), num_heads_fusion=[1, 1, 1, 1], args=a)
    model = VideoStep(bb, SimpleDecoding(1024, a))
    fill_state_dict_(model)
    return model.to(device)


def child(route, steps, warmup):
    import torch
    import lavt_hip
    from lavt_hip.detweights import det_inputs
    from lavt_hip.engine import TrainStep
    from lavt_hip.optim import FusedAdamW
    dev = torch.device("cuda:0")
    lavt_hip.set_compute_dtype(torch.bfloat16)
    model = build(dev).train()
    x, l, m, t = det_inputs(1, 384, 20, seed=1234, frames=8)
    step = TrainStep(model, x.to(dev), l.to(dev), m.to(dev), t.to(dev), use_graph=True)
    step.warmup_and_capture()
    opt = FusedAdamW(model.parameters(), lr=1e-5, weight_decay=0.01)
    for _ in range(warmup):
        step.step()
        opt.step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        step.step()
        opt.step()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    print(json.dumps({"workload": "video_swin_b_t8_384_w12", "route": route, "captured": bool(step.captured), "ms_per_clip": round(ms, 2),
                      "frames_per_s": round(8 * 1e3 / ms, 2), "loss": round(float(step.loss), 5),
                      "peak_mem_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2), "steps": steps}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--route", choices=["stream", "composed"], default=None, help="(internal) run one route in this process")
    a = ap.parse_args()
    if a.route:
        child(a.route, a.steps, a.warmup)
        return
    rc = 0
    for route in ("stream", "composed"):
        env = dict(os.environ)
        env.pop("LAVT_ATTN_COMPOSED", None)
        if route == "composed":
            env["LAVT_ATTN_COMPOSED"] = "1"
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--route", route, "--steps", str(a.steps), "--warmup", str(a.warmup)], env=env)
        rc = rc or r.returncode
        if r.returncode != 0:
            break
    sys.exit(rc)


if __name__ == "__main__":
    main()
