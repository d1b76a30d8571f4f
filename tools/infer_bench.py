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
  frames_load_frames    Predictor.load_frames: the uint8 upload (pinned staging) + the resize / normalise kernel into the same buffer

    --video-select IND   (opt-in, runs ONLY this) annotated-frame selection on the geometry of `bench.py --workload video_swin_b_t8_384` (Video-Swin-B, one clip
                         of T = 8 frames at 384^2, batch 1; A2D-Sentences / JHMDB annotate one frame per clip), two captured predictors in one process:
  video_all_frames_then_index   the all-frame Predictor replay followed by mask[sel] / iu[sel] (what a caller does without selection)
  video_valid_indices           Predictor(valid_indices=[IND]): the decoder and the mask kernel run on the one annotated frame

    --pairs N   (opt-in, runs ONLY this) N (image, expression) pairs over ceil(N / 3) images, on the Swin-B w12 480^2 bf16 workload above.  Both figures
                are milliseconds PER PAIR, the median over --calls repetitions of the whole loop (host wall clock, a synchronise on both sides):
  pairs_batch1_eval_meter       N batch-1 replays, each followed by EvalMeter.update(pred.iu) -- the evaluation loop as it stands: one device-to-host
                                read per prediction
  pairs_image_of_device_meter   ONE replay of Predictor(image_of=) with the DeviceEvalMeter appended to its body, and a single meter.read() at the end

    --text-encoder   (opt-in, runs ONLY this) lavt's separate BERT inside the prediction, on the --pairs 12 geometry (12 expressions over 4 images, one
                     image_of replay) with a bert-base encoder (random init) on 20 tokens.  Milliseconds per CALL, median over --calls device-synchronised
                     calls; the four regions alternate call by call; ms_p10 / ms_p90 / ms_min / ms_max give the spread; launches_eager_body is the K.prof
                     launch count of one eager body (for the first region: the eager encoder's launches plus the body's):
  text_eager_then_replay                         the evaluation loop as it stands: enc(ids, mask) eagerly, two copies, the image_of replay
  text_in_predictor                              Predictor(text_encoder=) replay
  text_in_predictor_fused_attention              ... with enc.fused_attention
  text_in_predictor_fused_attention_embeddings   ... and enc.fused_embeddings

    --jf   (opt-in, runs ONLY this) the J&F measure on the device.  MICROSECONDS per call from device events, median over --calls with p10 / p90 / min / max,
           the regions of a comparison alternating call by call:
  jf_boundary_counts        ops.boundary_counts alone (int64 target) at 8 x 384x384 (r = 5), 8 x 480x854 (r = 8), 36 x 720x1280 (r = 12), for object-like
                            masks (one ellipse per frame) and for pixel noise (every pixel a boundary pixel); bytes_read = n*H*W*9 and the rate it implies;
                            us_in_graph_* = the same call ten times in one captured graph, per call (no host enqueue cost between the three kernels)
  jf_torch_composition      the same counts from torch ops on the same GPU: boundary maps by slicing, F.conv2d with the disk as the weight, > 0
  jf_replay_without_meter   the Video-Swin-B replay (T = 8, 384^2, masks at 720x1280 through via_size) as a predictor without the meter launches it
  jf_replay_with_jf_meter   the same predictor with make_jf_meter()"""
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


def video_select(a, report):
    import lavt_hip
    from lavt_hip import ops
    from lavt_hip.detweights import det_inputs, fill_state_dict_
    from lavt_hip.engine import Predictor
    from lib._utils import LAVTVideo
    from lib.mask_predictor import SimpleDecoding
    from lib.video_swin_transformer import MultiModalSwinTransformer3D
    dev, T, size, ind = "cuda:0", 8, 384, int(a.video_select)
    if not 0 <= ind < T:
        raise SystemExit(f"--video-select: the annotated frame must lie in [0, {T})")
    lavt_hip.set_compute_dtype(torch.bfloat16 if a.dtype == "bf16" else torch.float32)
    args = SimpleNamespace()
    bb = MultiModalSwinTransformer3D(patch_size=(1, 4, 4), embed_dim=128, depths=[2, 2, 18, 2], num_heads=[4, 8, 16, 32], window_size=(8, 7, 7),
                                     drop_path_rate=0.3, patch_norm=True, out_indices=(0, 1, 2, 3), num_heads_fusion=[1, 1, 1, 1], args=args)
    parts = torch.nn.ModuleDict({"backbone": bb, "classifier": SimpleDecoding(1024, args)})
    fill_state_dict_(parts)
    parts.to(dev)
    clip, l, m, tgt = det_inputs(1, size, 20, seed=1234, frames=T)
    clip, l, m, tgt = clip.to(dev), l.to(dev), m.to(dev), tgt.to(dev)

    class _Text(torch.nn.Module):          # language features are the input, as for bench.py's video workload: BERT is outside the comparison
        def forward(self, ids, attention_mask=None):
            return (l.permute(0, 2, 1),)

    model = LAVTVideo.__new__(LAVTVideo)
    torch.nn.Module.__init__(model)
    model.backbone, model.classifier, model.text_encoder = parts["backbone"], parts["classifier"], _Text()
    model.lazy_pred, model.seg_last = False, False
    model.eval()
    ids, am = torch.zeros(1, 20, dtype=torch.long, device=dev), m.squeeze(-1).contiguous()
    sel = torch.tensor([ind], device=dev)
    p_all = Predictor(model, clip, ids, am, target=tgt, context=ops.StepContext())
    p_all.warmup_and_capture()
    p_sel = Predictor(model, clip, ids, am, target=tgt[sel].contiguous(), valid_indices=sel.int(), context=ops.StepContext())
    p_sel.warmup_and_capture()

    def all_then_index():
        p_all.step()
        return p_all.mask[sel], p_all.iu[sel].tolist()

    def selected():
        p_sel.step()
        return p_sel.mask, p_sel.iu.tolist()
    med_a, lo_a, hi_a = timed(all_then_index, a.calls, a.warmup)
    med_s, lo_s, hi_s = timed(selected, a.calls, a.warmup)
    (mask_a, iu_a), (mask_s, iu_s) = all_then_index(), selected()
    differ = int((mask_a != mask_s).sum())
    common = dict(variant="video_swin_b", size=size, frames=T, batch=1, annotated_frame=ind)
    report(path="video_all_frames_then_index", captured=p_all.captured, ms_median=round(med_a, 3), ms_min=round(lo_a, 3), ms_max=round(hi_a, 3), iu=iu_a[0], **common)
    report(path="video_valid_indices", captured=p_sel.captured, ms_median=round(med_s, 3), ms_min=round(lo_s, 3), ms_max=round(hi_s, 3), iu=iu_s[0],
           mask_pixels_differing_from_all_frames=differ, speedup=round(med_a / med_s, 3), **common)


def pairs(a, report):
    import lavt_hip
    from lavt_hip import ops
    from lavt_hip.detweights import det_inputs, fill_state_dict_
    from lavt_hip.engine import Predictor
    from lavt_hip.metrics import EvalMeter
    from lib import segmentation
    dev, N = "cuda:0", int(a.pairs)
    if N < 1:
        raise SystemExit("--pairs: at least one pair")
    B = (N + 2) // 3
    image_of = [j // 3 for j in range(N)]
    lavt_hip.set_compute_dtype(torch.bfloat16 if a.dtype == "bf16" else torch.float32)
    model = segmentation.lavt("", SimpleNamespace(swin_type=a.variant, window12=a.variant == "base", drop_path_rate=0.3))
    fill_state_dict_(model)
    model.to(dev).eval()
    x = det_inputs(B, a.size, 20, seed=1234)[0].to(dev)
    _, l, m, tgt = (t.to(dev) for t in det_inputs(N, a.size, 20, seed=77))
    single = Predictor(model, x[:1].clone(), l[:1].clone(), m[:1].clone(), target=tgt[:1].clone(), context=ops.StepContext())
    single.warmup_and_capture()
    host = EvalMeter()

    def batch1():
        host.reset()
        for j in range(N):
            single.x.copy_(x[image_of[j]:image_of[j] + 1])
            single.l.copy_(l[j:j + 1])
            single.m.copy_(m[j:j + 1])
            single.t.copy_(tgt[j:j + 1])
            single.step()
            host.update(single.iu)
        return host.summary()
    med_a, lo_a, hi_a = timed(batch1, a.calls, a.warmup)
    want = batch1()
    paired = Predictor(model, x.clone(), l.clone(), m.clone(), target=tgt.clone(), image_of=torch.tensor(image_of, dtype=torch.int32, device=dev),
                       context=ops.StepContext())
    meter = paired.make_meter(capacity=N)
    paired.warmup_and_capture()

    def one_replay():          # (both loops fill their static buffers from the same device tensors: the input stage is not what is compared)
        meter.reset()
        paired.x.copy_(x)
        paired.l.copy_(l)
        paired.m.copy_(m)
        paired.t.copy_(tgt)
        paired.set_image_of(image_of)
        paired.step()
        return meter.read().summary()
    med_b, lo_b, hi_b = timed(one_replay, a.calls, a.warmup)
    got = one_replay()
    common = dict(pairs=N, images=B, batch=1)
    report(path="pairs_batch1_eval_meter", captured=single.captured, ms_per_pair_median=round(med_a / N, 4), ms_per_pair_min=round(lo_a / N, 4),
           ms_per_pair_max=round(hi_a / N, 4), overall_iou=round(want["overall_iou"], 4), **common)
    report(path="pairs_image_of_device_meter", captured=paired.captured, ms_per_pair_median=round(med_b / N, 4), ms_per_pair_min=round(lo_b / N, 4),
           ms_per_pair_max=round(hi_b / N, 4), overall_iou=round(got["overall_iou"], 4), speedup=round(med_a / med_b, 3), **common)


def text_encoder(a, report):
    import lavt_hip
    from bert.modeling_bert import BertConfig, BertModel
    from lavt_hip import _capi as K
    from lavt_hip import ops
    from lavt_hip.detweights import det_inputs
    from lavt_hip.detweights import fill_state_dict_
    from lavt_hip.engine import Predictor
    from lib import segmentation
    dev, N, B, n_l = "cuda:0", 12, 4, 20
    image_of = [j // 3 for j in range(N)]
    lavt_hip.set_compute_dtype(torch.bfloat16 if a.dtype == "bf16" else torch.float32)
    model = segmentation.lavt("", SimpleNamespace(swin_type=a.variant, window12=a.variant == "base", drop_path_rate=0.3))
    fill_state_dict_(model)
    model.to(dev).eval()
    torch.manual_seed(1234)
    enc = BertModel(BertConfig()).to(dev).eval()          # bert-base geometry, random init
    enc.pooler = None
    x = det_inputs(B, a.size, n_l, seed=1234)[0].to(dev)
    _, _, m, tgt = (t.to(dev) for t in det_inputs(N, a.size, n_l, seed=77))
    mask = m.squeeze(-1).long().contiguous()
    ids = (torch.randint(1, enc.config.vocab_size, mask.shape, generator=torch.Generator().manual_seed(77)).to(dev) * mask).contiguous()
    io = torch.tensor(image_of, dtype=torch.int32, device=dev)

    def features():
        with torch.no_grad():
            return enc(ids, attention_mask=mask)[0].permute(0, 2, 1).contiguous(), mask.unsqueeze(-1).contiguous()
    enc.fused_attention = enc.fused_embeddings = False
    l0, m0 = features()
    outer = Predictor(model, x.clone(), l0.clone(), m0.clone(), target=tgt.clone(), image_of=io.clone(), context=ops.StepContext())
    outer.warmup_and_capture()

    def today():          # test.py:60-83 on this stack: the encoder eagerly in front of every replay, its output copied into the static buffers
        enc.fused_attention = enc.fused_embeddings = False
        l, mm = features()
        outer.l.copy_(l)
        outer.m.copy_(mm)
        outer.step()
    regions, launches, captured = [("text_eager_then_replay", today)], {}, {"text_eager_then_replay": outer.captured}
    for name, fa, fe in (("text_in_predictor", False, False), ("text_in_predictor_fused_attention", True, False),
                         ("text_in_predictor_fused_attention_embeddings", True, True)):
        enc.fused_attention, enc.fused_embeddings = fa, fe          # read at capture: the graph keeps the route it was captured with
        p = Predictor(model, x.clone(), ids.clone(), mask.clone(), target=tgt.clone(), image_of=io.clone(), text_encoder=enc, context=ops.StepContext())
        p.warmup_and_capture()
        captured[name] = p.captured
        with ops.use_context(p.context):
            K.prof.start()
            try:
                p._body()
            finally:
                launches[name] = len(K.prof.stop())
        regions.append((name, p.step))
    enc.fused_attention = enc.fused_embeddings = False
    K.prof.start()
    try:
        features()
    finally:
        n_text = len(K.prof.stop())
    with ops.use_context(outer.context):
        K.prof.start()
        try:
            outer._body()
        finally:
            launches["text_eager_then_replay"] = n_text + len(K.prof.stop())
    for _ in range(a.warmup):
        for _, fn in regions:
            fn()
    ts = {name: [] for name, _ in regions}
    for _ in range(a.calls):          # the regions alternate: drift of the machine lands on all of them alike
        for name, fn in regions:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[name].append((time.perf_counter() - t0) * 1e3)
    base = statistics.median(ts["text_eager_then_replay"])
    for name, _ in regions:
        v = sorted(ts[name])
        report(path=name, pairs=N, images=B, tokens=n_l, captured=captured[name], ms_median=round(statistics.median(v), 3), ms_min=round(v[0], 3),
               ms_max=round(v[-1], 3), ms_p10=round(v[len(v) // 10], 3), ms_p90=round(v[(9 * len(v)) // 10], 3), launches_eager_body=launches[name],
               text_launches_eager=n_text if name == "text_eager_then_replay" else None, speedup=round(base / statistics.median(v), 4))


def jf(a, report):
    """--jf: (1) lavt_boundary_counts alone against a torch composition and the bytes it must read, (2) the Video-Swin-B replay with and without the
    J&F meter.  Device-event times per call, the regions alternating call by call."""
    import torch.nn.functional as F
    import lavt_hip
    from lavt_hip import ops
    from lavt_hip.detweights import det_inputs, fill_state_dict_
    from lavt_hip.engine import Predictor
    from lavt_hip.metrics import davis_bound_pix
    from lib._utils import LAVTVideo
    from lib.mask_predictor import SimpleDecoding
    from lib.video_swin_transformer import MultiModalSwinTransformer3D
    dev = "cuda:0"

    def masks(n, H, W, kind, seed):
        g = torch.Generator("cpu").manual_seed(seed)
        if kind == "noise":          # every pixel a boundary pixel: the worst case of the boundary pass
            return (torch.rand(n, H, W, generator=g) < 0.5).to(torch.uint8)
        yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")          # "object": one ellipse per frame, drifting
        out = torch.zeros(n, H, W, dtype=torch.uint8)
        for k in range(n):
            cy, cx, ry, rx = (torch.rand(4, generator=g) * torch.tensor([H / 2, W / 2, H / 4, W / 4]) + torch.tensor([H / 4, W / 4, H / 8, W / 8])).tolist()
            out[k] = (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0).to(torch.uint8)
        return out

    def torch_counts(P, G, r):          # boundary maps by slicing, the disk as a convolution weight
        d = torch.arange(-r, r + 1, device=dev)
        w = ((d[:, None] ** 2 + d[None, :] ** 2) <= r * r).float()[None, None]

        def bmap(S):
            S = S != 0
            e, s, se = S.clone(), S.clone(), S.clone()          # (the last row / column compare with themselves: the toolkit's overwrite)
            e[:, :, :-1] = S[:, :, 1:]
            s[:, :-1, :] = S[:, 1:, :]
            se[:, :-1, :-1] = S[:, 1:, 1:]
            se[:, -1, :-1] = S[:, -1, 1:]
            se[:, :-1, -1] = S[:, 1:, -1]
            return (S ^ e) | (S ^ s) | (S ^ se)
        bp, bg = bmap(P), bmap(G)
        dp = F.conv2d(bp[:, None].float(), w, padding=r)[:, 0] > 0
        dg = F.conv2d(bg[:, None].float(), w, padding=r)[:, 0] > 0
        Pb, Gb = P != 0, G != 0
        cols = [Pb & Gb, Pb | Gb, bp, bg, bp & dg, bg & dp]
        return torch.stack([c.flatten(1).sum(1) for c in cols], 1).int()

    def alternate(fns, calls, warmup):
        for _ in range(warmup):
            for fn in fns.values():
                fn()
        ts = {k: [] for k in fns}
        for _ in range(calls):
            for k, fn in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ts[k].append(e0.elapsed_time(e1) * 1e3)
        return {k: sorted(v) for k, v in ts.items()}

    def spread(v):
        return dict(us_median=round(statistics.median(v), 2), us_p10=round(v[len(v) // 10], 2), us_p90=round(v[(9 * len(v)) // 10], 2), us_min=round(v[0], 2),
                    us_max=round(v[-1], 2))

    for n, H, W in ((8, 384, 384), (8, 480, 854), (36, 720, 1280)):
        r = davis_bound_pix(H, W)
        for kind in ("object", "noise"):
            P, G = masks(n, H, W, kind, 1).to(dev), masks(n, H, W, kind, 2).to(dev).long()
            out = torch.empty(n, 8, dtype=torch.int32, device=dev)
            got, want = ops.boundary_counts(P, G, r, out=out).clone(), torch_counts(P, G, r)
            ts = alternate({"hip": lambda: ops.boundary_counts(P, G, r, out=out), "torch": lambda: torch_counts(P, G, r)}, a.calls, a.warmup)
            nbytes = n * H * W * 9
            med = statistics.median(ts["hip"])
            # the same call ten times in one captured graph: the three kernels without the host's enqueue cost, which an eager call of this size is bound by
            g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                ops.boundary_counts(P, G, r, out=out)
            torch.cuda.current_stream().wait_stream(side)
            with torch.cuda.graph(g):
                for _ in range(10):
                    ops.boundary_counts(P, G, r, out=out)
            tg = alternate({"graph": g.replay}, a.calls, a.warmup)["graph"]
            in_graph = statistics.median(tg) / 10.0
            report(path="jf_boundary_counts", frames=n, H=H, W=W, bound_pix=r, masks=kind, equal_to_torch=bool(torch.equal(got[:, :6], want)), bytes_read=nbytes,
                   gb_per_s=round(nbytes / med / 1e3, 1), us_in_graph_median=round(in_graph, 2), us_in_graph_p10=round(tg[len(tg) // 10] / 10.0, 2),
                   us_in_graph_p90=round(tg[(9 * len(tg)) // 10] / 10.0, 2), gb_per_s_in_graph=round(nbytes / in_graph / 1e3, 1), **spread(ts["hip"]))
            report(path="jf_torch_composition", frames=n, H=H, W=W, bound_pix=r, masks=kind, speedup_of_hip=round(statistics.median(ts["torch"]) / med, 2),
                   **spread(ts["torch"]))
            del P, G
    # ---- the replay: Video-Swin-B, one clip of T = 8 frames at 384^2, masks at 720 x 1280 through via_size (test_ytvos.py:249-253)
    T, size, out_size = 8, 384, (720, 1280)
    lavt_hip.set_compute_dtype(torch.bfloat16 if a.dtype == "bf16" else torch.float32)
    args = SimpleNamespace()
    bb = MultiModalSwinTransformer3D(patch_size=(1, 4, 4), embed_dim=128, depths=[2, 2, 18, 2], num_heads=[4, 8, 16, 32], window_size=(8, 7, 7),
                                     drop_path_rate=0.3, patch_norm=True, out_indices=(0, 1, 2, 3), num_heads_fusion=[1, 1, 1, 1], args=args)
    parts = torch.nn.ModuleDict({"backbone": bb, "classifier": SimpleDecoding(1024, args)})
    fill_state_dict_(parts)
    parts.to(dev)
    clip, l, m, _ = det_inputs(1, size, 20, seed=1234, frames=T)
    clip, l, m = clip.to(dev), l.to(dev), m.to(dev)
    tgt = masks(T, out_size[0], out_size[1], "object", 3).to(dev).long()

    class _Text(torch.nn.Module):
        def forward(self, ids, attention_mask=None):
            return (l.permute(0, 2, 1),)

    model = LAVTVideo.__new__(LAVTVideo)
    torch.nn.Module.__init__(model)
    model.backbone, model.classifier, model.text_encoder = parts["backbone"], parts["classifier"], _Text()
    model.lazy_pred, model.seg_last = False, False
    model.eval()
    ids, am = torch.zeros(1, 20, dtype=torch.long, device=dev), m.squeeze(-1).contiguous()
    plain = Predictor(model, clip, ids, am, target=tgt, out_size=out_size, via_size=(size, size), context=ops.StepContext())
    plain.warmup_and_capture()
    with_jf = Predictor(model, clip, ids, am, target=tgt, out_size=out_size, via_size=(size, size), context=ops.StepContext())
    meter = with_jf.make_jf_meter(capacity=64)
    with_jf.warmup_and_capture()
    ts = alternate({"plain": plain.step, "jf": with_jf.step}, a.calls, a.warmup)
    s = meter.read().summary()
    common = dict(variant="video_swin_b", size=size, frames=T, out_size=list(out_size), bound_pix=davis_bound_pix(*out_size))
    report(path="jf_replay_without_meter", captured=plain.captured, **spread(ts["plain"]), **common)
    report(path="jf_replay_with_jf_meter", captured=with_jf.captured, masks_equal=bool(torch.equal(plain.mask, with_jf.mask)),
           added_us_median=round(statistics.median(ts["jf"]) - statistics.median(ts["plain"]), 2), J=round(s["J"], 4), F=round(s["F"], 4), **spread(ts["jf"]), **common)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", type=int, default=480)
    ap.add_argument("--variant", default="base", choices=["base", "tiny"])
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--frames-u8", default=None, metavar="HxW", help="also time the input stage for a uint8 frame of this size: CPU pipeline vs Predictor.load_frames")
    ap.add_argument("--video-select", default=None, metavar="IND", help="run ONLY the annotated-frame comparison on Video-Swin-B, T=8, 384^2: all frames + index vs valid_indices=[IND]")
    ap.add_argument("--pairs", type=int, default=None, metavar="N", help="run ONLY the pair-list comparison: N batch-1 replays + EvalMeter.update vs one image_of replay + device meter")
    ap.add_argument("--text-encoder", action="store_true", help="run ONLY the text-stage comparison: eager BERT in front of an image_of replay vs Predictor(text_encoder=)")
    ap.add_argument("--jf", action="store_true", help="run ONLY the J&F figures: lavt_boundary_counts against a torch composition, and the video replay with / without the J&F meter")
    a = ap.parse_args()
    if a.calls < 20:
        ap.error("--calls must be at least 20")
    if a.jf:
        lines = []

        def report_jf(**kw):
            kw.update(dtype=a.dtype, calls=a.calls)
            lines.append(json.dumps(kw))
            print(lines[-1], flush=True)
        jf(a, report_jf)
        if a.out:
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n")
        return
    if a.text_encoder:
        lines = []

        def report_text(**kw):
            kw.update(variant=a.variant, size=a.size, dtype=a.dtype, calls=a.calls)
            lines.append(json.dumps(kw))
            print(lines[-1], flush=True)
        text_encoder(a, report_text)
        if a.out:
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n")
        return
    if a.pairs is not None:
        lines = []

        def report_pairs(**kw):
            kw.update(variant=a.variant, size=a.size, dtype=a.dtype, calls=a.calls)
            lines.append(json.dumps(kw))
            print(lines[-1], flush=True)
        pairs(a, report_pairs)
        if a.out:
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n")
        return
    if a.video_select is not None:
        lines = []

        def report_video(**kw):
            kw.update(dtype=a.dtype, calls=a.calls)
            lines.append(json.dumps(kw))
            print(lines[-1], flush=True)
        video_select(a, report_video)
        if a.out:
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n")
        return
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
