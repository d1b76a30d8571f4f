"""GPU checks of annotated-frame selection (A2D-Sentences / JHMDB: one annotated frame per clip; train.py:282-285, 366-369 and test.py:182-205 of
the reference select with `index_select(output, 0, valid_indices)` before they score).

Kernels: lavt_upsample_{ce,dice}_sel_{fwd,bwd} and lavt_gather_samples against torch on the CPU (F.interpolate -> index_select -> the oracle's
criterion -> autograd) with the tolerances of test_upsample_cross_entropy / test_upsample_dice_golden, and against the existing un-selected op on
the explicitly gathered rows.  Harnesses: engine.TrainStep(valid_indices=, loss=) against plain autograd on a twin model, engine.Predictor
(valid_indices=) against the reference's eval logits (video_forward_feats fixture).  No bound below is taken from what the code gives."""
import functools
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from lavt_hip.detweights import det_inputs, fill_state_dict_

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = [torch.float32, torch.bfloat16]
# (B, sel, Hi, Wi, Ho, Wo): unsorted selection + ragged 8x8 tiles (tile backward); a permutation of all frames; a 16x upsample (the tile's full-resolution
# region exceeds LDS: wave-per-pixel backward); the identity upsample
CASES = {
    "unsorted_ragged": (5, (3, 1), 7, 9, 28, 36),
    "permutation": (3, (2, 0, 1), 13, 11, 52, 44),
    "wave_per_pixel": (4, (2,), 5, 6, 80, 96),
    "identity": (3, (0, 2), 13, 11, 13, 11),
}


SCALE = {"ce": 3.0, "dice": 1.0}


@pytest.fixture(autouse=True)
def _fp32():
    import lavt_hip
    lavt_hip.set_compute_dtype(torch.float32)
    yield
    lavt_hip.set_compute_dtype(torch.float32)


@functools.lru_cache(maxsize=None)
def _reference(case, crit, dtype):
    """torch on the CPU, computed once per (case, criterion, input rounding) and never modified: inputs, loss, d (k loss) / d x over ALL frames
    (k = 3 for the cross-entropy, as in test_upsample_cross_entropy; 1 for Dice, whose gradient gate is absolute), I, U"""
    from oracle import lavt_oracle as O
    B, sel, Hi, Wi, Ho, Wo = CASES[case]
    g = torch.Generator().manual_seed(5 + len(case))
    x = torch.randn(B * Hi * Wi, 2, generator=g) * (1.0 if crit == "ce" else 2.0)
    tgt = torch.randint(0, 2, (len(sel), Ho, Wo), generator=g)
    if crit == "ce" and case == "unsorted_ragged":
        tgt[0, :2, :3] = -100                                 # F.cross_entropy's ignore value
        tgt[1, 5, 7:11] = -100
    if crit == "dice" and len(sel) > 1:
        tgt[len(sel) - 1] = 0                                 # a sample without foreground: I1 = 0
    if dtype == torch.bfloat16:
        x = x.to(dtype).float()                               # both sides start from the same bf16-representable logits
    xr = x.clone().requires_grad_(True)
    up = F.interpolate(xr.view(B, Hi, Wi, 2).permute(0, 3, 1, 2), size=(Ho, Wo), mode="bilinear", align_corners=True)
    picked = torch.index_select(up, 0, torch.tensor(sel))
    loss = O.weighted_ce(picked, tgt) if crit == "ce" else O.multiclass_dice(picked, tgt)
    (SCALE[crit] * loss).backward()
    pred = picked.argmax(1)
    I, U = int(((pred == 1) & (tgt == 1)).sum()), int(((pred == 1) | (tgt == 1)).sum())
    return x, tgt, float(loss.detach()), xr.grad.clone(), I, U


def _run(op, x, tgt, B, dims, dtype, sel=None, scale=3.0, **kw):
    xg = x.to(DEV).to(dtype).requires_grad_(True)
    loss, stats = op(xg, tgt.to(DEV), B, *dims, sel=sel, **kw) if sel is not None else op(xg, tgt.to(DEV), B, *dims, **kw)
    (scale * loss).backward()
    return float(loss.detach()), stats.float().cpu(), xg.grad.float().cpu()


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("case", list(CASES))
def test_upsample_cross_entropy_selected(case, dtype):
    """lavt_upsample_ce_sel_{fwd,bwd}: loss 2e-5 * max(1, |ref|), I / U within 2, gradient 1e-5 (fp32) / 1e-2 (bf16) of its maximum -- the gates of
    test_upsample_cross_entropy; the gradient of every unselected frame is exactly zero"""
    from lavt_hip import ops
    B, sel, Hi, Wi, Ho, Wo = CASES[case]
    x, tgt, ref, ref_grad, I, U = _reference(case, "ce", dtype)
    seld = torch.tensor(sel, dtype=torch.int32, device=DEV)
    loss, stats, grad = _run(ops.upsample_cross_entropy, x, tgt, B, (Hi, Wi, Ho, Wo), dtype, sel=seld, weight=(0.9, 1.1))
    tol = 1e-5 if dtype == torch.float32 else 1e-2
    gerr = float((grad - ref_grad).abs().max()) / float(ref_grad.abs().max())
    print(f"\n[ce sel {case} {dtype}] loss {loss:.7f} ref {ref:.7f}  I/U {int(stats[2])}/{int(stats[3])} ref {I}/{U}  grad err / max {gerr:.3e}")
    assert abs(loss - ref) <= 2e-5 * max(1.0, abs(ref))
    valid = tgt[tgt >= 0]
    assert abs(float(stats[1]) - float(torch.tensor([0.9, 1.1])[valid].sum())) <= 1e-3 * float(stats[1])
    assert abs(int(stats[2]) - I) <= 2 and abs(int(stats[3]) - U) <= 2
    assert gerr <= tol, gerr
    rest = [b for b in range(B) if b not in sel]
    g3 = grad.view(B, Hi * Wi, 2)
    assert torch.equal(g3[rest], torch.zeros_like(g3[rest])), "unselected frames must receive exactly zero"
    if rest:
        assert float(ref_grad.view(B, -1)[rest].abs().max()) == 0.0
    # the existing un-selected op on the explicitly gathered rows
    xs = x.view(B, Hi * Wi, 2)[list(sel)].reshape(-1, 2)
    loss2, stats2, grad2 = _run(ops.upsample_cross_entropy, xs, tgt, len(sel), (Hi, Wi, Ho, Wo), dtype, weight=(0.9, 1.1))
    same = loss == loss2 and torch.equal(stats, stats2) and torch.equal(g3[list(sel)].reshape(-1, 2), grad2)
    print(f"[ce sel {case} {dtype}] against the un-selected op on gathered rows: {'bit-identical' if same else 'NOT bit-identical'}")
    assert abs(loss - loss2) <= 2e-5 * max(1.0, abs(ref))
    assert abs(float(stats[1]) - float(stats2[1])) <= 1e-3 * float(stats[1])
    assert abs(int(stats[2]) - int(stats2[2])) <= 2 and abs(int(stats[3]) - int(stats2[3])) <= 2
    assert float((g3[list(sel)].reshape(-1, 2) - grad2).abs().max()) <= tol * float(ref_grad.abs().max())


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("case", list(CASES))
def test_upsample_dice_selected(case, dtype):
    """lavt_upsample_dice_sel_{fwd,bwd}: loss 1e-5 (fp32) / 3e-3 (bf16), gradient 1e-6 absolute (fp32) / 2 % of its maximum (bf16) -- the gates of
    test_upsample_dice_golden; statistics per SELECTED sample; the gradient of every unselected frame is exactly zero"""
    from lavt_hip import ops
    B, sel, Hi, Wi, Ho, Wo = CASES[case]
    x, tgt, ref, ref_grad, _, _ = _reference(case, "dice", dtype)
    seld = torch.tensor(sel, dtype=torch.int32, device=DEV)
    loss, stats, grad = _run(ops.upsample_dice_loss, x, tgt, B, (Hi, Wi, Ho, Wo), dtype, sel=seld, scale=1.0)
    ltol = 1e-5 if dtype == torch.float32 else 3e-3
    gtol = 1e-6 if dtype == torch.float32 else 0.02 * float(ref_grad.abs().max())
    gerr = float((grad - ref_grad).abs().max())
    print(f"\n[dice sel {case} {dtype}] loss {loss:.7f} ref {ref:.7f}  grad err {gerr:.3e} (max |grad| {float(ref_grad.abs().max()):.3e}, gate {gtol:.3e})")
    assert abs(loss - ref) < ltol
    assert gerr <= gtol
    assert stats.numel() == 2 + 6 * len(sel)
    per = stats[2:].view(len(sel), 6)
    assert torch.equal(per[:, 5], (tgt == 1).flatten(1).sum(1).float()) and torch.equal(per[:, 4], (tgt == 0).flatten(1).sum(1).float())
    assert len(sel) == 1 or float(per[len(sel) - 1, 1]) == 0.0
    rest = [b for b in range(B) if b not in sel]
    g3 = grad.view(B, Hi * Wi, 2)
    assert torch.equal(g3[rest], torch.zeros_like(g3[rest])), "unselected frames must receive exactly zero"
    xs = x.view(B, Hi * Wi, 2)[list(sel)].reshape(-1, 2)
    loss2, stats2, grad2 = _run(ops.upsample_dice_loss, xs, tgt, len(sel), (Hi, Wi, Ho, Wo), dtype, scale=1.0)
    same = loss == loss2 and torch.equal(stats, stats2) and torch.equal(g3[list(sel)].reshape(-1, 2), grad2)
    print(f"[dice sel {case} {dtype}] against the un-selected op on gathered rows: {'bit-identical' if same else 'NOT bit-identical'}")
    assert abs(loss - loss2) < ltol
    assert float((g3[list(sel)].reshape(-1, 2) - grad2).abs().max()) <= gtol
    assert float((stats[2:] - stats2[2:]).abs().max()) <= ltol * float(stats2[2:].abs().max())


@pytest.mark.parametrize("B,sel,inner,dtype", [(6, (5, 0, 3), (2, 2, 256), torch.bfloat16), (4, (1, 3), (7, 9, 3), torch.float32)])
def test_gather_samples_equals_index_select(B, sel, inner, dtype):
    """whole samples, bit for bit; an NCHW-shaped view of NHWC memory goes in and comes out with the same strides.  2 x 2 x 256 bf16 = 2 KiB per sample:
    16-byte copies; 7 x 9 x 3 fp32 = 756 bytes: no multiple of 16, element copies"""
    from lavt_hip import ops
    x = torch.randn(B, *inner, generator=torch.Generator().manual_seed(3)).to(dtype).to(DEV).permute(0, 3, 1, 2)
    seld = torch.tensor(sel, dtype=torch.int32, device=DEV)
    y = ops.gather_samples(x, seld)
    assert y.shape == (len(sel),) + tuple(x.shape[1:]) and y.stride()[1:] == x.stride()[1:] and y.dtype == dtype
    assert y.permute(0, 2, 3, 1).is_contiguous(), "no layout change"
    assert torch.equal(y, torch.index_select(x, 0, seld.long()))
    with pytest.raises(ValueError):
        ops.gather_samples(x, seld.long())
    with pytest.raises(RuntimeError, match="GPU memory only"):
        ops.gather_samples(x, seld.cpu())


# ================================================================================================ harnesses on the micro Video-Swin
def _video_model(seed=1234):
    """the micro Video-Swin of test_predictor_video (embed 32, depths 2-2-2-2, window (8, 7, 7)), 2 clips x 4 frames x 64^2, the stub text encoder"""
    from lib._utils import LAVTVideo
    from lib.mask_predictor import SimpleDecoding
    from lib.video_swin_transformer import MultiModalSwinTransformer3D
    a = SimpleNamespace()
    bb = MultiModalSwinTransformer3D(patch_size=(1, 4, 4), embed_dim=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8], window_size=(8, 7, 7),
                                     drop_path_rate=0.0, patch_norm=True, out_indices=(0, 1, 2, 3), use_checkpoint=False,
                                     num_heads_fusion=[1, 1, 1, 1], fusion_drop=0.0, args=a)
    parts = torch.nn.ModuleDict({"backbone": bb, "classifier": SimpleDecoding(256, a)})
    fill_state_dict_(parts)
    parts.to(DEV)
    frames, l, m, tgt = det_inputs(2, 64, 22, seed=seed, frames=4)
    frames, l, m = frames.to(DEV), l.to(DEV), m.to(DEV)

    class _Text(torch.nn.Module):
        def forward(self, ids, attention_mask=None):
            return (l.permute(0, 2, 1),)

    model = LAVTVideo.__new__(LAVTVideo)
    torch.nn.Module.__init__(model)
    model.backbone, model.classifier, model.text_encoder = parts["backbone"], parts["classifier"], _Text()
    model.lazy_pred, model.seg_last = False, False
    ids, am = torch.zeros(2, 22, dtype=torch.long, device=DEV), m.squeeze(-1).contiguous()
    return model, frames, ids, am, tgt


# Biases of PWAM whose gradient is zero analytically: a constant added to every key leaves the word softmax unchanged, one added to every value is
# removed by the InstanceNorm behind W (the two that test_train_step_gradients_match_plain_autograd names), and f_query / W are themselves a 1x1
# convolution directly in front of an InstanceNorm, which removes a per-channel constant.  Both runs hold rounding noise there (1e-7 and below
# in fp32 against weight gradients of 1e-2), in different summation orders: a relative comparison of the two is meaningless.
ZERO_GRAD_BIASES = tuple(f"image_lang_att.{m}.0.bias" for m in ("f_key", "f_value", "f_query", "W"))


def test_train_step_selected_frames_match_plain_autograd():
    """TrainStep(valid_indices=[2, 5]) captured, fp32 compute, against `F.cross_entropy(index_select(model(x), 0, sel), t, weight).backward()` on an
    identically filled twin: the rule and numbers of test_train_step_gradients_match_plain_autograd's fused-loss case (relative L2 <= 3 % per
    parameter, no element further than 6 % of the parameter's scale, loss 2e-3) -- the bf16 numbers, kept for this fp32 run; the
    measured worst figure is printed.  Then the index buffer and the target change between replays: the graph reads the buffer."""
    from lavt_hip import ops
    from lavt_hip.engine import TrainStep
    w = torch.tensor([0.9, 1.1], device=DEV)
    ref_model, frames, ids, am, tgt = _video_model()
    ref_model.train()
    sel = torch.tensor([2, 5], device=DEV)
    t1 = tgt[[2, 5]].to(DEV)
    out = ref_model(frames, ids, am)
    assert tuple(out.shape) == (8, 2, 64, 64)
    loss_ref = F.cross_entropy(torch.index_select(out, 0, sel), t1, weight=w)
    loss_ref.backward()
    ref = {n: p.grad.clone() for n, p in ref_model.named_parameters() if p.grad is not None}
    # second selection: frames [3, 4] against the reference's own prediction there (a loss well below the first one's)
    sel2 = torch.tensor([3, 4], device=DEV)
    t2 = out.detach()[[3, 4]].argmax(1)
    loss_ref2 = float(F.cross_entropy(torch.index_select(out.detach(), 0, sel2), t2, weight=w))
    assert abs(loss_ref2 - float(loss_ref)) > 2e-2, "the two selections must give clearly different losses (10 x the loss gate)"

    model, _, _, _, _ = _video_model()
    model.train()
    vi = torch.zeros(2, dtype=torch.int32, device=DEV)
    tbuf = t1.clone()
    step = TrainStep(model, frames, ids, am, tbuf, context=ops.StepContext(), valid_indices=vi)
    step.set_valid_indices([2, 1], 4)
    step.warmup_and_capture(eager_iters=1)
    assert step.captured and step.fused_loss and vi.tolist() == [2, 5]
    step.step()
    torch.cuda.synchronize()
    loss1 = float(step.loss)
    bad, worst = [], (0.0, 0.0, "")
    for n, p in model.named_parameters():
        if n not in ref:
            continue
        scale = float(ref[n].abs().max())
        if n.endswith(ZERO_GRAD_BIASES):          # analytically zero: rounding noise on both sides, checked to BE noise
            wscale = float(ref[n[:-4] + "weight"].abs().max())
            assert scale <= 0.05 * wscale and float(p.grad.abs().max()) <= 0.05 * wscale, (n, scale, float(p.grad.abs().max()), wscale)
            continue
        err = float((p.grad - ref[n]).abs().max())
        rel = float((p.grad - ref[n]).norm()) / max(float(ref[n].norm()), scale * ref[n].numel() ** 0.5 * 0.1, 1e-9)
        worst = max(worst, (err / max(scale, 1e-9), rel, n))
        if err > 0.06 * scale + 1e-7 or rel > 0.03:
            bad.append((n, round(err / max(scale, 1e-9), 4), round(rel, 4), scale))
    print(f"\n[TrainStep valid_indices fp32 vs autograd] loss {loss1:.6f} ref {float(loss_ref):.6f}; worst (max-abs / scale, relative L2, name): {worst}")
    assert abs(loss1 - float(loss_ref)) < 2e-3
    assert abs(float(step.stats[0]) - loss1) == 0.0 and float(step.stats[1]) > 0
    for b in sorted(bad, key=lambda b: -b[1]):
        print("  outside the gate:", b)
    assert not bad, sorted(bad, key=lambda b: -b[1])[:12]
    step.set_valid_indices([3, 0], 4)
    tbuf.copy_(t2)
    step.step()
    torch.cuda.synchronize()
    loss2 = float(step.loss)
    print(f"[TrainStep valid_indices] after set_valid_indices([3, 0], 4): loss {loss2:.6f} ref {loss_ref2:.6f}")
    assert vi.tolist() == [3, 4]
    assert abs(loss2 - loss_ref2) < 2e-3 and abs(loss2 - loss1) > 1e-2


@pytest.mark.parametrize("selected", [False, True])
def test_train_step_mc_dice(selected):
    """TrainStep(loss="mc_dice"), with and without valid_indices, fp32: the loss of the first step against MultiClassDiceLoss (the oracle's
    restatement, on the CPU) of the plain model's full-resolution logits, within the fp32 Dice tolerance 1e-5"""
    from lavt_hip import ops
    from lavt_hip.engine import TrainStep
    from oracle import lavt_oracle as O
    ref_model, frames, ids, am, tgt = _video_model()
    ref_model.train()
    with torch.no_grad():
        out = ref_model(frames, ids, am).cpu()
    rows = [2, 5] if selected else list(range(8))
    ref = float(O.multiclass_dice(out[rows], tgt[rows]))
    model, _, _, _, _ = _video_model()
    model.train()
    vi = torch.tensor(rows, dtype=torch.int32, device=DEV) if selected else None
    step = TrainStep(model, frames, ids, am, tgt[rows].to(DEV), use_graph=False, context=ops.StepContext(), loss="mc_dice", valid_indices=vi)
    step.warmup_and_capture(eager_iters=1)
    torch.cuda.synchronize()
    print(f"\n[TrainStep mc_dice selected={selected}] loss {float(step.loss):.7f} ref {ref:.7f}")
    assert step.fused_loss and step.stats.numel() == 2 + 6 * len(rows)
    assert abs(float(step.loss) - ref) < 1e-5
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.classifier.parameters())


def _check_against_logits(mask, iu, ref_logits, tgt, cap, margin=2e-3):
    """the rule of test_gpu_infer: mask == argmax of the reference logits on pixels with reference margin > `margin`, whose complement is at most `cap`
    of a sample; |I - I_ref| and |U - U_ref| at most the number of excluded pixels, per sample"""
    d = ref_logits[:, 1] - ref_logits[:, 0]
    decisive = d.abs() > margin
    pred, ref_mask, gt = mask.cpu().bool(), d > 0, tgt != 0
    for b in range(ref_logits.shape[0]):
        ties = int((~decisive[b]).sum())
        assert ties <= cap * decisive[b].numel(), f"sample {b}: {ties} pixels below the margin (cap {cap})"
        assert torch.equal(pred[b][decisive[b]], ref_mask[b][decisive[b]]), f"sample {b}: {int((pred[b] != ref_mask[b])[decisive[b]].sum())} decisive pixels differ"
        I_ref, U_ref = int((ref_mask[b] & gt[b]).sum()), int((ref_mask[b] | gt[b]).sum())
        I, U = (int(v) for v in iu[b].tolist())
        assert abs(I - I_ref) <= ties and abs(U - U_ref) <= ties, (b, I, I_ref, U, U_ref, ties)


def test_predictor_decodes_only_the_annotated_frames(golden):
    """Predictor(valid_indices=[2, 5]) captured against rows [2, 5] of the reference's eval logits (video_forward_feats; margin 2e-3, cap 1 % -- the
    fixture has no pixel below the margin in frames 2, 3, 5 and 0.024 % in frame 4), then rows [3, 4] after set_valid_indices([3, 0], 4) and a
    replay.  The decoder sees batch 2, not 8."""
    from lavt_hip.engine import Predictor
    from lavt_hip.metrics import EvalMeter
    g = golden("video_forward_feats")
    logits = torch.as_tensor(g["logits"])
    model, frames, ids, am, tgt = _video_model(seed=int(g["seed"]))
    model.eval()
    seen = []
    folded = model.classifier.forward_folded

    def spy(x_c4, *rest):
        seen.append(int(x_c4.shape[0]))
        return folded(x_c4, *rest)
    model.classifier.forward_folded = spy
    vi = torch.tensor([2, 5], dtype=torch.int32, device=DEV)
    tbuf = tgt[[2, 5]].to(DEV)
    p = Predictor(model, frames, ids, am, target=tbuf, valid_indices=vi)
    p.warmup_and_capture()
    assert p.captured
    assert seen and set(seen) == {2}, f"the folded decoder must run on the 2 selected frames, saw batches {seen}"
    a1 = p.step().clone()
    iu1 = p.iu.clone()
    a2 = p.step()
    torch.cuda.synchronize()
    assert a2.dtype == torch.uint8 and tuple(a2.shape) == (2, 64, 64) and tuple(p.iu.shape) == (2, 2)
    assert torch.equal(a1, a2) and torch.equal(iu1, p.iu), "two replays must be byte-identical"
    _check_against_logits(a2, p.iu.cpu(), logits[[2, 5]], tgt[[2, 5]], cap=0.01)
    meter = EvalMeter()
    meter.update(p.iu)
    I, U = (int(v) for v in p.iu.sum(0).tolist())
    assert meter.summary()["overall_iou"] == pytest.approx(100.0 * I / U)
    p.set_valid_indices([3, 0], 4)
    tbuf.copy_(tgt[[3, 4]])
    a3 = p.step()
    torch.cuda.synchronize()
    assert vi.tolist() == [3, 4] and not torch.equal(a3, a1)
    _check_against_logits(a3, p.iu.cpu(), logits[[3, 4]], tgt[[3, 4]], cap=0.01)


def test_frame_selection_refusals():
    from lavt_hip.engine import Predictor
    model, frames, ids, am, tgt = _video_model()
    vi = torch.tensor([2, 5], dtype=torch.int32, device=DEV)
    model.eval()
    with pytest.raises(ValueError, match="expressions_per_image"):
        Predictor(model, frames, torch.zeros(4, 22, dtype=torch.long, device=DEV), am.repeat(2, 1), expressions_per_image=2, valid_indices=vi)
    with pytest.raises(ValueError, match="target"):
        Predictor(model, frames, ids, am, target=tgt.to(DEV), valid_indices=vi)          # 8 target samples for 2 indices
    with pytest.raises(ValueError, match="folded"):
        model.forward_lowres(frames, ids, am, folded=False, frames=vi)
    model.train()
    with pytest.raises(ValueError, match="training mode"):
        model.forward_lowres(frames, ids, am, folded=True, frames=vi)
