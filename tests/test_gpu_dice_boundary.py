"""GPU checks of the fused Dice+Boundary criterion (reference losses.py:142-244, `--loss dice_boundary`): lavt_upsample_dice_boundary_{fwd,bwd} and
their _sel_ forms through the C ABI against the fixtures the reference's own DiceBoundaryLoss wrote (tests/golden/dice_boundary_<tag>.npz), and,
where no fixture exists (bf16-rounded logits, selected frames, full-resolution logits, the harness), against the torch restatement that
test_dice_boundary_host.py pins to those fixtures (tests/dice_boundary_ref.py).

Gates.  fp32: |loss - ref| < 1e-5 (the Dice pair's gate) and max |dx - ref| <= 1e-4 * max |ref| over EVERY element: about ten times the spread between
the reference's own fp32 and fp64 gradients on these inputs (at most 1.2e-5 of max |dy|, printed by make_boundary_golden.py); an arg-max
resolved differently from torch's moves a gradient term to a neighbouring pixel and exceeds it.  bf16 storage: the gates of test_upsample_dice_golden
(loss 3e-3, gradient 2 % of its maximum).  No bound is taken from what the code gives."""
import functools
from types import SimpleNamespace

import pytest
import torch

import dice_boundary_ref as R
from lavt_hip.detweights import det_inputs, fill_state_dict_

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _fp32():
    import lavt_hip
    lavt_hip.set_compute_dtype(torch.float32)
    yield
    lavt_hip.set_compute_dtype(torch.float32)


def _abi(x, target, B, dims, rates, dtype=torch.float32, sel=None, dloss=None):
    """one forward + backward through the C ABI.  x [B*h*w, 2] (CPU), target (n, H, W); sel: a DEVICE int32 buffer -> (loss, stats, dx) on the CPU"""
    from lavt_hip import _capi as K
    h, w, H, W = dims
    n = B if sel is None else sel.numel()
    xd, td = x.to(DEV).to(dtype).contiguous(), target.to(DEV).contiguous()
    stats = torch.full((3 + 14 * n,), float("nan"), device=DEV)
    ws_n = K.lib.lavt_upsample_dice_boundary_ws(n, H, W)
    ws = torch.full((ws_n,), float("nan"), device=DEV)
    dx = torch.full_like(xd, float("nan"))
    dl = None if dloss is None else torch.tensor([dloss], device=DEV)
    st = K.stream()
    if sel is None:
        K.check(K.lib.lavt_upsample_dice_boundary_fwd(K.dt(dtype), K.ptr(xd), K.ptr(td), rates[0], rates[1], K.ptr(ws), ws_n, K.ptr(stats), B, h, w, H, W, st))
        K.check(K.lib.lavt_upsample_dice_boundary_bwd(K.dt(dtype), K.ptr(xd), K.ptr(td), rates[0], rates[1], K.ptr(stats), K.ptr(dl), K.ptr(ws), ws_n, K.ptr(dx),
                                                      B, h, w, H, W, st))
    else:
        K.check(K.lib.lavt_upsample_dice_boundary_sel_fwd(K.dt(dtype), K.ptr(xd), K.ptr(sel), n, K.ptr(td), rates[0], rates[1], K.ptr(ws), ws_n, K.ptr(stats),
                                                          B, h, w, H, W, st))
        K.check(K.lib.lavt_upsample_dice_boundary_sel_bwd(K.dt(dtype), K.ptr(xd), K.ptr(sel), n, K.ptr(td), rates[0], rates[1], K.ptr(stats), K.ptr(dl), K.ptr(ws),
                                                          ws_n, K.ptr(dx), B, h, w, H, W, st))
    torch.cuda.synchronize()
    return float(stats[0]), stats.cpu(), dx.float().cpu()


@pytest.mark.parametrize("tag", R.TAGS)
def test_fp32_against_the_reference_fixtures(tag):
    f = R.load(tag)
    B = f["dims"][0]
    loss, stats, dx = _abi(f["x"], f["target"], B, f["dims"][1:], f["rates"])
    peak = float(f["dy"].abs().max())
    gerr = float((dx - f["dy"]).abs().max())
    print(f"\n[dice_boundary fp32 {tag}] loss {loss:.8f} ref {f['loss']:.8f}  dice {float(stats[1]):.8f} ref {f['dice']:.8f}  boundary {float(stats[2]):.8f} "
          f"ref {f['boundary']:.8f}  max |dx - ref| {gerr:.3e} = {gerr / peak:.2e} of max |ref| {peak:.3e}")
    assert abs(loss - f["loss"]) < 1e-5
    assert abs(float(stats[1]) - f["dice"]) < 1e-5 and abs(float(stats[2]) - f["boundary"]) < 1e-5
    assert bool(torch.isfinite(dx).all()) and gerr <= 1e-4 * peak
    # the per-sample sums: pixel counts exactly, S4 = #gt_b against the restatement's own boundary map
    per = stats[3:].view(B, 14)
    t = f["target"]
    assert torch.equal(per[:, 4], (t == 0).flatten(1).sum(1).float()) and torch.equal(per[:, 5], (t == 1).flatten(1).sum(1).float())
    g = torch.stack([t == 0, t == 1], 1).float()
    assert torch.equal(per[:, [9, 13]], R._edge(1 - g).flatten(2).sum(2))
    if tag == "a":
        assert per[-1, [8, 9, 12, 13]].tolist() == [0.0] * 4          # the all-background sample: no boundary pixel, S3 = S4 = 0 for both classes
    # dloss scales the gradient
    _, _, dx3 = _abi(f["x"], f["target"], B, f["dims"][1:], f["rates"], dloss=3.0)
    assert float((dx3 - 3.0 * f["dy"]).abs().max()) <= 3e-4 * peak


@functools.lru_cache(maxsize=None)
def _bf16_reference(tag):
    f = R.load(tag)
    x = f["x"].bfloat16().float()                             # both sides start from the same bf16-representable logits
    return (x,) + R.lowres(x, f["target"], f["dims"], *f["rates"])


@pytest.mark.parametrize("tag", ["a", "b", "same", "blob"])
def test_bf16_storage(tag):
    """x and dx in bf16, arithmetic in fp32: the reference is the restatement on the bf16-rounded logits"""
    f = R.load(tag)
    x, ref, _, _, ref_dy = _bf16_reference(tag)
    loss, _, dx = _abi(x, f["target"], f["dims"][0], f["dims"][1:], f["rates"], dtype=torch.bfloat16)
    peak = float(ref_dy.abs().max())
    gerr = float((dx - ref_dy).abs().max())
    print(f"\n[dice_boundary bf16 {tag}] loss {loss:.7f} ref {ref:.7f}  max |dx - ref| {gerr:.3e} = {gerr / peak:.2e} of max |ref|")
    assert abs(loss - ref) < 3e-3
    assert gerr <= 0.02 * peak


@functools.lru_cache(maxsize=None)
def _selected_reference(sel):
    h, w, H, W = R.load("a")["dims"][1:]
    g = torch.Generator().manual_seed(77)
    x = torch.randn(4 * h * w, 2, generator=g) * 2.0
    tgt = torch.randint(0, 2, (2, H, W), generator=g)
    return (x, tgt) + R.lowres(x, tgt, (4, h, w, H, W), sel=list(sel))


def test_frame_selection_follows_the_device_buffer():
    """B = 4 frames, nsel = 2 on the shape of `a`: sel = [3, 1], then the SAME buffer refilled with [0, 2]; the unselected frames get exactly +0.0"""
    h, w, H, W = R.load("a")["dims"][1:]
    seld = torch.zeros(2, dtype=torch.int32, device=DEV)
    for sel in ((3, 1), (0, 2)):
        x, tgt, ref, _, _, ref_dy = _selected_reference(sel)
        seld.copy_(torch.tensor(sel, dtype=torch.int32))
        loss, stats, dx = _abi(x, tgt, 4, (h, w, H, W), (1.0, 0.05), sel=seld)
        peak = float(ref_dy.abs().max())
        gerr = float((dx - ref_dy).abs().max())
        print(f"\n[dice_boundary sel {sel}] loss {loss:.8f} ref {ref:.8f}  max |dx - ref| {gerr / peak:.2e} of max |ref|")
        assert abs(loss - ref) < 1e-5 and gerr <= 1e-4 * peak and stats.numel() == 3 + 14 * 2
        rest = [b for b in range(4) if b not in sel]
        g3 = dx.view(4, h * w * 2)
        assert torch.equal(g3[rest], torch.zeros_like(g3[rest])), "unselected frames must receive exactly zero"
        assert not bool(torch.signbit(g3[rest]).any()), "+0.0, not -0.0"
        assert float(ref_dy.view(4, -1)[rest].abs().max()) == 0.0 and float(g3[list(sel)].abs().max()) > 0
    # through the autograd op, bf16 storage: zeros of the unselected frames again exactly +0.0
    from lavt_hip import ops
    x, tgt, _, _, _, _ = _selected_reference((0, 2))
    xg = x.to(DEV).bfloat16().requires_grad_(True)
    loss, _ = ops.upsample_dice_boundary_loss(xg, tgt.to(DEV), 4, h, w, H, W, sel=seld)
    loss.backward()
    g3 = xg.grad.view(4, -1)[[1, 3]].cpu()
    assert torch.equal(g3, torch.zeros_like(g3)) and not bool(torch.signbit(g3.float()).any())
    # an entry outside [0, B) contributes nothing and is never dereferenced; the means stay over nsel samples
    seld.copy_(torch.tensor([2, 9], dtype=torch.int32))
    loss, stats, dx = _abi(x, tgt, 4, (h, w, H, W), (1.0, 0.05), sel=seld)
    assert stats[3 + 14:].abs().max() == 0 and bool(torch.isfinite(dx).all())
    assert torch.equal(dx.view(4, -1)[[0, 1, 3]], torch.zeros(3, h * w * 2))
    _, d1, b1, _ = R.lowres(x, tgt[:1], (4, h, w, H, W), sel=[2])
    assert abs(loss - 0.5 * (d1 + 0.05 * b1)) < 1e-5


def test_two_runs_are_bit_identical():
    f = R.load("b")
    runs = [_abi(f["x"], f["target"], f["dims"][0], f["dims"][1:], f["rates"]) for _ in range(2)]
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])


def test_drop_in_criterion_on_full_resolution_logits():
    """losses.DiceBoundaryLoss on (2, 2, 40, 36) logits: 1e-5 on the loss, 1e-4 of its maximum on the gradient; the given rates are used"""
    import losses
    g = torch.Generator().manual_seed(11)
    out = torch.randn(2, 2, 40, 36, generator=g) * 2.0
    tgt = torch.randint(0, 2, (2, 40, 36), generator=g)
    for args, rates in (((), (1.0, 0.05)), ((0.2, 0.5), (0.5, 0.2))):
        o = out.clone().requires_grad_(True)
        ref = R.criterion(o, tgt, *rates)[0]
        ref.backward()
        od = out.to(DEV).requires_grad_(True)
        loss = losses.DiceBoundaryLoss(*args)(od, tgt.to(DEV))
        loss.backward()
        gerr, peak = float((od.grad.cpu() - o.grad).abs().max()), float(o.grad.abs().max())
        print(f"\n[DiceBoundaryLoss{args}] loss {float(loss):.8f} ref {float(ref):.8f}  max |grad - ref| {gerr / peak:.2e} of max |ref|")
        assert abs(float(loss) - float(ref)) < 1e-5 and gerr <= 1e-4 * peak
    with pytest.raises(NotImplementedError):
        losses.DiceFocalLoss()


# ================================================================================================ the harness on the micro Video-Swin
def _video_model(seed=1234):
    """the micro Video-Swin of test_gpu_frame_select (embed 32, depths 2-2-2-2, window (8, 7, 7)), 2 clips x 4 frames x 64^2, the stub text encoder"""
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


# (analytically zero gradients: rounding noise on both sides -- see test_gpu_frame_select.ZERO_GRAD_BIASES)
ZERO_GRAD_BIASES = tuple(f"image_lang_att.{m}.0.bias" for m in ("f_key", "f_value", "f_query", "W"))


@pytest.mark.parametrize("selected", [False, True])
def test_train_step_dice_boundary(selected):
    """TrainStep(loss="dice_boundary") captures; its replayed loss is its eager loss bit for bit; loss (1e-5) and parameter gradients (the rule of
    test_train_step_selected_frames_match_plain_autograd: relative L2 <= 3 % per parameter, no element further than 6 % of the parameter's scale)
    equal those of the same step with fused_loss=False, which runs losses.DiceBoundaryLoss on the index_select-ed full-resolution logits"""
    from lavt_hip import ops
    from lavt_hip.engine import TrainStep
    rows = [2, 5] if selected else list(range(8))
    rates = {"dice_rate": 0.75, "boundary_rate": 0.5}

    def build(**kw):
        model, frames, ids, am, tgt = _video_model()
        model.train()
        vi = torch.tensor(rows, dtype=torch.int32, device=DEV) if selected else None
        return model, TrainStep(model, frames, ids, am, tgt[rows].to(DEV), context=ops.StepContext(), loss="dice_boundary", valid_indices=vi, **rates, **kw)

    ref_model, plain = build(fused_loss=False, use_graph=False)
    plain.step()
    torch.cuda.synchronize()
    assert not plain.fused_loss
    ref_loss = float(plain.loss)
    ref = {n: p.grad.clone() for n, p in ref_model.named_parameters() if p.grad is not None}

    model, step = build()
    eager = step.step().clone()
    step.warmup_and_capture(eager_iters=1)
    assert step.captured and step.fused_loss and step.stats.numel() == 3 + 14 * len(rows)
    step.step()
    torch.cuda.synchronize()
    loss = float(step.loss)
    print(f"\n[TrainStep dice_boundary selected={selected}] replayed loss {loss:.8f} eager {float(eager):.8f} fused_loss=False {ref_loss:.8f}")
    assert torch.equal(step.loss, eager), "replay and eager step must agree bit for bit"
    assert float(step.stats[0]) == loss
    assert abs(float(step.stats[0]) - (0.75 * float(step.stats[1]) + 0.5 * float(step.stats[2]))) < 1e-6
    assert abs(loss - ref_loss) < 1e-5
    bad, worst = [], (0.0, 0.0, "")
    for n, p in model.named_parameters():
        if n not in ref:
            continue
        scale = float(ref[n].abs().max())
        if n.endswith(ZERO_GRAD_BIASES):
            wscale = float(ref[n[:-4] + "weight"].abs().max())
            assert scale <= 0.05 * wscale and float(p.grad.abs().max()) <= 0.05 * wscale, (n, scale, float(p.grad.abs().max()), wscale)
            continue
        err = float((p.grad - ref[n]).abs().max())
        rel = float((p.grad - ref[n]).norm()) / max(float(ref[n].norm()), scale * ref[n].numel() ** 0.5 * 0.1, 1e-9)
        worst = max(worst, (err / max(scale, 1e-9), rel, n))
        if err > 0.06 * scale + 1e-7 or rel > 0.03:
            bad.append((n, round(err / max(scale, 1e-9), 4), round(rel, 4), scale))
    print(f"[TrainStep dice_boundary selected={selected}] worst (max-abs / scale, relative L2, name): {worst}")
    assert not bad, sorted(bad, key=lambda b: -b[1])[:12]
