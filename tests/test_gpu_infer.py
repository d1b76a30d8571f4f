"""GPU checks of the inference path: the three kernels of csrc/infer.hip against torch, the BatchNorm-folded decoder against the fixture captured
from the reference (decoder_c64) and the CPU oracle, and lavt_hip.engine.Predictor end to end against the reference's logits / mask / I / U
(e2e_swin_t_224, video_forward_feats) and the CPU oracle.  Every bound below is stated with its reason; none is taken from what the code gives."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lavt_hip.detweights import det_inputs, fill_state_dict_

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ARGS = SimpleNamespace(swin_type="tiny")
BF16_ULP = 2.0 ** -8          # relative spacing bound of bfloat16 (8 significant bits): round-to-nearest is within half of it


def randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator("cpu").manual_seed(seed))


@pytest.fixture(autouse=True)
def _fp32():
    import lavt_hip
    lavt_hip.set_compute_dtype(torch.float32)
    yield
    lavt_hip.set_compute_dtype(torch.float32)


def _sync():
    torch.cuda.synchronize()


# ================================================================================================ 1. fold kernel
@pytest.mark.parametrize("Cout,Cin,taps", [(8, 24, 9), (64, 96, 9), (512, 640, 9)])
def test_conv_bn_fold_kernel(Cout, Cin, taps):
    """fp32 copy and bias within 1e-6 relative (the fold is a few fp32 roundings: s and one product; for the bias `beta - mean * s` the roundings
    scale with the operands |beta| + |mean * s|, not with their difference, so that is what 'relative' refers to there); bf16 copy within one bf16 ulp."""
    from lavt_hip import _capi as K
    w = randn(1, Cout, Cin, 3, 3) * 0.1
    gamma, beta = 1.0 + 0.3 * randn(2, Cout), 0.2 * randn(3, Cout)
    mean, var = 0.3 * randn(4, Cout), 0.5 + torch.rand(Cout, generator=torch.Generator("cpu").manual_seed(5))
    eps = 1e-5
    s = gamma / torch.sqrt(var + eps)
    ref_w = (w * s[:, None, None, None]).permute(0, 2, 3, 1).reshape(Cout, taps * Cin)          # [co][tap][ci]
    ref_b = beta - mean * s
    d = [t.to(DEV).contiguous() for t in (w, gamma, beta, mean, var)]
    for dtype in (torch.float32, torch.bfloat16):
        wp = torch.full((Cout, taps * Cin), float("nan"), dtype=dtype, device=DEV)
        bias = torch.full((Cout,), float("nan"), device=DEV)
        K.check(K.lib.lavt_conv_bn_fold(*(K.ptr(t) for t in d), eps, K.dt(dtype), K.ptr(wp), K.ptr(bias), Cout, Cin, taps, K.stream()))
        _sync()
        ew = ((wp.float().cpu() - ref_w).abs() / ref_w.abs().clamp_min(1e-30)).max().item()
        eb = ((bias.cpu() - ref_b).abs() / (beta.abs() + (mean * s).abs())).max().item()
        print(f"\n[fold {Cout}x{Cin}x{taps} {dtype}] weight rel err {ew:.3e}  bias rel err {eb:.3e}")
        assert eb <= 1e-6
        assert ew <= (1e-6 if dtype == torch.float32 else BF16_ULP)
    # gamma / beta NULL = 1 / 0
    wp, bias = torch.empty(Cout, taps * Cin, device=DEV), torch.empty(Cout, device=DEV)
    K.check(K.lib.lavt_conv_bn_fold(K.ptr(d[0]), None, None, K.ptr(d[3]), K.ptr(d[4]), eps, K.F32, K.ptr(wp), K.ptr(bias), Cout, Cin, taps, K.stream()))
    s1 = 1.0 / torch.sqrt(var + eps)
    assert ((wp.cpu() - (w * s1[:, None, None, None]).permute(0, 2, 3, 1).reshape(Cout, -1)).abs() <= 1e-6 * (w.abs().max() * s1.max())).all()
    assert ((bias.cpu() + mean * s1).abs() <= 1e-6 * (mean * s1).abs().clamp_min(1e-30)).all()


# ================================================================================================ 2. split-K reduction with epilogue
@pytest.mark.parametrize("splits,M,N", [(3, 900, 512), (8, 900, 512), (2, 3600, 512), (4, 257, 64)])
def test_splitk_reduce_epi(splits, M, N):
    """sum (in the kernel's order: split 0 first) + bias -> relu in torch: fp32 output within 1e-6 relative, bf16 within one ulp; without bias and
    activation the bytes of lavt_splitk_reduce."""
    from lavt_hip import _capi as K
    parts = randn(11, splits, M, N).to(DEV)
    bias = randn(12, N).to(DEV)
    acc = torch.zeros(M, N, device=DEV)
    for s in range(splits):
        acc = acc + parts[s]
    ref = torch.relu(acc + bias).cpu()
    for dtype in (torch.float32, torch.bfloat16):
        out = torch.full((M, N), float("nan"), dtype=dtype, device=DEV)
        K.check(K.lib.lavt_splitk_reduce_epi(K.dt(dtype), K.ptr(parts), splits, M, N, K.ptr(bias), K.ACT_RELU, K.ptr(out), N, K.stream()))
        _sync()
        err = ((out.float().cpu() - ref).abs() / ref.abs().clamp_min(1e-30))[ref != 0]
        print(f"\n[splitk epi {splits}x{M}x{N} {dtype}] max rel err {err.max().item():.3e}")
        assert (out.float().cpu()[ref == 0] == 0).all()
        assert err.max().item() <= (1e-6 if dtype == torch.float32 else BF16_ULP)
        plain, epi = torch.zeros(M, N, dtype=dtype, device=DEV), torch.ones(M, N, dtype=dtype, device=DEV)
        K.check(K.lib.lavt_splitk_reduce(K.dt(dtype), K.ptr(parts), splits, M, N, K.ptr(plain), N, K.stream()))
        K.check(K.lib.lavt_splitk_reduce_epi(K.dt(dtype), K.ptr(parts), splits, M, N, None, K.ACT_NONE, K.ptr(epi), N, K.stream()))
        _sync()
        assert torch.equal(plain.view(torch.uint8), epi.view(torch.uint8)), "bias = NULL, act = NONE must store the bytes of lavt_splitk_reduce"


# ================================================================================================ 3-5. folded decoder
def _decoder_c64(golden):
    from lib.mask_predictor import SimpleDecoding
    g = golden("decoder_c64")
    dec = SimpleDecoding(64, ARGS)
    fill_state_dict_(dec)
    dec.to(DEV).eval()
    feats = [randn(int(s), 2, c, hw, hw).to(DEV) for s, (c, hw) in zip(g["seeds"], ((64, 4), (32, 8), (16, 16), (8, 32)))]
    return dec, feats, torch.as_tensor(g["y_eval"])


def test_folded_decoder_fp32_golden(golden):
    """forward_folded against y_eval captured from the real reference, within the existing eval test's 2e-4 (folding only reorders fp32 roundings)"""
    dec, feats, y_eval = _decoder_c64(golden)
    with torch.no_grad():
        y = dec.forward_folded(*feats).float().cpu()
    err = float((y - y_eval).abs().max())
    print(f"\n[folded decoder fp32 vs reference fixture] max abs err {err:.3e}")
    assert y.shape == y_eval.shape and err <= 2e-4
    with pytest.raises(RuntimeError):
        dec.train().forward_folded(*feats)


def test_folded_decoder_bf16_no_worse_than_unfolded(golden):
    """bf16: l2-relative error against y_eval at most 2x the unchanged unfolded bf16 eval path's on the same fixture (folding adds one independent bf16
    rounding, of w * s: sqrt(2) in rms, and removes the rounding between conv and BN; 2x is the margin over that)."""
    import lavt_hip
    dec, feats, y_eval = _decoder_c64(golden)
    with lavt_hip.use_dtype(torch.bfloat16), torch.no_grad():
        unf = dec(*feats).float().cpu()
        fol = dec.forward_folded(*feats).float().cpu()
    e_unf = float((unf - y_eval).norm() / y_eval.norm())
    e_fol = float((fol - y_eval).norm() / y_eval.norm())
    print(f"\n[decoder_c64 bf16, l2-relative error vs the reference's y_eval] unfolded {e_unf:.5f}  folded {e_fol:.5f}")
    assert e_fol <= 2.0 * e_unf


def _swin_b_decoder():
    from lib.mask_predictor import SimpleDecoding
    from oracle import lavt_oracle as O
    dec = SimpleDecoding(1024, ARGS)
    fill_state_dict_(dec)
    sd = {"classifier." + k: v.clone() for k, v in dec.state_dict().items()}
    feats = [randn(70 + i, 1, c, hw, hw) for i, (c, hw) in enumerate(((1024, 15), (512, 30), (256, 60), (128, 120)))]
    with torch.no_grad():
        ref = O.decoder(sd, "classifier", *feats, training=False)
    return dec.to(DEV).eval(), feats, ref


def test_folded_decoder_swin_b_geometry():
    """Batch 1 at Swin-B geometry (c4 = 1024 channels at 15^2, then 30^2, 60^2, 120^2) against oracle.lavt_oracle.decoder(training=False) on the CPU.

    fp32 compute: max error <= 2e-4 x max|ref| (the bound the folded path is held to: reordered fp32 roundings only).
    The split reduction exists for bf16 operands only (lavt_gemm_nt: conv_kc_split / conv_tap_split need the bf16 tap-walking kernel), so that
    it was taken -- in BOTH forms, channel pieces and tap groups -- is asserted on bf16 runs of the same problem; those are held to the bf16 rule of
    the previous test against the oracle: l2-relative error at most 2x the unfolded bf16 path's."""
    import lavt_hip
    from lavt_hip import _capi as K
    from lavt_hip import ops
    dec, feats, ref = _swin_b_decoder()
    dfe = [f.to(DEV) for f in feats]
    with torch.no_grad():
        y = dec.forward_folded(*dfe).float().cpu()
    err, scale = float((y - ref).abs().max()), float(ref.abs().max())
    print(f"\n[folded decoder, Swin-B geometry, fp32 vs oracle] max abs err {err:.3e}  max|ref| {scale:.3e}  ratio {err / scale:.3e}")
    assert err <= 2e-4 * scale

    def launches(fn):
        K.prof.start()
        try:
            out = fn()
        finally:
            rec = K.prof.stop()
        return out, [r[0] for r in rec if r[1] == "decoder"], [r[2]["shape"] for r in rec if r[1] == "decoder" and r[0] == "lavt_gemm_nt" and r[2]]

    with lavt_hip.use_dtype(torch.bfloat16), torch.no_grad():
        unf, names_unf, _ = launches(lambda: dec(*dfe).float().cpu())
        fol, names, shapes = launches(lambda: dec.forward_folded(*dfe).float().cpu())
        saved = ops._CONV_KC_SPLITS
        ops._CONV_KC_SPLITS = "0"          # no channel pieces: the split levels cut their reduction at tap boundaries instead
        try:
            fol_tap, names_tap, shapes_tap = launches(lambda: dec.forward_folded(*dfe).float().cpu())
        finally:
            ops._CONV_KC_SPLITS = saved
    e_unf = float((unf - ref).norm() / ref.norm())
    e_fol, e_tap = float((fol - ref).norm() / ref.norm()), float((fol_tap - ref).norm() / ref.norm())
    print(f"[bf16, l2-relative vs oracle] unfolded {e_unf:.5f}  folded (channel pieces) {e_fol:.5f}  folded (tap groups) {e_tap:.5f}")
    print(f"[decoder launches per call, bf16] unfolded {len(names_unf)}  folded {len(names)}")
    n_split, n_split_tap = names.count("lavt_splitk_reduce_epi"), names_tap.count("lavt_splitk_reduce_epi")
    assert n_split >= 1 and n_split_tap >= 1, "no level took the split path"
    assert any(" b" in s for s in shapes) and any(" b3 " in s + " " for s in shapes_tap), (shapes, shapes_tap)
    assert "lavt_norm_apply" not in names and "lavt_stats_finalize" not in names, "the folded decoder launches no BatchNorm kernel"
    assert len(names) < len(names_unf)
    assert e_fol <= 2.0 * e_unf and e_tap <= 2.0 * e_unf


# ================================================================================================ 6-8. mask kernel
SHAPES = [(2, 120, 120, 480, 480), (3, 56, 56, 224, 224), (1, 120, 120, 360, 640), (2, 40, 36, 157, 143)]


def _ref_logits(rows, B, Hi, Wi, out, via=None):
    y = rows.float().view(B, Hi, Wi, 2).permute(0, 3, 1, 2)
    if via is not None:
        y = F.interpolate(y, size=via, mode="bilinear", align_corners=True)
    return F.interpolate(y, size=out, mode="bilinear", align_corners=True)


def _check_mask(mask, ref, cap=5e-4):
    d = ref[:, 1] - ref[:, 0]
    decided = d.abs() >= 1e-4
    undecided = 1.0 - float(decided.float().mean())
    assert undecided <= cap, f"undecided share {undecided:.2e} > {cap:.0e}"
    want = (d > 0)
    got = mask.cpu().bool()
    assert set(mask.unique().tolist()) <= {0, 1}
    assert torch.equal(got[decided], want[decided]), f"{int((got[decided] != want[decided]).sum())} decided pixels differ"
    return undecided


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("via", [None, (480, 480)])
@pytest.mark.parametrize("shape", SHAPES)
def test_upsample_mask_kernel(shape, via, dtype):
    """against F.interpolate(..., align_corners=True).argmax(1) on the CPU from the SAME logit rows (bf16: from the bf16-rounded values); pixels with
    |v1 - v0| < 1e-4 in the reference are undecided (at most 5e-4 of them: asserted) and left out, all others agree exactly.  via = (480, 480): the
    two-stage interpolation of test_ytvos.py:249-253 against the two-stage reference."""
    from lavt_hip import ops
    B, Hi, Wi, Ho, Wo = shape
    rows = (randn(21, B * Hi * Wi, 2) * 2).to(dtype)
    ref = _ref_logits(rows, B, Hi, Wi, (Ho, Wo), via)
    mask, iu = ops.upsample_mask(rows.to(DEV), B, Hi, Wi, (Ho, Wo), via_size=via)
    _sync()
    assert iu is None and mask.dtype == torch.uint8 and tuple(mask.shape) == (B, Ho, Wo)
    und = _check_mask(mask, ref)
    print(f"\n[mask {shape} via={via} {dtype}] undecided share {und:.2e}")


def test_upsample_mask_two_stage_differs_from_one_stage():
    """on (1, 120, 120) -> (360, 640) the one-stage and the two-stage references disagree on ~0.5 % of the pixels: a kernel that ignored via_size fails above"""
    rows = randn(21, 120 * 120, 2) * 2
    one, two = _ref_logits(rows, 1, 120, 120, (360, 640)), _ref_logits(rows, 1, 120, 120, (360, 640), (480, 480))
    share = float((one.argmax(1) != two.argmax(1)).float().mean())
    print(f"\n[one-stage vs two-stage reference masks] disagree on {share:.4f}")
    assert share > 1e-3


@pytest.mark.parametrize("shape", SHAPES)
def test_upsample_mask_iu_counts(shape):
    """with a random target iu equals computeIoU (test.py:242-246) of the kernel's own mask exactly, per sample; a second launch gives the same numbers"""
    from lavt_hip import ops
    B, Hi, Wi, Ho, Wo = shape
    rows = (randn(22, B * Hi * Wi, 2) * 2).to(DEV)
    tgt = torch.randint(0, 3, (B, Ho, Wo), generator=torch.Generator("cpu").manual_seed(23))          # nonzero = foreground
    for dtype in (torch.float32, torch.bfloat16):
        r = rows.to(dtype)
        mask, iu = ops.upsample_mask(r, B, Hi, Wi, (Ho, Wo), target=tgt.to(DEV))
        mask2, iu2 = ops.upsample_mask(r, B, Hi, Wi, (Ho, Wo), target=tgt.to(DEV))
        _sync()
        pred, gt = mask.cpu().bool(), tgt != 0
        want = torch.stack([(pred & gt).flatten(1).sum(1), (pred | gt).flatten(1).sum(1)], 1)
        assert iu.dtype == torch.int32 and torch.equal(iu.cpu().long(), want), (iu.cpu(), want)
        assert torch.equal(iu2, iu) and torch.equal(mask2, mask)


# ================================================================================================ 9-11. Predictor end to end (2-D)
def _build(embed_dim, depths, heads, ws, dpr=0.3):
    from lib._utils import LAVT
    from lib.backbone import MultiModalSwinTransformer
    from lib.mask_predictor import SimpleDecoding
    bb = MultiModalSwinTransformer(embed_dim=embed_dim, depths=depths, num_heads=heads, window_size=ws, drop_path_rate=dpr, args=ARGS)
    model = LAVT(bb, SimpleDecoding(8 * embed_dim, ARGS))
    fill_state_dict_(model)
    return model


def _swin_t():
    return _build(96, [2, 2, 6, 2], [3, 6, 12, 24], 7)


def _e2e_inputs(g):
    x, l, _, tgt = det_inputs(1, 224, 20, seed=int(g["seed"]))
    m = torch.zeros(1, 20, 1)
    m[0, : int(g["valid"])] = 1
    return x, l, m, tgt


def _check_against_logits(mask, iu, ref_logits, tgt, cap, margin=2e-3):
    """mask == argmax of the reference logits on pixels with reference margin > `margin`; the share below it is asserted <= cap; |I - I_ref| and
    |U - U_ref| at most the number of excluded pixels, per sample (the rule of test_e2e_swin_t_224_golden)"""
    d = ref_logits[:, 1] - ref_logits[:, 0]
    decisive = d.abs() > margin
    for b in range(ref_logits.shape[0]):
        share = 1.0 - float(decisive[b].float().mean())
        assert share <= cap, f"sample {b}: {share:.4f} of the pixels below the margin (cap {cap})"
    pred, ref_mask = mask.cpu().bool(), d > 0
    assert torch.equal(pred[decisive], ref_mask[decisive]), f"{int((pred[decisive] != ref_mask[decisive]).sum())} decisive pixels differ"
    if iu is not None:
        gt = tgt != 0
        for b in range(ref_logits.shape[0]):
            ties = int((~decisive[b]).sum())
            I_ref, U_ref = int((ref_mask[b] & gt[b]).sum()), int((ref_mask[b] | gt[b]).sum())
            I, U = (int(v) for v in iu[b].tolist())
            assert abs(I - I_ref) <= ties and abs(U - U_ref) <= ties, (b, I, I_ref, U, U_ref, ties)


@pytest.mark.parametrize("use_graph", [False, True])
def test_predictor_e2e_swin_t_224_fp32(golden, use_graph):
    """Swin-T, 1 x 224^2 against the reference's logits, mask, I and U: the mask equals the fixture's on pixels with reference margin > 2e-3 (the
    fixture has 0.30 % below that; asserted <= 0.5 %), I / U within the number of excluded pixels, two steps byte-identical."""
    from lavt_hip.engine import Predictor
    from lavt_hip.metrics import EvalMeter
    g = golden("e2e_swin_t_224")
    model = _swin_t().to(DEV).eval()
    x, l, m, tgt = _e2e_inputs(g)
    p = Predictor(model, x.to(DEV), l.to(DEV), m.to(DEV), target=tgt.to(DEV), use_graph=use_graph)
    p.warmup_and_capture()
    assert p.captured == use_graph
    first = p.step().clone()
    iu1 = p.iu.clone()
    second = p.step()
    _sync()
    assert second.dtype == torch.uint8 and tuple(second.shape) == (1, 224, 224)
    assert torch.equal(first, second) and torch.equal(iu1, p.iu), "two steps must give byte-identical masks and the same counts (no accumulation)"
    ref_logits = torch.as_tensor(g["logits"])
    fix_mask = torch.as_tensor(np.unpackbits(g["mask"])[: 224 * 224].reshape(1, 224, 224)).bool()
    decisive = (ref_logits[:, 1] - ref_logits[:, 0]).abs() > 2e-3
    assert torch.equal(second.cpu().bool()[decisive], fix_mask[decisive]), "mask differs from the fixture's on decisive pixels"
    _check_against_logits(second, p.iu.cpu(), ref_logits, tgt, cap=0.005)
    ties = int(((ref_logits[:, 1] - ref_logits[:, 0]).abs() <= 2e-3).sum())
    I, U = (int(v) for v in p.iu[0].tolist())
    assert abs(I - int(g["I"])) <= ties and abs(U - int(g["U"])) <= ties
    meter = EvalMeter()
    meter.update(p.iu)
    assert meter.summary()["overall_iou"] == pytest.approx(100.0 * I / U)


def test_predictor_e2e_swin_t_224_bf16(golden):
    """the project's existing bf16 gate (test_e2e_bf16_close_to_fp32): agreement >= 0.97 on pixels with margin > 5 % of the logit range"""
    import lavt_hip
    from lavt_hip.engine import Predictor
    g = golden("e2e_swin_t_224")
    model = _swin_t().to(DEV).eval()
    x, l, m, tgt = _e2e_inputs(g)
    with lavt_hip.use_dtype(torch.bfloat16):
        p = Predictor(model, x.to(DEV), l.to(DEV), m.to(DEV), target=tgt.to(DEV))
        p.warmup_and_capture()
        a = p.step().clone()
        b = p.step()
        _sync()
    assert p.captured and torch.equal(a, b)
    ref = torch.as_tensor(g["logits"])
    rng = float(ref.max() - ref.min())
    decisive = (ref[:, 1] - ref[:, 0]).abs() > 0.05 * rng
    agree = float((b.cpu().bool()[decisive] == (ref[:, 1] > ref[:, 0])[decisive]).float().mean())
    print(f"\n[Predictor bf16 vs reference fp32 logits] mask agreement on decisive pixels {agree:.4f}")
    assert agree >= 0.97


def test_predictor_sees_changed_running_stats_and_weights(golden):
    """Staleness: after capture a decoder running_var and a conv weight change in place; the next step() must match the CPU oracle on the modified
    state (fp32, the gates of the e2e test; the oracle's logit map has 0.32 % of its pixels below the 2e-3 margin -- computed on the CPU -- asserted
    <= 1 %).  The modification moves 8 % of the oracle's mask pixels: a replay on stale folded weights fails."""
    from lavt_hip.engine import Predictor
    from oracle import lavt_oracle as O
    g = golden("e2e_swin_t_224")
    model = _swin_t()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    model.to(DEV).eval()
    x, l, m, tgt = _e2e_inputs(g)
    p = Predictor(model, x.to(DEV), l.to(DEV), m.to(DEV), target=tgt.to(DEV))
    p.warmup_and_capture()
    assert p.captured
    before = p.step().clone()
    with torch.no_grad():
        model.classifier.bn1_2.running_var.mul_(1.7)
        model.classifier.conv2_3.weight.mul_(0.8)
    sd["classifier.bn1_2.running_var"] = sd["classifier.bn1_2.running_var"] * 1.7
    sd["classifier.conv2_3.weight"] = sd["classifier.conv2_3.weight"] * 0.8
    with torch.no_grad():
        ref = O.lavt_forward(sd, x, l, m, "tiny", 7, training=False)
    after = p.step()
    _sync()
    assert float((after != before).float().mean()) > 0.01, "the modification must move the mask"
    _check_against_logits(after, p.iu.cpu(), ref, tgt, cap=0.01)


def test_predictor_expressions_share_stage0():
    """One 224^2 image, S = 3 expressions (different language seeds and valid lengths) through Predictor(expressions_per_image=3), fp32, against three
    batch-1 runs of the oracle: sample i equals oracle run i on pixels with margin > 2e-3 (share below: 0.24 / 0.26 / 0.29 % on the CPU, asserted
    <= 1 %).  A forward hook on the stage-0 / stage-1 blocks shows stage 0 ran on batch 1 and the later stages on batch 3."""
    from lavt_hip.engine import Predictor
    from oracle import lavt_oracle as O
    model = _swin_t()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    model.to(DEV).eval()
    x, _, _, tgt1 = det_inputs(1, 224, 20, seed=1234)
    ls, ms = [], []
    for seed, valid in ((101, 12), (202, 7), (303, 20)):
        ls.append(randn(seed, 1, 768, 20))
        mj = torch.zeros(1, 20, 1)
        mj[0, :valid] = 1
        ms.append(mj)
    with torch.no_grad():
        ref = torch.cat([O.lavt_forward(sd, x, lj, mj, "tiny", 7, training=False) for lj, mj in zip(ls, ms)])
    masks_ref = ref.argmax(1)
    assert float((masks_ref[0] != masks_ref[1]).float().mean()) > 0.05, "the expressions must give different masks"
    tgt = tgt1.expand(3, -1, -1).contiguous()
    seen = {0: [], 1: []}
    hooks = [model.backbone.layers[i].blocks[0].register_forward_hook(lambda mod, inp, out, i=i: seen[i].append(int(inp[0].shape[0]))) for i in (0, 1)]
    p = Predictor(model, x.to(DEV), torch.cat(ls).to(DEV), torch.cat(ms).to(DEV), target=tgt.to(DEV), expressions_per_image=3)
    p.warmup_and_capture()
    for h in hooks:
        h.remove()
    assert seen[0] and set(seen[0]) == {1}, f"stage 0's blocks must run once per image, saw batches {seen[0]}"
    assert seen[1] and set(seen[1]) == {3}, f"stage 1 runs per expression, saw batches {seen[1]}"
    assert p.captured
    mask = p.step()
    _sync()
    assert tuple(mask.shape) == (3, 224, 224) and tuple(p.iu.shape) == (3, 2)
    _check_against_logits(mask, p.iu.cpu(), ref, tgt, cap=0.01)
    with pytest.raises(ValueError):
        Predictor(model, x.to(DEV), torch.cat(ls[:2]).to(DEV), torch.cat(ms[:2]).to(DEV), expressions_per_image=3)


# ================================================================================================ 12. video
def test_predictor_video(golden):
    """LAVTVideo through Predictor against the logits of the reference's own _LAVTVideoSimpleDecode.forward_feats (video_forward_feats fixture, eval
    mode; the text encoder is the stub of test_lavt_video_forward_feats_golden on both sides): mask equal on pixels with reference margin > 2e-3
    (the fixture has 0.006 % below; asserted <= 1 %), I / U against a random target within the excluded count.  expressions_per_image=2 raises."""
    from lavt_hip.engine import Predictor
    from lib._utils import LAVTVideo
    from lib.mask_predictor import SimpleDecoding
    from lib.video_swin_transformer import MultiModalSwinTransformer3D
    g = golden("video_forward_feats")
    a = SimpleNamespace()
    bb = MultiModalSwinTransformer3D(patch_size=(1, 4, 4), embed_dim=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8], window_size=(8, 7, 7),
                                     drop_path_rate=0.0, patch_norm=True, out_indices=(0, 1, 2, 3), use_checkpoint=False,
                                     num_heads_fusion=[1, 1, 1, 1], fusion_drop=0.0, args=a)
    parts = torch.nn.ModuleDict({"backbone": bb, "classifier": SimpleDecoding(256, a)})
    fill_state_dict_(parts)
    parts.to(DEV)
    frames, l, m, tgt = det_inputs(2, 64, 22, seed=int(g["seed"]), frames=4)
    frames, l, m = frames.to(DEV), l.to(DEV), m.to(DEV)

    class _Text(torch.nn.Module):
        def forward(self, ids, attention_mask=None):
            return (l.permute(0, 2, 1),)

    model = LAVTVideo.__new__(LAVTVideo)
    torch.nn.Module.__init__(model)
    model.backbone, model.classifier, model.text_encoder = parts["backbone"], parts["classifier"], _Text()
    model.lazy_pred, model.seg_last = False, False
    model.eval()
    ids, am = torch.zeros(2, 22, dtype=torch.long, device=DEV), m.squeeze(-1).contiguous()
    p = Predictor(model, frames, ids, am, target=tgt.to(DEV))
    p.warmup_and_capture()
    assert p.captured
    a1 = p.step().clone()
    a2 = p.step()
    _sync()
    assert tuple(a2.shape) == (8, 64, 64) and torch.equal(a1, a2)
    _check_against_logits(a2, p.iu.cpu(), torch.as_tensor(g["logits"]), tgt, cap=0.01)
    with pytest.raises(NotImplementedError):
        Predictor(model, frames, torch.zeros(4, 22, dtype=torch.long, device=DEV), am.repeat(2, 1), expressions_per_image=2)
    with pytest.raises(NotImplementedError):
        model.forward_lowres(frames, torch.zeros(4, 22, dtype=torch.long, device=DEV), am.repeat(2, 1), expand=2)
