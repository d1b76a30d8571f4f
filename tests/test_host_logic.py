"""CPU tests (-m "not gpu"): host logic of the product (row maps, factories, state-dict keys), that the C-ABI
library loads and exports every symbol of include/lavt_hip.h, and that the product refuses to run without a GPU."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, ROOT
from lavt_hip import rowmaps
from oracle import lavt_oracle as O


@pytest.mark.parametrize("B,H,W,ws,shift", [(2, 10, 9, 7, 3), (1, 15, 15, 12, 6), (2, 14, 14, 7, 0), (1, 30, 30, 12, 6), (1, 7, 7, 7, 3)])
def test_window_map_matches_pad_roll_partition(B, H, W, ws, shift):
    """The gather table reproduces pad -> roll -> window_partition, and doubles as the reverse scatter."""
    C = 3
    x = torch.arange(B * H * W * C, dtype=torch.float32).view(B, H, W, C) + 1
    Hp, Wp = rowmaps.padded(H, ws), rowmaps.padded(W, ws)
    u = F.pad(x, (0, 0, 0, Wp - W, 0, Hp - H))
    if shift:
        u = torch.roll(u, (-shift, -shift), (1, 2))
    win = u.view(B, Hp // ws, ws, Wp // ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, C)
    m = torch.from_numpy(rowmaps.window_map_np(B, H, W, ws, shift).astype(np.int64))
    flat = torch.cat([x.view(-1, C), torch.zeros(1, C)])
    assert torch.equal(flat[m], win)
    real = m[m >= 0]
    assert real.numel() == B * H * W and torch.equal(real.sort().values, torch.arange(B * H * W))   # each token exactly once


@pytest.mark.parametrize("H,ws", [(126, 7), (36, 12), (24, 12), (7, 7), (14, 7), (30, 12)])
def test_region_ids_match_golden_masks(golden, H, ws):
    ids = torch.from_numpy(rowmaps.region_ids_np(H, H, ws, ws // 2).astype(np.int64))
    mask = torch.where(ids[:, :, None] == ids[:, None, :], 0.0, -100.0)
    assert torch.equal(mask, O.shift_mask(rowmaps.padded(H, ws), rowmaps.padded(H, ws), ws, ws // 2))
    g = golden("shift_masks")
    key = f"m_{rowmaps.padded(H, ws)}_{ws}"
    if key in g.files and H == rowmaps.padded(H, ws):
        assert np.array_equal(np.packbits((mask != 0).numpy().reshape(-1)), g[key])


@pytest.mark.parametrize("B,H,W", [(2, 8, 6), (2, 7, 5), (1, 15, 15)])
def test_merge_map(B, H, W):
    C = 2
    x = torch.arange(B * H * W * C, dtype=torch.float32).view(B, H, W, C) + 1
    z = F.pad(x, (0, 0, 0, W % 2, 0, H % 2))
    ref = torch.cat([z[:, 0::2, 0::2], z[:, 1::2, 0::2], z[:, 0::2, 1::2], z[:, 1::2, 1::2]], -1).reshape(-1, 4 * C)
    m = torch.from_numpy(rowmaps.merge_map_np(B, H, W).astype(np.int64))
    flat = torch.cat([x.view(-1, C), torch.zeros(1, C)])
    assert torch.equal(flat[m].reshape(-1, 4 * C), ref)


def test_library_exports_every_declared_symbol():
    from lavt_hip import _capi
    header = open(os.path.join(ROOT, "include", "lavt_hip.h")).read()
    declared = set(re.findall(r"\b(lavt_[a-z0-9_]+)\s*\(", header))
    assert declared, "no declarations parsed"
    assert declared == set(_capi.EXPORTED), declared ^ set(_capi.EXPORTED)
    for name in declared:
        assert hasattr(_capi.lib, name), f"liblavt_hip.so does not export {name}"
    assert _capi.lib.lavt_abi_version() == _capi.EXPECTED_ABI == 7


def test_struct_layout_matches_header():
    """ctypes mirrors of the parameter structs have one field per header member, in order."""
    from lavt_hip import _capi
    header = open(os.path.join(ROOT, "include", "lavt_hip.h")).read()
    for cname, st in (("lavt_gemm_nt", _capi.GemmNT), ("lavt_gemm_tn", _capi.GemmTN), ("lavt_gemm_nt_route", _capi.GemmNTRoute)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s_t;" % (cname, cname), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            for part in decl.split(","):
                names.append(re.findall(r"([A-Za-z_][A-Za-z0-9_]*)\s*$", part.strip())[0])
        assert names == [f[0] for f in st._fields_], (cname, names, [f[0] for f in st._fields_])


@pytest.mark.parametrize("variant,keys_file,w12", [("tiny", "state_dict_keys_swin_t.txt", False), ("base", "state_dict_keys_swin_b_w12.txt", True)])
def test_factory_state_dict_keys(variant, keys_file, w12):
    from lib import segmentation
    model = segmentation.lavt("", SimpleNamespace(swin_type=variant, window12=w12))
    keys = sorted(f"{k}|{'x'.join(map(str, v.shape))}" for k, v in model.state_dict().items())
    assert keys == open(os.path.join(GOLDEN, keys_file)).read().split()
    nodecay = [n for n, _ in model.backbone.named_parameters() if "norm" in n or "relative_position_bias_table" in n]
    assert nodecay and all(hasattr(model, a) for a in ("backbone", "classifier"))


def test_no_cpu_fallback():
    """The product path must fail loudly without a GPU: no CPU / eager fallback exists."""
    from lib import segmentation
    from lavt_hip.detweights import det_inputs
    model = segmentation.lavt("", SimpleNamespace(swin_type="tiny")).eval()
    x, l, m, _ = det_inputs(1, 64, 20)
    with pytest.raises(RuntimeError, match="GPU memory only"):
        model(x, l, m)


def test_sync_bn_conversion_is_seen():
    from lib.mask_predictor import SimpleDecoding
    dec = torch.nn.SyncBatchNorm.convert_sync_batchnorm(SimpleDecoding(64, SimpleNamespace()))
    assert isinstance(dec.bn1_4, torch.nn.SyncBatchNorm) and "bn1_4.running_var" in dec.state_dict()


# ---------------------------------------------------------------------------------------------------- video row maps
@pytest.mark.parametrize("dims,window", [((8, 10, 9), (8, 7, 7)), ((3, 10, 9), (8, 7, 7)), ((16, 7, 7), (8, 7, 7)), ((4, 13, 24), (4, 12, 12))])
@pytest.mark.parametrize("shifted", [0, 1])
def test_window_map3d_matches_pad_roll_partition(dims, window, shifted):
    """lib/video_swin_transformer.py:230-262: pad -> roll -> window_partition as one row map (+ the region table vs the oracle mask)"""
    from oracle import lavt_video_oracle as OV
    B, (D, H, W) = 2, dims
    win, shift = rowmaps.clip_window(dims, window, tuple(w // 2 for w in window) if shifted else (0, 0, 0))
    assert (win, shift) == OV.clip_window(dims, window, tuple(w // 2 for w in window) if shifted else (0, 0, 0))
    tok = torch.arange(B * D * H * W, dtype=torch.float32).view(B, D, H, W, 1) + 1          # 0 marks padding
    Dp, Hp, Wp = (rowmaps.padded(n, w) for n, w in zip(dims, win))
    u = torch.nn.functional.pad(tok, (0, 0, 0, Wp - W, 0, Hp - H, 0, Dp - D))
    if any(shift):
        u = torch.roll(u, tuple(-s for s in shift), (1, 2, 3))
    xw = u.view(B, Dp // win[0], win[0], Hp // win[1], win[1], Wp // win[2], win[2], 1).permute(0, 1, 3, 5, 2, 4, 6, 7).reshape(-1)
    m = rowmaps.window_map3d_np(B, D, H, W, win, shift)
    assert np.array_equal(m, xw.numpy().astype(np.int64) - 1)
    cover = m[m >= 0]
    assert len(np.unique(cover)) == B * D * H * W == len(cover)
    if any(shift):
        reg = rowmaps.region_ids3d_np(D, H, W, win, shift)
        mask = OV.shift_mask_3d(Dp, Hp, Wp, win, shift)
        assert np.array_equal(reg[:, :, None] != reg[:, None, :], (mask != 0).numpy())


SEPT_FLAGS = dict(sep_t_pwam=True, conv3d_kernel_size_t="3-3-3", conv3d_kernel_size_s="1-1-1", w_t3x3_s1x1=True, mm_t3x3_s1x1=True)


@pytest.mark.parametrize("tag,flags", [("pwam", {}), ("sept", SEPT_FLAGS)])
def test_video_factory_state_dict_keys(tag, flags):
    """lavt_video builds the reference's parameter set (names + shapes) for Video-Swin-B, default PWAM and the README SepTPWAM recipe"""
    from lib import segmentation
    model = segmentation.lavt_video("", SimpleNamespace(swin_type="base", bert_random_init=True, **flags))
    keys = sorted(f"{k}|{'x'.join(map(str, v.shape))}" for k, v in model.backbone.state_dict().items())
    assert keys == open(os.path.join(GOLDEN, f"state_dict_keys_video_swin_b_{tag}.txt")).read().split()      # backbone of the reference factory
    assert {k.split(".")[0] for k in model.state_dict()} == {"backbone", "classifier", "text_encoder"}


def test_video_unsupported_fusions_fail_loudly():
    from lib import segmentation
    with pytest.raises(NotImplementedError):
        segmentation.lavt_video("", SimpleNamespace(swin_type="tiny", ts_pwam=True, conv3d_kernel_size="3-1-1", bert_random_init=True))


# ---------------------------------------------------------------------------------------------------- checkpoint surgery
def test_checkpoint_loaders_match_reference(golden, tmp_path):
    """lavt_hip.checkpoint vs the reference's loaders run on the same synthetic checkpoints (mmcv_custom/checkpoint.py:287-360: prefix
    stripping + bicubic table resize; video_swin_transformer.py:759-805 inflate, :830-844 temporal sum of the 3-D patch embedding)"""
    from lavt_hip import checkpoint as ck
    from lavt_hip.detweights import fill_state_dict_
    from lib.backbone import MultiModalSwinTransformer
    from lib.video_swin_transformer import MultiModalSwinTransformer3D
    from synth_ckpt import synthetic_swin_checkpoint
    g = golden("checkpoint_surgery")
    a = SimpleNamespace()
    path = str(tmp_path / "swin2d.pth")
    torch.save({"state_dict": synthetic_swin_checkpoint()}, path)
    bb = MultiModalSwinTransformer(embed_dim=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8], window_size=7, ape=False, drop_path_rate=0.0,
                                   patch_norm=True, use_checkpoint=False, num_heads_fusion=[1, 1, 1, 1], fusion_drop=0.0, args=a)
    fill_state_dict_(bb)
    missing, unexpected = ck.load_swin_checkpoint(bb, path)
    assert unexpected == ["norm.weight"] and "layers.0.fusion.vis_project.0.weight" in missing and "layers.0.blocks.0.attn.qkv.weight" not in missing
    sd = bb.state_dict()
    for k in [k for k in g.files if k.startswith("swin2d|")]:
        assert np.array_equal(sd[k.split("|")[1]].numpy(), g[k]), k
    for tag, ckd in (("inflate", {"model": synthetic_swin_checkpoint(prefix="")}),
                     ("video3d", {"state_dict": {("backbone." + k): v for k, v in synthetic_swin_checkpoint(prefix="", patch_t=2, ws=7, index_n=392).items()}})):
        if tag == "video3d":
            for k in list(ckd["state_dict"]):
                if "relative_position_bias_table" in k:
                    ckd["state_dict"][k] = ckd["state_dict"][k].repeat(15, 1)
        path = str(tmp_path / (tag + ".pth"))
        torch.save(ckd, path)
        b3 = MultiModalSwinTransformer3D(patch_size=(1, 4, 4), embed_dim=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8], window_size=(8, 7, 7),
                                         drop_path_rate=0.0, patch_norm=True, out_indices=(0, 1, 2, 3), use_checkpoint=False,
                                         num_heads_fusion=[1, 1, 1, 1], fusion_drop=0.0, args=a)
        fill_state_dict_(b3)
        ck.load_video_swin_checkpoint(b3, path, inflate_2d=(tag == "inflate"))
        sd = b3.state_dict()
        for k in [k for k in g.files if k.startswith(tag + "|")]:
            assert np.array_equal(sd[k.split("|")[1]].numpy(), g[k]), k


def test_lavt_video_loads_2d_lavt_weights_as_train_py_does(golden, tmp_path):
    """train.py:572-578 of the reference: `model = segmentation.__dict__[args.model](...)`, then
    `model.load_from_pretrained2d_lavt_weights(path)` or `model.load_from_pretrained2d_lavt_weights_into_a_3d_model(path)`
    (lib/_utils.py:133-182 / :184-238): tables resized bicubically and repeated 2*Wd-1 times, patch embedding unsqueezed, index buffers dropped,
    and -- for the second form -- the 2-D `.fusion` tensors left out.  Expected tensors come from the reference's own methods (make_golden.py)."""
    from lib import segmentation
    from lavt_hip.detweights import fill_state_dict_
    from lib._utils import LAVTVideo
    from lib.mask_predictor import SimpleDecoding
    from lib.video_swin_transformer import MultiModalSwinTransformer3D
    from synth_ckpt import synthetic_lavt2d_checkpoint
    g = golden("lavt2d_into_video")
    path = str(tmp_path / "lavt2d.pth")
    torch.save({"model": synthetic_lavt2d_checkpoint()}, path)
    assert all(hasattr(segmentation.LAVTVideo, n) for n in ("forward_feats", "load_from_pretrained2d_lavt_weights", "load_from_pretrained2d_lavt_weights_into_a_3d_model"))
    a = SimpleNamespace(bert_random_init=True)
    for method in ("load_from_pretrained2d_lavt_weights", "load_from_pretrained2d_lavt_weights_into_a_3d_model"):
        b3 = MultiModalSwinTransformer3D(patch_size=(1, 4, 4), embed_dim=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8], window_size=(8, 7, 7),
                                         drop_path_rate=0.0, patch_norm=True, out_indices=(0, 1, 2, 3), use_checkpoint=False,
                                         num_heads_fusion=[1, 1, 1, 1], fusion_drop=0.0, args=a)
        model = LAVTVideo(b3, SimpleDecoding(256, a), a)
        text = {k: v.clone() for k, v in model.text_encoder.state_dict().items()}
        fill_state_dict_(model.backbone)            # keys as in the fixture's model: 'backbone.*' / 'classifier.*'
        with torch.no_grad():
            from lavt_hip.detweights import det_tensor
            for k, t in model.state_dict().items():
                if not k.startswith("text_encoder.") and not k.endswith("relative_position_index"):
                    t.copy_(det_tensor(k, t.shape, t.dtype))
        getattr(model, method)(path)
        sd = model.state_dict()
        keys = [k for k in g.files if k.startswith(method + "|")]
        assert len(keys) == 9
        for k in keys:
            assert np.array_equal(sd[k.split("|")[1]].numpy(), g[k]), k
        assert all(torch.equal(v, model.text_encoder.state_dict()[k]) for k, v in text.items())          # the text encoder is untouched


def test_init_weights_loads_a_checkpoint_path(tmp_path):
    """the factories' `pretrained` argument goes through the same loaders (lib/segmentation.py:59-64)"""
    from lib import segmentation
    from synth_ckpt import synthetic_swin_checkpoint
    path = str(tmp_path / "swin_tiny_window5.pth")
    torch.save({"model": synthetic_swin_checkpoint(embed=96, depths=(2, 2, 6, 2), heads=(3, 6, 12, 24), prefix="")}, path)
    model = segmentation.lavt(path, SimpleNamespace(swin_type="tiny"))
    want = synthetic_swin_checkpoint(embed=96, depths=(2, 2, 6, 2), heads=(3, 6, 12, 24), prefix="")["layers.2.blocks.3.attn.qkv.weight"]
    assert torch.equal(model.backbone.layers[2].blocks[3].attn.qkv.weight.detach(), want)


def test_grad_buckets_count_each_parameter_once():
    """A parameter may report 'gradient ready' twice per backward (fused accumulation + autograd's post-accumulate hook, which PyTorch runs
    even when the op returned no gradient tensor): a bucket must not launch before ALL of its parameters have reported."""
    from lavt_hip.ddp import GradBuckets
    net = torch.nn.Sequential(*[torch.nn.Linear(8, 8) for _ in range(4)])
    gb = GradBuckets(net, bucket_mib=1.0)
    assert len(gb.buckets) == 1
    gb.zero()
    ps = list(net.parameters())
    for p in ps[: len(ps) // 2]:
        gb._on_grad(p)
        gb._on_grad(p)                     # second report of the same parameter
    assert gb.launched == [False] and gb.pending == [len(ps) // 2]
    for p in ps[len(ps) // 2:]:
        gb._on_grad(p)
    assert gb.launched == [True]
    gb.zero()
    assert gb.pending == [0] and gb.launched == [False]


def test_grad_buckets_ignore_hooks_of_queued_weight_gradients():
    """Fused accumulation: a Linear whose weight gradient is queued for a grouped launch returns None from backward, and PyTorch runs the
    parameter's post-accumulate hook right away -- before the kernel exists.  Such a report must not count (the queue reports the parameter
    itself once the launch is enqueued), or the bucket would be reduced while the gradient is still being written."""
    from lavt_hip import ops
    from lavt_hip.ddp import GradBuckets
    net = torch.nn.Sequential(*[torch.nn.Linear(8, 8) for _ in range(2)])
    gb = GradBuckets(net, bucket_mib=1.0, fused_accumulation=True)
    try:
        gb.zero()
        ps = list(net.parameters())
        queued = ps[0]
        ops.wgrads.notify(queued)              # what _Linear.backward does after deferring the GEMM
        for p in ps:
            gb._on_grad(p)                     # autograd hooks of every parameter, the queued one included
        assert gb.launched == [False] and gb.pending == [len(ps) - 1]
        ops.wgrads.flush()                     # no queued GEMMs here; reports the parameter through sinks.on_ready
        assert gb.launched == [True] and not ops.wgrads.pending
    finally:
        ops.sinks.clear()
        ops.wgrads.ready, ops.wgrads.pending = [], set()


def test_grad_buckets_overlap_on_swin_b():
    """the parameters whose gradient exists only after backward (LayerNorm gamma / beta, relative_position_bias_table: one
    deferred reduction launch; layers.3.res_gate.*: never used) sit in ONE late bucket, so >= 95 % of the gradient bytes of Swin-B LAVT are in
    buckets that complete -- and are all-reduced -- while backward is still running.  Round 3 had 393 of 475 MB gated by 1 MB of such parameters."""
    from lib import segmentation
    from lavt_hip.ddp import GradBuckets, late_gradient_parameters
    model = segmentation.lavt("", SimpleNamespace(swin_type="base", window12=True))
    names = {id(p): n for n, p in model.named_parameters()}
    gb = GradBuckets(model, bucket_mib=32.0)
    late = {names[id(p)] for p in late_gradient_parameters(model)}
    assert "backbone.layers.3.res_gate.0.weight" in late and "backbone.layers.3.res_gate.2.weight" in late
    assert "backbone.layers.2.blocks.7.norm1.weight" in late and "backbone.layers.2.blocks.7.attn.relative_position_bias_table" in late
    assert "backbone.norm3.bias" in late and "backbone.layers.0.downsample.norm.weight" in late
    assert not any("qkv" in n or "fc1" in n or "classifier" in n or n.endswith("res_gate.0.weight") and "layers.3" not in n for n in late)
    deferred = [p for p in model.parameters() if names[id(p)] in late]
    # every late parameter is in the last bucket and no ordinary bucket holds one
    assert gb.late_bucket == len(gb.buckets) - 1
    assert all(gb.bucket_of[p] == gb.late_bucket for p in deferred)
    assert all(gb.bucket_of[p] != gb.late_bucket for p in model.parameters() if names[id(p)] not in late)
    clean = gb.overlappable_bytes()
    assert clean == sum(4 * (e - s) for b, (s, e) in enumerate(gb.buckets) if not any(gb.bucket_of[p] == b for p in deferred))
    assert clean >= 0.95 * gb.bytes_per_step(), (clean, gb.bytes_per_step())
    s, e = gb.buckets[gb.late_bucket]
    assert 4 * (e - s) < 12 << 20                       # 1.03 MB of norm / table parameters + the dead 2 x 1024 x 1024 gate
    # the views tile the flat buffer exactly once, in bucket order
    spans = sorted((gb.offset_of[id(p)], p.numel()) for p in model.parameters())
    off = 0
    for o, n in spans:
        assert o == off
        off += n
    assert off == gb.flat.numel()
    for p in model.parameters():
        assert p.grad.data_ptr() == gb.flat.data_ptr() + 4 * gb.offset_of[id(p)]


def test_grad_buckets_learn_unreported_parameters():
    """A parameter nothing reports during the first backward (unused in forward, unknown to late_gradient_parameters) is moved to the late
    bucket at the next zero(): from the second step on no ordinary bucket waits for finish()."""
    from lavt_hip.ddp import GradBuckets
    net = torch.nn.Sequential(*[torch.nn.Linear(8, 8, bias=False) for _ in range(4)])
    ps = list(net.parameters())
    gb = GradBuckets(net, bucket_mib=2 * 64 * 4 / (1 << 20))          # two weights per bucket
    assert len(gb.buckets) == 2 and gb.late_bucket is None
    dead = ps[2]
    from lavt_hip import ddp, optim
    gen0, grads0 = ddp.layout_generation[0], [p.grad.data_ptr() for p in ps]
    for step in range(3):
        gb.zero()
        if step == 1:
            # the relayout moved gradient views: the generation FusedAdamW keys its descriptor table on (also under check_tables=False) moved with it
            assert ddp.layout_generation[0] == gen0 + 1 and [p.grad.data_ptr() for p in ps] != grads0
            assert optim.ops_generation()[1] == ddp.layout_generation[0]
        if step == 2:
            assert ddp.layout_generation[0] == gen0 + 1
        for p in reversed(ps):
            if p is not dead:
                gb._on_grad(p)
        before = [l for l in gb.launch_log]
        gb.finish()
        if step == 0:
            assert [b for b, _, _ in before] == [1] and gb.launch_log[-1][2] == "finish"       # bucket 0 = {ps[3], ps[2]} waited for finish()
        else:
            assert gb.late_bucket == 2 and gb.bucket_of[dead] == 2
            assert sorted(b for b, _, w in before if w == "backward") == [0, 1]                 # both ordinary buckets complete during backward
            assert [(b, w) for b, _, w in gb.launch_log[len(before):]] == [(2, "finish")]
        assert all(gb.launched)


def test_grad_buckets_zero_fill_skip_list():
    """GradBuckets.set_zero_skip: zero() clears everything of the flat buffer EXCEPT the parameters whose gradient launch overwrites its buffer (the
    step harness verifies the list on the captured graph); the list dies with a layout change and with set_zero_skip(None)."""
    from lavt_hip.ddp import GradBuckets
    net = torch.nn.Sequential(torch.nn.Linear(8, 8), torch.nn.LayerNorm(8), torch.nn.Linear(8, 4), torch.nn.Linear(4, 4, bias=False))
    ps = list(net.parameters())
    gb = GradBuckets(net, bucket_mib=2 * 64 * 4 / (1 << 20))
    weights = [p for p in ps if p.dim() == 2]
    n = gb.set_zero_skip({id(p) for p in weights} | {12345})          # (an id it does not own is ignored)
    assert n == sum(p.numel() for p in weights)
    assert sum(v.numel() for v in gb._zero_views) + n == gb.flat.numel()
    gb.flat.fill_(7.0)
    gb.zero()
    for p in ps:
        want = 7.0 if p.dim() == 2 else 0.0
        assert float(p.grad.min()) == want and float(p.grad.max()) == want, (tuple(p.shape), want)
    assert float(gb.flat.sum()) == 7.0 * n                               # padding between buckets, if any, is cleared too
    gb.set_zero_skip(None)
    gb.flat.fill_(7.0)
    gb.zero()
    assert float(gb.flat.abs().sum()) == 0.0
    gb.set_zero_skip({id(weights[0])})
    gb._layout(gb.late_ids)                                              # a new layout invalidates the offsets the list was built from
    assert gb._zero_views is None


class _WgradCase:
    """ops._linear_wgrad driven on the CPU: n = 3 outputs, kd = 5 inputs, 7 rows (so that a transposed operand cannot pass), the A block at column 1
    of a [7, 4] matrix.  ops.gemm_tn is replaced by a fake that records its keyword arguments (and its row count, as Kd) and writes A[:, a_off:a_off + n]^T B
    and its column sums, over the rows it is given and through the row maps it is given."""
    n, kd, rows, a_off = 3, 5, 7, 1

    def __init__(self, monkeypatch, ops, dtype=torch.bfloat16, sink=True, enabled=False):
        g = torch.Generator().manual_seed(3)
        self.ops, self.dtype, self.calls, self.ready = ops, dtype, [], []
        self.A = torch.randn(self.rows, self.n + 1, generator=g).to(dtype)
        self.B = torch.randn(self.rows, self.kd, generator=g).to(dtype)
        blk = self.A[:, self.a_off:self.a_off + self.n].float()
        self.want_w, self.want_b = blk.T @ self.B.float(), blk.sum(0)
        self.w, self.b = torch.nn.Parameter(torch.zeros(self.n, self.kd)), torch.nn.Parameter(torch.zeros(self.n))
        if sink:
            self.w.grad, self.b.grad = torch.zeros(self.n, self.kd), torch.zeros(self.n)
            ops.sinks.set([self.w, self.b], on_ready=self.ready.append)
        ops.wgrads.enabled = enabled
        monkeypatch.setattr(ops, "gemm_tn", self.fake_tn)

    def fake_tn(self, dtype, I, J, Kd, A, lda, B, ldb, Cout, ldc, **kw):
        assert (I, J, lda, ldb, ldc) == (self.n, self.kd, self.n + 1, self.kd, self.kd) and Kd <= self.rows and Cout.shape == (I, J)
        self.calls.append(dict(kw, Kd=Kd))
        ra, rb = (kw.get(k) if kw.get(k) is not None else torch.arange(Kd) for k in ("a_rowmap", "b_rowmap"))       # Kd rows of each operand, through its map
        blk = A[ra, kw.get("a_off", 0):kw.get("a_off", 0) + I].float()
        Cout.copy_(blk.T @ B[rb].float())
        if kw.get("colsum") is not None:
            kw["colsum"].copy_(blk.sum(0))

    def run(self, bias=True, **tn):
        return self.ops._linear_wgrad(self.dtype, self.w, self.b if bias else None, self.n, self.kd, self.rows, self.A, self.n + 1, self.B, self.kd,
                                      a_off=self.a_off, **tn)

    def deferred(self):
        (kw,) = self.calls
        assert kw.get("defer") is None or kw["defer"] is self.ops.wgrads
        return kw.get("defer") is not None

    def ready_is(self, *params):
        return len(self.ready) == len(params) and all(r is p for r, p in zip(self.ready, params))


def test_linear_wgrad_without_sinks_returns_the_gradients(monkeypatch):
    from lavt_hip import ops
    with ops.use_context(ops.StepContext()):
        c = _WgradCase(monkeypatch, ops, sink=False, enabled=True)
        dW, db = c.run()
        assert not c.deferred()
        assert dW.shape == c.w.shape and db.shape == c.b.shape and torch.equal(dW, c.want_w) and torch.equal(db, c.want_b)
        assert not ops.wgrads.pending and not c.ready


def test_linear_wgrad_into_sinks_reports_each_parameter_once(monkeypatch):
    """sinks without the grouped launch: backward returns None for both, the sink views hold the result, on_ready once per parameter, w before b"""
    from lavt_hip import ops
    with ops.use_context(ops.StepContext()):
        c = _WgradCase(monkeypatch, ops, enabled=False)
        assert c.run() == (None, None) and not c.deferred()
        assert torch.equal(c.w.grad, c.want_w) and torch.equal(c.b.grad, c.want_b)
        assert c.ready_is(c.w, c.b) and not ops.wgrads.pending
        with pytest.raises(RuntimeError, match="second weight gradient for the same parameter"):       # _GradSinks.buf: one gradient per parameter per step
            c.run()


def test_linear_wgrad_grouped_holds_the_report_until_the_flush(monkeypatch):
    """the grouped launch: the member is queued (defer = the queue), both parameters are pending and unreported until flush() has enqueued the group"""
    from lavt_hip import ops
    with ops.use_context(ops.StepContext()):
        c = _WgradCase(monkeypatch, ops, enabled=True)
        assert c.run() == (None, None) and c.deferred()
        assert ops.wgrads.pending == {id(c.w), id(c.b)} and not c.ready
        ops.wgrads.flush()                     # the fake queued nothing: no launch, only the reports
        assert c.ready_is(c.w, c.b) and not ops.wgrads.pending
        with pytest.raises(RuntimeError, match="second weight gradient for the same parameter"):
            c.run()


@pytest.mark.parametrize("dtype,tn,grouped", [(torch.float32, {}, False),
                                              (torch.bfloat16, dict(a_rowscale=torch.ones(7), a_rowscale_binary=False), False),
                                              (torch.bfloat16, dict(a_rowscale=torch.ones(7), a_rowscale_binary=True, alpha=0.5), True)],
                         ids=["fp32", "rowscale", "binary-rowscale"])
def test_linear_wgrad_grouping_rule(monkeypatch, dtype, tn, grouped):
    """queue active + every target a sink is not enough: bf16 only, and a row scale only as a row mask"""
    from lavt_hip import ops
    with ops.use_context(ops.StepContext()):
        c = _WgradCase(monkeypatch, ops, dtype=dtype, enabled=True)
        assert c.run(**tn) == (None, None) and c.deferred() == grouped
        assert all(c.calls[0][k] is v for k, v in tn.items())                     # handed through to the launch as given
        assert torch.equal(c.w.grad, c.want_w) and torch.equal(c.b.grad, c.want_b)
        if grouped:
            assert ops.wgrads.pending == {id(c.w), id(c.b)} and not c.ready
        else:
            assert c.ready_is(c.w, c.b) and not ops.wgrads.pending


@pytest.mark.parametrize("enabled", [False, True], ids=["immediate", "grouped"])
def test_linear_wgrad_without_bias_touches_one_parameter(monkeypatch, enabled):
    """b = None (no bias, or its gradient is not needed): one buffer, one notification, no column sum"""
    from lavt_hip import ops
    with ops.use_context(ops.StepContext()):
        c = _WgradCase(monkeypatch, ops, enabled=enabled)
        assert c.run(bias=False) == (None, None) and c.deferred() == enabled
        assert c.calls[0]["colsum"] is None and ops.sinks.used == {id(c.w)}
        assert torch.equal(c.w.grad, c.want_w) and not c.b.grad.any()
        assert ops.wgrads.pending == ({id(c.w)} if enabled else set()) and c.ready_is(*(() if enabled else (c.w,)))
        ops.wgrads.flush()
        assert c.ready_is(c.w) and not ops.wgrads.pending


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["grouped", "immediate"])
def test_linear_wgrad_grouped_arguments_replace_the_launch_only_in_a_group(monkeypatch, dtype):
    """grouped= (the token-order form of _Linear): its row count and gemm_tn arguments replace the caller's in a launch that joins a group, and are
    ignored in one that does not"""
    from lavt_hip import ops
    with ops.use_context(ops.StepContext()):
        c = _WgradCase(monkeypatch, ops, dtype=dtype, enabled=True)
        given = dict(a_rowmap=torch.arange(c.rows), b_rowmap=None, a_rowscale=torch.ones(c.rows), a_rowscale_div=4, a_rowscale_binary=True, alpha=0.5)
        inv = torch.arange(c.rows - 1)
        assert c.run(grouped=dict(rows=c.rows - 1, a_rowmap=None, b_rowmap=inv, a_rowscale_div=2), **given) == (None, None)
        kw = c.calls[0]
        if c.deferred():
            assert dtype == torch.bfloat16
            assert kw["Kd"] == c.rows - 1 and kw["a_rowmap"] is None and kw["b_rowmap"] is inv and kw["a_rowscale_div"] == 2
            assert all(kw[k] is given[k] for k in ("a_rowscale", "a_rowscale_binary", "alpha"))      # what the group form does not name stays
            blk = c.A[:c.rows - 1, c.a_off:c.a_off + c.n].float()
            assert torch.equal(c.w.grad, blk.T @ c.B[:c.rows - 1].float()) and torch.equal(c.b.grad, blk.sum(0))
            assert ops.wgrads.pending == {id(c.w), id(c.b)} and not c.ready
        else:
            assert dtype == torch.float32
            assert kw["Kd"] == c.rows and all(kw[k] is v for k, v in given.items())
            assert torch.equal(c.w.grad, c.want_w) and torch.equal(c.b.grad, c.want_b)
            assert c.ready_is(c.w, c.b) and not ops.wgrads.pending


class _LnCase:
    """ops._LnBwd / ops._ln_bwd driven on the CPU: 7 rows x 8 channels, the two leaf launchers replaced by fakes that record their arguments, the
    parking arena shrunk to `arena` floats"""
    rows, C = 7, 8

    def __init__(self, monkeypatch, ops, sink=True, enabled=True, arena=1 << 12):
        g = torch.Generator().manual_seed(5)
        self.ops, self.partial, self.now, self.ready = ops, [], [], []
        self.gamma, self.beta = torch.nn.Parameter(torch.ones(self.C)), torch.nn.Parameter(torch.zeros(self.C))
        if sink:
            self.gamma.grad, self.beta.grad = torch.zeros(self.C), torch.zeros(self.C)
            ops.sinks.set([self.gamma, self.beta], on_ready=self.ready.append)
        ops.wgrads.enabled = enabled
        monkeypatch.setattr(ops._LnDeferred, "ARENA_FLOATS", arena)
        monkeypatch.setattr(ops, "_ln_bwd_partial", lambda *a, **kw: self.partial.append((a, kw)))
        monkeypatch.setattr(ops, "_ln_bwd_now", lambda *a: self.now.append(a))
        self.dy, self.x, self.dx, self.dres, self.xn = (torch.randn(self.rows, self.C, generator=g) for _ in range(5))
        self.mean, self.rstd = torch.randn(self.rows, generator=g), torch.rand(self.rows, generator=g)
        self.nblk = int(ops.K.lib.lavt_layernorm_bwd_blocks(ops.K.dt(torch.float32), self.rows, self.C))
        assert self.nblk >= 1

    def args(self):
        return self.dy, self.x, self.gamma, self.beta, self.mean, self.rstd, self.dx, self.dres, self.rows, self.C

    def is_rider(self, t, ws_floats):
        """the ten fields _WgradQueue.add(rider=) / flush() unpack: (dy, x, gamma, mean, rstd, dx, ws, dres, rows, C)"""
        dy_, x_, g_, mean_, rstd_, dx_, ws_, dres_, rows_, C_ = t
        same = all(a is b for a, b in ((dy_, self.dy), (x_, self.x), (mean_, self.mean), (rstd_, self.rstd), (dx_, self.dx), (dres_, self.dres)))
        return (same and g_.data_ptr() == self.gamma.data_ptr() and not g_.requires_grad and (rows_, C_) == (self.rows, self.C)
                and ws_.numel() == ws_floats and ws_.dtype == torch.float32 and ws_.data_ptr() == self.ops.ln_deferred.arena.data_ptr())

    def parked_row(self, ws):
        return (ws.data_ptr(), self.nblk, self.C, self.gamma.grad.data_ptr(), self.beta.grad.data_ptr())


def test_ln_handoff_without_sinks_reduces_at_once_and_returns_the_gradients(monkeypatch):
    from lavt_hip import ops
    with ops.use_context(ops.StepContext()):
        c = _LnCase(monkeypatch, ops, sink=False)
        g_g, g_b = ops._ln_bwd(*c.args())
        assert not c.partial and len(c.now) == 1
        dy, x, gather, gamma, beta, mean, rstd, dx, xn, dg, db, dres, rows, C = c.now[0]
        assert dy is c.dy and x is c.x and gather is None and beta is None and xn is None and mean is c.mean and rstd is c.rstd and dx is c.dx and dres is c.dres
        assert gamma.data_ptr() == c.gamma.data_ptr() and (rows, C) == (c.rows, c.C)
        assert g_g.shape == g_b.shape == (c.C,) and g_g.data_ptr() == dg.data_ptr() and g_b.data_ptr() == db.data_ptr() and dg.data_ptr() != db.data_ptr()
        assert not ops.ln_deferred.items and not ops.wgrads.pending


def test_ln_handoff_into_sinks_parks_the_partial_sums(monkeypatch):
    """sinks + the step harness: the partial-sum launcher gets an arena slice of nblk * 2 * C floats, ONE row lands in ln_deferred.items, both parameters
    are pending (reported at the flush), backward returns None for both"""
    from lavt_hip import ops
    with ops.use_context(ops.StepContext()):
        c = _LnCase(monkeypatch, ops)
        assert ops._ln_bwd(*c.args()) == (None, None)
        assert not c.now and len(c.partial) == 1
        a, kw = c.partial[0]
        assert c.is_rider(a, c.nblk * 2 * c.C) and kw == dict(gather=None, beta=None, xn=None, carry=True)
        assert ops.ln_deferred.items == [c.parked_row(a[6])]
        assert ops.wgrads.pending == {id(c.gamma), id(c.beta)} and not c.ready
        assert ops.sinks.used == {id(c.gamma), id(c.beta)}


@pytest.mark.parametrize("why", ["arena-too-small", "queue-off"])
def test_ln_handoff_into_sinks_that_cannot_park_reports_each_parameter_once(monkeypatch, why):
    from lavt_hip import ops
    with ops.use_context(ops.StepContext()):
        probe = _LnCase(monkeypatch, ops, sink=False)
        c = _LnCase(monkeypatch, ops, enabled=why != "queue-off", arena=probe.nblk * 2 * probe.C - (1 if why == "arena-too-small" else 0))
        assert ops._ln_bwd(*c.args()) == (None, None)
        assert not c.partial and len(c.now) == 1
        assert c.now[0][9].data_ptr() == c.gamma.grad.data_ptr() and c.now[0][10].data_ptr() == c.beta.grad.data_ptr()       # added straight into the sinks
        assert len(c.ready) == 2 and c.ready[0] is c.gamma and c.ready[1] is c.beta
        assert not ops.ln_deferred.items and not ops.wgrads.pending


@pytest.mark.parametrize("sink", [False, True], ids=["immediate", "parked"])
def test_ln_handoff_xn_form_passes_beta_and_xn_through(monkeypatch, sink):
    from lavt_hip import ops
    with ops.use_context(ops.StepContext()):
        c = _LnCase(monkeypatch, ops, sink=sink)
        gather = torch.zeros(c.rows, 4, dtype=torch.int32)
        ops._ln_bwd(*c.args(), gather=gather, xn=c.xn)
        if sink:
            (a, kw), = c.partial
            assert kw["xn"] is c.xn and kw["beta"].data_ptr() == c.beta.data_ptr() and not kw["beta"].requires_grad and kw["gather"] is gather and kw["carry"] is True
        else:
            (a,) = c.now
            assert a[8] is c.xn and a[4].data_ptr() == c.beta.data_ptr() and not a[4].requires_grad and a[2] is gather


def test_ln_handoff_rider_form(monkeypatch):
    """_WmsaFused.backward's use: the decision hands out the rider, the node queues its weight gradients, the completion launches nothing when told the
    rider rode -- and the partial-sum launch without a carried job when it did not.  Either way the arena slice is registered once."""
    from lavt_hip import ops
    for rode in (True, False):
        with ops.use_context(ops.StepContext()):
            c = _LnCase(monkeypatch, ops)
            ln = ops._LnBwd(*c.args())
            assert isinstance(ln.rider, tuple) and len(ln.rider) == 10 and c.is_rider(ln.rider, c.nblk * 2 * c.C)
            assert not c.partial and not c.now and not ops.ln_deferred.items          # nothing launched or registered by the decision
            assert ln.close(rode=rode, carry=False) == (None, None)
            assert not c.now and ops.ln_deferred.items == [c.parked_row(ln.rider[6])] and ops.wgrads.pending == {id(c.gamma), id(c.beta)}
            if rode:
                assert not c.partial
            else:
                (a, kw), = c.partial
                assert a == ln.rider and kw == dict(gather=None, beta=None, xn=None, carry=False)
    with ops.use_context(ops.StepContext()):
        c = _LnCase(monkeypatch, ops, sink=False)
        ln = ops._LnBwd(*c.args())
        assert ln.rider is None
        g_g, g_b = ln.close(rode=False, carry=False)
        assert len(c.now) == 1 and not c.partial and g_g.shape == (c.C,) and g_b.shape == (c.C,)


class _ConvCase:
    """ops._conv_contract driven on the CPU: a 3x3 convolution over 6 rows, ops.gemm_nt and the two reduction entry points replaced by recording fakes.
    The expected keyword arguments are those of the launches _ConvTaps.forward / .backward and conv3x3_bn_relu_folded spelled out before the helper."""
    M, N, taps = 6, 16, 9

    def __init__(self, monkeypatch, ops):
        self.ops, self.nt, self.reduce = ops, [], []
        monkeypatch.setattr(ops, "gemm_nt", lambda *a, **kw: self.nt.append((a, kw)) or "stats")
        monkeypatch.setattr(ops.K, "ptr", lambda t: None if t is None else t.data_ptr())
        monkeypatch.setattr(ops.K, "stream", lambda: 0)
        for name in ("lavt_splitk_reduce", "lavt_splitk_reduce_epi"):
            monkeypatch.setattr(ops.K.lib, name, lambda *a, _n=name: self.reduce.append((_n, a)) or 0, raising=False)
        self.out = torch.empty(self.M, self.N, dtype=torch.bfloat16)
        self.geom = (2, 3, 128, 0, 1, 1, 3, 3)

    def unset(self, kw, *names):
        defaults = dict(batch=1, strideB=0, strideC=0, c_f32=False, conv_tap_split=0, conv_kc_split=0, b_off=0, b_tap_stride=0, A2=None, bias=None,
                        act=self.ops.K.ACT_NONE, want_colstats=False, Cpre=None, b_kmajor=False)
        return all(n not in kw or (not torch.is_tensor(kw[n]) and kw[n] == defaults[n]) for n in names)          # absent, or gemm_nt's default


@pytest.mark.parametrize("split", [(0, False), (3, False), (2, True)], ids=["whole", "tap-groups", "channel-pieces"])
@pytest.mark.parametrize("epilogue", [False, True], ids=["plain", "bias-relu"])
def test_conv_contract_weight_major(monkeypatch, split, epilogue):
    """forward / folded forward: A2 / lda2 / a_split reach every launch; the epilogue (and Cpre, the statistics request) only the unsplit one; the pieces
    are summed by lavt_splitk_reduce, or by lavt_splitk_reduce_epi with the bias and the activation"""
    from lavt_hip import ops
    c = _ConvCase(monkeypatch, ops)
    M, N, taps, Kc, C1, C2 = c.M, c.N, c.taps, 128, 64, 64
    x1, x2, Wp = torch.empty(M, C1, dtype=torch.bfloat16), torch.empty(M, C2, dtype=torch.bfloat16), torch.empty(N, taps * Kc, dtype=torch.bfloat16)
    bias, act = (torch.zeros(N), ops.K.ACT_RELU) if epilogue else (None, ops.K.ACT_NONE)
    pre = torch.empty_like(c.out)
    got = ops._conv_contract(torch.bfloat16, split, M, N, Kc, taps, x1, C1, Wp, taps * Kc, c.out, c.geom, bias=bias, act=act, A2=x2, lda2=C2, a_split=C1,
                             Cpre=pre, ldcpre=N, want_colstats=True)
    (a, kw), = c.nt
    sp, over_ch = split
    assert a[:2] == (torch.bfloat16, M) and a[2] == N and a[4] is x1 and a[5] == C1 and a[6] is Wp and a[7] == taps * Kc and a[9] == N
    assert kw["A2"] is x2 and kw["lda2"] == C2 and kw["a_split"] == C1 and kw["conv"] == c.geom and c.unset(kw, "b_kmajor", "b_off", "b_tap_stride")
    if not sp:
        assert got == "stats" and a[3] == taps * Kc and a[8] is c.out and not c.reduce
        assert kw["bias"] is bias and kw["act"] == act and kw["Cpre"] is pre and kw["ldcpre"] == N and kw["want_colstats"] is True
        assert c.unset(kw, "batch", "strideB", "strideC", "c_f32", "conv_tap_split", "conv_kc_split")
        return
    parts = a[8]
    assert got is None and parts.shape == (sp, M, N) and parts.dtype == torch.float32
    assert kw["batch"] == sp and kw["strideC"] == M * N and kw["c_f32"] is True and c.unset(kw, "bias", "act", "want_colstats", "Cpre")
    if over_ch:
        assert a[3] == taps * (Kc // sp) == 576 and kw["conv_kc_split"] == Kc // sp == 64 and c.unset(kw, "conv_tap_split", "strideB")
    else:
        assert a[3] == (taps // sp) * Kc == 384 and kw["conv_tap_split"] == taps // sp == 3 and kw["strideB"] == (taps // sp) * Kc == 384 and c.unset(kw, "conv_kc_split")
    (name, r), = c.reduce
    head, tail = (ops.K.dt(torch.bfloat16), parts.data_ptr(), sp, M, N), (c.out.data_ptr(), N, 0)
    if epilogue:
        assert name == "lavt_splitk_reduce_epi" and r == head + (bias.data_ptr(), ops.K.ACT_RELU) + tail
    else:
        assert name == "lavt_splitk_reduce" and r == head + tail


@pytest.mark.parametrize("split", [(0, False), (3, False), (2, True)], ids=["whole", "tap-groups", "channel-pieces"])
def test_conv_contract_k_major_column_block(monkeypatch, split):
    """the data gradient onto one column block of the packed weight [Cout][taps][Cin]: b_kmajor with the tap stride Cin and the block's offset in every
    launch; tap groups need NO strideB in this layout; always the plain reduction"""
    from lavt_hip import ops
    c = _ConvCase(monkeypatch, ops)
    M, N, taps, Cout, Cin, boff = c.M, c.N, c.taps, 128, 80, 64
    dy, Wp = torch.empty(M, Cout, dtype=torch.bfloat16), torch.empty(Cout, taps * Cin, dtype=torch.bfloat16)
    geom = (2, 3, Cout, 1, 1, 1, 3, 3)
    got = ops._conv_contract(torch.bfloat16, split, M, N, Cout, taps, dy, Cout, Wp, taps * Cin, c.out, geom, b_kmajor=True, b_tap_stride=Cin, b_off=boff)
    (a, kw), = c.nt
    sp, over_ch = split
    assert a[:3] == (torch.bfloat16, M, N) and a[4] is dy and a[5] == Cout and a[6] is Wp and a[7] == taps * Cin and a[9] == N
    assert kw["b_kmajor"] is True and kw["b_tap_stride"] == Cin and kw["b_off"] == boff and kw["conv"] == geom
    assert c.unset(kw, "A2", "bias", "act", "want_colstats", "Cpre", "strideB")
    if not sp:
        assert got == "stats" and a[3] == taps * Cout and a[8] is c.out and not c.reduce
        assert c.unset(kw, "batch", "strideC", "c_f32", "conv_tap_split", "conv_kc_split")
        return
    parts = a[8]
    assert got is None and parts.shape == (sp, M, N) and parts.dtype == torch.float32
    assert kw["batch"] == sp and kw["strideC"] == M * N and kw["c_f32"] is True
    if over_ch:
        assert a[3] == taps * (Cout // sp) == 576 and kw["conv_kc_split"] == 64 and c.unset(kw, "conv_tap_split")
    else:
        assert a[3] == (taps // sp) * Cout == 384 and kw["conv_tap_split"] == 3 and c.unset(kw, "conv_kc_split")
    assert c.reduce == [("lavt_splitk_reduce", (ops.K.dt(torch.bfloat16), parts.data_ptr(), sp, M, N, c.out.data_ptr(), N, 0))]


@pytest.mark.parametrize("crit", ["ce", "dice", "dice_boundary"])
@pytest.mark.parametrize("which", ["fwd", "bwd"])
def test_criterion_entry_rule(monkeypatch, crit, which):
    """every fused criterion pass has a plain and a _sel_ entry point, the second with (selection pointer, int32 length) directly after x; ops._criterion_entry
    names exactly that entry point and inserts exactly those two arguments"""
    import ctypes as C
    from lavt_hip import _capi as K
    from lavt_hip import ops
    plain, sel = f"lavt_upsample_{crit}_{which}", f"lavt_upsample_{crit}_sel_{which}"
    assert plain in K._PROTOTYPES and sel in K._PROTOTYPES
    want = list(K._PROTOTYPES[plain])
    want[2:2] = [C.c_void_p, C.c_int32]
    assert K._PROTOTYPES[sel] == want

    class _Names:
        def __getattr__(self, name):
            return name
    monkeypatch.setattr(ops.K, "lib", _Names())
    assert ops._criterion_entry(crit, which, None) == (plain, ())
    frames = SimpleNamespace(is_cuda=True, data_ptr=lambda: 4096, numel=lambda: 3)
    assert ops._criterion_entry(crit, which, frames) == (sel, (4096, 3))


def test_syncbn_rank_statistics_combination():
    """SyncBN forward: the ranks' (sum, centred M2) pairs, gathered with ONE collective, combine to the statistics of the whole batch --
    also when the channel means are large compared with the spread (no E[x^2] - E[x]^2 cancellation)"""
    from lavt_hip.ops import combine_rank_stats
    g = torch.Generator().manual_seed(0)
    world, R, C = 3, 50, 7
    x = torch.randn(world, R, C, generator=g, dtype=torch.float64) * 0.01 + 100.0 * torch.arange(1, C + 1)
    per_rank = torch.stack([torch.stack([x[r].sum(0), ((x[r] - x[r].mean(0)) ** 2).sum(0)]) for r in range(world)]).float()
    s = combine_rank_stats(per_rank, R)
    flat = x.reshape(world * R, C)
    assert torch.allclose(s[0].double(), flat.sum(0), rtol=1e-6)
    assert torch.allclose(s[1].double(), ((flat - flat.mean(0)) ** 2).sum(0), rtol=2e-3)


# ---------------------------------------------------------------------------------------------- host input pipeline
_VOCAB = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", "the", "man", "in", "a", "red", "shirt", "##s", "left", "person", "play", "##ing", "frisbee",
          ",", ".", "'", "s", "woman", "2", "##nd", "from", "right", "cafe", "-", "top", "##most", "un", "##believ", "##able", "(", ")", "on", "!", "?",
          "guy", "w", "/", "hat", "3", "##rd", "giraffe", "##s", "中", "国"]
_SENTENCES = ["The man's red shirts, playing frisbee. 2nd from LEFT café", "woman on the right (top-most)!", "unbelievable giraffes?? 3rd guy w/ hat",
              "  person\tin   a\nred shirt  ", "xyzzy the 中国 man", "", "a" * 120 + " man", "[SEP] the [MASK] man"]


def test_bert_tokenizer_matches_transformers(tmp_path):
    """bert.tokenization_bert.BertTokenizer against the installed transformers.BertTokenizer on a synthetic vocab (no vocab.txt ships offline)"""
    import transformers
    from bert.tokenization_bert import BertTokenizer, pad_ids
    vf = tmp_path / "vocab.txt"
    vf.write_text("\n".join(_VOCAB) + "\n", encoding="utf-8")
    ours, theirs = BertTokenizer.from_pretrained(str(tmp_path)), transformers.BertTokenizer(str(vf))
    for s in _SENTENCES:
        assert ours.encode(text=s, add_special_tokens=True) == theirs.encode(s, add_special_tokens=True), s
    ids, mask = pad_ids(ours.encode(_SENTENCES[0]), 20)
    assert len(ids) == len(mask) == 20 and sum(mask) == min(20, len(ours.encode(_SENTENCES[0]))) and ids[0] == 2
    ids, mask = pad_ids(ours.encode(_SENTENCES[1]), 5)
    assert len(ids) == 5 and mask == [1] * 5


def test_image_transforms():
    """transforms.py of the reference on PIL: exact size, [0, 1] scaling, per-channel normalisation, nearest-neighbour targets"""
    from PIL import Image
    import transforms as T
    rng = np.random.default_rng(0)
    img = Image.fromarray(rng.integers(0, 256, (37, 53, 3), dtype=np.uint8), "RGB")
    tgt = Image.fromarray((rng.random((37, 53)) > 0.5).astype(np.uint8), "P")
    x, t = T.get_transform(48)(img, tgt)
    assert x.shape == (3, 48, 48) and x.dtype == torch.float32 and t.shape == (48, 48) and t.dtype == torch.int64
    assert set(t.unique().tolist()) <= {0, 1}
    ref = torch.from_numpy(np.asarray(img.resize((48, 48), Image.BILINEAR)).transpose(2, 0, 1).copy()).float() / 255
    mean, std = torch.tensor([0.485, 0.456, 0.406]).view(3, 1, 1), torch.tensor([0.229, 0.224, 0.225]).view(3, 1, 1)
    assert torch.allclose(x, (ref - mean) / std, atol=1e-6)
    same, _ = T.Resize(37, 53)(img, None)
    assert np.array_equal(np.asarray(same), np.asarray(img))


def test_fp8_twin_registry_and_sites_host_logic():
    """configs[4] host bookkeeping (lavt_hip/ops.py, no kernel launch): which convolutions get a quantisation site (fp8_act_site / fp8_dy_site follow the
    convolution's own fp8 conditions), a producer-written twin is picked up exactly once by the site it was written for, a twin of another site or shape is
    not, entries keep their tensor alive (no address re-use while they live), advance() forgets them, and in bf16 mode nothing asks for a site."""
    import lavt_hip
    from lavt_hip import ops
    w = torch.nn.Parameter(torch.zeros(512, 640, 3, 3))
    assert ops.fp8_act_site(w, 57600, 512, 128) is None and ops.fp8_dy_site(w, 57600, 512) is None          # bf16 mode
    st = ops._Fp8State()
    with lavt_hip.use_dtype("fp8"):
        assert ops.fp8_act_site(w, 57600, 512, 128) == id(w)                       # 450 x 4 tiles: fills the chip
        assert ops.fp8_act_site(w, 3600, 512, 128) is None                         # decoder level 4: 29 x 4 tiles stay bf16
        assert ops.fp8_act_site(w, 57600, 520, 128) is None                        # channels % 16
        assert ops.fp8_dy_site(w, 57600, 512) == (id(w), "dy") and ops.fp8_dy_site(w, 1800, 512) is None
        y = torch.zeros(64, 32, dtype=torch.bfloat16)
        q = torch.zeros(64, 32, dtype=torch.uint8)
        a_prev, a_cur = st.site_ptrs("site", y.device)
        assert a_cur != a_prev and st.site_ptrs("site", y.device) == (a_prev, a_cur)
        st.put_twin(y, q, a_prev)
        assert st.twins[(y.data_ptr(), y.numel())][2] is y                          # the entry holds the tensor
        got = st.quantize(y, "site")
        assert got[0] is q and got[1] == a_prev and not st.twins                    # picked up: no launch (a launch on CPU tensors would raise)
        st.put_twin(y, q, a_prev)
        with pytest.raises(RuntimeError):                                           # another site's scale: the twin is dropped and the quantiser must run -> refuses CPU memory
            st.quantize(y, "other site")
        assert not st.twins
        st.put_twin(y, q, a_prev)
        st.put_dy_amax(y, a_cur)
        assert st.twins and st.dy_amax
        st.slots.clear()                                                            # (no sites: advance() then launches nothing -- the roll-over kernel itself is a GPU test)
        st.advance()
        assert not st.twins and not st.dy_amax
        # the producer shortcuts exist only between advance() and end_step() (round-5 advisor: outside the step harness nothing zeroes the `cur` slot a
        # gradient |max| is max-ed into, and nothing drops unclaimed twins)
        assert st.step_active
        st.put_twin(y, q, a_prev)
        st.put_dy_amax(y, a_cur)
        st.end_step()
        assert not st.step_active and not st.twins and not st.dy_amax
    assert not ops._Fp8State().step_active, "a fresh state (an eager loop without the harness) never takes the producer path"


def test_env_switch_table_matches_the_tree():
    """Every LAVT_* environment variable the product reads -- getenv / env_int / env_is in csrc/, os.environ in lavt-rs_amd/**/*.py -- is a row of the
    "Environment switches" table of INTEGRATION.md and the table names nothing else; the C library reads the environment in tuning.hip alone (no launch
    path calls getenv); the anonymous LAVT_PROBE integers are gone."""
    pkg = os.path.join(ROOT, "lavt-rs_amd")
    csrc = os.path.join(pkg, "csrc")
    read, getenv_files, probe_files = set(), set(), set()
    for name in sorted(os.listdir(csrc)):
        if not name.endswith((".hip", ".h")):
            continue
        text = open(os.path.join(csrc, name)).read()
        read |= set(re.findall(r'\b(?:getenv|env_int|env_is)\(\s*"(LAVT_[A-Z0-9_]+)"', text))
        if "getenv" in text:
            getenv_files.add(name)
        if "LAVT_PROBE" in text or "probe[" in text:
            probe_files.add(name)
    for d, _, files in os.walk(pkg):
        for name in files:
            if name.endswith(".py"):
                text = open(os.path.join(d, name)).read()
                read |= set(re.findall(r'os\.environ(?:\.\w+)?\s*[\(\[]\s*["\'](LAVT_[A-Z0-9_]+)["\']', text))
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = doc.split("## Environment switches", 1)[1].split("\n## ", 1)[0]
    table = set(re.findall(r"^\| `(LAVT_[A-Z0-9_]+)` \|", section, flags=re.M))
    assert read == table, (sorted(read - table), sorted(table - read))
    assert getenv_files == {"tuning.hip"}
    assert not probe_files
