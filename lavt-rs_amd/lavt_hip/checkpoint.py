"""Checkpoint compatibility: load public Swin / Video-Swin weights and released 2-D LAVT weights into the drop-in
modules, with the reference's key surgery.  Host-side torch code (runs once, before training); everything returns
(missing_keys, unexpected_keys) of the final non-strict `load_state_dict`.

Reference behaviour mirrored here:
* lib/mmcv_custom/checkpoint.py:287-360 `load_checkpoint`: unwrap 'state_dict' / 'model'; strip a leading 'module.'; keep only and
  strip 'backbone.' (UperNet checkpoints) or 'encoder.' (MoBY); bicubic-resize `relative_position_bias_table` when the window differs;
  non-strict load.
* lib/video_swin_transformer.py:759-805 `inflate_weights` (2-D Swin -> 3-D): drop `relative_position_index` / `attn_mask`; patch-embed
  weight `unsqueeze(2).repeat(patch_t) / patch_t`; bias tables resized to (2Wh-1, 2Ww-1) then repeated (2Wd-1) times along the table axis.
* lib/video_swin_transformer.py:830-844 `init_weights` (3-D checkpoint): take 'state_dict', keep keys containing 'backbone.' with the
  first 9 characters removed, SUM the patch-embed weight over its temporal axis (keepdim).
* lib/_utils.py:133-238 (2-D LAVT weights into the video model): patch-embed `unsqueeze(2)`, tables as in inflate_weights, optionally
  dropping the '.fusion' tensors.

Training state (DESIGN.md "Checkpoint and resume"): save_train_state / load_train_state write and read the whole state of an engine.TrainStep -- the
reference's `{'model', 'optimizer', 'epoch', 'lr_scheduler', ...}` file (train.py:749-763) plus one more key, 'lavt_train_state' -- and the pure
parts of TrainStep.state_dict() / load_state_dict() live here: the configuration fingerprint's comparison, the names of the fp8 sites, the writer.
"""
import os
from collections import OrderedDict

import torch
import torch.nn.functional as F


def _unwrap(checkpoint):
    if not isinstance(checkpoint, dict):
        raise RuntimeError("no state_dict found in checkpoint")
    if "state_dict" in checkpoint:
        return checkpoint["state_dict"]
    if "model" in checkpoint:
        return checkpoint["model"]
    return checkpoint


def _resize_table(table, size_hw):
    """(L1, nH) -> (size_h*size_w, nH), bicubic over the square (S1, S1) source grid (mmcv_custom/checkpoint.py:347-353)"""
    L1, nH = table.shape
    S1 = int(L1 ** 0.5)
    r = F.interpolate(table.permute(1, 0).view(1, nH, S1, S1), size=tuple(size_hw), mode="bicubic")
    return r.view(nH, size_hw[0] * size_hw[1]).permute(1, 0)


def convert_swin_state_dict(checkpoint, model):
    """2-D Swin checkpoint -> state dict for lib.backbone.MultiModalSwinTransformer (reference load_checkpoint semantics)."""
    sd = _unwrap(checkpoint)
    keys = list(sd.keys())
    if keys[0].startswith("module."):
        sd = OrderedDict((k[7:], v) for k, v in sd.items())
    if list(sd.keys())[0].startswith("backbone."):
        sd = OrderedDict((k.replace("backbone.", ""), v) for k, v in sd.items() if k.startswith("backbone."))
    if sorted(sd.keys())[0].startswith("encoder"):
        sd = OrderedDict((k.replace("encoder.", ""), v) for k, v in sd.items() if k.startswith("encoder."))
    sd = OrderedDict(sd)
    sd.pop("absolute_pos_embed", None)                       # ape=False in every LAVT factory
    current = model.state_dict()
    for k in [k for k in sd if "relative_position_bias_table" in k]:
        if k not in current:
            continue
        L1, nH1 = sd[k].shape
        L2, nH2 = current[k].shape
        if nH1 != nH2:
            print(f"Error in loading {k}, pass")
        elif L1 != L2:
            S2 = int(L2 ** 0.5)
            sd[k] = _resize_table(sd[k], (S2, S2))
    return sd


def _load_tolerant(model, sd):
    """mmcv's load_state_dict (mmcv_custom/checkpoint.py:41-108) reports tensors of the wrong shape instead of raising; the constant
    `relative_position_index` / `attn_mask` buffers of a checkpoint are never needed."""
    current = model.state_dict()
    keep = OrderedDict()
    for k, v in sd.items():
        if "relative_position_index" in k or "attn_mask" in k:
            continue
        if k in current and tuple(current[k].shape) != tuple(v.shape):
            print(f"size mismatch for {k}: checkpoint {tuple(v.shape)} vs model {tuple(current[k].shape)}, skipped")
            continue
        keep[k] = v
    res = model.load_state_dict(keep, strict=False)
    return [k for k in res.missing_keys if "relative_position_index" not in k], list(res.unexpected_keys)


def load_swin_checkpoint(model, filename, map_location="cpu"):
    return _load_tolerant(model, convert_swin_state_dict(torch.load(filename, map_location=map_location, weights_only=False), model))


def _tables_to_3d(sd, model, window_size):
    wd, wh, ww = window_size
    current = model.state_dict()
    for k in [k for k in sd if "relative_position_bias_table" in k]:
        t = sd[k]
        L1, nH1 = t.shape
        nH2 = current[k].shape[1] if k in current else nH1
        L2 = (2 * wh - 1) * (2 * ww - 1)
        if nH1 != nH2:
            print(f"Error in loading {k}, passing")
        elif L1 != L2:
            t = _resize_table(t, (2 * wh - 1, 2 * ww - 1))
        sd[k] = t.repeat(2 * wd - 1, 1)
    return sd


def convert_video_swin_state_dict(checkpoint, model, inflate_2d=False):
    """-> state dict for lib.video_swin_transformer.MultiModalSwinTransformer3D"""
    if inflate_2d:
        sd = OrderedDict(checkpoint["model"])
        for k in [k for k in sd if "relative_position_index" in k or "attn_mask" in k]:
            del sd[k]
        pt = model.patch_size[0]
        sd["patch_embed.proj.weight"] = sd["patch_embed.proj.weight"].unsqueeze(2).repeat(1, 1, pt, 1, 1) / pt
        return _tables_to_3d(sd, model, model.window_size)
    sd = OrderedDict((k[9:], v) for k, v in checkpoint["state_dict"].items() if "backbone." in k)
    sd["patch_embed.proj.weight"] = sd["patch_embed.proj.weight"].sum(dim=2, keepdim=True)
    return sd


def load_video_swin_checkpoint(model, filename, inflate_2d=False, map_location="cpu"):
    return _load_tolerant(model, convert_video_swin_state_dict(torch.load(filename, map_location=map_location, weights_only=False), model, inflate_2d))


def convert_lavt2d_to_video_state_dict(checkpoint, video_model, drop_fusion=False):
    """released 2-D LAVT weights ('model' key, 'backbone.' / 'classifier.' prefixes) -> LAVTVideo (lib/_utils.py:133-238)"""
    sd = OrderedDict(checkpoint["model"])
    for k in [k for k in sd if "relative_position_index" in k or "attn_mask" in k or (drop_fusion and ".fusion" in k)]:
        del sd[k]
    assert "backbone.patch_embed.proj.weight" in sd
    sd["backbone.patch_embed.proj.weight"] = sd["backbone.patch_embed.proj.weight"].unsqueeze(2)
    return _tables_to_3d(sd, video_model, video_model.backbone.window_size)


def load_lavt2d_into_video(video_model, filename, drop_fusion=False, map_location="cpu"):
    return _load_tolerant(video_model, convert_lavt2d_to_video_state_dict(torch.load(filename, map_location=map_location, weights_only=False), video_model, drop_fusion))


# ------------------------------------------------------------------------------------------------ training state (engine.TrainStep)
TRAIN_STATE_FORMAT = 1
TRAIN_STATE_KEYS = ("model", "optimizer", "lavt_train_state")
# one more top-level entry, exactly when the step trains a separate text encoder (TrainStep(text_encoder=)): its state_dict() under the reference's key
# (train.py:612, 752-757).  Not in TRAIN_STATE_KEYS: a step without encoder writes the three keys above and nothing else.
TEXT_ENCODER_KEY = "bert_model"
# the fields of the fingerprint, in the order they are compared
CONFIG_FIELDS = ("criterion", "dice_rate", "boundary_rate", "accumulate", "amsgrad", "max_grad_norm", "skip_nonfinite", "deterministic", "compute_dtype",
                 "fp8", "world", "param_groups")


def _plain(v):
    """tuples -> lists, recursively: what a fingerprint looks like after a trip through a file is what it is compared as"""
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    return v


def compare_fingerprints(saved, current, who="TrainStep.load_state_dict"):
    """ValueError naming the FIRST field of CONFIG_FIELDS in which the checkpoint's fingerprint differs from this step's; for the parameter list, the first
    group and entry (a missing, extra, renamed or reshaped parameter).  'pair_slots' (N of a TrainStep(image_of=), engine._config) is an OPTIONAL field,
    present only in the fingerprint of a pair-list step -- a plain step's fingerprint is what it was -- and compared first: a plain run's checkpoint is
    refused by a pair run and the other way round."""
    if saved.get("pair_slots") != current.get("pair_slots"):
        def _say(v):
            return "without image_of (a plain batch)" if v is None else f"with image_of of {v} slots"
        raise ValueError(f"{who}: config field 'pair_slots' differs: the checkpoint was written {_say(saved.get('pair_slots'))}, this step runs {_say(current.get('pair_slots'))}")
    for f in CONFIG_FIELDS:
        if f not in saved:
            raise ValueError(f"{who}: the checkpoint's config has no field '{f}'")
        a, b = _plain(saved[f]), _plain(current[f])
        if a == b:
            continue
        if f != "param_groups":
            raise ValueError(f"{who}: config field '{f}' differs: the checkpoint was written with {f}={saved[f]!r}, this step runs with {f}={current[f]!r}")
        if len(a) != len(b):
            raise ValueError(f"{who}: config field 'param_groups' differs: the checkpoint has {len(a)} parameter groups, this step's optimizer {len(b)}")
        for gi, (ga, gb) in enumerate(zip(a, b)):
            for pi, (ea, eb) in enumerate(zip(ga, gb)):
                if ea != eb:
                    what = "was reshaped" if ea[0] == eb[0] else "is another parameter"
                    raise ValueError(f"{who}: config field 'param_groups' differs: group {gi}, entry {pi} {what}: the checkpoint has {ea[0]} {tuple(ea[1])}, "
                                     f"this step {eb[0]} {tuple(eb[1])}")
            if len(ga) != len(gb):
                extra, side = (ga[len(gb)], "the checkpoint") if len(ga) > len(gb) else (gb[len(ga)], "this step")
                raise ValueError(f"{who}: config field 'param_groups' differs: group {gi} has {len(ga)} parameters in the checkpoint and {len(gb)} in this "
                                 f"step: {extra[0]} {tuple(extra[1])} is in {side} only")
        raise ValueError(f"{who}: config field 'param_groups' differs")


def fp8_site_name(key, names):
    """The name a delayed-scaling site is saved under.  `key`: the site's key in _Fp8State.slots -- id(weight) for the activations the contraction with
    `weight` reads, (id(weight), 'dy') for the output gradient its backward quantises; names: {id(parameter): qualified name}.  Slot numbers follow the
    order of first use and mean nothing in another process; the consuming parameter's name does."""
    pid, kind = (key[0], str(key[1])) if isinstance(key, tuple) else (key, "act")
    if pid not in names:
        raise ValueError(f"fp8 site {key!r}: its consuming weight is not a parameter of the step's model")
    return f"{names[pid]}|{kind}"


def fp8_site_slots(slots, names):
    """{site name: slot number} of an _Fp8State.slots dict"""
    out = {}
    for key, i in slots.items():
        n = fp8_site_name(key, names)
        if n in out:
            raise ValueError(f"fp8 sites: two sites are named {n}")
        out[n] = int(i)
    return out


def match_fp8_sites(saved_names, own_names, who="TrainStep.load_state_dict"):
    """ValueError unless the checkpoint's sites are exactly this step's"""
    own = set(own_names)
    for n in saved_names:
        if n not in own:
            raise ValueError(f"{who}: fp8 site '{n}' of the checkpoint does not exist in this step (its model quantises "
                             f"{len(own)} sites: {', '.join(sorted(own)[:4])}{' ...' if len(own) > 4 else ''})")
    missing = sorted(own - set(saved_names))
    if missing:
        raise ValueError(f"{who}: fp8 site '{missing[0]}' of this step is not in the checkpoint")


def to_host(v):
    """tensors -> detached CPU copies, through dicts, lists and tuples (what torch.load(..., weights_only=True) reads back)"""
    if torch.is_tensor(v):
        return v.detach().to("cpu", copy=True)
    if isinstance(v, dict):
        return {k: to_host(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return type(v)(to_host(x) for x in v)
    return v


def write_atomic(path, obj, _save=torch.save):
    """torch.save to `path + '.tmp'`, then os.replace: a reader (and a run killed mid-write) sees the old file or the new one, never a torn one"""
    path = os.fspath(path)
    tmp = path + ".tmp"
    try:
        _save(obj, tmp)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def save_train_state(path, step, **extra):
    """Write step.state_dict() -- 'model', 'optimizer', 'lavt_train_state' -- with `extra` (the reference's 'epoch', 'lr_scheduler', any metadata
    torch.load(weights_only=True) can read) merged at the top level, atomically."""
    for k in extra:
        if k in TRAIN_STATE_KEYS:
            raise ValueError(f"save_train_state: '{k}' is written by the step itself")
        if k == TEXT_ENCODER_KEY:
            raise ValueError(f"save_train_state: '{k}' is the entry of a step that trains its text encoder (TrainStep(text_encoder=) writes it itself; "
                             "a step without one would refuse the file)")
    state = step.state_dict()
    state.update(extra)
    write_atomic(path, state)


def load_train_state(path, step):
    """Read a file of save_train_state into `step` (TrainStep.load_state_dict: after warmup_and_capture(), in place) -> the extra keys (the text
    encoder's 'bert_model' entry is the step's, not metadata)"""
    state = torch.load(os.fspath(path), map_location="cpu", weights_only=True)
    step.load_state_dict(state)
    return {k: v for k, v in state.items() if k not in TRAIN_STATE_KEYS and k != TEXT_ENCODER_KEY}
