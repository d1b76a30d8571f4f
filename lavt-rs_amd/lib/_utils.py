"""Top-level LAVT modules with the reference's forward signatures (lib/_utils.py:10-108).

    LAVT(backbone, classifier).forward(x, l_feats, l_mask)        -> (B, 2, H, W) fp32 logits
    LAVTOne(backbone, classifier, args).forward(x, text, l_mask)  (BERT inside)

The backbone / decoder arithmetic is liblavt_hip; the final align_corners bilinear upsample writes
the NCHW fp32 logits directly.  BERT (the absent ./bert package of the reference) is not part of the
hot path: LAVTOne uses `bert.modeling_bert.BertModel` when importable, else transformers' BertModel.
"""
import os

import torch
from torch import nn

from lavt_hip import ops
from lavt_hip.runtime import compute_dtype
from .mask_predictor import nchw_rows


def _upsample_logits(y, size):
    """y: (B, 2, h, w)-shaped decoder output -> (B, 2, H, W) fp32, bilinear align_corners=True (lib/_utils.py:21)."""
    B, _, h, w = y.shape
    return ops.logits_upsample(nchw_rows(y, y.dtype), B, h, w, int(size[0]), int(size[1]))


def fused_loss(y, target, weight=(0.9, 1.1), valid_indices=None):
    """The caller's `criterion(model(...), target)` (train.py:221-224; losses.py:7-11) on the LOW-resolution decoder output y
    ((B, 2, h, w)-shaped): bilinear upsample to target.shape[-2:] + weighted cross-entropy + I/U counts in one kernel pair.
    -> (loss, stats[loss, sum of weights, I, U])
    valid_indices (device int32 [nsel]: the flat frame numbers `i * t + ind` of train.py:283): the clips of A2D-Sentences / JHMDB carry one annotated
    frame each -- `criterion(torch.index_select(output, 0, valid_indices), masks)` of train.py:282-285 with target (nsel, H, W); the statistics are
    over the selected frames, the gradient of every other frame of y is exactly zero."""
    B, _, h, w = y.shape
    return ops.upsample_cross_entropy(nchw_rows(y, y.dtype), target, B, h, w, int(target.shape[-2]), int(target.shape[-1]), weight, sel=valid_indices)


def fused_dice_loss(y, target, valid_indices=None):
    """`MultiClassDiceLoss()(model(...), target)` (train.py:703-704; losses.py:38-77) on the LOW-resolution decoder output y: bilinear upsample
    + softmax + per-sample Dice sums in one kernel pair.  -> (loss, stats)
    valid_indices: as for fused_loss; the Dice mean is over the selected samples and the 2 classes."""
    B, _, h, w = y.shape
    return ops.upsample_dice_loss(nchw_rows(y, y.dtype), target, B, h, w, int(target.shape[-2]), int(target.shape[-1]), sel=valid_indices)


def fused_dice_boundary_loss(y, target, valid_indices=None, dice_rate=1.0, boundary_rate=0.05):
    """`DiceBoundaryLoss(boundary_rate, dice_rate)(model(...), target)` (train.py:709-711; losses.py:142-244) on the LOW-resolution decoder output y:
    bilinear upsample + softmax + the Dice sums + the boundary F1 stencil (3x3 and 5x5 max-pools) per output tile in LDS.  -> (loss, stats)
    valid_indices: as for fused_loss; both means are over the selected samples and the 2 classes."""
    B, _, h, w = y.shape
    return ops.upsample_dice_boundary_loss(nchw_rows(y, y.dtype), target, B, h, w, int(target.shape[-2]), int(target.shape[-1]), sel=valid_indices,
                                           dice_rate=dice_rate, boundary_rate=boundary_rate)


def fused_iu(y, target, valid_indices=None, loss=None):
    """The reference's training-log counts `IoU(output, masks)` (train.py:64-76: argmax, I = sum(pred * gt), U = sum(pred + gt) - I, pooled over the
    batch) on the LOW-resolution decoder output y, for the criteria whose statistics do not hold them (fused_dice_loss, fused_dice_boundary_loss):
    bilinear upsample + argmax + integer counts in one kernel pair, no gradient.  -> the device fp32[4] row {loss[0] or 0, 0, I, U}, the layout of
    fused_loss's stats (and the same I, U), which the training meters read.
    valid_indices: as for fused_loss.  loss: an optional device fp32 tensor (a criterion's stats) whose element 0 the kernel copies into row[0]."""
    B, _, h, w = y.shape
    return ops.upsample_iu(nchw_rows(y, y.dtype), target, B, h, w, int(target.shape[-2]), int(target.shape[-1]), sel=valid_indices, loss=loss)


def _check_frames(module, folded, frames):
    if frames is not None and (module.training or not folded):
        raise ValueError("forward_lowres: frames= needs the BatchNorm-folded decoder (folded=True, model.eval()); in training mode select in the "
                         "loss: fused_loss(y, target, valid_indices=frames)")


def _check_image_of(expand, frames, image_of):
    """image_of= (a pair-list batch, lib/backbone.py: forward; inference and training alike): one batch arrangement at a time"""
    if image_of is None:
        return
    if expand != 1:
        raise ValueError("forward_lowres: image_of= names the image of every expression; it cannot be combined with expand != 1")
    if frames is not None:
        raise ValueError("forward_lowres: image_of= cannot be combined with frames= (the annotated-frame selection of clip batches)")


def _backbone(backbone, x, l_feats, l_mask, expand, image_of):
    if image_of is not None:
        return backbone(x, l_feats, l_mask, image_of=image_of)
    return backbone(x, l_feats, l_mask, expand=expand) if expand != 1 else backbone(x, l_feats, l_mask)


def _decode(classifier, folded, x_c4, x_c3, x_c2, x_c1, frames=None):
    """frames (device int32 [nsel]): decode only those samples -- test.py:182-205 of the reference selects the annotated frame of every clip behind
    the decoder; the BatchNorm-folded decoder is per-sample independent, so the backbone outputs are gathered in front of it instead
    (ops.gather_samples: the 3 maps a lazy_pred decoder reads, else 4) and the result is (nsel, 2, H/4, W/4)-shaped.  Eval mode + folded only: the
    train-mode BatchNorm of the decoder takes its statistics over ALL frames in the reference, there the selection belongs to the loss
    (fused_loss(valid_indices=))."""
    if frames is not None:
        _check_frames(classifier, folded, frames)
        x_c4, x_c3, x_c2, x_c1 = (None if f is None else ops.gather_samples(f, frames) for f in (x_c4, x_c3, x_c2, x_c1))
    return classifier.forward_folded(x_c4, x_c3, x_c2, x_c1) if folded else classifier(x_c4, x_c3, x_c2, x_c1)


class _LAVTSimpleDecode(nn.Module):
    def __init__(self, backbone, classifier):
        super().__init__()
        self.backbone = backbone
        self.classifier = classifier

    def forward_lowres(self, x, l_feats, l_mask, folded=False, expand=1, frames=None, image_of=None):
        """decoder output before the final upsample, (B, 2, H/4, W/4)-shaped: feed it to `fused_loss`.
        Inference (lavt_hip.engine.Predictor): folded = the BatchNorm-folded decoder (eval mode); expand = S > 1 = S expressions per image (l_feats /
        l_mask hold B * S of them), stage 0 of the backbone shared between the expressions of an image; frames: see _decode.
        image_of (device int32 [N]): a pair-list batch, l_feats / l_mask hold N expressions and the result N samples (lib/backbone.py: forward);
        mutually exclusive with expand != 1 and with frames.  Also in training mode (engine.TrainStep(image_of=)): the decoder's BatchNorm then
        takes its statistics over the N slots, as it does over the N samples of a plain batch."""
        _check_frames(self, folded, frames)          # (raises in front of the backbone)
        _check_image_of(expand, frames, image_of)
        x_c1, x_c2, x_c3, x_c4 = _backbone(self.backbone, x, l_feats, l_mask, expand, image_of)
        return _decode(self.classifier, folded, x_c4, x_c3, x_c2, x_c1, frames)

    def forward(self, x, l_feats, l_mask):
        return _upsample_logits(self.forward_lowres(x, l_feats, l_mask), x.shape[-2:])


class LAVT(_LAVTSimpleDecode):
    pass


def _build_text_encoder(args):
    """`BertModel.from_pretrained(args.ck_bert)` of the reference (lib/_utils.py:38-40), on the liblavt_hip encoder (bert/modeling_bert.py).
    `args.ck_bert` must be a directory with config.json + weights: there is no hub download here, and a missing checkpoint raises instead of
    silently training / evaluating with an untrained text encoder.  Random bert-base-uncased geometry is available only on request:
    `args.bert_random_init = True` (benchmarks and tests on synthetic data) or LAVT_BERT_RANDOM_INIT=1."""
    from bert.modeling_bert import BertConfig, BertModel
    ck = getattr(args, "ck_bert", "bert-base-uncased")
    if os.path.isdir(str(ck)):
        enc = BertModel.from_pretrained(ck)
    elif getattr(args, "bert_random_init", False) or os.environ.get("LAVT_BERT_RANDOM_INIT", "0") == "1":
        import warnings
        warnings.warn(f"text encoder: ck_bert={ck!r} is not a checkpoint directory; building a RANDOMLY INITIALISED bert-base-uncased on request")
        enc = BertModel(BertConfig())
    else:
        raise FileNotFoundError(f"text encoder: ck_bert={ck!r} is not a directory with config.json + pytorch_model.bin / model.safetensors "
                                "(no hub download here); pass args.bert_random_init=True for a randomly initialised encoder")
    enc.pooler = None
    return enc


class _LAVTOneSimpleDecode(nn.Module):
    def __init__(self, backbone, classifier, args):
        super().__init__()
        self.backbone = backbone
        self.classifier = classifier
        self.text_encoder = _build_text_encoder(args)
        self.lazy_pred = bool(getattr(args, "lazy_pred", False))

    def forward_lowres(self, x, text, l_mask, folded=False, expand=1, frames=None, image_of=None):
        """token ids (B, N_l) + attention mask (B, N_l) -> decoder logits at 1/4 resolution (what the fused upsample + CE kernel consumes).
        folded / expand / frames / image_of: see LAVT.forward_lowres (with expand = S the ids and the mask hold B * S expressions, with image_of N)."""
        _check_frames(self, folded, frames)
        _check_image_of(expand, frames, image_of)
        l_feats = self.text_encoder(text, attention_mask=l_mask)[0].permute(0, 2, 1)      # (B, 768, N_l)
        l_mask = l_mask.unsqueeze(dim=-1)
        features = _backbone(self.backbone, x, l_feats, l_mask, expand, image_of)
        if self.lazy_pred:
            x_c1, (x_c2, x_c3, x_c4) = None, features
        else:
            x_c1, x_c2, x_c3, x_c4 = features
        return _decode(self.classifier, folded, x_c4, x_c3, x_c2, x_c1, frames)

    def forward(self, x, text, l_mask):
        return _upsample_logits(self.forward_lowres(x, text, l_mask), x.shape[-2:])


class LAVTOne(_LAVTOneSimpleDecode):
    pass


class _LAVTVideoSimpleDecode(nn.Module):
    """Reference lib/_utils.py:76-108: clip (B, T, 3, H, W) + token ids (B, N_l) + attention mask (B, N_l) -> (B*T, 2, H, W) logits.
    BERT runs inside (it is outside the hot path, as for LAVTOne); `forward_backbone` is the hot path proper on language features."""

    def __init__(self, backbone, classifier, args):
        super().__init__()
        self.backbone = backbone
        self.classifier = classifier
        self.text_encoder = _build_text_encoder(args)
        self.lazy_pred = bool(getattr(args, "lazy_pred", False))
        self.seg_last = bool(getattr(args, "seg_last", False))

    def forward_backbone(self, x, l_feats, l_mask):
        """x (B, T, 3, H, W); l_feats (B, 768, N_l); l_mask (B, N_l, 1)"""
        input_shape = x.shape[-2:]
        features = self.backbone(x.permute(0, 2, 1, 3, 4), l_feats, l_mask)          # (B, 3, T, H, W) view; the patch embed reads frames
        if self.lazy_pred:
            x_c1, (x_c2, x_c3, x_c4) = None, features
        else:
            x_c1, x_c2, x_c3, x_c4 = features
        y = self.classifier(x_c4, x_c3, x_c2, x_c1)
        if self.seg_last:
            return y
        return _upsample_logits(y, input_shape)

    def forward(self, x, text, l_mask):
        l_feats = self.text_encoder(text, attention_mask=l_mask)[0].permute(0, 2, 1)      # (B, 768, N_l)
        return self.forward_backbone(x, l_feats, l_mask.unsqueeze(dim=-1))

    def forward_lowres(self, x, text, l_mask, folded=False, expand=1, frames=None, image_of=None):
        """clip (B, T, 3, H, W) + token ids + attention mask -> decoder logits (B*T, 2, H/4, W/4)-shaped, before the final upsample.
        folded: the BatchNorm-folded decoder (eval mode).  The video backbone has no shared stage 0: expand > 1 and image_of raise NotImplementedError.
        frames (device int32 [nsel], flat numbers i * T + ind): only the annotated frames are decoded, -> (nsel, 2, H/4, W/4)-shaped; see _decode."""
        _check_frames(self, folded, frames)
        if image_of is not None:
            raise NotImplementedError("LAVTVideo.forward_lowres: image_of= (pair-list batches) needs a backbone that shares stage 0 between expressions; the video backbone does not")
        l_feats = self.text_encoder(text, attention_mask=l_mask)[0].permute(0, 2, 1)
        features = self.backbone(x.permute(0, 2, 1, 3, 4), l_feats, l_mask.unsqueeze(dim=-1), expand=expand)
        if self.lazy_pred:
            x_c1, (x_c2, x_c3, x_c4) = None, features
        else:
            x_c1, x_c2, x_c3, x_c4 = features
        return _decode(self.classifier, folded, x_c4, x_c3, x_c2, x_c1, frames)

    def forward_feats(self, x, text, l_mask):
        """Reference lib/_utils.py:110-131: -> (logits (B*T, 2, H, W) fp32, [x_c4, level-4, level-3, level-2 decoder features])."""
        input_shape = x.shape[-2:]
        l_feats = self.text_encoder(text, attention_mask=l_mask)[0].permute(0, 2, 1)
        features = self.backbone(x.permute(0, 2, 1, 3, 4), l_feats, l_mask.unsqueeze(dim=-1))
        if self.lazy_pred:
            x_c1, (x_c2, x_c3, x_c4) = None, features
        else:
            x_c1, x_c2, x_c3, x_c4 = features
        y, feats = self.classifier.forward_feats(x_c4, x_c3, x_c2, x_c1)
        return _upsample_logits(y, input_shape), feats

    def load_from_pretrained2d_lavt_weights(self, pretrained):
        """Reference lib/_utils.py:133-182 (called by train.py:575-576): released 2-D LAVT weights -> this video model (patch-embed
        `unsqueeze(2)`, bias tables bicubic-resized then repeated 2*Wd-1 times), non-strict load."""
        from lavt_hip.checkpoint import load_lavt2d_into_video
        missing, unexpected = load_lavt2d_into_video(self, pretrained, drop_fusion=False)
        print(f"=> loaded successfully '{pretrained}' (missing {len(missing)}, unexpected {len(unexpected)})")
        ops.weights.invalidate()
        return missing, unexpected

    def load_from_pretrained2d_lavt_weights_into_a_3d_model(self, pretrained):
        """Reference lib/_utils.py:184-238 (train.py:577-578): as above, but the '.fusion' tensors (2-D PWAM) are dropped."""
        from lavt_hip.checkpoint import load_lavt2d_into_video
        missing, unexpected = load_lavt2d_into_video(self, pretrained, drop_fusion=True)
        print(f"=> loaded successfully '{pretrained}' (missing {len(missing)}, unexpected {len(unexpected)})")
        ops.weights.invalidate()
        return missing, unexpected


class LAVTVideo(_LAVTVideoSimpleDecode):
    pass
