"""Step harness reproducing the reference caller's sequence (train.py:199-229) on the HIP model:

    zero grads -> out = model(image, l, l_mask) -> F.cross_entropy(out, target, weight=[0.9, 1.1]) -> backward
    -> gradient all-reduce (world > 1)

Gradient accumulation over micro-batches: TrainStep(accumulate=k) with an owned optimizer.  Every call of step() is one MICRO-step on whatever the
static buffers hold: its body is the one above, unchanged (every parameter still receives exactly one weight gradient per micro-step into a buffer
zeroed at its start; lavt_hip.ops.sinks still refuses a second one), then lavt_grad_accumulate folds the flat gradient, times 1/k, into a second
flat buffer (`acc`) and the optimizer's guarded kernels read `acc`.  The phase of the cycle lives on the device (the accumulating flag and the micro index of
FusedAdamW's control block; this module asks the optimizer for them -- micro_index(), reset_phase(), control_state() / load_control_state() -- and
never indexes the block): ONE captured graph serves all k micro-steps -- replays 1 .. k-1 leave parameters, moments, compute copies and the step counter bit for bit alone, replay k applies
one AdamW update from the mean of the k gradients (clip and non-finite skip act on that mean) and ticks the schedule once.  Per micro-step, as in
PyTorch under accumulation: BatchNorm normalises with (and its running statistics follow) each micro-batch's own statistics, DropPath draws new
masks, the fp8 |max| history advances; step() returns, and `stats` holds, that micro-batch's loss.  world > 1: the buckets are all-reduced in
every micro-step (correct by linearity -- the fold runs after GradBuckets.finish()); leaving out the all-reduce of the first k-1 micro-steps is not
done.

Checkpoint and resume: state_dict() / load_state_dict() (lavt_hip.checkpoint.save_train_state / load_train_state for files) hold the WHOLE state of a
captured run -- model, optimizer, the control block with the accumulation phase, `acc` when the checkpoint lies inside a cycle, the DropPath
generator, the fp8 |max| history, torch's CUDA generator -- and load it, after warmup_and_capture(), into the storage the captured graph reads.  In
deterministic mode on one GPU a run that is saved, torn down, rebuilt and resumed gives the bits of one that never stopped (DESIGN.md "Checkpoint
and resume").  A checkpoint may be taken at any micro-step; one from a cycle boundary (micro_step() == 0) carries no `acc`.

The whole step is ~1,000 kernel launches for Swin-B; issued from Python it is launch-bound, so on one GPU the
step is captured once into a hipGraph (torch.cuda.CUDAGraph on the stream our C-ABI launches go to) and
replayed: weight casts, DropPath masks, BatchNorm running-stat updates all happen inside the graph.
With world > 1 the same capture includes the collectives: the SyncBN statistic all-reduces on the capture stream and the
bucketed gradient all-reduces on the communication stream (forked from / joined to the capture stream with events), so a
replay issues forward, backward and the overlapped RCCL all-reduces without any Python in between.  RCCL supports stream
capture (its collectives become graph kernel nodes); `tools/nccl_graph_probe.py` and tests/test_gpu_modules.py exercise the
mechanics on one GPU in a 1-rank group.  LAVT_DDP_GRAPH=0 (or a failed capture) falls back to eager launching, where the
step is bound by the ~23 ms of host-side launch work.

The optimizer is the caller's by default (opt.step() after TrainStep.step()).  TrainStep.make_optimizer() / attach_optimizer() make the step OWN a
FusedAdamW on the step's context: its update then ends the step's body, inside the same capture, and one replay is one whole training iteration.

Training meters (TrainStep(meters=) / make_meters(); lavt_hip.meters): one more launch behind the optimizer's tick logs loss, lr, I, U, IoU, the gradient norm
and the update's verdict of every step() into a ring on the device and moves the epoch accumulators of the reference's log (train.py:463-500); the host reads
them with TrainMeters.poll(), which never waits.  The launch reads `meter_stats`, an fp32[4] row {loss, ., I, U}: under loss="ce" the criterion's own `stats`;
under "mc_dice" / "dice_boundary", whose `stats` hold no argmax counts, the row of lib._utils.fused_iu -- one more kernel pair behind the criterion's forward.
Off by default: a step built without meters launches what it launched before, for every criterion.

The separate text encoder of `--model lavt` (TrainStep(text_encoder=bert_model); DESIGN.md "Text encoder in the step"): the reference computes the language
features in every iteration, lets gradients flow back into `bert_model`, updates its encoder layers 0..9 with the same AdamW and saves it as the checkpoint's
'bert_model' entry (train.py:217-221, 612, 623-632, 752-757).  With the argument the static language buffers hold token ids and the attention mask, the body
starts with the encoder's forward, and everything the step owns spans both modules: the flat gradient buffer and its buckets, the zero fill, the all-reduce
sequence, the weight-copy refresh and stamp, make_optimizer()'s groups, the names handed out ('bert_model.' + the encoder's own) and the checkpoint.
None (the default): the step as it is without the argument.
"""
import os
import sys

import torch
import torch.nn.functional as F

from . import ops
from . import _capi as K
from .checkpoint import TEXT_ENCODER_KEY
from .ddp import GradBuckets
from .runtime import compute_dtype, fp8_enabled


def _in_context(fn):
    """run a TrainStep method inside the step's own ops.StepContext"""
    import functools

    @functools.wraps(fn)
    def wrapped(self, *a, **kw):
        with ops.use_context(self.context):
            return fn(self, *a, **kw)
    return wrapped


def flat_valid_indices(per_clip, frames_per_clip, n_frames, count=None):
    """`[i * t + ind for i, ind in enumerate(valid_indices)]` of the reference (train.py:283, test.py:182-205): the annotated frame `ind` of clip i as
    a row of the (B*T, ...) model output.  Host integers in, a list out; ValueError unless there are `count` entries (when given), every flat index
    lies in [0, n_frames) and no two are equal -- the checks the kernels cannot make (include/lavt_hip.h: the contract of sel)."""
    per_clip = [int(v) for v in per_clip]
    T = int(frames_per_clip)
    if T < 1:
        raise ValueError(f"valid indices: frames_per_clip must be >= 1, got {T}")
    if count is not None and len(per_clip) != count:
        raise ValueError(f"valid indices: {len(per_clip)} entries for an index buffer of {count}")
    flat = [i * T + ind for i, ind in enumerate(per_clip)]
    bad = [(i, ind) for i, (ind, f) in enumerate(zip(per_clip, flat)) if ind < 0 or not 0 <= f < n_frames]
    if bad:
        raise ValueError(f"valid indices: (clip, frame) {bad} outside the {n_frames} frames of the batch ({T} per clip)")
    if len(set(flat)) != len(flat):
        raise ValueError(f"valid indices: {per_clip} with {T} frames per clip name a frame twice (flat {flat})")
    return flat


def _check_index_buffer(who, valid_indices, target, n_frames):
    if not isinstance(valid_indices, torch.Tensor) or not valid_indices.is_cuda:
        raise RuntimeError("liblavt_hip operates on GPU memory only (got a CPU tensor for `valid_indices`); there is no CPU fallback")
    if valid_indices.dtype != torch.int32 or valid_indices.dim() != 1 or not valid_indices.is_contiguous() or not 1 <= valid_indices.numel() <= n_frames:
        raise ValueError(f"{who}: valid_indices must be a contiguous int32 vector of 1..{n_frames} frame numbers, got {valid_indices.dtype} {tuple(valid_indices.shape)}")
    if target is not None and target.shape[0] != valid_indices.numel():
        raise ValueError(f"{who}: {valid_indices.numel()} valid indices need a target of as many samples, got {tuple(target.shape)}")


def _check_pair_buffer(who, image_of, n_expressions, target):
    """the static `image_of` buffer of a pair-list batch (TrainStep, Predictor): checked before anything touches the GPU"""
    if not isinstance(image_of, torch.Tensor):
        raise RuntimeError(f"liblavt_hip operates on GPU memory only (got {type(image_of).__name__} for `image_of`); there is no CPU fallback")
    if image_of.dtype != torch.int32 or image_of.dim() != 1 or not image_of.is_contiguous() or image_of.numel() != n_expressions:
        raise ValueError(f"{who}: image_of must be a contiguous int32 vector with one entry per expression ({n_expressions}), got {image_of.dtype} {tuple(image_of.shape)}")
    if target is not None and target.shape[0] != image_of.numel():
        raise ValueError(f"{who}: {image_of.numel()} pairs need a target of as many samples, got {tuple(target.shape)}")
    if not image_of.is_cuda:          # (after the shape checks: a buffer of the wrong kind is named as such wherever it lives)
        raise RuntimeError("liblavt_hip operates on GPU memory only (got a CPU tensor for `image_of`); there is no CPU fallback")


class _ImageOf:
    """set_image_of of TrainStep and Predictor: `image_of` is a static device buffer like image and target"""
    image_of = None               # the static device int32 [N] buffer; None = not a pair-list batch
    _empty_slots = False          # may an entry be -1 (an empty slot)?  Predictor: yes.  TrainStep: no -- a zero-row slot would enter the criterion as a sample

    def set_image_of(self, image_of):
        """image_of[j] = the image of slot j (host integers): writes the static index buffer after checking the length and that every entry is one of
        the B images of the batch -- or, for a Predictor, -1 = an empty slot (ValueError).  An asynchronous copy through pinned memory on the current
        stream, nothing synchronises; usable between replays -- the captured kernels read the buffer on the device.  A TrainStep reads it in the
        forward AND the backward of a step: written here, between steps and on the stream the step runs on, it never changes inside one."""
        who = f"{type(self).__name__}.set_image_of"
        if self.image_of is None:
            raise ValueError(f"{who}: built without an image_of buffer")
        pairs = [int(v) for v in image_of]
        B = int(self.x.shape[0])
        if len(pairs) != self.image_of.numel():
            raise ValueError(f"{who}: {len(pairs)} entries for an index buffer of {self.image_of.numel()}")
        bad = [(j, v) for j, v in enumerate(pairs) if not (-1 if self._empty_slots else 0) <= v < B]
        if bad:
            raise ValueError(f"{who}: (slot, image) {bad} -- an entry is " + ("-1 (an empty slot) or " if self._empty_slots else "") + f"one of the {B} images of the batch"
                             + ("" if self._empty_slots else " (a train batch has no empty slots: sample full batches, drop the ragged last one)"))
        flat = torch.tensor(pairs, dtype=torch.int32)
        self.image_of.copy_(flat.pin_memory() if self.image_of.is_cuda else flat, non_blocking=True)


class _ValidIndices:
    """set_valid_indices of TrainStep and Predictor: `valid_indices` is a static device buffer like image and target"""

    def _n_frames(self):
        return self.x.numel() // (3 * int(self.x.shape[-2]) * int(self.x.shape[-1]))          # B, or B*T for a clip batch (B, T, 3, H, W)

    def set_valid_indices(self, per_clip, frames_per_clip):
        """per_clip[i] = the annotated frame of clip i (host integers): writes `i * frames_per_clip + per_clip[i]` (train.py:283) into the static
        index buffer after checking count, range and distinctness (ValueError).  An asynchronous copy on the current stream, nothing synchronises;
        usable between replays -- the captured kernels read the buffer on the device."""
        if self.valid_indices is None:
            raise ValueError(f"{type(self).__name__}.set_valid_indices: built without a valid_indices buffer")
        flat = torch.tensor(flat_valid_indices(per_clip, frames_per_clip, self._n_frames(), count=self.valid_indices.numel()), dtype=torch.int32)
        self._valid_per_clip = [int(v) for v in per_clip]          # (stage_batch(augment=): the mask of a clip moves with its annotated frame)
        if self.valid_indices.is_cuda:
            flat = flat.pin_memory()
        self.valid_indices.copy_(flat, non_blocking=True)


class _BatchInput:
    """load_batch / stage_batch / commit_batch of TrainStep and Predictor: the static `image` (and `target`) buffers filled from a raw host batch whose
    images all have their own size (RefCOCO / COCO) -- the reference's Resize -> ToTensor -> Normalize (transforms.py:20-31, 83-87, 106-113) on the
    device with PIL's pixels, one upload and one launch per kind (lavt_hip.preprocess.BatchPreprocessor).  Everything runs eagerly on the current
    stream in front of step(), as Predictor.load_frames does: nothing joins the captured graph; the host waits only for work two batches old (slot
    reuse), so it runs up to one iteration ahead of the device."""
    batch_preprocessor = None          # the BatchPreprocessor(network input size), made on first use (assign one for another mean / std)

    def _batch_preprocessor(self):
        from .preprocess import BatchPreprocessor
        if self.batch_preprocessor is None:
            self.batch_preprocessor = BatchPreprocessor((int(self.x.shape[-2]), int(self.x.shape[-1])), device=self.x.device)
        return self.batch_preprocessor

    def stage_batch(self, images, targets=None, repeat=None, *, frame_map=None, target_map=None, augment=None):
        """Pack the batch and start its upload; writes neither `image` nor `target`, so it may be called while the previous replay is still running.
        images: host list of PIL images / uint8 (Hs, Ws, 3) arrays, one per frame of the image buffer (B, or B*T for a clip buffer (B, T, 3, H, W),
        which is written as B*T frames); repeat=T: B still images, each repeated into a T-frame clip (`--pseudo_video_aug vanilla`, args.py:132-134).
        targets: host list of masks for a `target` buffer of network-input size, as many as it holds -- with `valid_indices` that is nsel, one mask per
        selected frame; under `repeat`, as many masks as the buffer holds are taken one to one, B masks for a buffer of B*T are repeated like the
        images.  frame_map / target_map: the source of every output frame / mask, for any other arrangement.  Frames are counted against the image
        buffer and masks against the target buffer separately, so a pair-list batch (image_of=) brings its B images and its N masks, mask j for slot
        j, as they are: every image is decoded, resized and uploaded once, however many slots name it.
        augment: a lavt_hip.preprocess.PseudoVideoAugment (`--pseudo_video_aug weak-rotate-translate-shear-crop`, args.py:134-137), with repeat=T on a
        clip buffer: every frame of a clip gets its own affine motion of the still image, drawn from the augmenter, warped on the device with
        Pillow's pixels before the resize; each image is still uploaded once.  A mask moves with its frame; one mask per clip (valid_indices) moves
        with the clip's annotated frame, which set_valid_indices must have named.
        ValueError for wrong counts or a target buffer of another size, TypeError for CUDA input, RuntimeError inside a graph capture: in every case
        before anything is written."""
        who = f"{type(self).__name__}.stage_batch"
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{who}: the input stage runs eagerly in front of step() (a host-side pack and an upload): call it outside the graph capture")
        if augment is not None:
            if repeat is None or self.x.dim() != 5 or target_map is not None:
                raise ValueError(f"{who}: augment= makes clips of still images: it needs repeat=T on a clip buffer (B, T, 3, H, W) and no target_map (the image buffer "
                                 f"is {tuple(self.x.shape)}, repeat is {repeat})")
            saved = augment.state_dict()
            try:
                return self._stage_batch(who, images, targets, repeat, frame_map, target_map, augment)
            except Exception:
                augment.load_state_dict(saved)          # a refused batch draws nothing
                raise
        return self._stage_batch(who, images, targets, repeat, frame_map, target_map, None)

    def _stage_batch(self, who, images, targets, repeat, frame_map, target_map, augment):
        from .preprocess import _BatchPlan, _host_list
        H, W = int(self.x.shape[-2]), int(self.x.shape[-1])
        if targets is not None:
            if self.t is None:
                raise ValueError(f"{who}: targets given, but there is no target buffer")
            if tuple(self.t.shape[-2:]) != (H, W):
                raise ValueError(f"{who}: the target buffer is {tuple(self.t.shape[-2:])}, not the network input size {(H, W)} (the via_size / out_size flow keeps "
                                 "targets at the original frame size): copy those into `target` yourself")
            if repeat is not None and target_map is None and isinstance(targets, (list, tuple)) and len(targets) == self.t.shape[0]:
                target_map = range(len(targets))          # one mask per target sample already (valid_indices: the annotated frame of every clip)
        warps = target_warps = None
        if augment is not None:
            T = int(repeat)
            images = _host_list(images, True, "pack_batch: images")
            clips = augment.draw([a.shape[:2] for a in images], T)
            warps = [w for clip in clips for w in clip]
            if targets is not None:
                n = len(_host_list(targets, False, "pack_batch: targets"))
                if n == len(warps):                        # one mask per frame
                    target_warps = warps
                elif target_map is not None:               # one mask per clip (set above): that of the annotated frame
                    per_clip = getattr(self, "_valid_per_clip", None)
                    if getattr(self, "valid_indices", None) is None or per_clip is None or len(per_clip) != n:
                        raise ValueError(f"{who}: augment= with one mask per clip needs the annotated frame of every clip: call set_valid_indices(per_clip, T) first")
                    target_warps = [clip[f] for clip, f in zip(clips, per_clip)]
                elif n == len(clips):                      # B masks for a target buffer of B*T: repeated like the images
                    target_warps = warps
                # (any other count is refused below, by the plan or against the target buffer)
        plan = _BatchPlan(images, targets, (H, W), frame_map, target_map, repeat, warps, target_warps)
        L = plan.layout
        if L.n_frames != self._n_frames():
            raise ValueError(f"{who}: {L.n_frames} frames for an image buffer of {self._n_frames()} ({tuple(self.x.shape)})")
        if L.n_targets and L.n_targets != self.t.shape[0]:
            raise ValueError(f"{who}: {L.n_targets} target masks for a target buffer of {self.t.shape[0]}")
        self._batch_preprocessor()._stage(plan)

    def commit_batch(self):
        """Launch the kernels of the staged batch into `image` (and `target`, when targets were staged) on the current stream -- the stream step()
        replays on, so they run after the previous replay and before the next."""
        who = f"{type(self).__name__}.commit_batch"
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{who}: the input stage runs eagerly in front of step(): call it outside the graph capture")
        pp = self.batch_preprocessor
        if pp is None or pp._staged is None:
            raise RuntimeError(f"{who}: no staged batch (call stage_batch() first; a batch is committed once)")
        pp.commit(self.x, self.t if pp._staged[1].n_targets else None)

    def load_batch(self, images, targets=None, repeat=None, *, frame_map=None, target_map=None, augment=None):
        """stage_batch + commit_batch"""
        self.stage_batch(images, targets, repeat, frame_map=frame_map, target_map=target_map, augment=augment)
        self.commit_batch()


TEXT_ENCODER_PREFIX = TEXT_ENCODER_KEY + "."          # 'bert_model.': the encoder's parameters wherever a step names parameters; 'bert_model' is the reference's checkpoint key (train.py:612)


class _StepModules(torch.nn.Module):
    """The two trainable modules of `--model lavt` as ONE module for GradBuckets and for every name the step hands out: the model's parameters under
    their own names, the separate text encoder's under 'bert_model.'.  The encoder comes first: its gradients are the last that backward produces, and
    GradBuckets lays the flat buffer out in reverse registration order."""

    def __init__(self, model, text_encoder):
        super().__init__()
        self.bert_model = text_encoder
        self.model = model

    def named_parameters(self, prefix="", recurse=True, remove_duplicate=True):
        yield from self.bert_model.named_parameters(prefix=prefix + TEXT_ENCODER_PREFIX[:-1], recurse=recurse, remove_duplicate=remove_duplicate)
        yield from self.model.named_parameters(prefix=prefix, recurse=recurse, remove_duplicate=remove_duplicate)


def _check_text_encoder(model, image, l_feats, l_mask, text_encoder, valid_indices):
    """the refusals of TrainStep(text_encoder=), before anything is built"""
    if valid_indices is not None:
        raise ValueError("TrainStep: text_encoder cannot be combined with valid_indices (the clip models carry their own encoder: LAVTVideo.text_encoder)")
    for name, t in (("l_feats", l_feats), ("l_mask", l_mask)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != 2:
            what = f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
            raise ValueError(f"TrainStep: with text_encoder the step computes the language features itself: {name} must be the static int64 (B, N_l) buffer of "
                             f"{'token ids' if name == 'l_feats' else 'the attention mask'}, got {what}" + (" (precomputed features belong to a step without text_encoder)"
                                                                                                              if name == "l_feats" and isinstance(t, torch.Tensor) and t.dtype.is_floating_point else ""))
    if tuple(l_feats.shape) != tuple(l_mask.shape):
        raise ValueError(f"TrainStep: l_feats (token ids) is {tuple(l_feats.shape)}, l_mask (attention mask) {tuple(l_mask.shape)}")
    devs = {p.device for p in text_encoder.parameters()}
    if devs != {image.device}:
        raise ValueError(f"TrainStep: text_encoder lives on {sorted(str(d) for d in devs)}, the step's buffers on {image.device}")
    if model.training and not text_encoder.training:
        raise ValueError("TrainStep: text_encoder is in eval mode while the model trains (the reference calls bert_model.train() beside model.train(): its dropout "
                         "is part of the iteration); call text_encoder.train()")


def check_sentences(ids, mask, shape, vocab_size, max_positions, who="Predictor.set_sentences"):
    """The refusals of Predictor.set_sentences as a pure function: token ids and attention mask for static int64 buffers of `shape` = (N, N_l), read by an
    encoder with `vocab_size` word rows and `max_positions` position rows and by PWAM, whose word axis holds ops.KV_LD tokens.  ValueError, naming the
    argument: a tensor of another shape or dtype than the buffers, N_l > max_positions, N_l > ops.KV_LD and -- for HOST tensors only -- an id outside
    [0, vocab_size).  Range is checked where the values come from the host (the rule of set_image_of); device tensors are the caller's promise: the
    kernels cannot raise and read word row 0 for an id out of range (include/lavt_hip.h: lavt_bert_embed_ln_fwd)."""
    shape = tuple(int(v) for v in shape)
    for name, t in (("ids", ids), ("mask", mask)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or tuple(t.shape) != shape:
            what = f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
            raise ValueError(f"{who}: {name} must be an int64 tensor of shape {shape} ({'token ids' if name == 'ids' else 'attention mask'}), got {what}")
    n_l = shape[1]
    if n_l > int(max_positions):
        raise ValueError(f"{who}: ids hold {n_l} tokens per sentence, the encoder has max_position_embeddings = {int(max_positions)}")
    if n_l > ops.KV_LD:
        raise ValueError(f"{who}: ids hold {n_l} tokens per sentence, the model's word axis holds ops.KV_LD = {ops.KV_LD}")
    if not ids.is_cuda and ids.numel():
        lo, hi = int(ids.min()), int(ids.max())
        if lo < 0 or hi >= int(vocab_size):
            bad = [(int(i), int(j), int(ids[i, j])) for i, j in ((ids < 0) | (ids >= int(vocab_size))).nonzero()[:4].tolist()]
            raise ValueError(f"{who}: ids (sentence, token, id) {bad} outside the vocabulary [0, {int(vocab_size)})")


def _check_predictor_text_encoder(model, image, lang, l_mask, text_encoder, valid_indices):
    """the refusals of Predictor(text_encoder=), after the existing checks and before anything is built"""
    for name, t in (("lang", lang), ("l_mask", l_mask)):
        if t.dtype != torch.int64 or t.dim() != 2:
            raise ValueError(f"Predictor: with text_encoder the predictor computes the language features itself: {name} must be the static int64 (N, N_l) buffer of "
                             f"{'token ids' if name == 'lang' else 'the attention mask'}, got {t.dtype} {tuple(t.shape)} (precomputed features belong to a predictor "
                             "without text_encoder)")
    if tuple(lang.shape) != tuple(l_mask.shape):
        raise ValueError(f"Predictor: lang (token ids) is {tuple(lang.shape)}, l_mask (attention mask) {tuple(l_mask.shape)}")
    if hasattr(model, "text_encoder"):
        raise ValueError(f"Predictor: text_encoder given, but {type(model).__name__} carries its own encoder (model.text_encoder runs inside forward_lowres): "
                         "feed it token ids without the argument")
    if valid_indices is not None:
        raise ValueError("Predictor: text_encoder cannot be combined with valid_indices (the clip models carry their own encoder: LAVTVideo.text_encoder)")
    devs = {p.device for p in text_encoder.parameters()}
    if devs != {image.device}:
        raise ValueError(f"Predictor: text_encoder lives on {sorted(str(d) for d in devs)}, the predictor's buffers on {image.device}")
    if text_encoder.training:
        raise RuntimeError("Predictor: text_encoder is in training mode -- call text_encoder.eval() first (dropout is not part of a prediction)")
    cfg = getattr(text_encoder, "config", None)
    n_l = int(lang.shape[1])
    if n_l > ops.KV_LD or (cfg is not None and n_l > cfg.max_position_embeddings):
        raise ValueError(f"Predictor: lang holds {n_l} tokens per sentence; the model's word axis holds ops.KV_LD = {ops.KV_LD}"
                         + (f", the encoder has max_position_embeddings = {cfg.max_position_embeddings}" if cfg is not None else ""))


class TrainStep(_ValidIndices, _ImageOf, _BatchInput):
    def __init__(self, model, image, l_feats, l_mask, target, world=1, use_graph=True, bucket_mib=32.0, fused_loss=True, refresh_weights_in_step=False, context=None,
                 *, loss="ce", valid_indices=None, dice_rate=1.0, boundary_rate=0.05, deterministic=None, accumulate=1, meters=None, image_of=None,
                 text_encoder=None):
        """context: the ops.StepContext this harness keeps its state in (gradient sinks, deferred-launch queues, weight copies, scratch).  None = the
        process-wide default context -- what the drop-in path and a single harness use.  Give every further model in the process its own
        `ops.StepContext()` (and its optimizer the same one: FusedAdamW(..., context=)): their steps can then alternate freely.
        loss: "ce" (losses.py:7-11, the default), "mc_dice" (MultiClassDiceLoss, losses.py:38-77; `--loss mc_dice` of train.py:703-704) or
        "dice_boundary" (DiceBoundaryLoss(boundary_rate, dice_rate), losses.py:142-244; `--loss dice_boundary` of train.py:709-711 with the
        `--dice_rate` / `--boundary_rate` of args.py:83-84; the other criteria ignore the two rates).
        valid_indices: device int32 [nsel], a static buffer like image and target -- the flat numbers of the annotated frames (A2D-Sentences / JHMDB:
        one per clip, train.py:282-285); target is then (nsel, H, W) and the criterion (and `stats`) covers `index_select(output, 0, valid_indices)`.
        Fill it with set_valid_indices(per_clip, frames_per_clip), before capture or between replays.
        deterministic: True / False sets the mode of the step's context, None keeps it (a context starts with LAVT_DETERMINISTIC).  In deterministic mode
        two steps from identical state (parameters, optimizer state, BatchNorm buffers, DropPath generator) on identical inputs give identical bits --
        loss, gradients, updated parameters, moments, running statistics -- eagerly and under graph replay, on ONE GPU (LAVT_FP8=1 included: its |max| history
        is part of the state): world > 1 and collectives forced in a 1-rank group raise NotImplementedError (DESIGN.md "Deterministic mode").
        accumulate: k >= 1 micro-batches per optimizer update (module docstring; DESIGN.md "Gradient accumulation").  1 = no accumulation: no second
        buffer, no further launch.  k > 1 needs an owned optimizer (make_optimizer / attach_optimizer) by warmup_and_capture(); the fold is element-wise,
        so the deterministic mode keeps its promise across cycles.
        meters: a lavt_hip.meters.TrainMeters (or make_meters() later, before warmup_and_capture()): the step's body then ends with ONE more launch,
        lavt_meter_append, which logs loss, lr, IoU, gradient norm and the update's verdict of every step() on the device (DESIGN.md "Training meters").
        None: the launches of a step built without the argument.  Needs a fused criterion (`stats`).  The logged I / U are the argmax counts of
        train.py:64-76 under every criterion: `meter_stats` is `stats` under loss="ce"; under "mc_dice" / "dice_boundary" a metered step makes it with one
        more kernel pair behind the criterion's forward (lib._utils.fused_iu), `stats` keeping the criterion's own layout.
        image_of: device int32 [N], a static buffer like image and target -- a PAIR-LIST train batch (include/lavt_hip.h: the image_of contract; DESIGN.md
        "Pair-list training").  `image` holds B images, l_feats / l_mask N expressions, target is (N, H, W); slot j trains expression j on image
        image_of[j].  Patch embedding and stage 0's Swin blocks run forward and backward once per IMAGE, ops.gather_pairs repeats their rows per slot
        and sums the slots' gradients per image (ascending slot order, fp32, no atomics: the same kernel in deterministic mode); everything behind runs
        on N samples, and loss, `stats` and the meters cover the N slots.  Fill it with set_image_of(pairs), before capture or between replays: every
        entry names one of the B images (no empty slots in training).  Needs a fused criterion and a backbone that shares stage 0; cannot be combined
        with valid_indices.  None (the default): the launches of a step built without the argument.
        text_encoder: the separate `bert_model` of `--model lavt` (train.py:595-602), trained INSIDE the step.  l_feats / l_mask are then the static int64
        (B, N_l) buffers of token ids and attention mask (N expressions under image_of), and the body starts with train.py:217-221 literally:
        `l = text_encoder(ids, attention_mask=mask)[0].permute(0, 2, 1)`, `m = mask.unsqueeze(-1)`.  Everything the step owns spans both modules: one flat
        gradient buffer and one bucket sequence, one zero fill; the encoder's parameters are named 'bert_model.<name>' wherever names appear (gradient norms,
        last_nonfinite(), the fingerprint, fp8 sites); make_optimizer() builds the reference's groups with the encoder's (train.py:623-632: encoder layers
        0..9 -- the other encoder parameters receive gradients and no update); state_dict() carries the reference's 'bert_model' entry.  Set
        text_encoder.fused_attention = True for the one-kernel attention core (bert/modeling_bert.py).  ValueError for floating-point l_feats, an encoder on
        another device or in eval mode while the model trains, or together with valid_indices.  None (the default): the step as it is without the argument."""
        import operator
        try:
            k = operator.index(accumulate)
        except TypeError:
            k = 0
        if k < 1:
            raise ValueError(f"TrainStep: accumulate must be an integer >= 1 (micro-batches per optimizer update), got {accumulate!r}")
        self.accumulate = k
        if loss not in ("ce", "mc_dice", "dice_boundary"):
            raise ValueError(f"TrainStep: loss must be 'ce', 'mc_dice' or 'dice_boundary', got {loss!r}")
        if text_encoder is not None:
            _check_text_encoder(model, image, l_feats, l_mask, text_encoder, valid_indices)
        self.text_encoder = text_encoder
        if image_of is not None:
            if valid_indices is not None:
                raise ValueError("TrainStep: image_of (pair-list batches) cannot be combined with valid_indices (annotated frames of clips)")
            _check_pair_buffer("TrainStep", image_of, l_feats.shape[0], target)
            if not fused_loss or not hasattr(model, "forward_lowres"):
                raise ValueError("TrainStep: image_of needs a fused criterion (fused_loss=True and a model with forward_lowres)")
            if not getattr(model.backbone, "shares_stage0", False):
                raise NotImplementedError(f"TrainStep: image_of needs a backbone that shares stage 0 between expressions; {type(model.backbone).__name__} does not")
        if valid_indices is not None:
            _check_index_buffer("TrainStep", valid_indices, target, image.numel() // (3 * int(image.shape[-2]) * int(image.shape[-1])))
        self.criterion, self.valid_indices, self.image_of = loss, valid_indices, image_of
        self.dice_rate, self.boundary_rate = float(dice_rate), float(boundary_rate)
        self.context = context if context is not None else ops.default_context()
        self._warmed = False
        self._dtype = None                       # (compute dtype, fp8) the launch sequence was warmed up and captured with
        self.set_deterministic(deterministic, world=world)
        with ops.use_context(self.context):
            self._init(model, image, l_feats, l_mask, target, world, use_graph, bucket_mib, fused_loss, refresh_weights_in_step)
        self.meters = None
        if meters is not None:
            self.attach_meters(meters)

    def _init(self, model, image, l_feats, l_mask, target, world, use_graph, bucket_mib, fused_loss, refresh_weights_in_step):
        self.model = model
        dev = image.device
        self.x, self.l, self.m, self.t = image, l_feats, l_mask, target
        self.w = torch.tensor([0.9, 1.1], device=dev)                    # losses.py:7-11
        # 32 MiB: the bucket that holds the earliest layers is reduced after backward has ended -- its all-reduce is the exposed tail of the step
        # (64 MiB ~ 0.4-0.8 ms over xGMI), while ~15 collectives of this size still run at full ring bandwidth.  LAVT_BUCKET_MIB overrides.
        bucket_mib = float(os.environ.get("LAVT_BUCKET_MIB", bucket_mib))
        # what the step trains, as one module: the model itself, or the model and the separate text encoder (its names prefixed 'bert_model.')
        self.trained = model if self.text_encoder is None else _StepModules(model, self.text_encoder)
        self.buckets = GradBuckets(self.trained, bucket_mib=bucket_mib, fused_accumulation=True)
        self.world = world
        self.graph = None
        self.loss = None
        self.use_graph = use_graph and (world == 1 or os.environ.get("LAVT_DDP_GRAPH", "1") != "0")
        self.captured = False
        self.zero_skip_values = 0                # gradient values left out of the captured zero fill (GradBuckets.set_zero_skip)
        ops.wgrads.enabled = True                # one weight gradient per parameter per step into the zeroed flat buffer: grouped, plainly stored
        self.fused_loss = fused_loss and hasattr(model, "forward_lowres")
        self.stats = None                        # fused loss: the criterion's statistics of the last step (device tensor; "ce": [loss, sum of weights, I, U])
        self.meter_stats = None                  # the fp32[4] row {loss, ., I, U} the meters log: `stats` itself under "ce"; under the Dice criteria the
                                                 # row of fused_iu when meters are attached, else None
        # The compute-dtype weight copies are refreshed by the optimizer (FusedAdamW.step re-casts them right after the update).  Set this when
        # the weights are changed by something else between replays of the captured step (a torch.optim optimizer, manual edits): the casts
        # (~0.3 ms for Swin-B) then run at the start of every step, inside the graph.
        self.refresh_in_step = refresh_weights_in_step or os.environ.get("LAVT_REFRESH_IN_STEP", "0") == "1"
        # A captured step runs no Python, so the per-parameter version check of the weight cache never fires on replay.  step() therefore compares
        # the parameters' version counters / storage addresses with what the compute copies were made from and re-casts them (eagerly, in front of
        # the replay) when anything but FusedAdamW has touched them: torch.optim optimizers, load_state_dict, manual edits all bump p._version.
        # FusedAdamW writes through raw pointers (versions do not move) and refreshes the copies itself.
        self._params = [p for p in self.trained.parameters()]
        self._seen = None
        self._one = None
        self.opt = None                          # the owned optimizer (make_optimizer / attach_optimizer): its step ends _body
        # accumulate > 1: the mean of the cycle's flat gradients so far, in the layout of buckets.flat.  Never zero-filled: the first fold of a cycle overwrites it
        self.acc = torch.zeros_like(self.buckets.flat) if self.accumulate > 1 else None

    def set_deterministic(self, deterministic, world=None):
        """Set the mode of the step's context (None: keep it).  Before warmup_and_capture() only: the captured launch sequence is frozen.  Raises
        NotImplementedError, naming it, for what the mode does not cover."""
        if self._warmed:
            raise RuntimeError("TrainStep: the deterministic mode must be set before warmup_and_capture() (the captured launch sequence is frozen)")
        mode = self.context.deterministic if deterministic is None else bool(deterministic)
        world = self.world if world is None else world
        if mode:
            if world > 1:
                raise NotImplementedError("TrainStep(deterministic=True): world > 1 is not covered (the reduction order of the gradient all-reduce is RCCL's)")
            from .ddp import FORCE_COLLECTIVES
            if FORCE_COLLECTIVES and torch.distributed.is_available() and torch.distributed.is_initialized():
                raise NotImplementedError("TrainStep(deterministic=True): collectives forced in a 1-rank group (LAVT_FORCE_COLLECTIVES=1, the LAVT_DDP_MODE "
                                          "routes at world 1) are not covered")
        self.context.deterministic = mode

    # ---- owned optimizer ----
    def make_optimizer(self, param_groups=None, *, text_encoder_layers=10, lang_enc_params="encoder-10", **adamw_kwargs):
        """Build a FusedAdamW on THIS step's context, attach it and return it.  param_groups=None: lavt_param_groups(model, text_encoder=the step's) when
        the model has a `backbone` and a `classifier` (the reference's groups; text_encoder_layers / lang_enc_params choose the language encoder's, as
        `--lang_enc_params` does), else all parameters the step trains.  adamw_kwargs go to FusedAdamW (lr, weight_decay,
        total_steps, power, max_grad_norm, skip_nonfinite, amsgrad, ...).  Before warmup_and_capture() only."""
        from .optim import FusedAdamW, lavt_param_groups
        self._check_attach_window()
        if "context" in adamw_kwargs:
            raise TypeError("TrainStep.make_optimizer: the optimizer is built on the step's own context")
        if param_groups is None:
            param_groups = (lavt_param_groups(self.model, text_encoder_layers, lang_enc_params=lang_enc_params, text_encoder=self.text_encoder)
                            if hasattr(self.model, "backbone") and hasattr(self.model, "classifier")
                            else [p for p in self.trained.parameters() if p.requires_grad])
        return self.attach_optimizer(FusedAdamW(param_groups, context=self.context, **adamw_kwargs))

    def attach_optimizer(self, opt):
        """Make an existing FusedAdamW part of the step (see make_optimizer).  It must maintain THIS step's context."""
        self._check_attach_window()
        if opt.context is not self.context:
            raise ValueError("TrainStep.attach_optimizer: the optimizer maintains the compute copies of another ops.StepContext than this step's: every "
                             "replay would read bf16 / packed weight copies that are never refreshed (training on frozen weights, silently).  "
                             "Construct it with FusedAdamW(..., context=step.context), or use step.make_optimizer()")
        self.opt = opt
        import weakref
        opt._owner = weakref.ref(self)           # (FusedAdamW.load_state_dict refuses once this step is captured: state_dict / load_state_dict below)
        return opt

    # ---- training meters ----
    def make_meters(self, **kw):
        """Build a lavt_hip.meters.TrainMeters(**kw) on the step's device, attach it and return it.  Before warmup_and_capture() only."""
        from .meters import TrainMeters
        kw.setdefault("device", self.x.device)
        return self.attach_meters(TrainMeters(**kw))

    def attach_meters(self, meters):
        """Make an existing TrainMeters part of the step: every step() appends one record.  Before warmup_and_capture() only."""
        if self._warmed:
            raise RuntimeError("TrainStep: meters must be attached before warmup_and_capture() (the captured launch sequence is frozen)")
        if self.meters is not None:
            raise RuntimeError("TrainStep: meters are already attached")
        if not self.fused_loss:
            raise ValueError("TrainStep: meters log the `stats` of a fused criterion (loss, I, U on the device); this step does not run one (fused_loss=False, "
                             "or a model without forward_lowres)")
        if meters.block.device != self.x.device:
            raise ValueError(f"TrainStep: the meters live on {meters.block.device}, the step on {self.x.device}")
        self.meters = meters
        return meters

    def _check_attach_window(self):
        if self._warmed:
            raise RuntimeError("TrainStep: the optimizer must be attached before warmup_and_capture() (the captured launch sequence is frozen)")
        if self.opt is not None:
            raise RuntimeError("TrainStep: an optimizer is already attached")

    # ---- gradient accumulation: the phase lives in the optimizer's control block ----
    def micro_step(self) -> int:
        """the micro index m of the running cycle, 0 <= m < accumulate: the next step() is micro-step m (synchronises).  0 = a cycle boundary."""
        if self.acc is None or self.opt is None:
            return 0
        return self.opt.micro_index()

    def reset_accumulation(self):
        """Restart the cycle: the next step() is its first micro-step (which overwrites `acc`) -- to drop the micro-batches of an open cycle, or after
        loading model and optimizer state dicts by hand.  load_state_dict() needs no such call: state_dict() saves `acc` and the phase inside a cycle,
        and a checkpoint from a cycle boundary sets the phase to 0 itself.  A host write (FusedAdamW.reset_phase()), like FusedAdamW.hold(): call it
        outside any capture; it waits for the device on both sides."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("TrainStep.reset_accumulation() is a host write: call it outside the graph capture")
        if self.acc is None or self.opt is None:
            return
        self.opt.reset_phase()

    text_encoder = None               # the separate `bert_model` the step trains beside the model (TrainStep(text_encoder=)); None = the model alone

    def _named_parameters(self):
        """(name, parameter) of everything the step trains: the model's own names, the text encoder's prefixed 'bert_model.'"""
        return self.model.named_parameters() if self.text_encoder is None else self.trained.named_parameters()

    # ---- checkpoint and resume (DESIGN.md "Checkpoint and resume") ----
    def _config(self):
        """the fingerprint a checkpoint is compared by (checkpoint.CONFIG_FIELDS): what decides the captured launch sequence and the layout of the state"""
        names = {id(p): n for n, p in self._named_parameters()}
        dtype, fp8 = self._dtype if self._dtype is not None else (compute_dtype(), fp8_enabled())
        groups = [[[names.get(id(p), f"<group {gi} entry {pi}: not a parameter of the model>"), [int(s) for s in p.shape]] for pi, p in enumerate(g["params"])]
                  for gi, g in enumerate(self.opt.param_groups)]
        return {"criterion": self.criterion, "dice_rate": self.dice_rate, "boundary_rate": self.boundary_rate, "accumulate": self.accumulate,
                "amsgrad": bool(self.opt.amsgrad), "max_grad_norm": float(self.opt.max_grad_norm), "skip_nonfinite": bool(self.opt.skip_nonfinite),
                "deterministic": bool(self.context.deterministic), "compute_dtype": str(dtype), "fp8": bool(fp8), "world": int(self.world),
                "param_groups": groups, **({} if self.image_of is None else {"pair_slots": int(self.image_of.numel())})}

    def _acc_layout(self):
        """[name, offset] of every parameter's gradient in the flat buffer `acc` mirrors, in offset order"""
        names = {id(p): n for n, p in self._named_parameters()}
        return sorted(([names.get(id(p), "?"), int(self.buckets.offset_of[id(p)])] for p in self.buckets.params), key=lambda e: e[1])

    def _fp8_sites(self):
        """{site name: slot} of the step's delayed-scaling sites; {} when fp8 is off"""
        from .checkpoint import fp8_site_slots
        f8 = self.context.fp8
        if not self._config()["fp8"] or f8.prev is None:
            return {}
        return fp8_site_slots(f8.slots, {id(p): n for n, p in self._named_parameters()})

    def _needs_owned_optimizer(self, who):
        if self.opt is None:
            raise RuntimeError(f"{who}: the step owns no optimizer (make_optimizer / attach_optimizer): only with one is a step() a whole training iteration "
                               "whose state is the step's to save")

    @staticmethod
    def _not_capturing(who):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{who} synchronises and copies between host and device: call it outside the graph capture")

    @_in_context
    def state_dict(self):
        """The whole state of the run, as CPU tensors and plain Python values (torch.load(..., weights_only=True) reads it back); synchronises.
          'model'             model.state_dict() -- the reference's key (train.py:610)
          'optimizer'         FusedAdamW.state_dict() -- torch.optim.AdamW's layout (train.py:724)
          'lavt_train_state'  format, config (the fingerprint load_state_dict compares), guard (the optimizer's control block; hold saved as 0), acc (+
                              its layout; only inside a cycle, micro_step() != 0 -- at a boundary it is dead), droppath (ops.droppath_state_dict() of the
                              step's context), fp8 ({'<consuming parameter>|act' or '|dy': [prev, cur]}; {} without fp8), torch_cuda_rng.
          'bert_model'        text_encoder.state_dict() -- the reference's key (train.py:612) -- exactly when the step has a text encoder
        Not state: gradients, the static input buffers, compute copies (re-made from the parameters), scratch.  checkpoint.save_train_state writes it."""
        from .checkpoint import TRAIN_STATE_FORMAT, to_host
        self._needs_owned_optimizer("TrainStep.state_dict")
        self._not_capturing("TrainStep.state_dict")
        dev = self._params[0].device
        torch.cuda.synchronize(dev)
        guard = self.opt.control_state()
        train = {"format": TRAIN_STATE_FORMAT, "config": self._config(), "guard": guard, "droppath": ops.droppath_state_dict(), "fp8": {},
                 "torch_cuda_rng": torch.cuda.get_rng_state(dev)}
        if self.micro_step() != 0:
            train["acc"] = self.acc.detach().to("cpu", copy=True)
            train["acc_layout"] = self._acc_layout()
        sites = self._fp8_sites()
        if sites:
            prev, cur = self.context.fp8.prev.cpu(), self.context.fp8.cur.cpu()
            train["fp8"] = {n: torch.stack([prev[i], cur[i]]) for n, i in sites.items()}
        state = {"model": to_host(self.model.state_dict()), "optimizer": to_host(self.opt.state_dict()), "lavt_train_state": train}
        if self.text_encoder is not None:          # the reference's key (train.py:612, 752-757): single_bert_model.load_state_dict(ckpt['bert_model'])
            state[TEXT_ENCODER_KEY] = to_host(self.text_encoder.state_dict())
        return state

    @_in_context
    def load_state_dict(self, state):
        """Continue the run `state` (a state_dict(), possibly through a file) was taken from: after warmup_and_capture() only, and IN PLACE -- parameters,
        buffers, both moments, max_exp_avg_sq, the weight average (FusedAdamW(ema_decay=...)), the step counter, the control block, acc, the DropPath generator, the fp8 |max| arrays and torch's CUDA
        generator are written into the storage they have, which is the storage the captured graph reads; then the compute copies are re-made and the
        next step() replays.  Before any write the checkpoint's fingerprint is compared with this step's (ValueError naming the first field that
        differs), and the model's, the optimizer's and the fp8 sites' entries are checked to fit: a load that raises has changed nothing.
        A checkpoint from a cycle boundary holds no acc: the phase is set to 0, as reset_accumulation() does.  world > 1: every rank loads its own file."""
        from .checkpoint import TRAIN_STATE_FORMAT, TRAIN_STATE_KEYS, compare_fingerprints, match_fp8_sites
        who = "TrainStep.load_state_dict"
        if not self._warmed or self._seen is None:
            raise RuntimeError(f"{who}: call warmup_and_capture() first.  Its eager iterations and validation replays advance forward-side state -- BatchNorm "
                               "running statistics and num_batches_tracked, the fp8 |max| history, the DropPath and torch generators -- so a state loaded "
                               "before it is not the state the first step() starts from; and the load writes into the storage the captured graph reads")
        self._needs_owned_optimizer(who)
        # ---- 1. everything that can be refused, before the first write
        missing = [k for k in TRAIN_STATE_KEYS if not isinstance(state, dict) or k not in state]
        if missing:
            raise ValueError(f"{who}: not a TrainStep.state_dict(): no '{missing[0]}'")
        train = state["lavt_train_state"]
        if train.get("format") != TRAIN_STATE_FORMAT:
            raise ValueError(f"{who}: format {train.get('format')!r} of 'lavt_train_state' is not {TRAIN_STATE_FORMAT}")
        if (TEXT_ENCODER_KEY in state) != (self.text_encoder is not None):
            raise ValueError(f"{who}: " + (f"this step trains a text encoder (TrainStep(text_encoder=)) and the checkpoint has no '{TEXT_ENCODER_KEY}' entry"
                                           if self.text_encoder is not None else
                                           f"the checkpoint has a '{TEXT_ENCODER_KEY}' entry (it was written by a step with text_encoder=) and this step has no text encoder"))
        compare_fingerprints(train["config"], self._config(), who)
        for key, module in (("model", self.model),) + (((TEXT_ENCODER_KEY, self.text_encoder),) if self.text_encoder is not None else ()):
            own = module.state_dict()
            for k, v in state[key].items():
                if k not in own:
                    raise ValueError(f"{who}: '{key}' has an entry {k} that this {'model' if key == 'model' else 'text encoder'} does not have")
                if tuple(v.shape) != tuple(own[k].shape):
                    raise ValueError(f"{who}: '{key}' entry {k} is {tuple(v.shape)} in the checkpoint, {tuple(own[k].shape)} in this {'model' if key == 'model' else 'text encoder'}")
            for k in own:
                if k not in state[key]:
                    raise ValueError(f"{who}: '{key}' has no entry {k}")
        plan = self.opt.check_state_dict_in_place(state["optimizer"])
        guard, acc = train.get("guard"), train.get("acc")
        self.opt.check_control_state(guard, who)
        if acc is not None:
            if self.acc is None or tuple(acc.shape) != tuple(self.acc.shape) or train.get("acc_layout") != self._acc_layout():
                raise ValueError(f"{who}: 'acc' of the checkpoint does not have the layout of this step's gradient buffer")
        sites = self._fp8_sites()
        match_fp8_sites(train["fp8"], sites, who)
        rng = train["torch_cuda_rng"]
        if not torch.is_tensor(rng) or rng.dtype != torch.uint8:
            raise ValueError(f"{who}: 'torch_cuda_rng' is not a generator state (a uint8 tensor)")
        # ---- 2. the writes: host copies on the current stream, between two synchronisations
        self._not_capturing(who)
        dev = self._params[0].device
        torch.cuda.synchronize(dev)
        with torch.no_grad():
            self.model.load_state_dict(state["model"], strict=True)          # copies into the parameters and buffers
            if self.text_encoder is not None:
                self.text_encoder.load_state_dict(state[TEXT_ENCODER_KEY], strict=True)
            self.opt.load_state_dict_in_place(state["optimizer"], plan)
            self.opt.load_control_state(guard, keep_phase=acc is not None)
            if acc is not None:
                self.acc.copy_(acc)
            ops.droppath_load_state_dict(train["droppath"])
            if sites:
                f8 = self.context.fp8
                order = sorted(sites, key=sites.get)
                idx = torch.tensor([sites[n] for n in order], dtype=torch.int64).to(dev)
                vals = torch.stack([train["fp8"][n].to(torch.float32) for n in order]).to(dev)
                f8.prev.index_copy_(0, idx, vals[:, 0].contiguous())
                f8.cur.index_copy_(0, idx, vals[:, 1].contiguous())
            torch.cuda.set_rng_state(rng, dev)
            ops.weights.refresh_all()                 # the compute copies the next replay reads, from the loaded parameters, into the storage they have
        torch.cuda.synchronize(dev)
        self._seen = self._param_stamp()

    def _param_stamp(self):
        return sum(p._version for p in self._params), sum(p.data_ptr() for p in self._params)

    def _language(self):
        """(l_feats, l_mask) as the model takes them: the static buffers, or -- with a text encoder -- train.py:217-221 on the id / attention-mask buffers"""
        if self.text_encoder is None:
            return self.l, self.m
        return self.text_encoder(self.l, attention_mask=self.m)[0].permute(0, 2, 1), self.m.unsqueeze(-1)

    @_in_context
    def _body(self):
        if self.acc is not None and (self.opt is None or self.opt._grad_source is None):
            raise RuntimeError("TrainStep(accumulate > 1): call make_optimizer() and warmup_and_capture() before step() (the owned optimizer reads `acc`)")
        if self.refresh_in_step:
            ops.weights.refresh_all()            # re-cast weights inside the step (for optimizers that do not maintain the compute copies)
        arena = ops.zero_arena.begin_step(self.x.device, defer=True)          # one fill for every small zero-initialised buffer of the step ...
        self.buckets.zero(also_zero=arena)                    # ... shared with the gradient buffer's
        ops.dtable_chain.job, ops.dtable_chain.keep = None, None          # (a backward that raised mid-way must not leave its binning job to the next step)
        if fp8_enabled():
            ops.fp8.advance()                    # delayed scaling: last step's |max| values become this step's quantisation scales
        if self.fused_loss:                       # upsample + criterion fused: the (B,2,H,W) logits are never written
            from lib._utils import fused_dice_boundary_loss, fused_dice_loss, fused_iu, fused_loss
            l, m = self._language()
            y = self.model.forward_lowres(self.x, l, m) if self.image_of is None else self.model.forward_lowres(self.x, l, m, image_of=self.image_of)
            if self.criterion == "ce":
                loss, self.stats = fused_loss(y, self.t, (0.9, 1.1), valid_indices=self.valid_indices)
                self.meter_stats = self.stats    # the cross-entropy pair counts the hard-mask I / U itself (stats[2:4])
            elif self.criterion == "mc_dice":
                loss, self.stats = fused_dice_loss(y, self.t, valid_indices=self.valid_indices)
            else:
                loss, self.stats = fused_dice_boundary_loss(y, self.t, valid_indices=self.valid_indices, dice_rate=self.dice_rate, boundary_rate=self.boundary_rate)
            if self.criterion != "ce":
                # the Dice criteria's `stats` hold soft sums at pinned offsets, no argmax counts: a metered step makes the log's row {loss, 0, I, U} with
                # one more kernel pair directly behind the criterion's forward (train.py:64-76 whatever --loss is); an unmetered step launches nothing
                self.meter_stats = fused_iu(y, self.t, valid_indices=self.valid_indices, loss=self.stats) if self.meters is not None else None
        else:
            out = self.model(self.x, *self._language())
            if self.valid_indices is not None:
                out = torch.index_select(out, 0, self.valid_indices)          # train.py:284, literally
            if self.criterion == "ce":
                loss = F.cross_entropy(out, self.t, weight=self.w)
            elif self.criterion == "mc_dice":
                from losses import MultiClassDiceLoss
                loss = MultiClassDiceLoss()(out, self.t)
            else:
                from losses import DiceBoundaryLoss
                loss = DiceBoundaryLoss(self.boundary_rate, self.dice_rate)(out, self.t)
        if self._one is None or self._one.shape != loss.shape or self._one.dtype != loss.dtype:
            self._one = torch.ones_like(loss)    # (first eager step) the root gradient as a persistent tensor: `loss.backward()` fills a fresh ones_like every step,
        loss.backward(self._one)                 # one more 4.5 us launch on the captured chain
        ops.wgrads.flush()                       # weight-gradient GEMMs still queued for a grouped launch
        ops.ln_deferred.flush()                  # all LayerNorm weight / bias partial sums of this backward: one reduction launch
        self.buckets.finish()                    # stragglers (never-used parameters) + join of the communication stream
        ops.zero_arena.end_step()
        ops.fp8.end_step()
        if self.acc is not None:
            # after buckets.finish() (world > 1: all-reduced already): acc = flat / k on the first micro-step of a cycle, acc += flat / k on the others;
            # sets the accumulating flag unless this micro-step ends the cycle -- the optimizer's kernels below then return before their first store
            K.check(K.lib.lavt_grad_accumulate(K.ptr(self.buckets.flat), K.ptr(self.acc), self.acc.numel(), self.accumulate, K.ptr(self.opt.guard), K.stream()))
        if self.opt is not None:
            # after buckets.finish(): with world > 1 the gradients are all-reduced already, the update needs no collective of its own.  Eager: the host-side
            # scan (re)builds the descriptor tables; inside the capture they are final (step(check_tables=False) raises if they are not).
            self.opt.step(check_tables=not torch.cuda.is_current_stream_capturing())
        if self.meters is not None:
            # the last launch of the iteration, behind the optimizer's tick: the record's lr is the one the NEXT update will use, as the reference logs it
            if self.opt is not None:
                ctl, cnt, hyper, total, power = self.opt.meter_args()
                self.meters.append(self.meter_stats, ctl, cnt, hyper, total, power)
            else:
                self.meters.append(self.meter_stats)
        return loss.detach()

    def warmup_and_capture(self, eager_iters=3):
        """With an owned optimizer (make_optimizer / attach_optimizer) the optimizer is on hold (FusedAdamW.hold) for every eager iteration and validation
        replay below, and released at the end: parameters, both moments, the optimizer's step and skipped-step counters and the compute copies are
        bit for bit what they were on entry (the copies are re-cast from the unchanged parameters).  The NaN-poison validation is unaffected: the
        update reads gradients and never writes them.
        Side effects beyond `eager_iters` steps: one more eager step when the bucket layout is still to settle (eager_iters = 1), and the zero-fill-skip validation below replays the captured step up to three more times on
        NaN-poisoned gradient buffers.  Each of those replays is a real training step of the forward pass -- BatchNorm running statistics and
        `num_batches_tracked`, the fp8 |max| history and the DropPath generator advance, and with world > 1 the poisoned buckets are all-reduced
        (NaN on every rank alike) -- the gradients of such a replay are discarded by the next step's fill.  LAVT_ZERO_SKIP=0 captures once.
        Accumulation (accumulate > 1): hold also stops the fold, so `acc` and the micro index leave the warm-up as they entered it -- the first step()
        afterwards starts a cycle."""
        if self.accumulate > 1:
            if self.opt is None:
                raise RuntimeError("TrainStep(accumulate > 1) needs an owned optimizer: the update that ends a cycle is part of the step.  Call "
                                   "make_optimizer() (or attach_optimizer()) before warmup_and_capture()")
            self.opt.set_grad_source(self.buckets.flat, self.acc)          # (creates the control block; outside any capture)
        self._warmed = True
        ops.note_raw_write()                     # (the forward passes below move the BatchNorm running statistics, as every step() does)
        if self.meters is not None:
            self.meters.pause()                  # the eager iterations and validation replays leave no record, with or without an owned optimizer
        try:
            if self.opt is None:
                return self._warmup_and_capture(eager_iters)
            self.opt.hold(True)
            try:
                return self._warmup_and_capture(eager_iters)
            finally:
                self.opt.hold(False)
        finally:
            if self.meters is not None:
                self.meters.resume()

    @_in_context
    def _warmup_and_capture(self, eager_iters):
        self._dtype = (compute_dtype(), fp8_enabled())
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for it in range(eager_iters):
                self.loss = self._body()
                if it == 0:                      # every compute copy exists now: one descriptor table for the one-launch refresh
                    ops.weights.build_multicast(compute_dtype())
                    ops.weights.refresh_all()
            if (self.use_graph or self.acc is not None) and self.buckets._relayout:          # (accumulation: `acc` follows the layout, which must not move inside a cycle)
                # GradBuckets lays the flat buffer out again in the zero() after its first step (parameters nothing reported join the late bucket): that
                # moves p.grad and must happen in an eager step -- inside the capture window zero() would raise and the harness would silently run eagerly
                self.loss = self._body()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        self._seen = self._param_stamp()
        if not self.use_graph:
            return
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            # ProcessGroupNCCL's watchdog thread retires the eager warm-up collectives by polling their events every ~100 ms.  Give it time to
            # empty its list before the capture window opens: a poll that lands inside the window was seen (1 run in ~10 of the 1-rank-group
            # test) to fail with hipErrorCapturedEvent and take the process down, also under the thread_local capture mode used below.
            # Explicit drain first: every warm-up collective has been waited for (GradBuckets.finish), the device is idle (synchronize above), and a
            # barrier puts all ranks at the same point -- after it no rank has an incomplete collective.  What remains is the watchdog's own
            # bookkeeping: it drops completed work objects from its list on its next poll, and PyTorch exposes no call to wait for that, so the
            # harness waits a few poll periods (TORCH_NCCL watchdog sleep: 100 ms) before opening the capture window.
            import time
            torch.distributed.barrier()
            torch.cuda.synchronize()
            time.sleep(float(os.environ.get("LAVT_CAPTURE_SETTLE_S", "0.35")))
        # Zero-fill skip: parameters whose gradient launch overwrote its buffer with plain stores in the last eager step (ops.sinks.assigned: members of the
        # grouped weight-gradient launches, the fused-tap convolution gradients) are CANDIDATES for being left out of the captured zero fill.  The captured
        # graph itself decides: the candidates' gradients are poisoned, the graph replayed once, and whatever still holds NaN -- a member the library cut
        # into pieces that meet through atomics, a buffer not fully written -- goes back into the fill and the step is captured again (at most three
        # rounds; the launch sequence of a captured step is frozen, so what passes here holds for every replay).
        cand = set(ops.sinks.assigned) if os.environ.get("LAVT_ZERO_SKIP", "1") != "0" else set()
        self.zero_skip_values = 0
        for attempt in range(4):
            skipped = self.buckets.set_zero_skip(cand if attempt < 3 else None)
            self._capture()
            if not self.captured:
                self.buckets.set_zero_skip(None)         # eager fallback: the full fill
                break
            if not skipped:
                break
            import math
            for v in self.buckets._skip_views:
                v.fill_(math.nan)
            self.graph.replay()
            torch.cuda.synchronize()
            flags = torch.stack([v.isnan().any() for v in self.buckets._skip_views]).tolist()
            if not any(flags):
                self.zero_skip_values = skipped
                break
            by_start = {self.buckets.flat.data_ptr() + 4 * self.buckets.offset_of[id(p)]: p for p in self.buckets.params}
            bad = [by_start[v.data_ptr()] for v, f in zip(self.buckets._skip_views, flags) if f]
            cand -= {id(p) for p in bad}
            if os.environ.get("LAVT_ZERO_SKIP_VERBOSE"):
                names = {id(p): n for n, p in self._named_parameters()}
                print(f"[lavt_hip.engine] zero-fill skip: {len(bad)} candidates are accumulated into or not fully written (e.g. {', '.join(names.get(id(p), '?') for p in bad[:4])}); "
                      "they stay in the fill, capturing again", file=sys.stderr)
            self.graph = None

    def _capture(self):
        self.captured = False
        try:
            g = torch.cuda.CUDAGraph()
            # thread_local: ProcessGroupNCCL's watchdog thread polls events of earlier (eager warm-up) collectives with hipEventQuery; under the
            # default "global" capture mode such a call from another thread, if it lands inside the capture window, aborts the capture with
            # hipErrorStreamCaptureUnsupported (seen as a c10::DistBackendError that takes the process down)
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                self.loss = self._body()
            self.graph = g
            self.captured = True
        except Exception as e:                                   # noqa: BLE001  (report and keep the eager path)
            print(f"[lavt_hip.engine] hipGraph capture failed, running eagerly: {type(e).__name__}: {e}", file=sys.stderr)
            self.graph = None
            torch.cuda.synchronize()

    @_in_context
    def step(self):
        if self.opt is not None and self.opt.ema_swapped:
            raise RuntimeError("TrainStep.step: the model's parameters hold the weight average (FusedAdamW.swap_ema() / inside ema_weights()): a step now "
                               "would train on the average -- swap back first")
        # eager or replay, with an optimizer or without: the train-mode BatchNorm kernels write running statistics through raw pointers on every forward
        ops.note_raw_write()
        if not self.refresh_in_step:
            stamp = self._param_stamp()
            if stamp != self._seen:                 # weights changed behind the compute copies' back (see __init__): refresh before the step
                if self._seen is not None:
                    ops.weights.refresh_all()
                self._seen = stamp
        if self.graph is not None:
            self.graph.replay()
        else:
            self.loss = self._body()
        return self.loss


_JF_WHOLE_SEQUENCES = ("Predictor: the J&F meter takes the frames of a step as whole sequences in frame order; it cannot be combined with "
                       "valid_indices, image_of or expressions_per_image > 1")


class Predictor(_ValidIndices, _ImageOf, _BatchInput):
    """The inference sibling of TrainStep: the reference's evaluation loop body (test.py:60-83, test_ytvos.py:230-260)

        model.eval(); with torch.no_grad(): out = model(image, l, l_mask); mask = out.argmax(1); I, U = computeIoU(mask, target)

    as one captured launch sequence: forward_lowres(folded=True, expand=S) -> ops.upsample_mask.  The BatchNorm layers of the decoder live in the
    convolution weights, the full-resolution logits are never written, the mask leaves as uint8 and the pixel counts as 2 integers per sample.

    image, lang, l_mask (and target) are STATIC device buffers: copy each sample into them, call step(), read `.mask` / `.iu`.
      lang        language features (B*S, 768, N_l) for LAVT; token ids (B*S, N_l) for LAVTOne / LAVTVideo (BERT runs inside the model)
      l_mask      (B*S, N_l, 1) for LAVT, (B*S, N_l) for LAVTOne / LAVTVideo -- what the model's forward takes
      target      optional int64 (B*S, Ho, Wo) ((B*T, Ho, Wo) for video), nonzero = foreground: `.iu` int32 (., 2) then holds per-sample I and U
      out_size    (Ho, Wo) of the mask, default = the network input size; via_size = (Hm, Wm): the two-stage interpolation of test_ytvos.py:249-253
                  (network input size first, then the original frame size)
      expressions_per_image   S: `image` holds B images, lang / l_mask B*S expressions (expression j of image i at i*S + j), mask sample i*S + j;
                  patch embedding and the stage-0 Swin blocks run once per image
      valid_indices   optional device int32 [nsel], a static buffer: the flat numbers of the annotated frames of the clips (A2D-Sentences / JHMDB,
                  test.py:182-205).  The backbone runs on all frames, the decoder and the mask kernel on the nsel selected ones: mask (nsel, Ho, Wo),
                  target (if given) (nsel, Ho, Wo), iu (nsel, 2).  set_valid_indices(per_clip, frames_per_clip) fills it, also between replays.
      image_of    optional device int32 [N], a static buffer, N = lang.shape[0]: a PAIR-LIST batch (include/lavt_hip.h: the image_of contract).  `image`
                  holds B images, lang / l_mask N expressions, slot j pairs expression j with image image_of[j]; N may be smaller or larger than B
                  (RefCOCO: a ragged number of sentences per referent, several referents per image), an entry outside [0, B) -- canonically -1 --
                  is an EMPTY slot: zero mask, iu row (0, 0), so the last batch of a dataset needs no second graph.  mask (N, Ho, Wo), target (if
                  given) (N, Ho, Wo), iu (N, 2).  set_image_of(seq) fills it, also between replays.  load_batch / stage_batch(target_map=) bring B
                  images and N target masks.
      meter       optional lavt_hip.metrics.DeviceEvalMeter (or make_meter() / attach_meter() later, before warmup_and_capture()): the body ends with
                  one more launch that does EvalMeter.update(pred.iu) on the device, for the live slots only.  Needs a target.
      text_encoder    optional: the separate `bert_model` of `--model lavt` (test.py:60-83 evaluates with it), in eval mode, run INSIDE the prediction
                  (DESIGN.md "Text encoder in the prediction").  lang / l_mask are then the static int64 (N, N_l) buffers of token ids and attention mask
                  (N = B * expressions_per_image, or the slot count under image_of; an empty slot's ids are encoded and its logits never read), and the
                  body opens with `l = text_encoder(ids, attention_mask=mask)[0].permute(0, 2, 1)`, `m = mask.unsqueeze(-1)`.  The stamp step() compares
                  covers the encoder's parameters and buffers too.  set_sentences(ids, mask) fills the buffers, also between replays.  Set
                  text_encoder.fused_attention / .fused_embeddings for the one-kernel attention core and opening (bert/modeling_bert.py): the
                  predictor sets neither.  ValueError for floating-point lang or a non-integer l_mask, a model that carries its own encoder, together
                  with valid_indices, an encoder on another device; RuntimeError for an encoder in training mode.
      jf_meter    optional lavt_hip.metrics.DeviceJFMeter (or make_jf_meter() / attach_jf_meter() later, before warmup_and_capture()): the video
                  measure J&F of the DAVIS 2017 evaluation on the device.  Behind the mask kernel, and behind the evaluation meter's append if there
                  is one, the body runs ops.boundary_counts(mask, target) into the static `jf` (int32 (frames, 8)) and one append of its sequence
                  means.  Needs a target; the target is at out_size, so with out_size / via_size the measure runs at the original frame size.
                  jf_frames_per_sequence: frames of one sequence, default T of a 5-D (B, T, 3, H, W) image, else all frames of the batch.
                  ValueError together with valid_indices, image_of or expressions_per_image > 1.  Paused during warm-up and capture like `meter`.
    step() never synchronises: it returns the static mask tensor, the caller decides when to read it (EvalMeter.update(pred.iu) reads `.iu` with one
    copy per call; a DeviceEvalMeter reads nothing until poll() / read()).  Built with none of image_of, meter, text_encoder and jf_meter, the launches
    are those of a predictor without the four arguments."""

    def __init__(self, model, image, lang, l_mask, *, target=None, out_size=None, via_size=None, expressions_per_image=1, use_graph=True, context=None,
                 valid_indices=None, image_of=None, meter=None, text_encoder=None, jf_meter=None, jf_frames_per_sequence=None):
        if model.training:
            raise RuntimeError("Predictor: the model is in training mode -- call model.eval() first (BatchNorm is folded from the running statistics, DropPath is off)")
        for name, t in (("image", image), ("lang", lang), ("l_mask", l_mask), ("target", target)):
            if t is not None and not t.is_cuda:
                raise RuntimeError(f"liblavt_hip operates on GPU memory only (got a CPU tensor for `{name}`); there is no CPU fallback")
        if not hasattr(model, "forward_lowres"):
            raise TypeError("Predictor: the model has no forward_lowres (LAVT, LAVTOne, LAVTVideo have)")
        S = int(expressions_per_image)
        if S < 1:
            raise ValueError("Predictor: expressions_per_image must be >= 1")
        if jf_meter is not None and (valid_indices is not None or image_of is not None or S > 1):
            raise ValueError(_JF_WHOLE_SEQUENCES)
        if valid_indices is not None:
            if S > 1:
                raise ValueError("Predictor: valid_indices selects frames of clips; it cannot be combined with expressions_per_image > 1")
            _check_index_buffer("Predictor", valid_indices, target, image.numel() // (3 * int(image.shape[-2]) * int(image.shape[-1])))
        self.valid_indices = valid_indices
        if image_of is not None:
            if S != 1:
                raise ValueError("Predictor: image_of names the image of every expression; it cannot be combined with expressions_per_image != 1")
            if valid_indices is not None:
                raise ValueError("Predictor: image_of (pair-list batches) cannot be combined with valid_indices (annotated frames of clips)")
            if not getattr(model.backbone, "shares_stage0", False):
                raise NotImplementedError(f"Predictor: image_of needs a backbone that shares stage 0 between expressions; {type(model.backbone).__name__} does not")
            _check_pair_buffer("Predictor", image_of, lang.shape[0], target)
        self.image_of = image_of
        if S > 1 and not getattr(model.backbone, "shares_stage0", False):
            raise NotImplementedError(f"Predictor: expressions_per_image > 1 needs a backbone that shares stage 0 between expressions; {type(model.backbone).__name__} does not")
        if image_of is None and lang.shape[0] != image.shape[0] * S:
            raise ValueError(f"Predictor: {lang.shape[0]} expressions for {image.shape[0]} images x {S} expressions per image")
        if text_encoder is not None:
            _check_predictor_text_encoder(model, image, lang, l_mask, text_encoder, valid_indices)
        self.text_encoder = text_encoder
        self.context = context if context is not None else ops.default_context()
        self.model, self.x, self.l, self.m, self.t = model, image, lang, l_mask, target
        self.S = S
        self.in_size = (int(image.shape[-2]), int(image.shape[-1]))
        self.out_size = (int(out_size[0]), int(out_size[1])) if out_size is not None else self.in_size
        self.via_size = (int(via_size[0]), int(via_size[1])) if via_size is not None else None
        self.use_graph = use_graph
        self.graph = None
        self.captured = False
        self.mask = None                         # uint8 (samples, Ho, Wo): static once captured
        self.iu = None                           # int32 (samples, 2) with a target, else None
        self.preprocessor = None                 # load_frames' FramePreprocessor(in_size), made on first use (assign one for another mean / std)
        # a replay runs no Python: neither the weight cache's version checks nor the BatchNorm fold's.  step() compares this stamp over parameters AND
        # buffers (the running statistics are folded into weights) and re-casts / re-folds eagerly, into the same storage, when anything moved
        self._state = [t for t in list(model.parameters()) + list(model.buffers())]
        if text_encoder is not None:          # the encoder's compute copies live in the same context and are read by the same graph
            self._state += list(text_encoder.parameters()) + list(text_encoder.buffers())
        self._seen = None
        self._warmed = False
        self.meter = None
        if meter is not None:
            self.attach_meter(meter)
        self.jf = None                           # int32 (frames, 8) with a J&F meter: {I, U, n_fg, n_gt, m_fg, m_gt, 0, 0} per frame at out_size
        self.jf_meter = None
        self.jf_frames_per_sequence = None if jf_frames_per_sequence is None else int(jf_frames_per_sequence)
        if jf_meter is not None:
            self.attach_jf_meter(jf_meter)
        elif jf_frames_per_sequence is not None and target is not None:
            self._jf_sequence_length()           # (refuse a bad length at construction, with or without a meter yet)

    _empty_slots = True          # pair-list batches (_ImageOf.set_image_of): -1 marks an empty slot

    # ---- J&F on the device ----
    def _jf_sequence_length(self):
        """frames per sequence of the J&F meter: jf_frames_per_sequence, else T of a 5-D (B, T, 3, H, W) image, else all frames of the batch"""
        frames = int(self.t.shape[0])          # (the mask has a frame per target frame: B*T for a video model)
        T = self.jf_frames_per_sequence
        if T is None:
            T = int(self.x.shape[1]) if self.x.dim() == 5 else frames
        if T < 1 or frames % T:
            raise ValueError(f"Predictor: the {frames} frames of a step are not whole sequences of {T} (jf_frames_per_sequence)")
        return T

    def make_jf_meter(self, **kw):
        """Build a lavt_hip.metrics.DeviceJFMeter(**kw) on the predictor's device, attach it and return it.  Before warmup_and_capture() only."""
        from .metrics import DeviceJFMeter
        kw.setdefault("device", self.x.device)
        return self.attach_jf_meter(DeviceJFMeter(**kw))

    def attach_jf_meter(self, meter):
        """Make an existing DeviceJFMeter part of the prediction step: behind the mask kernel (and the evaluation meter's append) the body runs
        ops.boundary_counts(mask, target) into `jf` and lavt_jf_meter_append on it: every step() adds its sequences.  Before warmup_and_capture()
        only; needs a `target`; refused with valid_indices, image_of and expressions_per_image > 1 (the frames of a step must be whole sequences)."""
        if self._warmed:
            raise RuntimeError("Predictor: a J&F meter must be attached before warmup_and_capture() (the captured launch sequence is frozen)")
        if self.jf_meter is not None:
            raise RuntimeError("Predictor: a J&F meter is already attached")
        if self.t is None:
            raise ValueError("Predictor: the J&F meter compares `mask` with a ground truth; this predictor was built without a target")
        if self.valid_indices is not None or self.image_of is not None or self.S > 1:
            raise ValueError(_JF_WHOLE_SEQUENCES)
        if meter.block.device != self.x.device:
            raise ValueError(f"Predictor: the J&F meter lives on {meter.block.device}, the predictor on {self.x.device}")
        self._jf_sequence_length()
        self.jf_meter = meter
        return meter

    # ---- the evaluation log on the device ----
    def make_meter(self, **kw):
        """Build a lavt_hip.metrics.DeviceEvalMeter(**kw) on the predictor's device, attach it and return it.  Before warmup_and_capture() only."""
        from .metrics import DeviceEvalMeter
        kw.setdefault("device", self.x.device)
        return self.attach_meter(DeviceEvalMeter(**kw))

    def attach_meter(self, meter):
        """Make an existing DeviceEvalMeter part of the prediction step: the body then ends with ONE more launch, lavt_eval_meter_append on `iu`, which
        counts every live sample of every step().  Before warmup_and_capture() only; needs a `target`."""
        if self._warmed:
            raise RuntimeError("Predictor: a meter must be attached before warmup_and_capture() (the captured launch sequence is frozen)")
        if self.meter is not None:
            raise RuntimeError("Predictor: a meter is already attached")
        if self.t is None:
            raise ValueError("Predictor: a meter logs the I / U counts of `iu`; this predictor was built without a target")
        if meter.block.device != self.x.device:
            raise ValueError(f"Predictor: the meter lives on {meter.block.device}, the predictor on {self.x.device}")
        self.meter = meter
        return meter

    def _stamp(self):
        # (ops.raw_writes: the fused optimizer, the train-mode BatchNorm kernels, an in-place checkpoint load and the weight-average swap write through
        # raw pointers -- no version moves.  A predictor built on the model that is being trained re-folds at its first step() after any of them)
        return sum(t._version for t in self._state), sum(t.data_ptr() for t in self._state), ops.raw_writes()

    @_in_context
    def _body(self):
        with torch.no_grad():
            l, m = self.l, self.m
            if self.text_encoder is not None:          # the text stage of TrainStep._language and LAVTOne.forward_lowres, on the id / attention-mask buffers
                l, m = self.text_encoder(l, attention_mask=m)[0].permute(0, 2, 1), m.unsqueeze(-1)
            if self.image_of is not None:
                y = self.model.forward_lowres(self.x, l, m, folded=True, image_of=self.image_of)
            elif self.valid_indices is None:
                y = self.model.forward_lowres(self.x, l, m, folded=True, expand=self.S)
            else:
                y = self.model.forward_lowres(self.x, l, m, folded=True, frames=self.valid_indices)
            n, _, h, w = y.shape
            from lib.mask_predictor import nchw_rows
            n_images = int(self.x.shape[0]) if self.image_of is not None else None
            self.mask, self.iu = ops.upsample_mask(nchw_rows(y, y.dtype), n, h, w, self.out_size, via_size=self.via_size, target=self.t, image_of=self.image_of,
                                                   n_images=n_images)
            if self.meter is not None:          # the last launch of the step
                self.meter.append(self.iu, self.image_of, n_images or 0)
            if self.jf_meter is not None:       # the J&F counts at out_size, then their sequence means
                self.jf = ops.boundary_counts(self.mask, self.t)
                self.jf_meter.append(self.jf, self._jf_sequence_length())
        return self.mask

    def warmup_and_capture(self, eager_iters=2):
        """eager_iters eager runs on a side stream (every compute copy and row map exists afterwards), then -- use_graph -- the body is captured into one
        torch.cuda.CUDAGraph on that stream: a straight-line sequence, no forked branches.  A failed capture is reported and the eager path kept.
        An attached meter is on hold (DeviceEvalMeter.pause) for the eager runs and the capture and released at the end: its count is what it was."""
        self._warmed = True
        meters = [m for m in (self.meter, self.jf_meter) if m is not None]
        if not meters:
            return self._warmup_and_capture(eager_iters)
        for m in meters:
            m.pause()
        try:
            return self._warmup_and_capture(eager_iters)
        finally:
            for m in meters:
                m.resume()

    @_in_context
    def _warmup_and_capture(self, eager_iters):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for it in range(max(int(eager_iters), 1)):
                self._body()
                if it == 0:
                    ops.weights.build_multicast(compute_dtype())
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        self._seen = self._stamp()
        if not self.use_graph:
            return
        self.captured = False
        try:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                self._body()
            self.graph, self.captured = g, True
        except Exception as e:                                   # noqa: BLE001  (report and keep the eager path)
            print(f"[lavt_hip.engine] hipGraph capture of the prediction step failed, running eagerly: {type(e).__name__}: {e}", file=sys.stderr)
            self.graph = None
            torch.cuda.synchronize()

    def set_sentences(self, ids, mask):
        """Copy token ids and attention mask (int64 (N, N_l), host or device tensors) into the static `lang` / `l_mask` buffers of a predictor built with
        text_encoder; usable between replays -- the captured text stage reads the buffers on the device.  check_sentences() runs first and refuses
        (ValueError) before any copy: another shape or dtype than the buffers, and, for host tensors, an id outside the encoder's vocabulary.  Host
        tensors go through pinned memory on the current stream, nothing synchronises."""
        who = "Predictor.set_sentences"
        if self.text_encoder is None:
            raise ValueError(f"{who}: built without text_encoder (lang / l_mask hold the caller's features: copy into them yourself)")
        cfg = self.text_encoder.config
        check_sentences(ids, mask, self.l.shape, cfg.vocab_size, cfg.max_position_embeddings, who=who)
        for dst, src in ((self.l, ids), (self.m, mask)):
            dst.copy_(src if src.is_cuda else src.contiguous().pin_memory(), non_blocking=True)

    def load_frames(self, frames_u8, targets_u8=None):
        """Fill the static `image` buffer (and `target`) from uint8 frames: the reference's Resize -> ToTensor -> Normalize (test.py:70-76,
        test_ytvos.py:236-243) on the device, with PIL's pixels (lavt_hip.preprocess.FramePreprocessor: what it accepts is accepted here).
        frames_u8: (n, Hs, Ws, 3) RGB, n = the frames the image buffer holds (B, or B*T for LAVTVideo: the buffer is written as (B*T, 3, H, W));
        targets_u8: (n', Hs, Ws) masks for a `target` of network-input size, resized with NEAREST.  Runs eagerly on the current stream in front of
        step(): nothing of it is part of the captured graph, nothing synchronises the host (host input is uploaded first, in one copy)."""
        from .preprocess import FramePreprocessor
        if self.preprocessor is None:
            self.preprocessor = FramePreprocessor(self.in_size)
        H, W = self.in_size
        n = self.x.numel() // (3 * H * W)
        pp = self.preprocessor
        frames = pp._to_device(frames_u8, 4)
        if frames.shape[0] != n:
            raise ValueError(f"Predictor.load_frames: {frames.shape[0]} frames for an image buffer of {n} ({tuple(self.x.shape)})")
        masks = None
        if targets_u8 is not None:
            if self.t is None:
                raise ValueError("Predictor.load_frames: targets given, but the predictor was built without a target buffer")
            if tuple(self.t.shape[-2:]) != self.in_size:
                raise ValueError(f"Predictor.load_frames: the target buffer is {tuple(self.t.shape[-2:])}, not the network input size {self.in_size} (the "
                                 "via_size / out_size flow keeps targets at the original frame size): copy those into `target` yourself")
            masks = pp._to_device(targets_u8, 3)
            if masks.shape[0] != self.t.shape[0]:
                raise ValueError(f"Predictor.load_frames: {masks.shape[0]} target masks for a target buffer of {self.t.shape[0]}")
        pp.images(frames, out=self.x)
        if masks is not None:
            pp.targets(masks, out=self.t)

    @_in_context
    def step(self):
        """-> the mask tensor (static when captured).  No host synchronisation."""
        if self.model.training:
            raise RuntimeError("Predictor.step: the model was put back into training mode")
        if self.text_encoder is not None and self.text_encoder.training:
            raise RuntimeError("Predictor.step: the text_encoder was put back into training mode")
        stamp = self._stamp()
        if stamp != self._seen:
            if self._seen is not None:
                ops.weights.refresh_all()          # casts, LayerNorm folds and BatchNorm folds, eagerly, into the storage the graph reads
            self._seen = stamp
        if self.graph is not None:
            self.graph.replay()
        else:
            self._body()
        return self.mask
