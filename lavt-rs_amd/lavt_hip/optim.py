"""Fused AdamW + poly learning-rate schedule for the LAVT step (the caller's optimizer, train.py:615-700).

    params_to_optimize = lavt_param_groups(model)                      # the reference's groups: no weight decay on norm / bias-table
    opt = FusedAdamW(params_to_optimize, lr=5e-5, weight_decay=1e-2, total_steps=len(loader) * epochs, power=0.9)
    ... loss.backward(); opt.step()                                    # ONE multi-tensor launch (+ a 1-thread tick) for all tensors

`torch.optim.Optimizer`-shaped (param_groups, state_dict / load_state_dict in torch.optim.AdamW's layout) so that the reference's
checkpoint code (train.py:749-763) keeps working.  The step counter and the schedule live on the device: the optimizer step can be
captured into the same hipGraph as forward/backward and still follows (1 - it/T)^0.9 on every replay (a LambdaLR on the host would be
frozen at capture time): engine.TrainStep.make_optimizer() does exactly that.

amsgrad=True (train.py:689-693, --amsgrad) is torch.optim.AdamW's rule: a third flat fp32 buffer holds state[p]["max_exp_avg_sq"], the running maximum
of the uncorrected second moment, which replaces it in the denominator (lavt_adamw_step_chunks_amsgrad, guarded or not).  The flag is optimizer-wide:
every group carries the constructor's value, and a checkpoint written with the other value is refused rather than half-loaded.

The guard (opt-in: max_grad_norm > 0, skip_nonfinite=True, or hold()): a device fp32[8] control block `opt.guard` = [global gradient norm, clip
coefficient, skip flag, skipped-step count, hold flag, accumulating flag, micro index, 0] -- the slots are named once, CTL_* below (LAVT_CTL_* of
include/lavt_hip.h), and the block is read and written from the host by this class alone: hold(), micro_index(), reset_phase(), control_state() /
load_control_state() for engine.TrainStep's checkpoints.  lavt_grad_norm fills the first three from the gradients the
update is about to read, the guarded update multiplies every gradient by the coefficient and does nothing at all (no store, no tick of the step
counter) when skip or hold is set -- no device-to-host synchronisation and no data-dependent launch, so it survives graph capture.

Gradient accumulation (set_grad_source; engine.TrainStep(accumulate=k)): the update reads its gradients from a second flat buffer into which
lavt_grad_accumulate folds each micro-batch's flat gradient.  guard[5] (accumulating: this micro-step does not end its cycle) is written by that
fold and obeyed by the norm, the update and the tick exactly like hold -- guard[0..3] and the step counter keep the values of the last applied
cycle; guard[6] is the micro index m, moved by the guarded tick ((m + 1) % k; not under hold).  Clip and the non-finite skip therefore act once per
cycle, on the accumulated gradient.  The accumulation buffer and the phase are not part of THIS state_dict(): engine.TrainStep.state_dict() saves them
(and everything else a captured run needs to continue bit for bit), and TrainStep.load_state_dict() restores the optimizer through
load_state_dict_in_place() -- into the tensors it has, because a captured graph keeps their addresses.  load_state_dict(), which installs new tensors,
refuses an optimizer whose step has been captured.

Weight EMA (ema_decay=d, off by default; DESIGN.md "Weight EMA"): a further flat fp32 buffer holds state[p]["ema"], torch's
AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(d)) of the parameter, maintained by the update kernel itself (lavt_adamw_step_chunks_ema) -- a graph
replay runs no Python, and a stream of the update obeys the control block with the moments: a skipped, held or accumulating step leaves it alone.  It
travels through state_dict() (`ema` per parameter, `ema_decay` in every group; a checkpoint with another decay, or with the average on one side only,
is refused before anything is written).  swap_ema() / ema_weights() exchange parameters and average in place for an evaluation, ema_state_dict(model)
exports the average; while swapped, step(), state_dict() and the loads raise.

Per-tensor gradient norms (tensor_norms=True, off by default; DESIGN.md "Training meters"): lavt_grad_norm's first pass already leaves one sum of squares per
chunk, and the chunk table lists every tensor's chunks contiguously -- lavt_grad_norm_tensors, one launch behind it, adds them per tensor in fp64 and notes
the first tensor that is not finite.  grad_norms() / last_nonfinite() read them (and synchronise); nothing of it enters state_dict() or a fingerprint.
"""
import os
from typing import Iterable, NamedTuple, Optional

import torch

from . import _capi as K


# The device protocol of the optimizer's kernels (include/lavt_hip.h: LAVT_CTL_*, LAVT_ADAMW_*; tests/test_optim_protocol_host.py compares the two): the
# slots of the control block, and how many columns a row of the descriptor / hyper-parameter table has.  Nothing else in Python knows the layout.
CTL_NORM, CTL_CLIP, CTL_SKIP, CTL_SKIPPED, CTL_HOLD, CTL_ACCUMULATING, CTL_MICRO = range(7)
CTL_FLOATS = 8
DESC_COLS = 6          # param, grad, exp_avg, exp_avg_sq, numel, copy
HYPER_COLS = 5         # lr, weight_decay, beta1, beta2, eps


def initial_control_block():
    """the control block as the kernels expect to find it before the first launch (a CPU tensor): zeros, and a clip coefficient of 1"""
    g = torch.zeros(CTL_FLOATS, dtype=torch.float32)
    g[CTL_CLIP] = 1.0
    return g


class _Tables(NamedTuple):
    """what one _build() leaves for step(): the key it was built for, the device tables and their sizes"""
    key: tuple
    desc: torch.Tensor            # int64 [count][DESC_COLS]
    hyper: torch.Tensor           # fp32 [count][HYPER_COLS]
    count: int
    chunks: torch.Tensor          # int32 [nchunks][2] = {desc row, chunk of that tensor}
    nchunks: int
    fused: dict                   # {compute-copy key: address} of the bf16 copies the update writes itself
    vmax: Optional[torch.Tensor]  # int64 [count]: one max_exp_avg_sq address per desc row; None without amsgrad
    ema: Optional[torch.Tensor]   # int64 [count]: one ema address per desc row; None without the average


LANG_ENC_PARAMS = ("encoder-10", "encoder-all", "embeddings+encoder-10", "embeddings+encoder-all")


def lavt_param_groups(model, text_encoder_layers: int = 10, *, lang_enc_params: str = "encoder-10", text_encoder=None):
    """The reference's parameter groups (train.py:615-686): backbone tensors whose name contains 'norm', 'absolute_pos_embed' or
    'relative_position_bias_table' get weight_decay 0; the rest of the backbone and the classifier use the default; then the language encoder's
    groups (only tensors with requires_grad), chosen by `lang_enc_params` (--lang_enc_params):
      'encoder-10'  the first `text_encoder_layers` BERT encoder layers        'encoder-all'  encoder.parameters()
      'embeddings+encoder-10' / 'embeddings+encoder-all'  a group of embeddings.parameters() in front of that encoder group.
    text_encoder: the separate `bert_model` of --model lavt (train.py:623-632); default model.text_encoder (a model without one gets no language group)."""
    if lang_enc_params not in LANG_ENC_PARAMS:
        raise ValueError(f"lavt_param_groups: lang_enc_params must be one of {LANG_ENC_PARAMS}, not {lang_enc_params!r}")
    no_decay, decay = [], []
    for name, p in model.backbone.named_parameters():
        (no_decay if ("norm" in name or "absolute_pos_embed" in name or "relative_position_bias_table" in name) else decay).append(p)
    groups = [{"params": no_decay, "weight_decay": 0.0}, {"params": decay},
              {"params": [p for p in model.classifier.parameters() if p.requires_grad]}]
    enc = text_encoder if text_encoder is not None else getattr(model, "text_encoder", None)
    if enc is not None and hasattr(enc, "encoder"):
        if lang_enc_params.startswith("embeddings+"):
            groups.append({"params": [p for p in enc.embeddings.parameters() if p.requires_grad]})
        if lang_enc_params.endswith("encoder-all"):
            groups.append({"params": [p for p in enc.encoder.parameters() if p.requires_grad]})
        else:
            groups.append({"params": [p for i in range(text_encoder_layers) for p in enc.encoder.layer[i].parameters() if p.requires_grad]})
    return groups


def ops_generation():
    """what a descriptor table depends on besides the gradient pointers it lists: the compute copies' buffers (ops.weights.generation) and the layout
    of the flat gradient buffer (ddp.layout_generation: GradBuckets re-lays it out once, in the second zero())"""
    from . import ops, ddp
    return (ops.weights.generation, ddp.layout_generation[0])


def _check_ema_decay(d):
    """None, or the decay as a float strictly between 0 and 1 (0 would be the iterate itself, 1 a constant): ValueError for anything else"""
    if d is None:
        return None
    if isinstance(d, bool) or not isinstance(d, (int, float)) or not 0.0 < float(d) < 1.0:
        raise ValueError(f"FusedAdamW: ema_decay must be None or a number strictly between 0 and 1, got {d!r}")
    return float(d)


def _ema_of_groups(groups):
    """the set of ema_decay values a state dict's param_groups carry (None: no average)"""
    return {None if g.get("ema_decay") is None else float(g["ema_decay"]) for g in groups}


class FusedAdamW(torch.optim.Optimizer):
    def __init__(self, params: Iterable, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, total_steps=0, power=0.9, context=None,
                 max_grad_norm=0.0, skip_nonfinite=False, ema_decay=None, *, tensor_norms=False):
        """max_grad_norm > 0: clip by the global L2 norm (torch.nn.utils.clip_grad_norm_'s coefficient); skip_nonfinite: leave parameters, moments, compute
        copies and the step counter untouched when that norm is NaN / Inf (counted in skipped_steps()).  With both off and hold() never called, step()
        is the unguarded launch sequence: no control block, no extra launch.
        context: the ops.StepContext whose compute-dtype weight copies this optimizer maintains (None = the process-wide default; pass the one given to
        engine.TrainStep when the model runs in a private context)
        ema_decay: None = no average (no buffer, no table, the launches of an optimizer built without the argument).  A number d in (0, 1): the update kernel
        also maintains state[p]["ema"], torch.optim.swa_utils.AveragedModel's exponential moving average with get_ema_multi_avg_fn(d) -- the first applied
        update copies the parameter, every later one is ema += (1 - d) * (p - ema); skip, hold and accumulating micro-steps leave it alone, as they
        leave the moments.  swap_ema() / ema_weights() put it in the parameters' place for an evaluation, ema_state_dict(model) exports it.
        tensor_norms: True selects the guarded path (as hold() does: the global norm is computed, with max_grad_norm = 0 and skip_nonfinite off it changes
        no bit of the update) and adds ONE launch behind lavt_grad_norm, lavt_grad_norm_tensors, which adds every tensor's per-chunk partial sums: grad_norms()
        reads the per-tensor norms of the last applied or skipped cycle, last_nonfinite() names the first tensor whose gradient was NaN / Inf the last time
        any was.  Not part of state_dict(), not part of a checkpoint's fingerprint."""
        from . import ops
        self.context = context if context is not None else ops.default_context()
        self.amsgrad = bool(amsgrad)          # optimizer-wide (one kernel for the whole chunk table): add_param_group reads it during super().__init__
        self.ema_decay = _check_ema_decay(ema_decay)          # optimizer-wide as well (a kernel argument)
        self.ema_swapped = False              # swap_ema(): the parameters hold the average, state[p]["ema"] the iterate
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=self.amsgrad)
        if self.ema_decay is not None:
            defaults["ema_decay"] = self.ema_decay
        super().__init__(params, defaults)
        self.total_steps, self.power = float(total_steps), float(power)
        self.fuse_copies = os.environ.get("LAVT_ADAMW_FUSE_COPIES", "1") != "0"
        self._tables = None
        self._probe = []
        self._step = None
        self.max_grad_norm, self.skip_nonfinite = float(max_grad_norm), bool(skip_nonfinite)
        self.guard = None          # the device control block (see the module docstring); None = the unguarded path
        self._norm_ws = None       # lavt_grad_norm's per-chunk partial sums
        self._grad_source = None   # set_grad_source: (flat, acc) -- read gradients from `acc` at the offsets p.grad has in `flat`
        self.tensor_norms = bool(tensor_norms)
        self._tn = None            # tensor_norms: (first-chunk table int32[count + 1], out fp64[count], parameters in desc order); _tn_bad: int32[4], kept across rebuilds
        self._tn_bad = None
        self._lr_row = 0           # the desc / hyper row of the first described parameter of group 0: the lr TrainMeters logs
        self._owner = None         # weak reference to the engine.TrainStep this optimizer is attached to (attach_optimizer)
        if self._wants_norm():
            self._make_guard()

    def add_param_group(self, param_group):
        if isinstance(param_group, dict) and "amsgrad" in param_group and bool(param_group["amsgrad"]) != self.amsgrad:
            raise ValueError(f"FusedAdamW: amsgrad is optimizer-wide: a group with amsgrad={param_group['amsgrad']} cannot join an optimizer built with "
                             f"amsgrad={self.amsgrad}")
        if isinstance(param_group, dict) and "ema_decay" in param_group and _ema_of_groups([param_group]) != {self.ema_decay}:
            raise ValueError(f"FusedAdamW: ema_decay is optimizer-wide: a group with ema_decay={param_group['ema_decay']} cannot join an optimizer built with "
                             f"ema_decay={self.ema_decay}")
        super().add_param_group(param_group)

    # ---- the guard ----
    def _wants_norm(self):
        return self.max_grad_norm > 0.0 or self.skip_nonfinite or self.tensor_norms

    def _device(self):
        return next(p for g in self.param_groups for p in g["params"]).device

    def _make_guard(self):
        if self.guard is None:
            dev = self._device()
            if dev.type != "cuda":
                raise RuntimeError("FusedAdamW runs on GPU memory only (no CPU fallback)")
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("FusedAdamW: the control block cannot be created inside a graph capture (construct with the guard options, or call hold() first)")
            self.guard = initial_control_block().to(dev)
        return self.guard

    def _host_write(self, who, write):
        """write(control block) from the host between two waits for the device (ordered against work on every stream); refused inside a capture"""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{who} is a host write: call it outside the graph capture")
        g = self._make_guard()
        torch.cuda.synchronize(g.device)
        write(g)
        torch.cuda.synchronize(g.device)

    def hold(self, flag=True):
        """While held, step() changes nothing -- parameters, moments, compute copies, step counter, skipped-step count -- whatever the gradients hold
        (TrainStep uses it for its warm-up iterations and validation replays).  A host write of the hold slot: call it outside any capture; it waits for
        the device on both sides, so it is ordered against work on every stream."""
        self._host_write("FusedAdamW.hold()", lambda g: g[CTL_HOLD:CTL_HOLD + 1].fill_(1.0 if flag else 0.0))

    # ---- the phase of an accumulation cycle and the block as a whole: what engine.TrainStep asks of the control block ----
    def micro_index(self) -> int:
        """the micro index m of the running accumulation cycle (synchronises); 0 without a control block"""
        return int(self.guard[CTL_MICRO].item()) if self.guard is not None else 0

    def reset_phase(self):
        """accumulating flag and micro index back to 0: the next step is the first micro-step of a cycle.  A host write, like hold()."""
        self._host_write("FusedAdamW.reset_phase()", lambda g: g[CTL_ACCUMULATING:CTL_MICRO + 1].zero_())

    def control_state(self):
        """a CPU copy of the control block with hold saved as 0 (a checkpoint never holds), or None without one; the caller has synchronised"""
        if self.guard is None:
            return None
        g = self.guard.detach().to("cpu", copy=True)
        g[CTL_HOLD] = 0.0
        return g

    def check_control_state(self, saved, who):
        """ValueError unless `saved` (a control_state(), or None) fits this optimizer: a block on both sides or on neither, of CTL_FLOATS words.  No write."""
        if (saved is None) != (self.guard is None) or (saved is not None and tuple(saved.shape) != (CTL_FLOATS,)):
            raise ValueError(f"{who}: the checkpoint has {'no' if saved is None else 'a'} control block ('guard'), this step's optimizer has {'none' if self.guard is None else 'one'}")

    def load_control_state(self, saved, keep_phase):
        """a checked control_state() into the block this optimizer has (a host copy: the caller synchronises around it); hold comes back as 0, and so
        does the phase unless keep_phase (without it the checkpoint was taken at a cycle boundary)"""
        if saved is not None:
            g = saved.detach().to(torch.float32).clone()
            g[CTL_HOLD] = 0.0
            if not keep_phase:
                g[CTL_ACCUMULATING:CTL_MICRO + 1] = 0.0
            self.guard.copy_(g)

    def set_grad_source(self, flat=None, acc=None):
        """Read every gradient from `acc` at the offset its p.grad has inside `flat` (two flat fp32 buffers of one layout: GradBuckets.flat and the
        buffer lavt_grad_accumulate folds it into) instead of from p.grad itself; None, None: back to p.grad.  The descriptor tables are still keyed
        and probed by p.grad, so a re-layout of the flat buffer rebuilds them as before.  Creates the control block (as hold() does: outside a
        capture) and thereby selects the guarded launches: the fold's accumulating flag lives in guard[5]."""
        if (flat is None) != (acc is None):
            raise ValueError("FusedAdamW.set_grad_source: give both buffers, or neither")
        if flat is not None:
            if not (flat.is_cuda and acc.is_cuda and flat.dtype == acc.dtype == torch.float32 and flat.dim() == acc.dim() == 1 and flat.numel() == acc.numel()
                    and flat.is_contiguous() and acc.is_contiguous() and flat.data_ptr() != acc.data_ptr()):
                raise ValueError("FusedAdamW.set_grad_source: flat and acc must be two distinct contiguous 1-d float32 GPU buffers of one size")
            self._make_guard()
        self._grad_source = (flat, acc) if flat is not None else None
        self._tables = None

    def _grad_address(self, p):
        """the address the update reads p's gradient at"""
        if self._grad_source is None:
            return p.grad.data_ptr()
        flat, acc = self._grad_source
        off = p.grad.data_ptr() - flat.data_ptr()
        if off < 0 or off % 4 or off + 4 * p.numel() > 4 * flat.numel():
            raise RuntimeError("FusedAdamW: set_grad_source() is in effect, but a parameter's .grad is not a view into that flat buffer")
        return acc.data_ptr() + off

    def last_grad_norm(self):
        """global gradient norm of the last guarded step (synchronises); None when no norm is computed"""
        return float(self.guard[CTL_NORM].item()) if self.guard is not None and self._wants_norm() else None

    def skipped_steps(self) -> int:
        return int(self.guard[CTL_SKIPPED].item()) if self.guard is not None else 0

    def _owner_step(self):
        """the engine.TrainStep this optimizer is attached to, or None (never attached, or the step is gone)"""
        return self._owner() if self._owner is not None else None

    def _trainable(self):
        return [p for g in self.param_groups for p in g["params"] if p.requires_grad]

    def _tensor_names(self):
        """what grad_norms() / last_nonfinite() call every described tensor: its name in the owning step's model, else its index in the tables"""
        if self._tn is None:
            raise RuntimeError("FusedAdamW: per-tensor norms exist with tensor_norms=True, after the first step()")
        owner = self._owner_step()
        names = {id(p): k for k, p in owner._named_parameters()} if owner is not None else {}
        return [names.get(id(p), i) for i, p in enumerate(self._tn[2])]

    def grad_norms(self):
        """{parameter name (with an owning TrainStep) or table index: L2 norm of its gradient} as of the last cycle that computed a norm (synchronises);
        under accumulation that is the accumulated gradient's"""
        if not self.tensor_norms:
            raise RuntimeError("FusedAdamW.grad_norms: build the optimizer with tensor_norms=True")
        names = self._tensor_names()
        return dict(zip(names, self._tn[1].sqrt().tolist()))

    def last_nonfinite(self):
        """the first tensor (name or index, as grad_norms() keys it) whose gradient norm was NaN / Inf in the most recent cycle that had one; None when
        none ever was (synchronises).  Sticky: clean cycles afterwards do not clear it."""
        if not self.tensor_norms:
            raise RuntimeError("FusedAdamW.last_nonfinite: build the optimizer with tensor_norms=True")
        if self._tn_bad is None:
            return None
        t = int(self._tn_bad[2].item())
        return self._tensor_names()[t] if t >= 0 else None

    def meter_args(self):
        """(control block or None, step counter, address of the hyper row whose lr is logged, total_steps, power): what TrainMeters.append reads of an
        optimizer -- valid once the tables exist (after the first step())"""
        if self._tables is None or self._step is None:
            raise RuntimeError("FusedAdamW.meter_args: the optimizer's tables do not exist yet (the first step() creates them)")
        return self.guard, self._step, self._tables.hyper.data_ptr() + 4 * HYPER_COLS * self._lr_row, self.total_steps, self.power

    # ---- flat optimizer state + device descriptor tables (built lazily: gradients must exist / be re-pointed first) ----
    def _build(self):
        ps = [(g, p) for g in self.param_groups for p in g["params"] if p.requires_grad]
        assert ps, "FusedAdamW: no parameters"
        dev = ps[0][1].device
        if dev.type != "cuda":
            raise RuntimeError("FusedAdamW runs on GPU memory only (no CPU fallback)")
        total = sum(p.numel() for _, p in ps)
        if self._step is None:
            self._step = torch.zeros(1, dtype=torch.float32, device=dev)
        if not all("exp_avg" in self.state[p] for _, p in ps):
            flat_m, flat_v = torch.zeros(total, dtype=torch.float32, device=dev), torch.zeros(total, dtype=torch.float32, device=dev)
            flat_x = torch.zeros(total, dtype=torch.float32, device=dev) if self.amsgrad else None
            flat_e = torch.empty(total, dtype=torch.float32, device=dev) if self.ema_decay is not None else None
            off = 0
            for _, p in ps:
                n = p.numel()
                st = self.state[p]
                st.setdefault("step", self._step)
                st["exp_avg"], st["exp_avg_sq"] = flat_m[off:off + n].view_as(p), flat_v[off:off + n].view_as(p)
                if self.amsgrad:
                    st["max_exp_avg_sq"] = flat_x[off:off + n].view_as(p)
                if self.ema_decay is not None:
                    st["ema"] = flat_e[off:off + n].view_as(p)
                    st["ema"].copy_(p.detach())          # (the first applied update overwrites it: until then the average of no iterates is the parameter)
                off += n
        if self.amsgrad and not all("max_exp_avg_sq" in self.state[p] for _, p in ps):
            raise ValueError("FusedAdamW(amsgrad=True): a parameter's state has exp_avg but no max_exp_avg_sq (it was written without amsgrad); the running "
                             "maximum is not started at zero silently")
        if self.ema_decay is not None and not all("ema" in self.state[p] for _, p in ps):
            raise ValueError("FusedAdamW(ema_decay=...): a parameter's state has exp_avg but no ema (it was written without the average); averaging is not "
                             "started silently in the middle of a run -- load a matching checkpoint, or call reset_ema() to start it from the current parameters")
        from . import ops
        desc, hyper, missing, chunks, fused, vmax, ema = [], [], [], [], {}, [], []
        first, described, lr_row = [], [], None          # tensor_norms: the first chunk of every desc row; the parameter behind it
        ce = int(K.lib.lavt_adamw_chunk_elems())
        for g, p in ps:
            if p.grad is None:
                missing.append(p)
                continue
            assert p.dtype == torch.float32 and p.grad.dtype == torch.float32 and p.is_contiguous() and p.grad.is_contiguous()
            st = self.state[p]
            # the parameter's bf16 compute copy in the parameter's own layout (Linear / 1x1 weights: lavt_hip.ops.weights, kind 'lin') is written by
            # the update kernel itself; packed conv weights, e4m3 copies and LayerNorm folds are refreshed after it (ops.weights.refresh_all)
            ck = (id(p), torch.bfloat16, "lin")
            ent = ops.weights.store.get(ck) if self.fuse_copies else None
            copy = 0
            if ent is not None and ent[2]() is p and ent[1].numel() == p.numel() and ent[1].is_contiguous():
                copy = ent[1].data_ptr()
                fused[ck] = copy
            first.append(len(chunks))
            described.append(p)
            if lr_row is None and g is self.param_groups[0]:
                lr_row = len(desc)
            for c in range(-(-p.numel() // ce)):
                chunks.append([len(desc), c])
            desc.append([p.data_ptr(), self._grad_address(p), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel(), copy])
            hyper.append([g["lr"], g["weight_decay"], g["betas"][0], g["betas"][1], g["eps"]])
            if self.amsgrad:
                vmax.append(st["max_exp_avg_sq"].data_ptr())
            if self.ema_decay is not None:
                assert st["ema"].dtype == torch.float32 and st["ema"].is_contiguous() and st["ema"].numel() == p.numel()
                ema.append(st["ema"].data_ptr())
        # (the copies' addresses are baked into the table: ops.weights.generation moves whenever one of them gets a new buffer)
        key = self._current_key()          # tracks p.grad (also under set_grad_source: desc[.][1] is then an address inside the accumulation buffer)
        # (every described parameter with the gradient address the table holds: step(check_tables=False) compares them all -- integer work on the host,
        # no device synchronisation; three probed addresses missed a single re-created .grad)
        self._probe = [(p, p.grad.data_ptr()) for _, p in ps if p.grad is not None]
        assert all(len(row) == DESC_COLS for row in desc) and all(len(row) == HYPER_COLS for row in hyper)
        self._tables = _Tables(key, torch.tensor(desc, dtype=torch.int64).to(dev), torch.tensor(hyper, dtype=torch.float32).to(dev), len(desc),
                               torch.tensor(chunks, dtype=torch.int32).to(dev), len(chunks), dict(fused),
                               torch.tensor(vmax, dtype=torch.int64).to(dev) if self.amsgrad else None,
                               torch.tensor(ema, dtype=torch.int64).to(dev) if self.ema_decay is not None else None)
        self._lr_row = lr_row or 0
        if self._wants_norm():
            need = int(K.lib.lavt_grad_norm_ws(len(chunks)))
            if self._norm_ws is None or self._norm_ws.numel() < need:
                self._norm_ws = torch.empty(need, dtype=torch.float32, device=dev)
        if self.tensor_norms:
            # (the chunk table lists every tensor's chunks contiguously, in ascending order: tensor t owns partials first[t] .. first[t + 1])
            self._tn = (torch.tensor(first + [len(chunks)], dtype=torch.int32).to(dev), torch.zeros(len(desc), dtype=torch.float64, device=dev), described)
            if self._tn_bad is None:
                self._tn_bad = torch.tensor([-1, 0, -1, 0], dtype=torch.int32).to(dev)

    def _current_key(self):
        out = []
        hy = []
        for g in self.param_groups:
            for p in g["params"]:
                if p.requires_grad and p.grad is not None:
                    out.append(p.grad.data_ptr())
                    hy.append((g["lr"], g["weight_decay"], g["betas"][0], g["betas"][1], g["eps"]))
        return tuple(out) + tuple(hy) + (ops_generation(),)

    @torch.no_grad()
    def step(self, closure=None, check_tables=True):
        from . import ops
        self._refuse_swapped("step")
        ops.note_raw_write()          # parameters (and compute copies) are written through raw pointers: engine.Predictor watches this counter
        with ops.use_context(self.context):
            return self._step_in_context(closure, check_tables)

    # ---- the weight average ----
    def _refuse_swapped(self, what):
        if self.ema_swapped:
            raise RuntimeError(f"FusedAdamW.{what}: the parameters hold the weight average (swap_ema() / inside ema_weights()): training on the average, or "
                               "saving it as the iterate, is never silent -- swap back first")

    def _needs_ema(self, what):
        if self.ema_decay is None:
            raise RuntimeError(f"FusedAdamW.{what}: this optimizer keeps no weight average (ema_decay=None)")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"FusedAdamW.{what} is a host call: it is refused inside a graph capture")

    def _ema_pairs(self, what):
        ps = self._trainable()
        if not all("ema" in self.state.get(p, ()) for p in ps):          # (.get: looking must not create empty state entries)
            raise RuntimeError(f"FusedAdamW.{what}: the optimizer's state does not exist yet (the first step() creates it)")
        return [(p, self.state[p]["ema"]) for p in ps]

    @torch.no_grad()
    def reset_ema(self):
        """ema <- p for every parameter: the explicit way to (re)start the average from the current iterate -- also on a state that has moments but no
        average yet (installed by hand from a run without one; the tables are then rebuilt by the next step()).  A host call outside any capture; it
        waits for the device on both sides, like hold()."""
        from . import ops
        self._needs_ema("reset_ema")
        self._refuse_swapped("reset_ema")
        ps = self._trainable()
        if not all("exp_avg" in self.state.get(p, ()) for p in ps):
            raise RuntimeError("FusedAdamW.reset_ema: the optimizer's state does not exist yet (the first step() creates it, with the average at the parameters)")
        dev = ps[0].device
        torch.cuda.synchronize(dev)
        for p in ps:
            st = self.state[p]
            if "ema" in st:
                st["ema"].copy_(p.detach())          # in place: a captured update keeps the address
            else:
                st["ema"] = p.detach().clone()
                self._tables = None
        ops.note_raw_write()
        torch.cuda.synchronize(dev)

    @torch.no_grad()
    def swap_ema(self):
        """Exchange every parameter with its average, in place (lavt_ema_swap: one launch over the update's own tables; the bf16 copies the update
        maintains are written from the new parameter), then refresh every other compute copy of the optimizer's context.  Toggles `ema_swapped`; while
        it is set, step(), state_dict() and the load_state_dict family raise.  Refused inside a capture.  Two calls restore every bit."""
        from . import ops
        self._needs_ema("swap_ema")
        with ops.use_context(self.context):
            if self._tables is None:
                raise RuntimeError("FusedAdamW.swap_ema: the optimizer's state and tables do not exist yet (the first step() creates them)")
            if self._tables.key != self._current_key():
                owner = self._owner_step()
                if owner is not None and owner.graph is not None:
                    raise RuntimeError("FusedAdamW.swap_ema: a compute copy was re-allocated, a gradient moved or a hyper-parameter was edited after the step "
                                       "was captured: the tables the captured update reads no longer describe the optimizer")
                self._build()
            T = self._tables
            K.check(K.lib.lavt_ema_swap(K.ptr(T.desc), K.ptr(T.ema), K.ptr(T.chunks), T.nchunks, K.stream()))
            self.ema_swapped = not self.ema_swapped
            ops.note_raw_write()
            ops.weights.refresh_all(done=T.fused)          # (as after step(): packed conv weights, e4m3 copies, LayerNorm and BatchNorm folds follow)

    def ema_weights(self):
        """`with opt.ema_weights(): evaluate` -- swap_ema() on entry and on exit (also when the body raises)"""
        import contextlib

        @contextlib.contextmanager
        def swapped():
            self.swap_ema()
            try:
                yield self
            finally:
                self.swap_ema()
        return swapped()

    @torch.no_grad()
    def ema_state_dict(self, model):
        """model.state_dict() with every averaged parameter replaced by a CPU copy of its average; parameters this optimizer does not update and all
        buffers as they are (torch's AveragedModel(use_buffers=False)): what to write as 'model_ema' next to 'model'.  Correct in either swap state."""
        if self.ema_decay is None:
            raise RuntimeError("FusedAdamW.ema_state_dict: this optimizer keeps no weight average (ema_decay=None)")
        avg = {id(p): (p if self.ema_swapped else e) for p, e in self._ema_pairs("ema_state_dict")}
        return {k: avg.get(id(v), v).detach().to("cpu", copy=True) for k, v in model.state_dict(keep_vars=True).items()}

    def _step_in_context(self, closure=None, check_tables=True):
        """check_tables=False skips the (host-side) scan for re-allocated gradients / edited hyper-parameters: use it when the gradients
        live in a fixed flat buffer (lavt_hip.ddp.GradBuckets) and the call is being captured into a hipGraph."""
        loss = closure() if closure is not None else None
        if self._tables is None or (check_tables and self._tables.key != self._current_key()):
            self._build()
        T = self._tables
        if not check_tables and (T.key[-1] != ops_generation() or any(p.grad is None or p.grad.data_ptr() != a for p, a in self._probe)):
            # (captured steps skip the host-side scan, but a copy that moved since the table was built would be written at its OLD address, and a
            # gradient buffer that was laid out again -- GradBuckets moves unreported parameters to the late bucket in its second zero() -- would be
            # read at its OLD offsets)
            raise RuntimeError("FusedAdamW.step(check_tables=False): a compute copy was re-allocated or the flat gradient buffer was laid out again "
                               "after the descriptor table was built; call step() once with check_tables=True (outside a capture) first")
        desc, hyper, chunks, step, guard = K.ptr(T.desc), K.ptr(T.hyper), K.ptr(T.chunks), K.ptr(self._step), K.ptr(self.guard)
        if self.guard is not None and self._wants_norm():
            K.check(K.lib.lavt_grad_norm(desc, chunks, T.nchunks, K.ptr(self._norm_ws), guard, self.max_grad_norm, int(self.skip_nonfinite), K.stream()))
            if self.tensor_norms:
                K.check(K.lib.lavt_grad_norm_tensors(K.ptr(self._norm_ws), T.nchunks, K.ptr(self._tn[0]), T.count, guard, K.ptr(self._tn[1]), K.ptr(self._tn_bad), K.stream()))
        if T.ema is not None:
            K.check(K.lib.lavt_adamw_step_chunks_ema(desc, K.ptr(T.vmax), K.ptr(T.ema), hyper, chunks, T.nchunks, step, self.total_steps, self.power, self.ema_decay,
                                                     guard, K.stream()))
        elif self.amsgrad:
            K.check(K.lib.lavt_adamw_step_chunks_amsgrad(desc, K.ptr(T.vmax), hyper, chunks, T.nchunks, step, self.total_steps, self.power, guard, K.stream()))
        elif self.guard is None:
            K.check(K.lib.lavt_adamw_step_chunks(desc, hyper, chunks, T.nchunks, step, self.total_steps, self.power, K.stream()))
        else:
            K.check(K.lib.lavt_adamw_step_chunks_guarded(desc, hyper, chunks, T.nchunks, step, self.total_steps, self.power, guard, K.stream()))
        # The kernel writes the parameters through raw pointers: p._version does not move, so the cached compute copies (bf16 Linear weights,
        # packed conv weights) are stale now.  They are part of the optimizer's output (fp32 master weights + the compute-dtype copies the next
        # forward reads, as in any mixed-precision trainer): re-cast them here, on the same stream, so that the forward/backward step itself
        # carries no cast kernels (the step harness refreshes them only when asked to: TrainStep(refresh_weights_in_step=True)).
        # (after a skipped or held step the same casts run on unchanged weights: harmless, and the launch sequence stays fixed for a capture)
        from . import ops
        ops.weights.refresh_all(done=T.fused)          # the copies in `fused` were written by the update kernel: only their stamps move
        return loss

    def steps_taken(self) -> int:
        return int(self._step.item()) if self._step is not None else 0

    def current_lr_factor(self) -> float:
        k = self.steps_taken()
        return max(1.0 - k / self.total_steps, 0.0) ** self.power if self.total_steps > 0 else 1.0

    def state_dict(self):
        self._refuse_swapped("state_dict")
        sd = super().state_dict()
        sd["lavt_schedule"] = {"total_steps": self.total_steps, "power": self.power, "steps_taken": self.steps_taken()}
        if self.guard is not None:
            sd["lavt_schedule"]["skipped_steps"] = self.skipped_steps()
        return sd

    def _check_amsgrad_of(self, state_dict, who):
        """refuse a checkpoint written with the other amsgrad setting (a plain one would start max_exp_avg_sq at zero, an AMSGrad one would lose it)"""
        theirs = {bool(g.get("amsgrad", False)) for g in state_dict["param_groups"]}
        if theirs != {self.amsgrad}:
            raise ValueError(f"{who}: the checkpoint's param_groups have amsgrad={sorted(theirs)} but this optimizer was built with amsgrad={self.amsgrad}")

    def _check_ema_of(self, state_dict, who):
        """refuse, before any write, a checkpoint whose weight average is not this optimizer's: present on one side only (averaging would start, or end,
        silently in the middle of a run) or kept with another decay"""
        theirs = _ema_of_groups(state_dict["param_groups"])
        if theirs != {self.ema_decay}:
            raise ValueError(f"{who}: the checkpoint's param_groups have ema_decay={sorted(theirs, key=lambda d: -1.0 if d is None else d)} but this optimizer "
                             f"was built with ema_decay={self.ema_decay}: the weight average (ema) is not started, dropped or re-weighted silently")
        has = {"ema" in st for st in state_dict["state"].values() if "exp_avg" in st}
        if has and has != {self.ema_decay is not None}:
            raise ValueError(f"{who}: the checkpoint's per-parameter state {'lacks' if self.ema_decay is not None else 'carries'} the weight average "
                             f"('ema'), this optimizer was built with ema_decay={self.ema_decay}")

    # ---- in-place load: for a captured step, whose graph holds the addresses of the moments and the counters ----
    _HYPER = ("lr", "weight_decay", "betas", "eps")

    def check_state_dict_in_place(self, state_dict):
        """Everything load_state_dict_in_place() will do, decided and checked without a write: -> the plan it takes.  ValueError for a state dict that does
        not fit -- amsgrad, the number of groups or of their parameters, a moment of another shape -- or that asks for what a captured launch sequence
        cannot follow: total_steps / power are kernel arguments and the groups' hyper-parameters a device table built with the descriptor tables, so they
        must be the ones this optimizer was constructed with."""
        who = "FusedAdamW.load_state_dict_in_place"
        self._refuse_swapped("load_state_dict_in_place")
        self._check_amsgrad_of(state_dict, who)
        self._check_ema_of(state_dict, who)
        groups = state_dict["param_groups"]
        if len(groups) != len(self.param_groups):
            raise ValueError(f"{who}: the checkpoint has {len(groups)} parameter groups, this optimizer {len(self.param_groups)}")
        sched = state_dict.get("lavt_schedule")
        if sched is not None and (float(sched["total_steps"]), float(sched["power"])) != (self.total_steps, self.power):
            raise ValueError(f"{who}: the checkpoint's schedule (total_steps={sched['total_steps']}, power={sched['power']}) is not this optimizer's "
                             f"(total_steps={self.total_steps}, power={self.power}), which the captured launches carry as arguments")
        pairs = []
        for gi, (sg, g) in enumerate(zip(groups, self.param_groups)):
            if len(sg["params"]) != len(g["params"]):
                raise ValueError(f"{who}: group {gi} has {len(sg['params'])} parameters in the checkpoint, {len(g['params'])} here")
            if sched is not None:          # (a torch.optim.AdamW checkpoint under a LambdaLR holds the scheduled lr: the group keeps its own, as load_state_dict's 'initial_lr' rule does)
                for h in self._HYPER:
                    a, b = sg.get(h, g[h]), g[h]
                    if (tuple(float(v) for v in a) != tuple(float(v) for v in b)) if h == "betas" else float(a) != float(b):
                        raise ValueError(f"{who}: group {gi} was saved with {h}={a}, this optimizer has {h}={b}: the device table of the captured step keeps "
                                         "the constructor's hyper-parameters")
            pairs += list(zip(sg["params"], g["params"]))
        keys = ("exp_avg", "exp_avg_sq") + (("max_exp_avg_sq",) if self.amsgrad else ()) + (("ema",) if self.ema_decay is not None else ())
        saved, plan, steps = state_dict["state"], [], None
        for sid, p in pairs:
            if not p.requires_grad:
                continue
            st = self.state.get(p)
            if st is None or any(k not in st for k in keys) or self._step is None:
                raise RuntimeError(f"{who}: this optimizer has no state yet to load into (it is created by the first step(): load in place after the warm-up)")
            src = saved.get(sid)
            for k in keys:
                if src is None:
                    plan.append((st[k], None if k != "ema" else p))          # (no entry: the parameter had seen no gradient; its moments start at zero, its average at the parameter)
                    continue
                if k not in src:
                    raise ValueError(f"{who}: the checkpoint's state of parameter {sid} has no '{k}'")
                if tuple(src[k].shape) != tuple(st[k].shape):
                    raise ValueError(f"{who}: '{k}' of parameter {sid} is {tuple(src[k].shape)} in the checkpoint, {tuple(st[k].shape)} here")
                plan.append((st[k], src[k]))
            if src is not None and steps is None and "step" in src:
                steps = float(src["step"].item()) if torch.is_tensor(src["step"]) else float(src["step"])
        if sched is not None:
            steps = float(sched["steps_taken"])
        skipped = float(sched["skipped_steps"]) if sched is not None and "skipped_steps" in sched else None
        if skipped and self.guard is None:
            raise ValueError(f"{who}: the checkpoint counts {int(skipped)} skipped steps, this optimizer has no control block to keep the count in")
        return plan, float(steps or 0.0), skipped

    @torch.no_grad()
    def load_state_dict_in_place(self, state_dict, plan=None):
        """load_state_dict for an optimizer whose tensors a captured graph reads: both moments, max_exp_avg_sq, the step counter and the skipped-step count
        are WRITTEN INTO the storage they have (host writes: outside any capture); no tensor is replaced, the descriptor tables stay.  The groups keep
        their hyper-parameters, which must equal the checkpoint's (check_state_dict_in_place: everything is checked before the first write).
        engine.TrainStep.load_state_dict() is the caller that also restores what the optimizer does not own."""
        self._refuse_swapped("load_state_dict_in_place")
        moments, steps, skipped = plan if plan is not None else self.check_state_dict_in_place(state_dict)          # (pure host checks: before touching the device)
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("FusedAdamW.load_state_dict_in_place() writes from the host: call it outside the graph capture")
        from . import ops
        ops.note_raw_write()          # (TrainStep.load_state_dict writes parameters and buffers around this call)
        for dst, src in moments:
            if src is None:
                dst.zero_()
            else:
                dst.copy_(src)
        self._step.fill_(steps)
        if skipped is not None and self.guard is not None:
            self.guard[CTL_SKIPPED:CTL_SKIPPED + 1].fill_(skipped)

    def load_state_dict(self, state_dict):
        owner = self._owner_step()
        if owner is not None and owner.graph is not None:
            raise RuntimeError("FusedAdamW.load_state_dict: this optimizer is part of a TrainStep whose step has been captured: the graph keeps the addresses "
                               "of the moments and the step counter this call would replace, and would go on training from the old ones.  Use "
                               "TrainStep.load_state_dict(), which loads in place")
        self._refuse_swapped("load_state_dict")
        sched = state_dict.get("lavt_schedule")
        self._check_ema_of(state_dict, "FusedAdamW.load_state_dict")
        self._check_amsgrad_of(state_dict, "FusedAdamW.load_state_dict")
        super().load_state_dict({k: v for k, v in state_dict.items() if k != "lavt_schedule"})
        steps = None
        if sched is not None:
            self.total_steps, self.power, steps = float(sched["total_steps"]), float(sched["power"]), sched["steps_taken"]
        else:
            for st in self.state.values():          # a torch.optim.AdamW checkpoint: per-parameter 'step'
                if "step" in st:
                    steps = int(st["step"].item()) if torch.is_tensor(st["step"]) else int(st["step"])
                    break
            if self.total_steps > 0:
                for g in self.param_groups:          # a LambdaLR left its scheduled lr in the group and the base in 'initial_lr': (1 - it/T)^power is applied here
                    if "initial_lr" in g:
                        g["lr"] = g["initial_lr"]
        dev = self.param_groups[0]["params"][0].device
        self._step = torch.full((1,), float(steps or 0), dtype=torch.float32, device=dev)
        for st in self.state.values():
            st["step"] = self._step
        if sched is not None and "skipped_steps" in sched and (self.guard is not None or sched["skipped_steps"]):
            self._make_guard()[CTL_SKIPPED:CTL_SKIPPED + 1].fill_(float(sched["skipped_steps"]))
        self._tables = None
