"""Training meters on the device: the reference's per-iteration log (train.py:231-235, 463-500 -- loss.item(), IoU(output, masks), precision@X,
cumulative I / U, metric_logger.update(loss=, lr=, iou=)) without a host synchronisation per step.

    step = TrainStep(model, ...); opt = step.make_optimizer(..., tensor_norms=True); meters = step.make_meters()
    step.warmup_and_capture()
    for it, batch in enumerate(loader):
        step.load_batch(*batch); step.step()
        if it % print_freq == 0:
            snap = meters.poll()                 # enqueues a copy, never waits; the newest snapshot whose copy has arrived (None before the first)
            if snap is not None: print(snap)     # "lr: 4.9e-05  loss: 0.7500 (0.7708)  iou: 0.3100 (0.2984)"
    print(meters.epoch_summary()); meters.reset_epoch()

lavt_meter_append (csrc/meters.hip), the last launch of TrainStep's body, writes one record per iteration into a ring on the device and moves the epoch
accumulators; the block's layout is the contract of include/lavt_hip.h and is restated here as numpy dtypes.  poll() copies the whole block to one of
two pinned host buffers on the current stream -- ordered between two replays, so the copy cannot be torn -- and hands out what an earlier copy brought.
A snapshot's `loss`, `lr`, `iou` and `grad_norm` have the properties of the reference's utils.SmoothedValue (median, avg, global_avg, max, value),
computed on the host from the ring copy over the last min(window_size, iterations this epoch) records.

One deliberate departure from the reference: a non-finite loss is counted (`nonfinite_losses`) and left out of the epoch's loss sum -- the reference's
running sum would be NaN for the rest of the epoch.  The ring keeps the raw value, so `value` / `median` of a window that holds one still show it.

reference_log() is the same arithmetic on the host from plain (loss, I, U) sequences: what the tests compare the device block against, itself checked
bit for bit against the reference's own classes (tests/golden/train_meter_cases.npz).
"""
import numpy as np
import torch

from . import _capi as K

HEADER_DOUBLES = 32
RECORD_BYTES = 40
RECORD_DTYPE = np.dtype([("loss", "<f4"), ("I", "<f4"), ("U", "<f4"), ("lr", "<f4"), ("grad_norm", "<f4"), ("flags", "<u4"), ("iou", "<f8"), ("it", "<i8")])
assert RECORD_DTYPE.itemsize == RECORD_BYTES
APPLIED, SKIPPED, ACCUMULATING, LOSS_NONFINITE = 1, 2, 4, 8
# header words (fp64)
H_CAPACITY, H_HOLD, H_N, H_EPOCH_START, H_ITERS, H_LOSS_SUM, H_LOSS_COUNT, H_LOSS_NONFINITE, H_IOU_SUM, H_CUM_I, H_CUM_U, H_SEG0 = range(12)
H_APPLIED, H_SKIPPED, H_ACCUMULATING, H_LR_SUM, H_NORM_SUM, H_NORM_COUNT = range(16, 22)
EPOCH_WORDS = slice(H_ITERS, H_NORM_COUNT + 1)          # what reset_epoch() zeroes
SEG_THRESHOLDS = (0.5, 0.6, 0.7, 0.8, 0.9)


def meter_bytes(capacity: int) -> int:
    """the documented size of a meter block (lavt_meter_bytes)"""
    return 8 * HEADER_DOUBLES + int(capacity) * RECORD_BYTES if capacity > 0 else 0


def iou_of(I, U) -> float:
    """train.py:64-76: 0 when the intersection or the union is empty, else I / U in double precision"""
    I, U = float(I), float(U)
    return 0.0 if I == 0.0 or U == 0.0 else I / U


class Smoothed:
    """utils.SmoothedValue's properties over a window of values that is already cut, with the epoch's total and count"""

    def __init__(self, window, total, count, fmt="{median:.4f} ({global_avg:.4f})"):
        self.window, self.total, self.count, self.fmt = [float(v) for v in window], float(total), count, fmt

    @property
    def median(self):
        return torch.tensor(self.window).median().item()          # (torch's lower median, on float32, as the reference computes it)

    @property
    def avg(self):
        return torch.tensor(self.window, dtype=torch.float32).mean().item()

    @property
    def global_avg(self):
        return self.total / self.count

    @property
    def max(self):
        return max(self.window)

    @property
    def value(self):
        return self.window[-1]

    def __str__(self):
        return self.fmt.format(median=self.median, avg=self.avg, global_avg=self.global_avg, max=self.max, value=self.value)


class Snapshot:
    """One copy of the meter block, decoded: `header` (float64[32]), `ring` (RECORD_DTYPE[capacity], slot = it % capacity) and the meters over them."""

    def __init__(self, raw, capacity, window_size):
        raw = np.array(raw, dtype=np.uint8, copy=True)
        self.header = raw[:8 * HEADER_DOUBLES].view(np.float64)
        self.ring = raw[8 * HEADER_DOUBLES:].view(RECORD_DTYPE)
        self.capacity, self.window_size = int(capacity), int(window_size)

    @property
    def n(self) -> int:
        """records appended since the block was made: the `it` of the next record"""
        return int(self.header[H_N])

    @property
    def iterations(self) -> int:
        """records of this epoch"""
        return int(self.header[H_ITERS])

    def records(self, count=None):
        """the last `count` records of this epoch that the ring still holds, oldest first (default: all of them)"""
        have = min(self.iterations, self.capacity)
        count = have if count is None else min(int(count), have)
        return self.ring[np.arange(self.n - count, self.n, dtype=np.int64) % self.capacity]

    def _meter(self, field, window_size, total, count, fmt="{median:.4f} ({global_avg:.4f})"):
        w = self.records(window_size)
        if len(w) == 0:
            raise ValueError("TrainMeters: no record in this epoch yet")
        return Smoothed(w[field].tolist(), total, count, fmt)

    @property
    def loss(self):
        return self._meter("loss", self.window_size, self.header[H_LOSS_SUM], int(self.header[H_LOSS_COUNT]))

    @property
    def iou(self):
        return self._meter("iou", self.window_size, self.header[H_IOU_SUM], self.iterations)

    @property
    def lr(self):
        return self._meter("lr", 1, self.header[H_LR_SUM], self.iterations, "{value}")          # train.py:201: SmoothedValue(window_size=1, fmt='{value}')

    @property
    def grad_norm(self):
        return self._meter("grad_norm", self.window_size, self.header[H_NORM_SUM], int(self.header[H_NORM_COUNT]))

    def __str__(self):
        """MetricLogger.__str__ with delimiter two spaces, the meters in the reference's order (lr is added first, train.py:201)"""
        return "  ".join(f"{k}: {getattr(self, k)}" for k in ("lr", "loss", "iou"))

    def state_dict(self):
        """header and ring as CPU tensors and plain values (torch.load(weights_only=True) reads it back); the hold word is saved as 0"""
        header = torch.from_numpy(self.header.copy())
        header[H_HOLD] = 0.0
        return {"format": 1, "capacity": self.capacity, "window_size": self.window_size, "header": header,
                "ring": torch.from_numpy(self.ring.copy().view(np.uint8))}

    def summary(self):
        """train.py:487-500: mean IoU and overall IoU in percent, precision@X in percent, and the counts"""
        h = self.header
        its = self.iterations
        nan = float("nan")
        return {"mean_iou": float(100 * (h[H_IOU_SUM] / its)) if its else nan,
                "precision": {t: float(h[H_SEG0 + j] * 100. / its) if its else nan for j, t in enumerate(SEG_THRESHOLDS)},
                "overall_iou": float(h[H_CUM_I] * 100. / h[H_CUM_U]) if h[H_CUM_U] else nan,
                "mean_loss": float(h[H_LOSS_SUM] / h[H_LOSS_COUNT]) if h[H_LOSS_COUNT] else nan,
                "iterations": its, "applied": int(h[H_APPLIED]), "skipped": int(h[H_SKIPPED]), "nonfinite_losses": int(h[H_LOSS_NONFINITE])}


def reference_log(losses, Is, Us, capacity, window_size, lrs=None, grad_norms=None, flags=None):
    """The block lavt_meter_append leaves after appending (losses[i], Is[i], Us[i]) in turn to a fresh block, computed on the host with the same
    arithmetic in the same order -> Snapshot.  losses are rounded to fp32 first (the device reads an fp32 scalar); lrs / grad_norms default to 0,
    flags to 0 (no optimizer), with the non-finite bit added here.  grad_norms[i] None: that append had no control block (0 in the ring, not counted)."""
    raw = np.zeros(meter_bytes(capacity), dtype=np.uint8)
    h, ring = raw[:8 * HEADER_DOUBLES].view(np.float64), raw[8 * HEADER_DOUBLES:].view(RECORD_DTYPE)
    h[H_CAPACITY] = capacity
    for i, (loss, I, U) in enumerate(zip(losses, Is, Us)):
        loss, I, U = np.float32(loss), np.float32(I), np.float32(U)
        lr = np.float32(lrs[i]) if lrs is not None else np.float32(0)
        has_ctl = grad_norms is not None and grad_norms[i] is not None
        gn = np.float32(grad_norms[i]) if has_ctl else np.float32(0)
        fl = int(flags[i]) if flags is not None else 0
        ok = bool(np.isfinite(loss))
        fl |= 0 if ok else LOSS_NONFINITE
        iou = iou_of(I, U)
        it = int(h[H_N])
        ring[it % capacity] = (loss, I, U, lr, gn, fl, iou, it)
        h[H_N] += 1.0
        h[H_ITERS] += 1.0
        if ok:
            h[H_LOSS_SUM] += float(loss)
            h[H_LOSS_COUNT] += 1.0
        else:
            h[H_LOSS_NONFINITE] += 1.0
        h[H_IOU_SUM] += iou
        h[H_CUM_I] += float(I)
        h[H_CUM_U] += float(U)
        for j, t in enumerate(SEG_THRESHOLDS):
            if iou >= t:
                h[H_SEG0 + j] += 1.0
        h[H_APPLIED] += 1.0 if fl & APPLIED else 0.0
        h[H_SKIPPED] += 1.0 if fl & SKIPPED else 0.0
        h[H_ACCUMULATING] += 1.0 if fl & ACCUMULATING else 0.0
        h[H_LR_SUM] += float(lr)
        if has_ctl and not fl & ACCUMULATING and bool(np.isfinite(gn)):
            h[H_NORM_SUM] += float(gn)
            h[H_NORM_COUNT] += 1.0
    return Snapshot(raw, capacity, window_size)


class DeviceBlock:
    """A block of fp64 words on the device -- word 0 the capacity, word 1 the hold word, as both meter layouts of include/lavt_hip.h have them -- with
    two pinned host buffers: the looking (poll / read) and the host writes (pause / resume, between two synchronisations) of TrainMeters and of
    lavt_hip.metrics.DeviceEvalMeter.  A subclass sets `nbytes`, `capacity`, `header_doubles` before _host_init() and decodes a copy in _decode()."""
    header_doubles = HEADER_DOUBLES

    def _host_init(self, device):
        who = type(self).__name__
        self._not_capturing(f"{who}()")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError(f"{who} lives in GPU memory only (no CPU fallback)")
        words = torch.zeros(self.nbytes // 8, dtype=torch.float64)
        words[H_CAPACITY] = float(self.capacity)
        self.block = words.to(dev)                               # fp64 words: 8-byte aligned; the ring is addressed in bytes behind the header
        self.header = self.block[:self.header_doubles]
        self._host = [torch.empty(self.nbytes, dtype=torch.uint8).pin_memory() for _ in range(2)]
        self._events = [torch.cuda.Event(), torch.cuda.Event()]
        self._inflight = None                                    # index of the buffer a copy is on its way to
        self._next = 0
        self._latest = None

    @staticmethod
    def _not_capturing(who):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{who} is a host call: it is refused inside a graph capture")

    def _decode(self, raw):
        raise NotImplementedError

    # ---- looking
    def _collect(self):
        i = self._inflight
        if i is not None and self._events[i].query():
            self._latest = self._decode(self._host[i].numpy())
            self._inflight = None

    def _enqueue(self):
        i = self._next
        with torch.no_grad():
            self._host[i].copy_(self.block.view(torch.uint8), non_blocking=True)
        self._events[i].record()
        self._inflight, self._next = i, 1 - i

    def poll(self):
        """Enqueue a device-to-host copy of the block on the CURRENT stream and record an event; never waits.  -> the newest Snapshot whose copy has
        completed (None before the first): it may be one poll old.  While an earlier copy is still on its way no further one is enqueued."""
        self._not_capturing(f"{type(self).__name__}.poll")
        self._collect()
        if self._inflight is None:
            self._enqueue()
        return self._latest

    def read(self):
        """poll(), then wait for that one copy -> its Snapshot: the block as of everything enqueued on the current stream so far"""
        self._not_capturing(f"{type(self).__name__}.read")
        if self._inflight is not None:
            self._events[self._inflight].synchronize()
            self._collect()
        self._enqueue()
        self._events[self._inflight].synchronize()
        self._collect()
        return self._latest

    # ---- host writes, between two synchronisations like FusedAdamW.hold()
    def _host_write(self, who, fn):
        self._not_capturing(who)
        torch.cuda.synchronize(self.block.device)
        with torch.no_grad():
            fn()
        torch.cuda.synchronize(self.block.device)

    def pause(self):
        """appends do nothing until resume() (warmup_and_capture pauses its eager iterations, the capture and the validation replays)"""
        self._host_write(f"{type(self).__name__}.pause", lambda: self.header[H_HOLD:H_HOLD + 1].fill_(1.0))

    def resume(self):
        self._host_write(f"{type(self).__name__}.resume", lambda: self.header[H_HOLD:H_HOLD + 1].fill_(0.0))


class TrainMeters(DeviceBlock):
    """The device block and two pinned host buffers.  capacity: records the ring holds (>= window_size); window_size: the reference's
    SmoothedValue(window_size=20).  device: where the block lives (default: the current CUDA device).  Attach to a step with
    TrainStep(..., meters=) or step.make_meters()."""

    def __init__(self, capacity=256, window_size=20, device=None):
        capacity, window_size = int(capacity), int(window_size)
        if capacity < 1 or window_size < 1 or window_size > capacity:
            raise ValueError(f"TrainMeters: need 1 <= window_size <= capacity, got capacity={capacity}, window_size={window_size}")
        self.capacity, self.window_size = capacity, window_size
        self.nbytes = int(K.lib.lavt_meter_bytes(capacity))
        if self.nbytes != meter_bytes(capacity):
            raise RuntimeError("TrainMeters: the library's block size is not the documented formula")
        self._host_init(device)

    def _decode(self, raw):
        return Snapshot(raw, self.capacity, self.window_size)

    # ---- the launch (TrainStep._body ends with it)
    def append(self, stats, ctl=None, step=None, hyper=None, total_steps=0.0, power=0.0):
        """enqueue lavt_meter_append on the current stream; capturable.  stats: the device fp32[4] row {loss, ., I, U} (TrainStep.meter_stats: the
        cross-entropy criterion's stats, or the row of lib._utils.fused_iu under the Dice criteria); ctl / step: device tensors (None without an optimizer);
        hyper: the fp32[5] hyper row whose base lr is logged, as a tensor or as its device address (FusedAdamW.meter_args gives a row of its table)"""
        K.check(K.lib.lavt_meter_append(K.ptr(stats), K.ptr(ctl), K.ptr(step), hyper if isinstance(hyper, int) else K.ptr(hyper), float(total_steps), float(power),
                                        K.ptr(self.block), self.capacity, K.stream()))

    def epoch_summary(self):
        """train.py:487-500 (synchronises once): mean IoU, precision@.5 .. .9 and overall IoU in percent, mean loss over the finite losses, and the
        iterations, applied / skipped updates and non-finite losses of the epoch"""
        return self.read().summary()

    def reset_epoch(self):
        """zero the epoch accumulators and start the window here; `it` keeps counting"""
        def write():
            self.header[H_EPOCH_START:H_EPOCH_START + 1].copy_(self.header[H_N:H_N + 1])
            self.header[EPOCH_WORDS].zero_()
        self._host_write("TrainMeters.reset_epoch", write)

    # ---- checkpoint: an extra key of checkpoint.save_train_state(path, step, meters=meters.state_dict())
    def state_dict(self):
        """header and ring as CPU tensors and plain values (torch.load(weights_only=True) reads it back); the hold word is saved as 0; synchronises"""
        self._not_capturing("TrainMeters.state_dict")
        torch.cuda.synchronize(self.block.device)
        return Snapshot(self.block.detach().cpu().view(torch.uint8).numpy(), self.capacity, self.window_size).state_dict()

    def load_state_dict(self, state):
        """write a state_dict() into the block this object has (a captured graph keeps its address); the hold word keeps its current value"""
        if state.get("format") != 1 or int(state["capacity"]) != self.capacity:
            raise ValueError(f"TrainMeters.load_state_dict: the state was saved with capacity={state.get('capacity')}, format={state.get('format')}; "
                             f"these meters have capacity={self.capacity}, format=1")
        header, ring = state["header"], state["ring"]
        if tuple(header.shape) != (HEADER_DOUBLES,) or header.dtype != torch.float64 or ring.dtype != torch.uint8 or ring.numel() != self.capacity * RECORD_BYTES:
            raise ValueError("TrainMeters.load_state_dict: header / ring do not have the block's layout")

        def write():
            hold = self.header[H_HOLD:H_HOLD + 1].clone()
            self.block.copy_(torch.cat([header, ring.view(torch.float64)]))
            self.header[H_HOLD:H_HOLD + 1].copy_(hold)
        self._host_write("TrainMeters.load_state_dict", write)
        self._latest, self._inflight = None, None
