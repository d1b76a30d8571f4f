"""Evaluation metrics of the reference's test loop (test.py:84-108): EvalMeter on the host, DeviceEvalMeter on the device.

EvalMeter accumulates per-sample intersection / union pixel counts -- what `lavt_hip.engine.Predictor.iu` holds after a step -- and reports mean IoU,
precision@{0.5 ... 0.9} and overall IoU in percent.  It runs on the host: `update` copies the counts it is given (a device tensor is read with one
device-to-host copy at that point, never inside Predictor.step()).  DeviceEvalMeter (below) keeps the same accumulators in a block on the device that
a Predictor's captured body appends to: no copy per step, the host looks with poll() / read().
"""
import numpy as np

THRESHOLDS = (0.5, 0.6, 0.7, 0.8, 0.9)          # test.py:61 eval_seg_iou_list


class EvalMeter:
    def __init__(self):
        self.reset()

    def reset(self):
        self.cum_I = 0
        self.cum_U = 0
        self.ious = []
        self.correct = [0] * len(THRESHOLDS)
        self.count = 0

    def update(self, iu):
        """iu: per-sample (I, U) counts, shape (n, 2) or (2,): a torch tensor (any device), numpy array or nested sequence of integers."""
        if hasattr(iu, "detach"):
            iu = iu.detach().cpu().numpy()
        iu = np.asarray(iu, dtype=np.int64).reshape(-1, 2)
        for I, U in iu.tolist():
            this_iou = 0.0 if U == 0 else I * 1.0 / U          # test.py:86-89
            self.ious.append(this_iou)
            self.cum_I += I
            self.cum_U += U
            for k, th in enumerate(THRESHOLDS):
                self.correct[k] += this_iou >= th                # test.py:93-95
            self.count += 1

    def summary(self):
        """-> {"mean_iou", "precision@0.5" ... "precision@0.9", "overall_iou"} in percent (test.py:100-108)"""
        if self.count == 0:
            raise RuntimeError("EvalMeter.summary: no samples")
        out = {"mean_iou": float(np.mean(np.array(self.ious)) * 100.0)}
        for k, th in enumerate(THRESHOLDS):
            out[f"precision@{th}"] = self.correct[k] * 100.0 / self.count
        out["overall_iou"] = (self.cum_I * 100.0 / self.cum_U) if self.cum_U else 0.0
        return out

    def __str__(self):
        s = self.summary()
        lines = ["Final results:", "Mean IoU is %.2f" % s["mean_iou"]]
        lines += ["    precision@%s = %.2f" % (th, s[f"precision@{th}"]) for th in THRESHOLDS]
        lines.append("    overall IoU = %.2f" % s["overall_iou"])
        return "\n".join(lines)


# ------------------------------------------------------------------------------------------ the same log kept on the device
# The evaluation meter block of include/lavt_hip.h ("Evaluation meter"), restated as numpy dtypes: lavt_eval_meter_append (csrc/meters.hip), the
# last launch of a Predictor's body, does EvalMeter.update's arithmetic for every live slot of a prediction batch; the host copies the block out when
# it wants to look.
#
#     pred = Predictor(model, image, lang, l_mask, target=target, image_of=buf); meter = pred.make_meter(); pred.warmup_and_capture()
#     for k, batch in enumerate(loader):
#         ...; pred.set_image_of(pairs); pred.step()
#         if k % 50 == 0: print(meter.poll())             # never waits: the newest snapshot that has arrived (None before the first)
#     print(meter.read())                                 # one synchronisation, at the end
EVAL_HEADER_DOUBLES = 16
EVAL_RECORD_BYTES = 16
EVAL_RECORD_DTYPE = np.dtype([("I", "<i4"), ("U", "<i4"), ("sample", "<i8")])
assert EVAL_RECORD_DTYPE.itemsize == EVAL_RECORD_BYTES
# header words (fp64)
E_CAPACITY, E_HOLD, E_N, E_COUNT, E_IOU_SUM, E_CUM_I, E_CUM_U, E_CORRECT0 = range(8)
E_ACCUMULATORS = slice(E_COUNT, E_CORRECT0 + len(THRESHOLDS))          # what reset() zeroes


def eval_meter_bytes(capacity: int) -> int:
    """the documented size of an evaluation meter block (lavt_eval_meter_bytes)"""
    return 8 * EVAL_HEADER_DOUBLES + int(capacity) * EVAL_RECORD_BYTES if capacity > 0 else 0


class EvalSnapshot:
    """One copy of the evaluation meter block, decoded: `header` (float64[16]) and `ring` (EVAL_RECORD_DTYPE[capacity], slot = sample % capacity).
    summary() and str() are EvalMeter's: same keys, percent units and text."""

    def __init__(self, raw, capacity):
        raw = np.array(raw, dtype=np.uint8, copy=True)
        self.header = raw[:8 * EVAL_HEADER_DOUBLES].view(np.float64)
        self.ring = raw[8 * EVAL_HEADER_DOUBLES:].view(EVAL_RECORD_DTYPE)
        self.capacity = int(capacity)

    @property
    def n(self) -> int:
        """samples appended since the block was made: the running sample number of the next record"""
        return int(self.header[E_N])

    @property
    def count(self) -> int:
        """samples since the last reset()"""
        return int(self.header[E_COUNT])

    @property
    def cum_I(self) -> int:
        return int(self.header[E_CUM_I])

    @property
    def cum_U(self) -> int:
        return int(self.header[E_CUM_U])

    @property
    def correct(self):
        return [int(v) for v in self.header[E_CORRECT0:E_CORRECT0 + len(THRESHOLDS)]]

    def records(self, count=None):
        """the last `count` records since the last reset() that the ring still holds, oldest first (default: all of them): the per-sample list
        the reference keeps (mean_IoU), as (I, U, running sample number)"""
        have = min(self.count, self.capacity)
        count = have if count is None else min(int(count), have)
        return self.ring[np.arange(self.n - count, self.n, dtype=np.int64) % self.capacity]

    def summary(self):
        """-> {"mean_iou", "precision@0.5" ... "precision@0.9", "overall_iou"} in percent (test.py:100-108), as EvalMeter.summary()"""
        if self.count == 0:
            raise RuntimeError("DeviceEvalMeter: no samples")
        out = {"mean_iou": float(self.header[E_IOU_SUM] / self.count * 100.0)}
        for k, th in enumerate(THRESHOLDS):
            out[f"precision@{th}"] = self.correct[k] * 100.0 / self.count
        out["overall_iou"] = (self.cum_I * 100.0 / self.cum_U) if self.cum_U else 0.0
        return out

    __str__ = EvalMeter.__str__          # (the text is built from summary() alone)

    def state_dict(self):
        """header and ring as CPU tensors and plain values (torch.load(weights_only=True) reads it back); the hold word is saved as 0"""
        import torch
        header = torch.from_numpy(self.header.copy())
        header[E_HOLD] = 0.0
        return {"format": 1, "capacity": self.capacity, "header": header, "ring": torch.from_numpy(self.ring.copy().view(np.uint8))}


def reference_block(iu_rows, capacity, live=None):
    """The block lavt_eval_meter_append leaves after appending the (I, U) rows in turn to a fresh block (live[i] False: an empty slot), computed on
    the host with the same arithmetic in the same order -> EvalSnapshot"""
    raw = np.zeros(eval_meter_bytes(capacity), dtype=np.uint8)
    h, ring = raw[:8 * EVAL_HEADER_DOUBLES].view(np.float64), raw[8 * EVAL_HEADER_DOUBLES:].view(EVAL_RECORD_DTYPE)
    h[E_CAPACITY] = capacity
    for i, (I, U) in enumerate(iu_rows):
        if live is not None and not live[i]:
            continue
        I, U = int(I), int(U)
        iou = 0.0 if U == 0 else I * 1.0 / U
        sample = int(h[E_N])
        ring[sample % capacity] = (I, U, sample)
        h[E_N] += 1.0
        h[E_COUNT] += 1.0
        h[E_IOU_SUM] += iou
        h[E_CUM_I] += float(I)
        h[E_CUM_U] += float(U)
        for k, th in enumerate(THRESHOLDS):
            if iou >= th:
                h[E_CORRECT0 + k] += 1.0
    return EvalSnapshot(raw, capacity)


from . import _capi as K  # noqa: E402  (the device meter needs the library; EvalMeter above does not use it)
from .meters import DeviceBlock  # noqa: E402


class DeviceEvalMeter(DeviceBlock):
    """EvalMeter's accumulators and per-sample list in a block on the device.  capacity: records the ring holds (the accumulators cover every sample
    whatever the capacity).  device: where the block lives (default: the current CUDA device).  Attach with Predictor(..., meter=), attach_meter()
    or make_meter(), before warmup_and_capture().  poll() (never waits), read() (synchronises), pause() and resume() are DeviceBlock's: the
    mechanism of TrainMeters."""
    header_doubles = EVAL_HEADER_DOUBLES

    def __init__(self, capacity=4096, device=None):
        capacity = int(capacity)
        if capacity < 1:
            raise ValueError(f"DeviceEvalMeter: capacity must be >= 1, got {capacity}")
        self.capacity = capacity
        self.nbytes = int(K.lib.lavt_eval_meter_bytes(capacity))
        if self.nbytes != eval_meter_bytes(capacity):
            raise RuntimeError("DeviceEvalMeter: the library's block size is not the documented formula")
        self._host_init(device)

    def _decode(self, raw):
        return EvalSnapshot(raw, self.capacity)

    # ---- the launch (Predictor._body ends with it)
    def append(self, iu, image_of=None, n_images=0):
        """enqueue lavt_eval_meter_append on the current stream; capturable.  iu: device int32 [n, 2]; image_of: the pair list's device int32 [n]
        with n_images (entries outside [0, n_images) are empty slots), None = every row counts"""
        import torch
        if iu.dtype != torch.int32 or iu.dim() != 2 or iu.shape[1] != 2 or not iu.is_contiguous():
            raise ValueError(f"DeviceEvalMeter.append: iu must be a contiguous int32 [n, 2], got {iu.dtype} {tuple(iu.shape)}")
        if image_of is not None and (image_of.dtype != torch.int32 or image_of.numel() != iu.shape[0] or not image_of.is_contiguous() or int(n_images) < 1):
            raise ValueError(f"DeviceEvalMeter.append: image_of must be a contiguous int32 vector of {iu.shape[0]} entries with n_images >= 1")
        K.check(K.lib.lavt_eval_meter_append(K.ptr(iu), K.ptr(image_of), int(n_images), int(iu.shape[0]), K.ptr(self.block), self.capacity, K.stream()))

    def reset(self):
        """zero the accumulators (count, sum of iou, cumulative I / U, the precision counters); the running sample number keeps counting"""
        self._host_write("DeviceEvalMeter.reset", lambda: self.header[E_ACCUMULATORS].zero_())
        self._latest, self._inflight = None, None

    # ---- checkpoint
    def state_dict(self):
        """header and ring as CPU tensors and plain values (torch.load(weights_only=True) reads it back); the hold word is saved as 0; synchronises"""
        import torch
        self._not_capturing("DeviceEvalMeter.state_dict")
        torch.cuda.synchronize(self.block.device)
        return EvalSnapshot(self.block.detach().cpu().view(torch.uint8).numpy(), self.capacity).state_dict()

    def load_state_dict(self, state):
        """write a state_dict() into the block this object has (a captured graph keeps its address); the hold word keeps its current value"""
        import torch
        if state.get("format") != 1 or int(state["capacity"]) != self.capacity:
            raise ValueError(f"DeviceEvalMeter.load_state_dict: the state was saved with capacity={state.get('capacity')}, format={state.get('format')}; "
                             f"this meter has capacity={self.capacity}, format=1")
        header, ring = state["header"], state["ring"]
        if tuple(header.shape) != (EVAL_HEADER_DOUBLES,) or header.dtype != torch.float64 or ring.dtype != torch.uint8 or ring.numel() != self.capacity * EVAL_RECORD_BYTES:
            raise ValueError("DeviceEvalMeter.load_state_dict: header / ring do not have the block's layout")

        def write():
            hold = self.header[E_HOLD:E_HOLD + 1].clone()
            self.block.copy_(torch.cat([header, ring.view(torch.float64)]))
            self.header[E_HOLD:E_HOLD + 1].copy_(hold)
        self._host_write("DeviceEvalMeter.load_state_dict", write)
        self._latest, self._inflight = None, None
