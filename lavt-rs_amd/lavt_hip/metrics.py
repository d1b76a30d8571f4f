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


# ------------------------------------------------------------------------------------------ J&F: the video measure (DAVIS 2017)
# Refer-YouTube-VOS and Ref-DAVIS results are reported as J (region similarity), F (boundary F-measure) and J&F (their mean).  What follows restates
# the DAVIS 2017 toolkit's db_eval_iou, db_eval_boundary and _seg2bmap WITHOUT void pixels (include/lavt_hip.h "J&F measure" has the contract in
# full); the toolkit's recall and decay statistics are not computed.  Conventions that differ from EvalMeter above: U == 0 gives J = 1 (two empty
# masks agree); an empty boundary on one side only gives precision / recall (1, 0) or (0, 1), on both sides (1, 1).
#
#     pred = Predictor(model, clip, ids, mask, target=target, out_size=(720, 1280), via_size=(480, 480)); jf = pred.make_jf_meter(); pred.warmup_and_capture()
#     for clip in loader: ...; pred.step()                # pred.jf: int32 (frames, 8) = {I, U, n_fg, n_gt, m_fg, m_gt, 0, 0} at the original frame size
#     print(jf.read().summary())                          # {"J", "F", "J&F", "sequences", "frames"} in percent; one synchronisation, at the end
#
# A video that is split over several steps is grouped on the host: JFMeter().update(pred.jf, sequence_ids).
JF_HEADER_DOUBLES = 16
JF_RECORD_BYTES = 32
JF_RECORD_DTYPE = np.dtype([("frames", "<i4"), ("zero", "<i4"), ("J", "<f8"), ("F", "<f8"), ("sequence", "<i8")])
assert JF_RECORD_DTYPE.itemsize == JF_RECORD_BYTES
JF_CAPACITY, JF_HOLD, JF_N, JF_SEQS, JF_JSEQ_SUM, JF_FSEQ_SUM, JF_FRAMES, JF_JFRAME_SUM, JF_FFRAME_SUM = range(9)
JF_ACCUMULATORS = slice(JF_SEQS, JF_FFRAME_SUM + 1)          # what reset() zeroes
BOUNDARY_MAX_RADIUS = 40                                     # LAVT_BOUNDARY_MAX_RADIUS


def davis_bound_pix(H, W, bound_th=0.008):
    """the disk radius of db_eval_boundary for an H x W frame: ceil(0.008 * sqrt(H*H + W*W)) in fp64 (8 at 480x854, 12 at 720x1280)"""
    import math
    return int(math.ceil(bound_th * math.sqrt(float(H) * float(H) + float(W) * float(W))))


def _seg2bmap(S):
    """the toolkit's boundary map of a boolean (H, W) mask at its own size"""
    e, s, se = np.zeros_like(S), np.zeros_like(S), np.zeros_like(S)
    e[:, :-1] = S[:, 1:]
    s[:-1, :] = S[1:, :]
    se[:-1, :-1] = S[1:, 1:]
    b = (S ^ e) | (S ^ s) | (S ^ se)
    b[-1, :] = S[-1, :] ^ e[-1, :]
    b[:, -1] = S[:, -1] ^ s[:, -1]
    b[-1, -1] = False
    return b


def _disk_dilate(b, r):
    """OR of b over the disk dy*dy + dx*dx <= r*r, positions outside the frame ignored: one horizontal run per dy"""
    H, W = b.shape
    csum = np.concatenate([np.zeros((H, 1), np.int64), np.cumsum(b, axis=1, dtype=np.int64)], axis=1)
    x = np.arange(W)
    out = np.zeros_like(b)
    for dy in range(-r, r + 1):
        k = int(np.floor(np.sqrt(float(r * r - dy * dy))))
        while (k + 1) * (k + 1) + dy * dy <= r * r:
            k += 1
        while k * k + dy * dy > r * r:
            k -= 1
        lo, hi = np.clip(x - k, 0, W), np.clip(x + k + 1, 0, W)
        run = (csum[:, hi] - csum[:, lo]) > 0          # row y: is any b[y, x-k .. x+k] set
        ys = np.arange(max(0, -dy), min(H, H - dy))    # output rows whose source row y + dy lies in the frame
        if len(ys):
            out[ys] |= run[ys + dy]
    return out


def boundary_counts_numpy(pred, target, r):
    """what ops.boundary_counts computes, in plain numpy: pred, target (n, H, W) or (H, W), nonzero = foreground -> int32 (n, 8) rows
    {I, U, n_fg, n_gt, m_fg, m_gt, 0, 0}"""
    P, G = np.asarray(pred) != 0, np.asarray(target) != 0
    if P.shape != G.shape or P.ndim not in (2, 3) or P.size == 0:
        raise ValueError(f"boundary_counts_numpy: pred and target must both be (n, H, W) or (H, W), got {P.shape} and {G.shape}")
    r = int(r)
    if r < 1:
        raise ValueError(f"boundary_counts_numpy: the radius must be >= 1, got {r}")
    P, G = P.reshape((-1,) + P.shape[-2:]), G.reshape((-1,) + G.shape[-2:])
    out = np.zeros((P.shape[0], 8), dtype=np.int32)
    for j, (p, g) in enumerate(zip(P, G)):
        bp, bg = _seg2bmap(p), _seg2bmap(g)
        out[j, :6] = ((p & g).sum(), (p | g).sum(), bp.sum(), bg.sum(), (bp & _disk_dilate(bg, r)).sum(), (bg & _disk_dilate(bp, r)).sum())
    return out


def _jf_of_row(I, U, n_fg, n_gt, m_fg, m_gt):
    """(J, F) of one frame from its six integers, every step one fp64 rounding"""
    J = 1.0 if U == 0 else float(I) / float(U)
    if n_fg == 0 and n_gt > 0:
        p, r = 1.0, 0.0
    elif n_fg > 0 and n_gt == 0:
        p, r = 0.0, 1.0
    elif n_fg == 0 and n_gt == 0:
        p, r = 1.0, 1.0
    else:
        p, r = float(m_fg) / float(n_fg), float(m_gt) / float(n_gt)
    F = 0.0 if p + r == 0.0 else ((2.0 * p) * r) / (p + r)
    return J, F


def _count_rows(counts):
    if hasattr(counts, "detach"):
        counts = counts.detach().cpu().numpy()
    counts = np.asarray(counts, dtype=np.int64)
    if counts.ndim == 1:
        counts = counts.reshape(1, -1)
    if counts.ndim != 2 or counts.shape[1] < 6:
        raise ValueError(f"J&F count rows are (n, 6) or (n, 8) integers {{I, U, n_fg, n_gt, m_fg, m_gt}}, got {counts.shape}")
    return counts[:, :6]


def jf_from_counts(counts):
    """counts (n, 6 or 8) -> (J, F): two float64 vectors, one value per frame"""
    rows = _count_rows(counts).tolist()
    jf = [_jf_of_row(*row) for row in rows]
    return np.array([v[0] for v in jf], dtype=np.float64), np.array([v[1] for v in jf], dtype=np.float64)


def _jf_summary(n_seq, j_sum, f_sum, frames):
    J, F = float(j_sum) / n_seq * 100.0, float(f_sum) / n_seq * 100.0
    return {"J": J, "F": F, "J&F": (J + F) / 2.0, "sequences": int(n_seq), "frames": int(frames)}


class JFMeter:
    """J&F on the host with arbitrary grouping: update(counts, sequence_ids) adds frame j to the sequence sequence_ids[j] (any hashable; a scalar
    names one sequence for all rows), in the order given -- a video split over several steps keeps its id.  A device tensor is read with one copy."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.sequences = {}          # id -> [sum of J, sum of F, frames], the sums in frame order

    def update(self, counts, sequence_ids):
        rows = _count_rows(counts).tolist()
        if isinstance(sequence_ids, (str, bytes, int)) or not hasattr(sequence_ids, "__len__"):
            sequence_ids = [sequence_ids] * len(rows)
        if hasattr(sequence_ids, "tolist"):
            sequence_ids = sequence_ids.tolist()
        if len(sequence_ids) != len(rows):
            raise ValueError(f"JFMeter.update: {len(rows)} count rows, {len(sequence_ids)} sequence ids")
        for row, sid in zip(rows, sequence_ids):
            J, F = _jf_of_row(*row)
            acc = self.sequences.setdefault(sid, [0.0, 0.0, 0])
            acc[0] += J
            acc[1] += F
            acc[2] += 1

    def per_sequence(self):
        """-> {id: (J_seq, F_seq, frames)}"""
        return {sid: (a[0] / a[2], a[1] / a[2], a[2]) for sid, a in self.sequences.items()}

    def summary(self):
        """-> {"J", "F", "J&F", "sequences", "frames"}: the first three in percent, the means of the sequence means"""
        if not self.sequences:
            raise RuntimeError("JFMeter.summary: no sequences")
        j_sum = f_sum = 0.0
        frames = 0
        for a in self.sequences.values():
            j_sum += a[0] / a[2]
            f_sum += a[1] / a[2]
            frames += a[2]
        return _jf_summary(len(self.sequences), j_sum, f_sum, frames)

    def __str__(self):
        s = self.summary()
        return "J&F: %.2f  J: %.2f  F: %.2f  (%d sequences, %d frames)" % (s["J&F"], s["J"], s["F"], s["sequences"], s["frames"])


def jf_meter_bytes(capacity: int) -> int:
    """the documented size of a J&F meter block (lavt_jf_meter_bytes)"""
    return 8 * JF_HEADER_DOUBLES + int(capacity) * JF_RECORD_BYTES if capacity > 0 else 0


class JFSnapshot:
    """One copy of the J&F meter block, decoded: `header` (float64[16]) and `ring` (JF_RECORD_DTYPE[capacity], slot = sequence % capacity)."""

    def __init__(self, raw, capacity):
        raw = np.array(raw, dtype=np.uint8, copy=True)
        self.header = raw[:8 * JF_HEADER_DOUBLES].view(np.float64)
        self.ring = raw[8 * JF_HEADER_DOUBLES:].view(JF_RECORD_DTYPE)
        self.capacity = int(capacity)

    @property
    def n(self) -> int:
        """sequences appended since the block was made: the running sequence number of the next record"""
        return int(self.header[JF_N])

    @property
    def sequences(self) -> int:
        """sequences since the last reset()"""
        return int(self.header[JF_SEQS])

    @property
    def frames(self) -> int:
        return int(self.header[JF_FRAMES])

    def records(self, count=None):
        """the last `count` records since the last reset() that the ring still holds, oldest first (default: all of them)"""
        have = min(self.sequences, self.capacity)
        count = have if count is None else min(int(count), have)
        return self.ring[np.arange(self.n - count, self.n, dtype=np.int64) % self.capacity]

    def frame_means(self):
        """-> (mean J, mean F) over FRAMES in percent: not the DAVIS value (that is summary()), the same quantity pooled without sequences"""
        if self.frames == 0:
            raise RuntimeError("DeviceJFMeter: no frames")
        return float(self.header[JF_JFRAME_SUM] / self.frames * 100.0), float(self.header[JF_FFRAME_SUM] / self.frames * 100.0)

    def summary(self):
        """-> {"J", "F", "J&F", "sequences", "frames"}, the first three in percent, as JFMeter.summary()"""
        if self.sequences == 0:
            raise RuntimeError("DeviceJFMeter: no sequences")
        return _jf_summary(self.sequences, self.header[JF_JSEQ_SUM], self.header[JF_FSEQ_SUM], self.frames)

    __str__ = JFMeter.__str__          # (the text is built from summary() alone)

    def state_dict(self):
        """header and ring as CPU tensors and plain values (torch.load(weights_only=True) reads it back); the hold word is saved as 0"""
        import torch
        header = torch.from_numpy(self.header.copy())
        header[JF_HOLD] = 0.0
        return {"format": 1, "capacity": self.capacity, "header": header, "ring": torch.from_numpy(self.ring.copy().view(np.uint8))}


def reference_jf_block(counts, frames_per_seq, capacity, live=None, block=None, hold=False):
    """The block lavt_jf_meter_append leaves after ONE append of the count rows (n a multiple of frames_per_seq; live[j] false: frame j is not read)
    to a fresh block -- or to `block`, a JFSnapshot of an earlier state, which is not modified -- computed on the host with the same arithmetic in
    the same order -> JFSnapshot.  hold: the block's hold word is set for this append (nothing is stored)."""
    rows = _count_rows(counts).tolist()
    T = int(frames_per_seq)
    if T < 1 or len(rows) % T:
        raise ValueError(f"reference_jf_block: {len(rows)} frames are not whole sequences of {T}")
    if block is None:
        raw = np.zeros(jf_meter_bytes(capacity), dtype=np.uint8)
        raw[:8].view(np.float64)[0] = capacity
    else:
        raw = np.concatenate([block.header.view(np.uint8), block.ring.view(np.uint8)])
    h, ring = raw[:8 * JF_HEADER_DOUBLES].view(np.float64), raw[8 * JF_HEADER_DOUBLES:].view(JF_RECORD_DTYPE)
    if hold or h[JF_HOLD] != 0.0:
        return JFSnapshot(raw, capacity)
    js = fs = 0.0
    cnt = 0
    for j, row in enumerate(rows):
        if live is None or live[j]:
            J, F = _jf_of_row(*row)
            js += J
            fs += F
            cnt += 1
            h[JF_FRAMES] += 1.0
            h[JF_JFRAME_SUM] += J
            h[JF_FFRAME_SUM] += F
        if (j + 1) % T == 0:
            if cnt:
                seq = int(h[JF_N])
                Js, Fs = js / cnt, fs / cnt
                ring[seq % capacity] = (cnt, 0, Js, Fs, seq)
                h[JF_N] += 1.0
                h[JF_SEQS] += 1.0
                h[JF_JSEQ_SUM] += Js
                h[JF_FSEQ_SUM] += Fs
            js = fs = 0.0
            cnt = 0
    return JFSnapshot(raw, capacity)


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


class DeviceJFMeter(DeviceBlock):
    """The J&F sequence means in a block on the device (include/lavt_hip.h "J&F measure").  capacity: per-sequence records the ring holds (the
    accumulators cover every sequence whatever the capacity).  device: where the block lives (default: the current CUDA device).  Attach with
    Predictor(..., jf_meter=), attach_jf_meter() or make_jf_meter(), before warmup_and_capture().  poll() (never waits), read() (synchronises),
    pause() and resume() are DeviceBlock's."""
    header_doubles = JF_HEADER_DOUBLES

    def __init__(self, capacity=4096, device=None):
        capacity = int(capacity)
        if capacity < 1:
            raise ValueError(f"DeviceJFMeter: capacity must be >= 1, got {capacity}")
        self.capacity = capacity
        self.nbytes = int(K.lib.lavt_jf_meter_bytes(capacity))
        if self.nbytes != jf_meter_bytes(capacity):
            raise RuntimeError("DeviceJFMeter: the library's block size is not the documented formula")
        self._host_init(device)

    def _decode(self, raw):
        return JFSnapshot(raw, self.capacity)

    # ---- the launch (Predictor._body ends with it)
    def append(self, counts, frames_per_seq, live=None):
        """enqueue lavt_jf_meter_append on the current stream; capturable.  counts: device int32 [n, 8], the rows of ops.boundary_counts, n a
        multiple of frames_per_seq (sequence k = frames k*T .. k*T + T - 1); live: device int32 [n], 0 = the frame is not read, None = all live"""
        import torch
        T = int(frames_per_seq)
        if counts.dtype != torch.int32 or counts.dim() != 2 or counts.shape[1] != 8 or not counts.is_contiguous():
            raise ValueError(f"DeviceJFMeter.append: counts must be a contiguous int32 [n, 8], got {counts.dtype} {tuple(counts.shape)}")
        if T < 1 or counts.shape[0] % T:
            raise ValueError(f"DeviceJFMeter.append: {counts.shape[0]} frames are not whole sequences of {T}")
        if live is not None and (live.dtype != torch.int32 or live.numel() != counts.shape[0] or not live.is_contiguous()):
            raise ValueError(f"DeviceJFMeter.append: live must be a contiguous int32 vector of {counts.shape[0]} entries")
        K.check(K.lib.lavt_jf_meter_append(K.ptr(counts), K.ptr(live), int(counts.shape[0]), T, K.ptr(self.block), self.capacity, K.stream()))

    def reset(self):
        """zero the accumulators (sequences, frames and the four sums); the running sequence number keeps counting"""
        self._host_write("DeviceJFMeter.reset", lambda: self.header[JF_ACCUMULATORS].zero_())
        self._latest, self._inflight = None, None

    # ---- checkpoint
    def state_dict(self):
        """header and ring as CPU tensors and plain values (torch.load(weights_only=True) reads it back); the hold word is saved as 0; synchronises"""
        import torch
        self._not_capturing("DeviceJFMeter.state_dict")
        torch.cuda.synchronize(self.block.device)
        return JFSnapshot(self.block.detach().cpu().view(torch.uint8).numpy(), self.capacity).state_dict()

    def load_state_dict(self, state):
        """write a state_dict() into the block this object has (a captured graph keeps its address); the hold word keeps its current value"""
        import torch
        if state.get("format") != 1 or int(state["capacity"]) != self.capacity:
            raise ValueError(f"DeviceJFMeter.load_state_dict: the state was saved with capacity={state.get('capacity')}, format={state.get('format')}; "
                             f"this meter has capacity={self.capacity}, format=1")
        header, ring = state["header"], state["ring"]
        if tuple(header.shape) != (JF_HEADER_DOUBLES,) or header.dtype != torch.float64 or ring.dtype != torch.uint8 or ring.numel() != self.capacity * JF_RECORD_BYTES:
            raise ValueError("DeviceJFMeter.load_state_dict: header / ring do not have the block's layout")

        def write():
            hold = self.header[JF_HOLD:JF_HOLD + 1].clone()
            self.block.copy_(torch.cat([header, ring.view(torch.float64)]))
            self.header[JF_HOLD:JF_HOLD + 1].copy_(hold)
        self._host_write("DeviceJFMeter.load_state_dict", write)
        self._latest, self._inflight = None, None


def jf_snapshot_from_state(state):
    """a state_dict() of a DeviceJFMeter (or of a JFSnapshot) -> JFSnapshot, on the host"""
    raw = np.concatenate([state["header"].numpy().view(np.uint8), state["ring"].numpy()])
    return JFSnapshot(raw, int(state["capacity"]))
