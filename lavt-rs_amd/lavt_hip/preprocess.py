"""Device-side frame preprocessing: the reference's `Resize -> ToTensor -> Normalize` (transforms.py:20-31, 83-87, 106-113; the per-frame loop of
test_ytvos.py:236-243) on uint8 frames that are already on the GPU, with the results PIL gives.

PIL's antialiased bilinear resize of 8-bit images is integer arithmetic on fixed-point coefficient tables, one table per axis.  The tables are
built here on the host (float64, the recipe below), cached per (in, out) size pair, uploaded once per device, and applied by
`lavt_resize_norm_u8` (csrc/preprocess.hip): every pixel of the integer stage equals `PIL.Image.resize(..., BILINEAR)`, the fp32 finish is the
reference's own three operations.  Targets go through `lavt_resize_nearest_u8` with PIL's NEAREST index tables.

The passes run width first, then height, as the recipe says.  That is what PIL returns for every frame-shaped source; for a source more than 100
times taller than wide that is downscaled along its height, Pillow 12.2 was seen to return the height-first result instead (off by one on some
pixels).  Such strips are outside what this module reproduces.

This module is host logic: it imports without the shared library and without a GPU.  Everything that touches pixels runs in HIP; there is no CPU
fallback (transforms.get_transform is the CPU pipeline, unchanged)."""
import math

import numpy as np
import torch

PRECISION_BITS = 22          # PIL: 32 - 8 - 2: 8 bits of pixel, 2 of headroom
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)          # train.py:37-47
_NO_CPU = "liblavt_hip operates on GPU memory only ({}); there is no CPU fallback"

_host_resample, _host_nearest = {}, {}
_dev_resample, _dev_nearest = {}, {}


def _build_resample(in_size, out_size):
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = fs                                             # bilinear: filter support 1.0, stretched when downscaling
    ksize = int(math.ceil(support)) * 2 + 1
    c = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((c - support + 0.5).astype(np.int64), 0)          # int(): truncation toward zero, as the cast
    n = np.minimum((c + support + 0.5).astype(np.int64), in_size) - xmin
    w = np.zeros((out_size, ksize), dtype=np.float64)
    ww = np.zeros(out_size, dtype=np.float64)
    for x in range(ksize):                                   # the weight sum runs over the taps in order, as a scalar loop would
        wx = np.maximum(0.0, 1.0 - np.abs((x + xmin - c + 0.5) / fs))
        wx[x >= n] = 0.0
        w[:, x] = wx
        ww += wx
    nz = ww != 0.0
    w[nz] /= ww[nz, None]
    coef = (0.5 + w * (1 << PRECISION_BITS)).astype(np.int64).astype(np.int32)          # weights of this filter are never negative
    bounds = np.stack([xmin, n], 1).astype(np.int32)
    return np.ascontiguousarray(coef), np.ascontiguousarray(bounds)


def resample_tables(in_size, out_size):
    """One axis of PIL's bilinear (antialiased) resample of 8-bit data: -> (coef int32 [out][ksize], bounds int32 [out][2] = (xmin, n)).
    out[xx] = clip((2**21 + sum_{x < n} coef[xx][x] * pix[xmin + x]) >> 22, 0, 255); slots x >= n are zero.  Cached per (in, out); treat as read-only."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError(f"resample_tables: sizes must be positive, got {in_size} -> {out_size}")
    key = (in_size, out_size)
    if key not in _host_resample:
        _host_resample[key] = _build_resample(in_size, out_size)
    return _host_resample[key]


def nearest_table(in_size, out_size):
    """PIL's NEAREST source index per output index: int32 [out].  The coordinate is a RUNNING double sum (xo += in/out), not a product: the two
    differ in the last bit often enough to move tens of thousands of pixels of a 720x1280 -> 480^2 mask."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError(f"nearest_table: sizes must be positive, got {in_size} -> {out_size}")
    key = (in_size, out_size)
    if key not in _host_nearest:
        a = in_size / out_size
        xo = a * 0.5
        idx = np.empty(out_size, dtype=np.int32)
        for i in range(out_size):
            idx[i] = min(max(int(xo), 0), in_size - 1)
            xo += a
        _host_nearest[key] = idx
    return _host_nearest[key]


def apply_tables_numpy(img, out_h, out_w):
    """The integer stage on the host, for tests and fixture generation only: uint8 (H, W[, C]) -> uint8 (out_h, out_w[, C]) by the tables: width
    first, rounded to uint8, then height."""
    a = np.asarray(img)
    squeeze = a.ndim == 2
    if squeeze:
        a = a[:, :, None]

    def axis1(src, coef, bounds):
        out = np.empty((src.shape[0], coef.shape[0], src.shape[2]), dtype=np.uint8)
        s = src.astype(np.int64)
        for xx in range(coef.shape[0]):
            x0, n = int(bounds[xx, 0]), int(bounds[xx, 1])
            acc = (1 << (PRECISION_BITS - 1)) + np.einsum("hkc,k->hc", s[:, x0:x0 + n], coef[xx, :n].astype(np.int64))
            out[:, xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
        return out

    h = axis1(a, *resample_tables(a.shape[1], out_w))
    v = axis1(h.transpose(1, 0, 2), *resample_tables(a.shape[0], out_h)).transpose(1, 0, 2)
    return np.ascontiguousarray(v[:, :, 0] if squeeze else v)


def _upload(cache, key, arrays, device):
    k = key + (str(device),)
    if k not in cache:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"lavt_hip.preprocess: the tables for sizes {key} are not on {device} yet and cannot be uploaded inside a graph capture: "
                               "run the preprocessing once eagerly first")
        cache[k] = tuple(torch.from_numpy(a).to(device) for a in arrays)
    return cache[k]


def device_resample_tables(in_size, out_size, device):
    """-> (coef, bounds) as int32 tensors on `device`: uploaded on the first request for this size pair, cached afterwards"""
    return _upload(_dev_resample, (int(in_size), int(out_size)), resample_tables(in_size, out_size), device)


def device_nearest_table(in_size, out_size, device):
    return _upload(_dev_nearest, (int(in_size), int(out_size)), (nearest_table(in_size, out_size),), device)[0]


class FramePreprocessor:
    """`images(frames_u8)`: uint8 (N, Hs, Ws, 3) RGB frames -> fp32 (N, 3, Ho, Wo), PIL's bilinear resize then (v / 255 - mean) / std.
    `targets(masks_u8)`: uint8 (N, Hs, Ws) masks -> int64 (N, Ho, Wo), PIL's nearest resize.

    Both take a CUDA uint8 tensor (a slice of a larger upload is fine: only the frame stride may be irregular), or host data -- a numpy array, or a
    list of same-sized PIL images / arrays -- which is stacked and uploaded in one copy; through pinned memory when `reserve_staging` was called
    for that many bytes.  A single frame (Hs, Ws, 3) / mask (Hs, Ws) is taken as N = 1.  `out` receives the result when given (its leading
    dimensions may be split differently, e.g. (B, T, 3, H, W)); everything runs on the current stream, nothing synchronises the host."""

    def __init__(self, out_size, mean=MEAN, std=STD, device=None):
        self.out_size = (int(out_size), int(out_size)) if isinstance(out_size, int) else (int(out_size[0]), int(out_size[1]))
        if min(self.out_size) < 1:
            raise ValueError(f"FramePreprocessor: out_size must be positive, got {self.out_size}")
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        if len(self.mean) != 3 or len(self.std) != 3 or any(s == 0.0 for s in self.std):
            raise ValueError("FramePreprocessor: mean and std are three values each, std nonzero")
        self.device = device
        self._staging = {}          # nbytes -> (pinned uint8 buffer, event of the last copy out of it)

    def _device(self):
        if not torch.cuda.is_available():
            raise RuntimeError(_NO_CPU.format("no GPU is available"))
        return torch.device(self.device if self.device is not None else f"cuda:{torch.cuda.current_device()}")

    def reserve_staging(self, shape):
        """allocate a pinned host buffer for uint8 host input of this shape: uploads of that many bytes then go through it, asynchronously"""
        nbytes = int(np.prod(shape))
        self._device()
        if nbytes not in self._staging:
            self._staging[nbytes] = (torch.empty(nbytes, dtype=torch.uint8).pin_memory(), None)

    def _to_device(self, frames, ndim):
        """-> CUDA uint8 tensor with `ndim` dimensions (N first)"""
        if isinstance(frames, torch.Tensor):
            if not frames.is_cuda:
                raise RuntimeError(_NO_CPU.format("got a CPU tensor; pass a CUDA uint8 tensor, a numpy array or PIL images"))
            t = frames
        else:
            dev = self._device()
            a = np.stack([np.asarray(f) for f in frames]) if isinstance(frames, (list, tuple)) else np.asarray(frames)
            if a.dtype != np.uint8:
                raise TypeError(f"FramePreprocessor: frames must be uint8, got {a.dtype}")
            a = np.ascontiguousarray(a)
            slot = self._staging.get(a.nbytes)
            if slot is not None:
                buf, ev = slot
                if ev is not None:
                    ev.synchronize()          # the previous upload out of this buffer (long finished in a steady loop)
                buf.numpy()[:] = a.reshape(-1)
                t = buf.to(dev, non_blocking=True).view(a.shape)
                ev = torch.cuda.Event()
                ev.record()
                self._staging[a.nbytes] = (buf, ev)
            else:
                t = torch.from_numpy(a).to(dev)
        if t.dtype != torch.uint8:
            raise TypeError(f"FramePreprocessor: frames must be uint8, got {t.dtype}")
        if t.dim() == ndim - 1:
            t = t.unsqueeze(0)
        if t.dim() != ndim:
            raise ValueError(f"FramePreprocessor: expected {ndim - 1} or {ndim} dimensions, got shape {tuple(t.shape)}")
        return t

    def images(self, frames_u8, out=None):
        from . import ops
        src = self._to_device(frames_u8, 4)
        if src.shape[-1] != 3:
            raise ValueError(f"FramePreprocessor.images: frames are (N, H, W, 3) RGB, got shape {tuple(src.shape)}")
        N = src.shape[0]
        Ho, Wo = self.out_size
        if out is None:
            out = torch.empty(N, 3, Ho, Wo, dtype=torch.float32, device=src.device)
        ops.resize_normalize_u8(src, _as_frames(out, (N, 3, Ho, Wo), torch.float32, "images"), self.mean, self.std)
        return out

    def targets(self, masks_u8, out=None):
        from . import ops
        src = self._to_device(masks_u8, 3)
        N = src.shape[0]
        Ho, Wo = self.out_size
        if out is None:
            out = torch.empty(N, Ho, Wo, dtype=torch.int64, device=src.device)
        ops.resize_nearest_u8(src, _as_frames(out, (N, Ho, Wo), torch.int64, "targets"))
        return out


def _as_frames(out, shape, dtype, what):
    """`out` viewed with the frames in one leading dimension; refuses anything that is not that many contiguous elements of `dtype` on the GPU"""
    if not out.is_cuda:
        raise RuntimeError(_NO_CPU.format("got a CPU tensor for `out`"))
    n = 1
    for s in shape:
        n *= s
    if out.dtype != dtype or not out.is_contiguous() or out.numel() != n or tuple(out.shape[-2:]) != tuple(shape[-2:]):
        raise ValueError(f"FramePreprocessor.{what}: `out` must be a contiguous {dtype} tensor holding {tuple(shape)}, got {out.dtype} {tuple(out.shape)}")
    return out.view(shape)
