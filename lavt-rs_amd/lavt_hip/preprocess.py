"""Device-side frame preprocessing: the reference's `Resize -> ToTensor -> Normalize` (transforms.py:20-31, 83-87, 106-113; the per-frame loop of
test_ytvos.py:236-243) on uint8 frames that are already on the GPU, with the results PIL gives.

PIL's antialiased bilinear resize of 8-bit images is integer arithmetic on fixed-point coefficient tables, one table per axis.  The tables are
built here on the host (float64, the recipe below), cached per (in, out) size pair, uploaded once per device, and applied by
`lavt_resize_norm_u8` (csrc/preprocess.hip): every pixel of the integer stage equals `PIL.Image.resize(..., BILINEAR)`, the fp32 finish is the
reference's own three operations.  Targets go through `lavt_resize_nearest_u8` with PIL's NEAREST index tables.

The passes run width first, then height, as the recipe says.  That is what PIL returns for every frame-shaped source; for a source more than 100
times taller than wide that is downscaled along its height, Pillow 12.2 was seen to return the height-first result instead (off by one on some
pixels).  Such strips are outside what this module reproduces.

Sources of mixed sizes -- a training batch of RefCOCO / COCO images -- go through the batched stage at the end of this module: `pack_batch` lays images,
masks, the tables they need and one descriptor per output frame out as ONE blob, `BatchPreprocessor` uploads it in one copy and runs one launch per
kind (`lavt_resize_norm_u8_batch`, `lavt_resize_nearest_u8_batch`); `apply_packed_numpy` reads a blob as the kernels do, for tests.

Clips made of still images (`--pseudo_video_aug weak-rotate-translate-shear-crop`): `PseudoVideoAugment` draws one affine motion per frame, `pack_batch(warps=,
target_warps=)` adds a warp descriptor per warped frame, and `lavt_affine_u8_batch` / `lavt_affine_nearest_u8_batch` warp the uploaded sources on the device, with
the pixels of `PIL.Image.transform(AFFINE)`, in front of the resize (`affine_bilinear_numpy` / `affine_nearest_numpy` restate Pillow's arithmetic).

This module is host logic: it imports without the shared library and without a GPU.  Everything that touches pixels runs in HIP; there is no CPU
fallback (transforms.get_transform is the CPU pipeline, unchanged)."""
import math
from typing import NamedTuple

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


# ================================================================================================ batched input stage: sources of mixed sizes
# One training batch (RefCOCO / COCO: every image has its own size) is packed on the host into ONE blob -- descriptors, int32 tables, pixels, masks --
# uploaded in one copy and resized by one launch per kind (lavt_resize_norm_u8_batch, lavt_resize_nearest_u8_batch; DESIGN.md "Batched input stage").
ITEM_DTYPE = np.dtype([("src_off", "<i8"), ("mask_off", "<i8"), ("Hs", "<i4"), ("Ws", "<i4"), ("coef_x", "<i4"), ("bounds_x", "<i4"), ("ksize_x", "<i4"),
                       ("coef_y", "<i4"), ("bounds_y", "<i4"), ("ksize_y", "<i4"), ("idx_y", "<i4"), ("idx_x", "<i4"), ("reserved0", "<i4"), ("reserved1", "<i4")])
assert ITEM_DTYPE.itemsize == 64          # lavt_pp_item_t (include/lavt_hip.h)
SECTION_ALIGN = 16


class BatchLayout(NamedTuple):
    """Where the sections of a packed batch lie.  Offsets are bytes from the start of the blob, every section starts 16-byte aligned; the offsets
    INSIDE descriptors are relative to their section (bytes into pixels / masks, int32 elements into tables)."""
    nbytes: int             # the blob: descriptors | tables | pixels | masks
    out_size: tuple         # (Ho, Wo)
    n_frames: int           # image descriptors = output frames
    n_targets: int          # target descriptors = output masks (0: packed without targets)
    items_off: int          # image descriptors, ITEM_DTYPE [n_frames]
    titems_off: int         # target descriptors, ITEM_DTYPE [n_targets]
    tables_off: int
    table_elems: int
    pixels_off: int         # the images, HWC, back to back (odd offsets are normal)
    pixel_bytes: int
    masks_off: int
    mask_bytes: int
    tables: tuple           # (("resample" | "nearest", in, out), element offset) of every stored table: one per distinct size pair


def _align(n):
    return -(-n // SECTION_ALIGN) * SECTION_ALIGN


# ---- pseudo-video augmentation: Pillow's affine transform, restated (DESIGN.md "Pseudo-video augmentation") ----
WARP_DTYPE = np.dtype([("src_off", "<i8"), ("dst_off", "<i8"), ("Hs", "<i4"), ("Ws", "<i4"), ("mode", "<i4"), ("idx_x", "<i4"), ("idx_y", "<i4"), ("reserved0", "<i4"),
                       ("a", "<f8", (6,)), ("A", "<i4", (6,)), ("reserved1", "<i4", (4,))])
assert WARP_DTYPE.itemsize == 128          # lavt_pp_warp_t (include/lavt_hip.h)
WARP_FIXED, WARP_TABLES = 0, 1             # LAVT_WARP_FIXED, LAVT_WARP_TABLES
SIDE_MAX = 8192                            # the largest side the warp entries take


class WarpLayout(NamedTuple):
    """Where the warp sections of a batch packed with `warps=` / `target_warps=` lie.  The warp descriptors follow the masks inside the blob (byte
    offsets from its start, 16-byte aligned, counted in BatchLayout.nbytes); the warped uint8 frames are written on the DEVICE into scratch that
    follows the blob in the same buffer: images first, then masks, every frame 16-byte aligned.  A warp descriptor's src_off is relative to the pixel
    (mask) section, its dst_off to the scratch; the resize descriptor of a warped frame names `scratch_off - pixels_off + dst_off` (masks:
    `- masks_off`), so its launch is given everything from its section's start to device_bytes to read."""
    image_warps_off: int          # WARP_DTYPE [n_image_warps]
    n_image_warps: int
    mask_warps_off: int           # WARP_DTYPE [n_mask_warps]
    n_mask_warps: int
    scratch_off: int              # = BatchLayout.nbytes: the first byte behind the uploaded blob
    scratch_bytes: int
    image_scratch_bytes: int      # bytes of warped images (the frames alone, without alignment gaps)
    mask_scratch_bytes: int
    device_bytes: int             # scratch_off + scratch_bytes: what the device buffer must hold


def _coefficients(c, what):
    c = tuple(float(v) for v in c)
    if len(c) != 6:
        raise ValueError(f"{what}: a warp is None or six coefficients, got {len(c)}")
    if not all(math.isfinite(v) for v in c):
        raise ValueError(f"{what}: coefficients must be finite, got {c}")
    return c


def affine_bilinear_numpy(img, coeffs):
    """`Image.fromarray(img).transform((Ws, Hs), Image.AFFINE, coeffs, resample=Image.BILINEAR)` (fill 0) of a uint8 (Hs, Ws[, C]) image, restated:
    Pillow's affine_transform + bilinear filter in float64, every product and sum rounded on its own, the result truncated.  What
    lavt_affine_u8_batch computes; for tests and for apply_packed_numpy."""
    a0, a1, a2, a3, a4, a5 = _coefficients(coeffs, "affine_bilinear_numpy")
    a = np.asarray(img)
    squeeze = a.ndim == 2
    if squeeze:
        a = a[:, :, None]
    Hs, Ws = a.shape[:2]
    x, y = np.arange(Ws, dtype=np.float64) + 0.5, (np.arange(Hs, dtype=np.float64) + 0.5)[:, None]
    xin, yin = a0 * x + a1 * y + a2, a3 * x + a4 * y + a5
    inside = ~((xin < 0.0) | (xin >= Ws) | (yin < 0.0) | (yin >= Hs))
    xin, yin = np.where(inside, xin, 0.5) - 0.5, np.where(inside, yin, 0.5) - 0.5
    fx, fy = np.floor(xin), np.floor(yin)
    dx, dy = (xin - fx)[:, :, None], (yin - fy)[:, :, None]
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    xa, xb, ya = np.clip(x0, 0, Ws - 1), np.clip(x0 + 1, 0, Ws - 1), np.clip(y0, 0, Hs - 1)          # columns and the first row clamp
    below = (y0 + 1 >= 0) & (y0 + 1 < Hs)                                                            # the second row does not: past the last row v2 = v1
    yb = np.where(below, y0 + 1, 0)
    p = a.astype(np.float64)
    v1 = p[ya, xa] + (p[ya, xb] - p[ya, xa]) * dx
    v2 = np.where(below[:, :, None], p[yb, xa] + (p[yb, xb] - p[yb, xa]) * dx, v1)
    v = v1 + (v2 - v1) * dy
    out = np.where(inside[:, :, None], v.astype(np.int64), 0).astype(np.uint8)
    return np.ascontiguousarray(out[:, :, 0] if squeeze else out)


def _fix(v):
    return math.floor(v * 65536.0 + 0.5)


def warp_fixed_coefficients(coeffs, Hs, Ws):
    """Pillow's 16.16 fixed-point form (A0..A5) of six affine coefficients, for a NEAREST transform that is not axis-aligned; ValueError where the
    coordinates at a corner of the Hs x Ws frame leave int32 (Pillow's own `int` would overflow)"""
    a0, a1, a2, a3, a4, a5 = _coefficients(coeffs, "warp_fixed_coefficients")
    A = (_fix(a0), _fix(a1), _fix(a2 + a0 * 0.5 + a1 * 0.5), _fix(a3), _fix(a4), _fix(a5 + a3 * 0.5 + a4 * 0.5))
    lo, hi = -2 ** 31, 2 ** 31 - 1
    corners = [c + cy * yy + cx * xx for c, cy, cx in ((A[2], A[1], A[0]), (A[5], A[4], A[3])) for xx in (0, Ws) for yy in (0, Hs)]
    if not all(lo <= v <= hi for v in A + tuple(corners)):
        raise ValueError(f"warp coefficients {coeffs} on a {Hs} x {Ws} mask: the 16.16 fixed-point coordinates overflow int32")
    return A


def warp_axis_table(offset, step, n):
    """Pillow's index table of one axis of an axis-aligned NEAREST transform of an n-pixel side (ImagingScaleAffine): the coordinate is a running
    double sum, as in nearest_table -> int32 [n], -1 = outside"""
    o = offset + step * 0.5
    idx = np.full(n, -1, dtype=np.int32)
    for i in range(n):
        if 0.0 <= o < n:
            idx[i] = int(o)
        o += step
    return idx


def affine_nearest_numpy(mask, coeffs):
    """`Image.fromarray(mask).transform((Ws, Hs), Image.AFFINE, coeffs, resample=Image.NEAREST)` (fill 0) of a uint8 (Hs, Ws) mask, restated: the
    index tables when a1 == 0 and a3 == 0, 16.16 fixed point otherwise.  What lavt_affine_nearest_u8_batch computes."""
    c = _coefficients(coeffs, "affine_nearest_numpy")
    m = np.asarray(mask)
    Hs, Ws = m.shape
    if c[1] == 0.0 and c[3] == 0.0:
        xi, yi = warp_axis_table(c[2], c[0], Ws).astype(np.int64)[None, :], warp_axis_table(c[5], c[4], Hs).astype(np.int64)[:, None]
    else:
        A = warp_fixed_coefficients(c, Hs, Ws)
        x, y = np.arange(Ws, dtype=np.int64)[None, :], np.arange(Hs, dtype=np.int64)[:, None]
        xi, yi = (A[2] + A[1] * y + A[0] * x) >> 16, (A[5] + A[4] * y + A[3] * x) >> 16
    inside = (xi >= 0) & (xi < Ws) & (yi >= 0) & (yi < Hs)
    return np.where(inside, m[np.clip(yi, 0, Hs - 1), np.clip(xi, 0, Ws - 1)], 0).astype(np.uint8)


def _warp_list(warps, n, what):
    """one entry per output frame: None (the frame is not warped) or six finite floats"""
    if warps is None:
        return [None] * n
    warps = list(warps)
    if len(warps) != n:
        raise ValueError(f"pack_batch: {what} has {len(warps)} entries for {n} output {'frames' if what == 'warps' else 'masks'} (one each, None = not warped)")
    return [None if w is None else _coefficients(w, f"pack_batch: {what}[{i}]") for i, w in enumerate(warps)]


def _host_u8(x, channels, what):
    """one host image (H, W, 3) / mask (H, W) as a uint8 array; device data is refused with the route that takes it"""
    if isinstance(x, torch.Tensor):
        if x.is_cuda:
            raise TypeError(f"{what}: got a CUDA tensor; the batched input stage packs HOST data (PIL images, uint8 arrays) into one upload -- "
                            "FramePreprocessor.images / .targets is the route for data that is already on the device")
        x = x.numpy()
    a = np.asarray(x)
    if a.dtype != np.uint8:
        raise TypeError(f"{what}: must be uint8, got {a.dtype}")
    if (a.ndim != 3 or a.shape[2] != 3) if channels else a.ndim != 2:
        raise ValueError(f"{what}: expected {'(H, W, 3) RGB' if channels else '(H, W)'}, got shape {a.shape}")
    if min(a.shape[:2]) < 1:
        raise ValueError(f"{what}: empty input {a.shape}")
    return a


def _host_list(xs, channels, what):
    if isinstance(xs, torch.Tensor) and xs.is_cuda:
        _host_u8(xs, channels, what)
    if isinstance(xs, np.ndarray) and xs.ndim == (3 if channels else 2):
        xs = [xs]          # a single image / mask
    return [_host_u8(x, channels, f"{what}[{i}]") for i, x in enumerate(xs)]


def _source_map(m, n_src, what):
    m = [int(v) for v in m]
    bad = [v for v in m if not 0 <= v < n_src]
    if bad or not m:
        raise ValueError(f"pack_batch: {what} must name sources 0..{n_src - 1} for at least one output frame, got {m}")
    return m


class _BatchPlan:
    """a batch laid out but not yet written: `layout`, and `write(buf)` that fills the first layout.nbytes bytes of a uint8 array"""

    def __init__(self, images, targets, out_size, frame_map, target_map, repeat, warps=None, target_warps=None):
        Ho, Wo = (int(out_size), int(out_size)) if isinstance(out_size, int) else (int(out_size[0]), int(out_size[1]))
        if min(Ho, Wo) < 1:
            raise ValueError(f"pack_batch: out_size must be positive, got {(Ho, Wo)}")
        self.images = _host_list(images, True, "pack_batch: images")
        self.masks = _host_list(targets, False, "pack_batch: targets") if targets is not None else []
        if not self.images:
            raise ValueError("pack_batch: no images")
        if targets is not None and not self.masks:
            raise ValueError("pack_batch: an empty list of targets (pass None for none)")
        if repeat is not None:
            T = int(repeat)
            if T < 1 or frame_map is not None:
                raise ValueError("pack_batch: repeat must be >= 1 and stands in place of frame_map")
            frame_map = [i for i in range(len(self.images)) for _ in range(T)]
            if target_map is None and self.masks:
                target_map = [i for i in range(len(self.masks)) for _ in range(T)]
        frame_map = _source_map(range(len(self.images)) if frame_map is None else frame_map, len(self.images), "frame_map")
        if self.masks:
            target_map = _source_map(range(len(self.masks)) if target_map is None else target_map, len(self.masks), "target_map")
        elif target_map is not None:
            raise ValueError("pack_batch: target_map without targets")
        else:
            target_map = []
        if max(len(frame_map), len(target_map)) > 65535:
            raise ValueError("pack_batch: at most 65535 output frames per batch")
        if target_warps is not None and not self.masks:
            raise ValueError("pack_batch: target_warps without targets")
        warped = warps is not None or target_warps is not None
        warps, target_warps = _warp_list(warps, len(frame_map), "warps"), _warp_list(target_warps, len(target_map), "target_warps")

        self.tables, where, elems = [], {}, 0          # [(element offset, int32 array)]; one entry per distinct (kind, in, out)

        def table(kind, n_in, n_out):
            nonlocal elems
            key = (kind, n_in, n_out)
            if key not in where:
                arrays = resample_tables(n_in, n_out) if kind == "resample" else (nearest_table(n_in, n_out),)
                offs = []
                for a in arrays:
                    offs.append(elems)
                    self.tables.append((elems, a))
                    elems += a.size
                where[key] = tuple(offs) + ((arrays[0].shape[1],) if kind == "resample" else ())
            return where[key]

        src_off, off = [], 0
        for a in self.images:
            src_off.append(off)
            off += a.size
        pixel_bytes = off
        mask_off, off = [], 0
        for a in self.masks:
            mask_off.append(off)
            off += a.size
        mask_bytes = off

        self.items = np.zeros(len(frame_map), dtype=ITEM_DTYPE)
        for it, s in zip(self.items, frame_map):
            Hs, Ws = self.images[s].shape[:2]
            it["src_off"], it["Hs"], it["Ws"] = src_off[s], Hs, Ws
            it["coef_x"], it["bounds_x"], it["ksize_x"] = table("resample", Ws, Wo)
            it["coef_y"], it["bounds_y"], it["ksize_y"] = table("resample", Hs, Ho)
        self.titems = np.zeros(len(target_map), dtype=ITEM_DTYPE)
        for it, s in zip(self.titems, target_map):
            Hs, Ws = self.masks[s].shape
            it["mask_off"], it["Hs"], it["Ws"] = mask_off[s], Hs, Ws
            it["idx_y"], it["idx_x"] = table("nearest", Hs, Ho)[0], table("nearest", Ws, Wo)[0]

        # warps: one descriptor and one scratch frame per warped output frame / mask; a frame whose warp is None keeps the descriptor it has
        def warp_items(which, srcs, source_map, offs, channels):
            nonlocal elems
            rows = [(i, w) for i, w in enumerate(which) if w is not None]
            out, dst = np.zeros(len(rows), dtype=WARP_DTYPE), 0
            for it, (i, w) in zip(out, rows):
                Hs, Ws = srcs[source_map[i]].shape[:2]
                if max(Hs, Ws) > SIDE_MAX:
                    raise ValueError(f"pack_batch: a warped source has at most {SIDE_MAX} pixels a side, got {Hs} x {Ws}")
                it["src_off"], it["dst_off"], it["Hs"], it["Ws"], it["a"] = offs[source_map[i]], dst, Hs, Ws, w
                if not channels:
                    if w[1] == 0.0 and w[3] == 0.0:          # Pillow's axis-aligned route: index tables, built as it builds them
                        it["mode"] = WARP_TABLES
                        for field, a in (("idx_x", warp_axis_table(w[2], w[0], Ws)), ("idx_y", warp_axis_table(w[5], w[4], Hs))):
                            it[field] = elems
                            self.tables.append((elems, a))
                            where[("warp_" + field[-1], i, a.size)] = (elems,)
                            elems += a.size
                    else:
                        it["mode"], it["A"] = WARP_FIXED, warp_fixed_coefficients(w, Hs, Ws)
                dst = _align(dst + Hs * Ws * (3 if channels else 1))
            return out, [i for i, _ in rows], dst, sum(int(it["Hs"]) * int(it["Ws"]) * (3 if channels else 1) for it in out)

        self.witems, wrows, img_scratch, img_frames = warp_items(warps, self.images, frame_map, src_off, True)
        self.wtitems, wtrows, mask_scratch, mask_frames = warp_items(target_warps, self.masks, target_map, mask_off, False)
        if elems >= 2 ** 31:
            raise ValueError("pack_batch: the tables of this batch exceed 2^31 elements")

        items_off = 0
        titems_off = _align(items_off + self.items.nbytes)
        tables_off = _align(titems_off + self.titems.nbytes)
        pixels_off = _align(tables_off + 4 * elems)
        masks_off = _align(pixels_off + pixel_bytes)
        nbytes = _align(masks_off + mask_bytes)
        self.warp_layout = None
        if warped:
            image_warps_off = nbytes
            mask_warps_off = _align(image_warps_off + self.witems.nbytes)
            nbytes = _align(mask_warps_off + self.wtitems.nbytes)
            self.wtitems["dst_off"] += img_scratch          # the warped masks follow the warped images
            self.warp_layout = WarpLayout(image_warps_off=image_warps_off, n_image_warps=len(wrows), mask_warps_off=mask_warps_off, n_mask_warps=len(wtrows), scratch_off=nbytes,
                                          scratch_bytes=img_scratch + mask_scratch, image_scratch_bytes=img_frames, mask_scratch_bytes=mask_frames,
                                          device_bytes=nbytes + img_scratch + mask_scratch)
            for i, w in zip(wrows, self.witems):          # the resize descriptor of a warped frame reads the scratch, counted from its own section
                self.items["src_off"][i] = nbytes - pixels_off + int(w["dst_off"])
            for i, w in zip(wtrows, self.wtitems):
                self.titems["mask_off"][i] = nbytes - masks_off + int(w["dst_off"])
        self.layout = BatchLayout(nbytes=nbytes, out_size=(Ho, Wo), n_frames=len(frame_map), n_targets=len(target_map), items_off=items_off,
                                  titems_off=titems_off, tables_off=tables_off, table_elems=elems, pixels_off=pixels_off, pixel_bytes=pixel_bytes, masks_off=masks_off,
                                  mask_bytes=mask_bytes, tables=tuple((k, v[0]) for k, v in where.items()))
        self._src_off, self._mask_off = src_off, mask_off

    def write(self, buf):
        L = self.layout
        if buf.dtype != np.uint8 or buf.ndim != 1 or buf.size < L.nbytes:
            raise ValueError(f"pack_batch: the destination must be a flat uint8 array of at least {L.nbytes} bytes")
        buf[L.items_off:L.items_off + self.items.nbytes] = self.items.view(np.uint8)
        buf[L.titems_off:L.titems_off + self.titems.nbytes] = self.titems.view(np.uint8)
        for off, a in self.tables:
            buf[L.tables_off + 4 * off:L.tables_off + 4 * (off + a.size)] = a.reshape(-1).view(np.uint8)
        for off, a in zip(self._src_off, self.images):
            buf[L.pixels_off + off:L.pixels_off + off + a.size] = a.reshape(-1)
        for off, a in zip(self._mask_off, self.masks):
            buf[L.masks_off + off:L.masks_off + off + a.size] = a.reshape(-1)
        W = self.warp_layout
        if W is not None:
            buf[W.image_warps_off:W.image_warps_off + self.witems.nbytes] = self.witems.view(np.uint8)
            buf[W.mask_warps_off:W.mask_warps_off + self.wtitems.nbytes] = self.wtitems.view(np.uint8)


def pack_batch(images, targets=None, *, out_size, frame_map=None, target_map=None, repeat=None, warps=None, target_warps=None):
    """Pack host images (PIL or uint8 (H, W, 3) arrays, every one its own size) and optionally masks (PIL 'L' / 'P' or uint8 (H, W)) for the batched
    kernels -> (blob, layout): one contiguous uint8 array and the BatchLayout that says where its sections and descriptors lie.
    Sections, each 16-byte aligned: image descriptors, target descriptors, int32 tables, pixels, masks.  The tables are the cached resample_tables /
    nearest_table, stored once per distinct (in, out) size pair of the batch.
    frame_map[i] / target_map[i] = the source of output frame / mask i (default: identity; a source may be named more than once, in any order);
    repeat=T is shorthand for every source T times in a row: a still image as a T-frame clip (`--pseudo_video_aug vanilla`, args.py:132-134).
    warps / target_warps (`--pseudo_video_aug weak-rotate-translate-shear-crop`): one entry per output frame / mask, None or the six coefficients of
    `PIL.Image.transform(size, AFFINE, coeffs)` (PseudoVideoAugment draws them).  With both absent the blob is today's, byte for byte.  With either
    given -> (blob, layout, warp_layout): the blob also carries one warp descriptor per warped frame behind the masks and, in the table section, the
    index tables of axis-aligned mask warps; the WarpLayout says where, and how much device scratch the warped sources need.  Every source is still
    stored once; a frame whose entry is None is resized from its source directly, exactly as without warps."""
    plan = _BatchPlan(images, targets, out_size, frame_map, target_map, repeat, warps, target_warps)
    blob = np.zeros(plan.layout.nbytes, dtype=np.uint8)
    plan.write(blob)
    return (blob, plan.layout) if plan.warp_layout is None else (blob, plan.layout, plan.warp_layout)


def _resample_rows(src, coef, bounds):
    """the integer stage along axis 1 of src (A, B, C) by one table pair -> uint8 (A, out, C)"""
    out = np.empty((src.shape[0], coef.shape[0], src.shape[2]), dtype=np.uint8)
    s = src.astype(np.int64)
    for xx in range(coef.shape[0]):
        x0, n = int(bounds[xx, 0]), int(bounds[xx, 1])
        acc = (1 << (PRECISION_BITS - 1)) + np.einsum("hkc,k->hc", s[:, x0:x0 + n], coef[xx, :n].astype(np.int64))
        out[:, xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def apply_packed_numpy(blob, layout, mean=MEAN, std=STD, integer_stage=False, warp_layout=None):
    """A packed batch read exactly as the kernels read it -- the descriptors and tables OF THE BLOB, the same offsets, the same integer stage, the same
    three fp32 operations in numpy float32 -- for tests only: packing is checked without a GPU.
    -> (images fp32 (n_frames, 3, Ho, Wo), targets int64 (n_targets, Ho, Wo) or None); integer_stage=True: images as uint8 (n_frames, Ho, Wo, 3).
    warp_layout (a batch packed with warps): the warp descriptors are applied first, as the warp kernels apply them, into scratch behind the blob."""
    L, W = layout, warp_layout
    Ho, Wo = L.out_size
    blob = np.asarray(blob)
    tables = blob[L.tables_off:L.tables_off + 4 * L.table_elems].view(np.int32)
    pixels, masks = blob[L.pixels_off:L.pixels_off + L.pixel_bytes], blob[L.masks_off:L.masks_off + L.mask_bytes]
    pixel_bytes, mask_bytes = L.pixel_bytes, L.mask_bytes
    if W is not None:
        mem = np.zeros(W.device_bytes, dtype=np.uint8)          # the device buffer: the blob, then the scratch
        mem[:L.nbytes] = blob[:L.nbytes]
        scratch = mem[W.scratch_off:]
        for off, n, ch, section, total in ((W.image_warps_off, W.n_image_warps, 3, pixels, L.pixel_bytes), (W.mask_warps_off, W.n_mask_warps, 1, masks, L.mask_bytes)):
            for it in blob[off:off + 128 * n].view(WARP_DTYPE):
                Hs, Ws, o, d = int(it["Hs"]), int(it["Ws"]), int(it["src_off"]), int(it["dst_off"])
                assert 0 < Hs <= SIDE_MAX and 0 < Ws <= SIDE_MAX and 0 <= o and o + Hs * Ws * ch <= total, "a warp source outside its section"
                assert 0 <= d and d + Hs * Ws * ch <= W.scratch_bytes, "a warped frame outside the scratch"
                if ch == 3:
                    out = affine_bilinear_numpy(section[o:o + Hs * Ws * 3].reshape(Hs, Ws, 3), it["a"])
                else:
                    m = section[o:o + Hs * Ws].reshape(Hs, Ws)
                    if int(it["mode"]) == WARP_TABLES:
                        ix, iy = int(it["idx_x"]), int(it["idx_y"])
                        assert 0 <= ix and ix + Ws <= L.table_elems and 0 <= iy and iy + Hs <= L.table_elems, "a warp table outside the table section"
                        xi, yi = tables[ix:ix + Ws].astype(np.int64)[None, :], tables[iy:iy + Hs].astype(np.int64)[:, None]
                    else:
                        A = [int(v) for v in it["A"]]
                        x, y = np.arange(Ws, dtype=np.int64)[None, :], np.arange(Hs, dtype=np.int64)[:, None]
                        xi, yi = (A[2] + A[1] * y + A[0] * x) >> 16, (A[5] + A[4] * y + A[3] * x) >> 16
                    inside = (xi >= 0) & (xi < Ws) & (yi >= 0) & (yi < Hs)
                    out = np.where(inside, m[np.clip(yi, 0, Hs - 1), np.clip(xi, 0, Ws - 1)], 0).astype(np.uint8)
                scratch[d:d + out.size] = out.reshape(-1)
        pixels, masks = mem[L.pixels_off:], mem[L.masks_off:]          # what the resize launches of a warped batch are given to read
        pixel_bytes, mask_bytes = W.device_bytes - L.pixels_off, W.device_bytes - L.masks_off

    def tab(off, rows, cols):
        assert 0 <= off and off + rows * cols <= L.table_elems, "a table outside the table section"
        return tables[off:off + rows * cols].reshape(rows, cols)

    u8 = np.empty((L.n_frames, Ho, Wo, 3), dtype=np.uint8)
    for i, it in enumerate(blob[L.items_off:L.items_off + 64 * L.n_frames].view(ITEM_DTYPE)):
        Hs, Ws, o = int(it["Hs"]), int(it["Ws"]), int(it["src_off"])
        assert 0 <= o and o + Hs * Ws * 3 <= pixel_bytes, "a source outside the pixel section"
        src = pixels[o:o + Hs * Ws * 3].reshape(Hs, Ws, 3)
        h = _resample_rows(src, tab(int(it["coef_x"]), Wo, int(it["ksize_x"])), tab(int(it["bounds_x"]), Wo, 2))
        u8[i] = _resample_rows(h.transpose(1, 0, 2), tab(int(it["coef_y"]), Ho, int(it["ksize_y"])), tab(int(it["bounds_y"]), Ho, 2)).transpose(1, 0, 2)
    tg = None
    if L.n_targets:
        tg = np.empty((L.n_targets, Ho, Wo), dtype=np.int64)
        for i, it in enumerate(blob[L.titems_off:L.titems_off + 64 * L.n_targets].view(ITEM_DTYPE)):
            Hs, Ws, o = int(it["Hs"]), int(it["Ws"]), int(it["mask_off"])
            assert 0 <= o and o + Hs * Ws <= mask_bytes, "a mask outside the mask section"
            m = masks[o:o + Hs * Ws].reshape(Hs, Ws)
            tg[i] = m[tab(int(it["idx_y"]), Ho, 1)[:, 0]][:, tab(int(it["idx_x"]), Wo, 1)[:, 0]]
    if integer_stage:
        return u8, tg
    v = u8.transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255)
    m32, s32 = np.asarray(mean, dtype=np.float32).reshape(1, 3, 1, 1), np.asarray(std, dtype=np.float32).reshape(1, 3, 1, 1)
    return np.ascontiguousarray((v - m32) / s32), tg


class PseudoVideoAugment:
    """`--pseudo_video_aug weak-rotate-translate-shear-crop` (args.py:132-137): every frame of a clip made from one still image gets its own gentle
    affine motion  p' = c + t + s R(theta) Sh(sx, sy) (p - c),  c = (Ws / 2, Hs / 2): a rotation by theta (degrees), a shear Sh = [[1, tan sx],
    [tan sy, 1]] (degrees), a zoom s (>= 1 zooms in: the 'crop' of the flag's name) and a translation t (a fraction of each side).  Every parameter is
    drawn uniformly from its (low, high) range, per image and frame.  The defaults are a choice -- 'weak', as the flag's help text demands -- not a
    measurement.  The photometric part of the reference's augmenter class (imgaug, cv2) is not reproduced.

    draw(sizes, T) -> per image a list of T entries, None or the six coefficients that `PIL.Image.transform(size, AFFINE, coeffs)` takes: the INVERSE
    of the motion, in closed form in float64.  One entry serves an image and its mask (pack_batch: warps / target_warps).  keep_first: frame 0 of
    every clip is None, the unwarped image.
    The randomness is the augmenter's own numpy Generator; state_dict() / load_state_dict() carry its bit-generator state, so that a resumed run
    continues the sequence: save it beside the training checkpoint (lavt_hip.checkpoint does not know about it)."""

    def __init__(self, rotate=(-10.0, 10.0), translate=(-0.1, 0.1), scale=(1.0, 1.2), shear=(-5.0, 5.0), keep_first=True, seed=None):
        def pair(v, what):
            lo, hi = (float(v[0]), float(v[1]))
            if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi):
                raise ValueError(f"PseudoVideoAugment: {what} is a finite (low, high) range, got {v}")
            return lo, hi
        self.rotate, self.translate, self.scale, self.shear = pair(rotate, "rotate"), pair(translate, "translate"), pair(scale, "scale"), pair(shear, "shear")
        if self.scale[0] <= 0.0:
            raise ValueError(f"PseudoVideoAugment: scale must be positive, got {scale}")
        if max(abs(v) for v in self.shear) >= 45.0:
            raise ValueError(f"PseudoVideoAugment: shear angles stay inside (-45, 45) degrees (at 45 both ways the motion has no inverse), got {shear}")
        self.keep_first = bool(keep_first)
        self._rng = np.random.Generator(np.random.PCG64(seed))

    @staticmethod
    def motion(size, angle=0.0, translate=(0.0, 0.0), scale=1.0, shear=(0.0, 0.0)):
        """the forward motion of an (Hs, Ws) frame as a 3 x 3 float64 matrix on (x, y, 1)"""
        Hs, Ws = size
        cx, cy = Ws / 2, Hs / 2
        th, tx, ty = math.radians(angle), math.tan(math.radians(shear[0])), math.tan(math.radians(shear[1]))
        M = scale * (np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]]) @ np.array([[1.0, tx], [ty, 1.0]]))
        t = np.array([cx + translate[0] * Ws, cy + translate[1] * Hs]) - M @ np.array([cx, cy])
        return np.array([[M[0, 0], M[0, 1], t[0]], [M[1, 0], M[1, 1], t[1]], [0.0, 0.0, 1.0]])

    @staticmethod
    def coefficients(size, angle=0.0, translate=(0.0, 0.0), scale=1.0, shear=(0.0, 0.0)):
        """Pillow's six coefficients (output pixel -> source position) of that motion: its inverse in closed form"""
        Hs, Ws = size
        cx, cy = Ws / 2, Hs / 2
        th, tx, ty = math.radians(angle), math.tan(math.radians(shear[0])), math.tan(math.radians(shear[1]))
        c, s = math.cos(th), math.sin(th)
        m00, m01, m10, m11 = scale * (c - s * ty), scale * (c * tx - s), scale * (s + c * ty), scale * (s * tx + c)
        det = m00 * m11 - m01 * m10
        if not math.isfinite(det) or det == 0.0:
            raise ValueError(f"PseudoVideoAugment: the motion (angle {angle}, scale {scale}, shear {shear}) has no inverse")
        a0, a1, a3, a4 = m11 / det + 0.0, -m01 / det + 0.0, -m10 / det + 0.0, m00 / det + 0.0          # (+ 0.0: no negative zeros)
        px, py = cx + translate[0] * Ws, cy + translate[1] * Hs          # where the centre goes
        return (a0, a1, cx - (a0 * px + a1 * py), a3, a4, cy - (a3 * px + a4 * py))

    def draw(self, sizes, T):
        T = int(T)
        if T < 1:
            raise ValueError(f"PseudoVideoAugment.draw: T must be >= 1, got {T}")
        u = self._rng.uniform
        clips = []
        for Hs, Ws in sizes:
            clip = []
            for f in range(T):
                if f == 0 and self.keep_first:
                    clip.append(None)
                    continue
                angle, tx, ty, scale, sx, sy = u(*self.rotate), u(*self.translate), u(*self.translate), u(*self.scale), u(*self.shear), u(*self.shear)
                clip.append(self.coefficients((int(Hs), int(Ws)), angle, (tx, ty), scale, (sx, sy)))
            clips.append(clip)
        return clips

    def state_dict(self):
        return {"bit_generator": self._rng.bit_generator.state}

    def load_state_dict(self, state):
        self._rng.bit_generator.state = state["bit_generator"]


def collate_raw(samples):
    """`collate_fn` of a DataLoader whose dataset returns (image, mask, ...) UNtransformed: images and masks stay lists of uint8 arrays (every one its
    own size: what TrainStep.stage_batch / load_batch take), everything after them is collated as usual -> (images, masks, *rest)"""
    from torch.utils.data import default_collate
    samples = list(samples)
    images = [_host_u8(s[0], True, f"collate_raw: image of sample {i}") for i, s in enumerate(samples)]
    masks = [_host_u8(s[1], False, f"collate_raw: mask of sample {i}") for i, s in enumerate(samples)]
    rest = default_collate([tuple(s[2:]) for s in samples]) if len(samples[0]) > 2 else []
    return (images, masks, *rest)


class BatchPreprocessor:
    """The batched input stage: host images of mixed sizes (and masks) -> fp32 (n, 3, Ho, Wo) (and int64 (n', Ho, Wo)) on the device with one upload
    and one launch per kind.

    stage(images, targets=None, frame_map=None, target_map=None, repeat=None, warps=None, target_warps=None) packs into one of two pinned host slots and starts ONE asynchronous
    upload on the preprocessor's own copy stream into the matching one of two device slots; it touches no output, so it may run while the consumer of
    the previous batch's output is still busy.  commit(out_images, out_targets=None) makes the current stream wait for that upload and launches the
    kernels into `out`.  batch(...) does both and returns the outputs.
    Slot reuse is ordered by events: before a pinned slot is rewritten the host waits for the previous upload out of it; before a device slot is
    overwritten the host waits for the kernels that last read it -- those of the commit before the last one, so in a steady loop the host runs at
    most one iteration ahead of the device and never waits for the batch in flight.  Slots grow geometrically (outside any capture: stage and
    commit refuse to run inside one).
    warps / target_warps (pack_batch; PseudoVideoAugment draws them): commit first warps the named frames and masks (lavt_affine_u8_batch,
    lavt_affine_nearest_u8_batch) into scratch that follows the blob in the device slot -- the device slot of such a batch is larger than the pinned
    one by WarpLayout.scratch_bytes, and is the slot's in every other respect: the same growth, the same events -- then resizes as usual, all on the
    committing stream."""

    def __init__(self, out_size, mean=MEAN, std=STD, device=None):
        self.out_size = (int(out_size), int(out_size)) if isinstance(out_size, int) else (int(out_size[0]), int(out_size[1]))
        if min(self.out_size) < 1:
            raise ValueError(f"BatchPreprocessor: out_size must be positive, got {self.out_size}")
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        if len(self.mean) != 3 or len(self.std) != 3 or any(s == 0.0 for s in self.std):
            raise ValueError("BatchPreprocessor: mean and std are three values each, std nonzero")
        self.device = device
        self._host, self._dev = [None, None], [None, None]          # pinned uint8 / device uint8, per slot
        self._uploaded = [None, None]          # event on the copy stream: the last upload out of pinned slot i (into device slot i) has ended
        self._consumed = [None, None]          # event on the committing stream: the kernels that last read device slot i have ended
        self._next, self._staged, self._copy_stream = 0, None, None

    def _device(self):
        if not torch.cuda.is_available():
            raise RuntimeError(_NO_CPU.format("no GPU is available"))
        return torch.device(self.device if self.device is not None else f"cuda:{torch.cuda.current_device()}")

    @staticmethod
    def _not_capturing(who):
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"BatchPreprocessor.{who}: the input stage runs eagerly in front of the captured step (pinned slots, an upload on a copy stream): "
                               "call it outside the graph capture")

    def _reserve(self, slot, nbytes, dev, device_bytes):
        have = 0 if self._host[slot] is None else self._host[slot].numel()
        have_dev = 0 if self._dev[slot] is None else self._dev[slot].numel()
        if have >= nbytes and have_dev >= device_bytes:
            return
        for ev in (self._uploaded[slot], self._consumed[slot]):          # nothing in flight may still use the buffers that are let go
            if ev is not None:
                ev.synchronize()
        if have < nbytes:
            self._host[slot] = torch.empty(max(nbytes, 2 * have, 1 << 16), dtype=torch.uint8).pin_memory()
        if have_dev < device_bytes:          # (blob + the scratch of a warped batch; without warps the two sizes are equal and grow together)
            self._dev[slot] = torch.empty(max(device_bytes, 2 * have_dev, 1 << 16), dtype=torch.uint8, device=dev)
        self._uploaded[slot], self._consumed[slot] = None, None
        self._copy_stream.wait_stream(torch.cuda.current_stream(dev))          # (the allocator may hand out memory the current stream still works on)

    def stage(self, images, targets=None, *, frame_map=None, target_map=None, repeat=None, warps=None, target_warps=None):
        """-> the BatchLayout of the staged batch.  A batch staged before and never committed is dropped."""
        self._not_capturing("stage")
        return self._stage(_BatchPlan(images, targets, self.out_size, frame_map, target_map, repeat, warps, target_warps))          # (every refusal of the input comes first)

    def _stage(self, plan):
        dev = self._device()
        if self._copy_stream is None:
            self._copy_stream = torch.cuda.Stream(dev)
        slot, self._next = self._next, self._next ^ 1
        nbytes = plan.layout.nbytes
        W = plan.warp_layout
        self._reserve(slot, nbytes, dev, nbytes if W is None else W.device_bytes)
        if self._uploaded[slot] is not None:
            self._uploaded[slot].synchronize()          # the previous upload out of this pinned slot (long finished in a steady loop)
        plan.write(self._host[slot].numpy())
        cs = self._copy_stream
        if self._consumed[slot] is not None:
            # The kernels that last read this device slot: those of the commit before the last one.  The HOST waits for them, not the copy stream: a
            # stream that waits for an event of the stream a captured step replays on was measured to cost every replay ~0.3 ms (DESIGN.md "Batched
            # input stage"), a host wait nothing -- it keeps the host at most one iteration ahead of the device, with a whole replay still queued
            self._consumed[slot].synchronize()
        with torch.cuda.stream(cs):
            self._dev[slot][:nbytes].copy_(self._host[slot][:nbytes], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(cs)
        self._uploaded[slot] = ev
        self._staged = (slot, plan.layout, W)
        return plan.layout

    def commit(self, out_images, out_targets=None):
        """launch the kernels of the staged batch into `out_images` (contiguous fp32 holding (n_frames, 3, Ho, Wo); leading dimensions may be split,
        e.g. (B, T, 3, H, W)) and `out_targets` (int64 (n_targets, Ho, Wo)) on the current stream -> (out_images, out_targets)"""
        from . import ops
        self._not_capturing("commit")
        if self._staged is None:
            raise RuntimeError("BatchPreprocessor.commit: no staged batch (call stage() first; a batch is committed once)")
        slot, L, W = self._staged
        Ho, Wo = L.out_size
        img = _batch_out(out_images, (L.n_frames, 3, Ho, Wo), torch.float32, "out_images")
        if (out_targets is None) != (L.n_targets == 0):
            raise ValueError(f"BatchPreprocessor.commit: the staged batch has {L.n_targets} targets, out_targets is {'missing' if out_targets is None else 'given'}")
        tgt = _batch_out(out_targets, (L.n_targets, Ho, Wo), torch.int64, "out_targets") if out_targets is not None else None
        self._staged = None
        cur = torch.cuda.current_stream(self._dev[slot].device)
        cur.wait_event(self._uploaded[slot])
        host = self._host[slot].numpy()
        try:
            if W is not None and W.n_image_warps:
                ops.affine_u8_batch(self._dev[slot], host, L, W)
            if W is not None and W.n_mask_warps:
                ops.affine_nearest_u8_batch(self._dev[slot], host, L, W)
            ops.resize_normalize_u8_batch(self._dev[slot], host, L, img, self.mean, self.std, W)
            if tgt is not None:
                ops.resize_nearest_u8_batch(self._dev[slot], host, L, tgt, W)
        finally:
            ev = torch.cuda.Event()
            ev.record(cur)
            self._consumed[slot] = ev
        return out_images, out_targets

    def batch(self, images, targets=None, *, out_images=None, out_targets=None, frame_map=None, target_map=None, repeat=None, warps=None, target_warps=None):
        """stage + commit -> (images fp32 (n_frames, 3, Ho, Wo), targets int64 (n_targets, Ho, Wo) or None), into `out_*` when given"""
        self._not_capturing("batch")
        plan = _BatchPlan(images, targets, self.out_size, frame_map, target_map, repeat, warps, target_warps)
        L, dev = plan.layout, self._device()
        Ho, Wo = L.out_size
        if out_images is None:
            out_images = torch.empty(L.n_frames, 3, Ho, Wo, dtype=torch.float32, device=dev)
        if out_targets is None and L.n_targets:
            out_targets = torch.empty(L.n_targets, Ho, Wo, dtype=torch.int64, device=dev)
        self._stage(plan)
        return self.commit(out_images, out_targets)


def _batch_out(out, shape, dtype, what):
    """_as_frames for BatchPreprocessor.commit"""
    if not isinstance(out, torch.Tensor) or not out.is_cuda:
        raise RuntimeError(_NO_CPU.format(f"got a CPU tensor for `{what}`"))
    n = 1
    for s in shape:
        n *= s
    if out.dtype != dtype or not out.is_contiguous() or out.numel() != n or tuple(out.shape[-2:]) != tuple(shape[-2:]):
        raise ValueError(f"BatchPreprocessor.commit: `{what}` must be a contiguous {dtype} tensor holding {tuple(shape)} (the frames of the staged batch), "
                         f"got {out.dtype} {tuple(out.shape)}")
    return out.view(shape)


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
