"""GPU checks of the pseudo-video augmentation: lavt_affine_u8_batch / lavt_affine_nearest_u8_batch (csrc/preprocess.hip) alone through the C ABI,
then through BatchPreprocessor.batch(warps=, target_warps=) and TrainStep.load_batch / stage_batch(augment=).

References: the numpy restatement of Pillow's affine transform (lavt_hip.preprocess.affine_bilinear_numpy / affine_nearest_numpy, which
tests/test_pseudo_video_host.py holds equal to the installed Pillow) and Pillow itself where the machine has it; for whole batches
apply_packed_numpy, which reads the blob as the kernels do.  Every comparison is exact equality: the contract is Pillow's result, pixel for pixel,
and the fp32 finish is three IEEE operations in the reference's order, so there is nothing to tolerate.

No source side exceeds 96 and out_size is at most 64: the kernels can go wrong at edges (tiles of 64 x 4 output pixels, byte offsets of any
alignment, the frame border), not at size."""

import numpy as np
import pytest
import torch

from lavt_hip import preprocess as P
from lavt_hip.preprocess import PseudoVideoAugment as A
from test_pseudo_video_host import SIZES, pil_affine, sources, transforms

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GPU_SIZES = SIZES + ((67, 96),)          # 96 = one full tile of 64 columns and half of one, 67 = sixteen groups of 4 rows and 3: more than one block each way
GUARD = 0xAB


def _launch(kind, warps, src, dst, tables=None):
    """one launch of either entry through the C ABI -> its return code.  warps: WARP_DTYPE array (the host copy; uploaded here)"""
    from lavt_hip import _capi as K
    from lavt_hip import ops          # noqa: F401  (binds the library)
    wdev = torch.from_numpy(warps.view(np.uint8).copy()).to(DEV)
    host = np.ascontiguousarray(warps)
    if kind == "image":
        return K.lib.lavt_affine_u8_batch(wdev.data_ptr(), host.ctypes.data, len(warps), src.data_ptr(), src.numel(), dst.data_ptr(), dst.numel(), K.stream())
    tdev = torch.from_numpy(tables).to(DEV) if tables is not None and tables.size else None
    return K.lib.lavt_affine_nearest_u8_batch(wdev.data_ptr(), host.ctypes.data, len(warps), tdev.data_ptr() if tdev is not None else None,
                                              tables.ctypes.data if tdev is not None else None, tables.size if tdev is not None else 0, src.data_ptr(), src.numel(),
                                              dst.data_ptr(), dst.numel(), K.stream())


def _case_batch(channels):
    """every case of the host list (and of a 67 x 96 source) as ONE batch: the sources back to back (the 1 x 7 first, so the later ones start at odd
    bytes), one descriptor per case (sixteen descriptors name each source), destinations back to back too, one guard byte between them
    -> (descriptors, source bytes, tables, [(size, name, coefficients, source array, dst offset)], dst bytes)"""
    srcs, offs, off = [], [], 0
    for size in GPU_SIZES:
        a = sources(size)[0 if channels == 3 else 1]
        srcs.append(a)
        offs.append(off)
        off += a.size
    assert any(o % 2 for o in offs)
    cases = [(si, size, name, c) for si, size in enumerate(GPU_SIZES) for name, c in transforms(size)]
    warps, tables, rows, dst = np.zeros(len(cases), dtype=P.WARP_DTYPE), [], [], 1
    for w, (si, (Hs, Ws), name, c) in zip(warps, cases):
        w["src_off"], w["dst_off"], w["Hs"], w["Ws"], w["a"] = offs[si], dst, Hs, Ws, c
        if channels == 1:
            if c[1] == 0.0 and c[3] == 0.0:
                w["mode"] = P.WARP_TABLES
                for field, t in (("idx_x", P.warp_axis_table(c[2], c[0], Ws)), ("idx_y", P.warp_axis_table(c[5], c[4], Hs))):
                    w[field] = sum(t.size for t in tables)
                    tables.append(t)
            else:
                w["mode"], w["A"] = P.WARP_FIXED, P.warp_fixed_coefficients(c, Hs, Ws)
        rows.append(((Hs, Ws), name, c, srcs[si], dst))
        dst += Hs * Ws * channels + 1
    return warps, np.concatenate([a.reshape(-1) for a in srcs]), (np.concatenate(tables) if tables else np.zeros(0, np.int32)), rows, dst


@pytest.mark.parametrize("kind", ["image", "mask"])
def test_kernel_alone_equals_the_restatement_and_pillow(kind):
    channels = 3 if kind == "image" else 1
    warps, src, tables, rows, nbytes = _case_batch(channels)
    assert len(rows) >= 80 and len({int(o) for o in warps["src_off"]}) == len(GPU_SIZES), "many descriptors name one source"
    dst = torch.full((nbytes,), GUARD, dtype=torch.uint8, device=DEV)
    assert _launch(kind, warps, torch.from_numpy(src).to(DEV), dst, tables) == 0
    got = dst.cpu().numpy()
    try:
        import PIL.Image          # noqa: F401
        pillow = True
    except ImportError:
        pillow = False
    for (Hs, Ws), name, c, a, off in rows:
        out = got[off:off + a.size].reshape(a.shape)
        want = P.affine_bilinear_numpy(a, c) if channels == 3 else P.affine_nearest_numpy(a, c)
        assert np.array_equal(out, want), f"{kind} {Hs} x {Ws} {name}: {int((out != want).sum())} values differ from the restatement"
        if pillow:
            assert np.array_equal(out, pil_affine(a, c, channels == 1)), f"{kind} {Hs} x {Ws} {name}: differs from Pillow"
        assert got[off - 1] == GUARD and got[off + a.size] == GUARD, f"{kind} {Hs} x {Ws} {name}: a byte outside the frame was written"


def test_host_entries_refuse_without_launching():
    from lavt_hip import _capi as K
    img, mask = sources((37, 53))
    ok = np.zeros(2, dtype=P.WARP_DTYPE)
    ok["Hs"], ok["Ws"], ok["a"], ok["dst_off"] = 37, 53, (1.0, 0.0, 0.0, 0.0, 1.0, 0.0), (0, 37 * 53 * 3)
    ok["A"] = P.warp_fixed_coefficients((1.0, 0.0, 0.0, 0.0, 1.0, 0.0), 37, 53)          # (mode 0 = LAVT_WARP_FIXED; the identity through the general route)

    def bad(**fields):
        w = ok.copy()
        for k, v in fields.items():
            w[k][1] = v
        return w
    overflow = list(ok["A"][0])
    overflow[0] = 30000 << 16          # fits int32 itself; times the 53 columns of the far corners it does not
    refusals = [("image", bad(src_off=1), "outside the .* bytes of pixels"), ("mask", bad(src_off=37 * 53 * 2 + 1), "outside the .* bytes of masks"),
                ("image", bad(dst_off=37 * 53 * 3 + 1), "outside the .* bytes of the destination"),
                ("image", bad(a=(1.0, 0.0, float("nan"), 0.0, 1.0, 0.0)), "not finite"), ("image", bad(a=(float("inf"), 0.0, 0.0, 0.0, 1.0, 0.0)), "not finite"),
                ("mask", bad(A=overflow), "overflow int32"), ("image", bad(Hs=8193), "sides are 1..8192"), ("mask", bad(Ws=8193), "sides are 1..8192"),
                ("mask", bad(mode=2), "neither LAVT_WARP_FIXED nor LAVT_WARP_TABLES"), ("mask", bad(mode=P.WARP_TABLES, idx_x=40), "index table")]
    src3, src1 = torch.from_numpy(img).to(DEV).view(-1), torch.from_numpy(np.concatenate([mask, mask, mask])).to(DEV).view(-1)
    dst = torch.full((2 * 37 * 53 * 3,), GUARD, dtype=torch.uint8, device=DEV)
    for kind, warps, message in refusals:
        rc = _launch(kind, warps, src3 if kind == "image" else src1, dst, np.zeros(37 + 53, np.int32))
        assert rc == -22, (kind, message, rc)          # LAVT_ERR_INVALID
        with pytest.raises(RuntimeError, match="rc=-22.*warp 1.*" + message):
            K.check(rc)
    rc = _launch("mask", bad(mode=P.WARP_TABLES, idx_x=0, idx_y=53), src1, dst, np.full(37 + 53, 53, np.int32))
    with pytest.raises(RuntimeError, match=r"rc=-22.*warp 1: idx_x\[0\] = 53 is neither -1 nor a column"):
        K.check(rc)
    torch.cuda.synchronize()
    assert bool((dst == GUARD).all()), "a refused call launched nothing"
    # the same descriptors, unspoiled, run: both frames are the source
    assert _launch("image", ok, src3, dst) == 0 and torch.equal(dst.view(2, 37, 53, 3)[1].cpu(), torch.from_numpy(img))
    assert _launch("mask", ok[:1], src1, dst) == 0 and torch.equal(dst[:37 * 53].view(37, 53).cpu(), torch.from_numpy(mask))


def _batches():
    out = (48, 64)
    a = [sources((37, 53), 1), sources((64, 48), 1)]
    b = [sources((67, 96), 2), sources((7, 1), 2)]
    return [([p[0] for p in pairs], [p[1] for p in pairs]) for pairs in (a, b)], out


def _flat_warps(images, T, seed):
    clips = A(seed=seed).draw([a.shape[:2] for a in images], T)
    clips[1][2] = A.coefficients(images[1].shape[:2], 0.0, (0.04, -0.03), 1.12)          # an axis-aligned frame: the masks' table route
    return [w for clip in clips for w in clip]


def test_batch_preprocessor_with_warps():
    (b1, b2), out = _batches()
    T = 3
    pp = P.BatchPreprocessor(out)
    van_x, van_t = pp.batch(*b1, repeat=T)
    van_x, van_t = van_x.clone(), van_t.clone()
    for images, masks in (b1, b2, b1):          # three batches: both slots, and the first again after it grew for the second
        warps = _flat_warps(images, T, seed=len(images[0]))
        x, t = pp.batch(images, masks, repeat=T, warps=warps, target_warps=warps, out_images=torch.full((2 * T, 3, *out), float("nan"), device=DEV),
                        out_targets=torch.full((2 * T, *out), -1, dtype=torch.int64, device=DEV))
        blob, L, W = P.pack_batch(images, masks, out_size=out, repeat=T, warps=warps, target_warps=warps)
        ex, et = P.apply_packed_numpy(blob, L, warp_layout=W)
        assert torch.equal(x.cpu(), torch.from_numpy(ex)), f"{int((x.cpu() != torch.from_numpy(ex)).sum())} image values differ from the blob read on the host"
        assert torch.equal(t.cpu(), torch.from_numpy(et)), "masks differ from the blob read on the host"
        if images is b1[0]:
            for f in (0, T):
                assert torch.equal(x[f], van_x[f]) and torch.equal(t[f], van_t[f]), "frame 0 of a clip is the repeat=T frame"
            assert not torch.equal(x[1], van_x[1]) and not torch.equal(t[1], van_t[1])
    # a vanilla batch through a slot that held a warped one is today's
    x, t = pp.batch(*b1, repeat=T)
    assert torch.equal(x, van_x) and torch.equal(t, van_t)


def test_train_step_with_augment():
    """the micro Video-Swin model of the suite's clip tests (2 clips x 4 frames x 64^2), targets for every frame"""
    import lavt_hip
    from lavt_hip import ops
    from lavt_hip.engine import TrainStep
    from test_gpu_deterministic import _video
    model, frames, ids, am, _ = _video("pwam")
    B, T = frames.shape[:2]
    S = tuple(frames.shape[-2:])
    rng = np.random.default_rng(8)

    def smooth(h, w):          # smooth content (a coarse random grid enlarged), so that the loss is not that of noise
        return np.kron(rng.integers(0, 256, (h // 8 + 1, w // 8 + 1, 3), dtype=np.uint8), np.ones((8, 8, 1), dtype=np.uint8))[:h, :w]

    def blob_mask(h, w):
        yy, xx = np.mgrid[:h, :w]
        return (((yy - h / 2) / (h / 3)) ** 2 + ((xx - w / 2) / (w / 4)) ** 2 < 1).astype(np.uint8)
    batch1 = ([smooth(50, 90), smooth(77, 41)], [blob_mask(50, 90), blob_mask(77, 41)])
    batch2 = ([smooth(64, 64), smooth(30, 96)], [blob_mask(64, 64), blob_mask(30, 96)])

    def expected(batch, aug):
        warps = [w for clip in aug.draw([a.shape[:2] for a in batch[0]], T) for w in clip]
        blob, L, W = P.pack_batch(*batch, out_size=S, repeat=T, warps=warps, target_warps=warps)
        ex, et = P.apply_packed_numpy(blob, L, warp_layout=W)
        return torch.from_numpy(ex).view(B, T, 3, *S).to(DEV), torch.from_numpy(et).to(DEV)
    host_aug = A(seed=3)
    ex1, et1 = expected(batch1, host_aug)
    ex2, et2 = expected(batch2, host_aug)
    assert int(et1.sum()) > 0 and not torch.equal(et1[0], et1[1]) and not torch.equal(ex1[0, 0], ex1[0, 1]), "the frames of a clip move"

    with lavt_hip.use_dtype(torch.float32):
        x, t = torch.zeros_like(frames), torch.zeros(B * T, *S, dtype=torch.int64, device=DEV)
        step = TrainStep(model, x, ids, am, t, context=ops.StepContext(), deterministic=True)
        step.warmup_and_capture()
        assert step.captured
        graph = step.graph

        aug = A(seed=3)
        step.load_batch(*batch1, repeat=T, augment=aug)
        assert step.x is x and torch.equal(x, ex1) and torch.equal(t, et1), "load_batch(augment=) fills image and target with the expected clip"
        loss1 = step.step().clone()
        step.load_batch(*batch2, repeat=T, augment=aug)
        assert torch.equal(x, ex2) and torch.equal(t, et2), "the augmenter's sequence continues from batch to batch"
        loss2 = step.step().clone()
        assert bool(torch.isfinite(loss1)) and bool(torch.isfinite(loss2)) and not torch.equal(loss1, loss2)

        # the same two batches, the second staged while the replay of the first is still queued behind a matrix product
        aug = A(seed=3)
        busy = torch.randn(2048, 2048, device=DEV)
        step.load_batch(*batch1, repeat=T, augment=aug)
        busy @ busy
        loss1b = step.step().clone()
        step.stage_batch(*batch2, repeat=T, augment=aug)
        assert torch.equal(x, ex1) and torch.equal(t, et1), "stage_batch writes neither image nor target"
        step.commit_batch()
        assert torch.equal(x, ex2) and torch.equal(t, et2)
        loss2b = step.step().clone()
        torch.cuda.synchronize()
        assert torch.equal(loss1b, loss1) and torch.equal(loss2b, loss2), (float(loss1), float(loss1b), float(loss2), float(loss2b))
        assert step.graph is graph, "nothing re-captures"

        # refusals: nothing is written, nothing is drawn
        keep_x, keep_t, state = x.clone(), t.clone(), aug.state_dict()
        with pytest.raises(ValueError, match="repeat=T"):
            step.load_batch(batch1[0] * T, batch1[1] * T, augment=aug)
        with pytest.raises(ValueError, match="frames"):
            step.load_batch(batch1[0][:1], batch1[1][:1], repeat=T, augment=aug)
        with pytest.raises(TypeError, match=r"FramePreprocessor\.images"):
            step.load_batch([torch.from_numpy(a).to(DEV) for a in batch1[0]], batch1[1], repeat=T, augment=aug)
        torch.cuda.synchronize()
        assert torch.equal(x, keep_x) and torch.equal(t, keep_t) and aug.state_dict()["bit_generator"] == state["bit_generator"]
