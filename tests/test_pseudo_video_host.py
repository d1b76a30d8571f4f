"""Host-side checks of the pseudo-video augmentation (no GPU): the numpy restatements of Pillow's affine transform in lavt_hip.preprocess
(affine_bilinear_numpy, affine_nearest_numpy: what lavt_affine_u8_batch / lavt_affine_nearest_u8_batch compute) against the installed Pillow, the
packing of warps into the batch blob (pack_batch / apply_packed_numpy), the augmenter, and the refusals.  Every pixel comparison is exact: the
contract is Pillow's result, pixel for pixel, so there is nothing to tolerate."""
import math

import numpy as np
import pytest
import torch

from lavt_hip import preprocess as P
from lavt_hip.engine import _BatchInput, _ValidIndices
from lavt_hip.preprocess import PseudoVideoAugment as A

SIZES = ((1, 7), (7, 1), (37, 53), (64, 48))          # (Hs, Ws)


def sources(size, seed=0):
    """-> (image uint8 (Hs, Ws, 3), mask uint8 (Hs, Ws) with labels 0..3) of random content: every pixel differs from its neighbours"""
    rng = np.random.default_rng(1000 * size[0] + size[1] + seed)
    return rng.integers(0, 256, size + (3,), dtype=np.uint8), rng.integers(0, 4, size, dtype=np.uint8)


def transforms(size):
    """the case list of one source size -> [(name, six coefficients)]"""
    Hs, Ws = size
    rng = np.random.default_rng(7 * Hs + Ws)
    cases = [("identity", (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)),
             ("integer translation", (1.0, 0.0, 3.0, 0.0, 1.0, -2.0)),          # coordinates land exactly on pixel boundaries
             ("mostly outside", (1.0, 0.0, 0.6 * Ws, 0.0, 1.0, 0.55 * Hs)),     # more than half the frame reads the fill
             ("last row", (1.0, 0.0, 0.25, 0.0, 1.0, 0.75)),                    # yin reaches past the centre of the last row: v2 = v1
             ("half-pixel rotation", A.coefficients(size, 7.0, (0.01, -0.02))),
             ("zoom, unequal axes", (0.8, 0.0, 0.1 * Ws, 0.0, 0.9, 0.03 * Hs)),          # axis-aligned: Pillow's index-table route for masks
             ("zoom out", (1.3, 0.0, -0.2 * Ws, 0.0, 1.15, -0.1 * Hs)),
             ("mirror zoom", (-0.9, 0.0, 0.95 * Ws, 0.0, 1.0 / 1.2, 0.1 * Hs)),
             ("pure zoom of the augmenter", A.coefficients(size, 0.0, (0.0, 0.0), 1.17)),
             ("zoom and shift of the augmenter", A.coefficients(size, 0.0, (0.07, -0.04), 1.09))]
    for k in range(6):          # general rotate / shear / scale / translate, stronger than the augmenter's defaults
        cases.append((f"general {k}", A.coefficients(size, rng.uniform(-30, 30), tuple(rng.uniform(-0.2, 0.2, 2)), rng.uniform(0.8, 1.4), tuple(rng.uniform(-15, 15, 2)))))
    return cases


CASES = [(size, name, c) for size in SIZES for name, c in transforms(size)]


def pil_affine(src, c, nearest):
    from PIL import Image
    im = Image.fromarray(src)
    return np.asarray(im.transform((src.shape[1], src.shape[0]), Image.AFFINE, c, resample=Image.NEAREST if nearest else Image.BILINEAR))


# ================================================================================================ the restatement against Pillow
def test_restatement_equals_the_installed_pillow():
    pytest.importorskip("PIL.Image")
    assert len(CASES) >= 40
    tables = fixed = filled = last_row = 0
    for size, name, c in CASES:
        img, mask = sources(size)
        got, want = P.affine_bilinear_numpy(img, c), pil_affine(img, c, False)
        assert np.array_equal(got, want), f"{size} {name}: {int((got != want).sum())} image values differ from Pillow's"
        got, want = P.affine_nearest_numpy(mask, c), pil_affine(mask, c, True)
        assert np.array_equal(got, want), f"{size} {name}: {int((got != want).sum())} mask pixels differ from Pillow's"
        tables += c[1] == 0.0 and c[3] == 0.0
        fixed += not (c[1] == 0.0 and c[3] == 0.0)
        ones = pil_affine(np.full(size, 255, np.uint8), c, True)
        filled += (ones == 0).mean() > 0.5
        yin = c[3] * (np.arange(size[1]) + 0.5)[None, :] + c[4] * (np.arange(size[0]) + 0.5)[:, None] + c[5]
        last_row += bool(((yin >= size[0] - 0.5) & (yin < size[0])).any())
    assert tables >= 8 and fixed >= 8 and filled >= 4 and last_row >= 4, "the case list exercises both mask routes, the fill and the v2 = v1 rule"


def test_identity_and_integer_translation_are_what_they_say():
    img, mask = sources((37, 53))
    assert np.array_equal(P.affine_bilinear_numpy(img, (1, 0, 0, 0, 1, 0)), img) and np.array_equal(P.affine_nearest_numpy(mask, (1, 0, 0, 0, 1, 0)), mask)
    out, mout = P.affine_bilinear_numpy(img, (1, 0, 3, 0, 1, -2)), P.affine_nearest_numpy(mask, (1, 0, 3, 0, 1, -2))
    assert np.array_equal(out[2:, :-3], img[:-2, 3:]) and not out[:2].any() and not out[:, -3:].any()
    assert np.array_equal(mout[2:, :-3], mask[:-2, 3:]) and not mout[:2].any() and not mout[:, -3:].any()


def test_fixed_point_form_and_its_int32_condition():
    c = A.coefficients((37, 53), 12.0, (0.05, 0.02), 1.1, (3.0, -2.0))
    Af = P.warp_fixed_coefficients(c, 37, 53)
    assert Af[0] == math.floor(c[0] * 65536 + 0.5) and Af[2] == math.floor((c[2] + c[0] * 0.5 + c[1] * 0.5) * 65536 + 0.5)
    with pytest.raises(ValueError, match="overflow int32"):
        P.warp_fixed_coefficients((1.0, 0.001, 40000.0, 0.0, 1.0, 0.0), 37, 53)          # the offset alone
    with pytest.raises(ValueError, match="overflow int32"):
        P.warp_fixed_coefficients((600.0, 0.5, 0.0, 0.0, 1.0, 0.0), 37, 96)               # every coefficient fits, the far corner does not


# ================================================================================================ packing
def _batch(seed=5):
    sizes = [(37, 53), (64, 48)]
    pairs = [sources(s, seed) for s in sizes]
    return [p[0] for p in pairs], [p[1] for p in pairs], (32, 40)


def _clip_warps(sizes, T, seed=3):
    """keep_first clips with one axis-aligned frame among the drawn ones -> flat list of B*T entries"""
    clips = A(seed=seed).draw(sizes, T)
    clips[0][1] = A.coefficients(sizes[0], 0.0, (0.03, -0.05), 1.15)          # a pure zoom and shift: the table route
    return [w for clip in clips for w in clip]


def test_without_warps_the_blob_is_todays():
    images, masks, out = _batch()
    a, La = P.pack_batch(images, masks, out_size=out, repeat=3)
    packed = P.pack_batch(images, masks, out_size=out, repeat=3, warps=None, target_warps=None)
    assert len(packed) == 2 and np.array_equal(a, packed[0]) and La == packed[1]
    # all-None warps: the sections of today's blob are unchanged, byte for byte, and no scratch is asked for
    b, Lb, W = P.pack_batch(images, masks, out_size=out, repeat=3, warps=[None] * 6, target_warps=[None] * 6)
    assert np.array_equal(a, b[:La.nbytes]) and Lb[1:] == La[1:] and (W.n_image_warps, W.n_mask_warps, W.scratch_bytes) == (0, 0, 0)


def test_warped_blob_keeps_every_source_once_and_none_frames_vanilla():
    images, masks, out = _batch()
    T = 3
    warps = _clip_warps([a.shape[:2] for a in images], T)
    vb, vL = P.pack_batch(images, masks, out_size=out, repeat=T)
    blob, L, W = P.pack_batch(images, masks, out_size=out, repeat=T, warps=warps, target_warps=warps)
    assert L.pixel_bytes == vL.pixel_bytes == sum(a.size for a in images) and L.mask_bytes == vL.mask_bytes, "the pixel section holds every source once"
    assert np.array_equal(blob[L.pixels_off:L.pixels_off + L.pixel_bytes], vb[vL.pixels_off:vL.pixels_off + vL.pixel_bytes])
    assert W.n_image_warps == W.n_mask_warps == 4 and blob.size == L.nbytes == W.scratch_off and W.device_bytes == W.scratch_off + W.scratch_bytes
    assert W.image_scratch_bytes == 2 * sum(a.size for a in images) and W.mask_scratch_bytes == 2 * sum(m.size for m in masks)
    assert all(o % 16 == 0 for o in (W.image_warps_off, W.mask_warps_off, W.scratch_off)) and L.masks_off + L.mask_bytes <= W.image_warps_off
    items, vitems = blob[L.items_off:L.items_off + 64 * 6].view(P.ITEM_DTYPE), vb[vL.items_off:vL.items_off + 64 * 6].view(P.ITEM_DTYPE)
    assert items["src_off"][0] == vitems["src_off"][0] and items["src_off"][3] == vitems["src_off"][3], "a None frame's descriptor points at the original source"
    wm = blob[W.mask_warps_off:W.mask_warps_off + 128 * 4].view(P.WARP_DTYPE)
    assert list(wm["mode"]) == [P.WARP_TABLES, P.WARP_FIXED, P.WARP_FIXED, P.WARP_FIXED], "the axis-aligned mask warp goes through index tables"
    assert L.table_elems == vL.table_elems + images[0].shape[0] + images[0].shape[1]

    u8, tg = P.apply_packed_numpy(blob, L, integer_stage=True, warp_layout=W)
    vu8, vtg = P.apply_packed_numpy(vb, vL, integer_stage=True)
    for f in (0, 3):
        assert np.array_equal(u8[f], vu8[f]) and np.array_equal(tg[f], vtg[f]), "a None frame is the repeat=T frame"
    assert not np.array_equal(u8[1], vu8[1]) and not np.array_equal(tg[1], vtg[1])


def test_packed_warps_equal_pillow_warp_then_resize():
    pytest.importorskip("PIL.Image")
    from test_preprocess_batch_host import expected_images, expected_targets
    images, masks, out = _batch(9)
    T = 3
    warps = _clip_warps([a.shape[:2] for a in images], T, seed=11)
    blob, L, W = P.pack_batch(images, masks, out_size=out, repeat=T, warps=warps, target_warps=warps)
    src = [s for s in range(2) for _ in range(T)]
    want = [P.apply_tables_numpy(images[s] if w is None else pil_affine(images[s], w, False), *out) for s, w in zip(src, warps)]
    wmask = [masks[s] if w is None else pil_affine(masks[s], w, True) for s, w in zip(src, warps)]
    wmask = [m[P.nearest_table(m.shape[0], out[0])][:, P.nearest_table(m.shape[1], out[1])] for m in wmask]
    u8, tg = P.apply_packed_numpy(blob, L, integer_stage=True, warp_layout=W)
    f32, tg2 = P.apply_packed_numpy(blob, L, warp_layout=W)
    assert np.array_equal(u8, np.stack(want)), "the integer stage differs from Pillow's warp then resize"
    assert f32.dtype == np.float32 and torch.equal(torch.from_numpy(f32), expected_images(want)), "the fp32 finish differs from the reference's"
    assert tg.dtype == np.int64 and np.array_equal(tg, tg2) and torch.equal(torch.from_numpy(tg), expected_targets(wmask)), "masks differ from Pillow's"
    # images warped, targets one per clip and unwarped; and the other way round
    blob, L, W = P.pack_batch(images, masks, out_size=out, repeat=T, target_map=[0, 1], warps=warps)
    u8b, tgb = P.apply_packed_numpy(blob, L, integer_stage=True, warp_layout=W)
    assert W.n_mask_warps == 0 and np.array_equal(u8b, u8) and np.array_equal(tgb, tg[[0, 3]])
    blob, L, W = P.pack_batch(images, masks, out_size=out, repeat=T, target_map=[0, 1], target_warps=[warps[1], warps[5]])
    u8c, tgc = P.apply_packed_numpy(blob, L, integer_stage=True, warp_layout=W)
    assert W.n_image_warps == 0 and np.array_equal(u8c[1], u8[0]) and np.array_equal(tgc, tg[[1, 5]])


# ================================================================================================ the augmenter
def test_neutral_parameters_are_the_identity_exactly():
    for size in SIZES + ((480, 640), (333, 500)):
        assert A.coefficients(size) == (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
    aug = A(rotate=(0, 0), translate=(0, 0), scale=(1, 1), shear=(0, 0), keep_first=False, seed=0)
    assert aug.draw([(37, 53)], 2) == [[(1.0, 0.0, 0.0, 0.0, 1.0, 0.0)] * 2]


def test_coefficients_invert_the_motion():
    rng = np.random.default_rng(2)
    for size in SIZES + ((480, 640),):
        for _ in range(10):
            p = dict(angle=rng.uniform(-30, 30), translate=tuple(rng.uniform(-0.2, 0.2, 2)), scale=rng.uniform(0.7, 1.5), shear=tuple(rng.uniform(-20, 20, 2)))
            c = A.coefficients(size, **p)
            inv = np.array([[c[0], c[1], c[2]], [c[3], c[4], c[5]], [0.0, 0.0, 1.0]])
            prod = A.motion(size, **p) @ inv
            scale = np.array([[1.0, 1.0, max(size)]] * 2 + [[1.0, 1.0, 1.0]])          # the translation column is in pixels
            assert np.abs((prod - np.eye(3)) / scale).max() < 1e-12, (size, p, prod)
    # the motion is what the docstring says: the centre goes to centre + translation
    M = A.motion((48, 64), 10.0, (0.1, -0.05), 1.2, (3.0, 2.0))
    assert np.allclose(M @ [32.0, 24.0, 1.0], [32.0 + 6.4, 24.0 - 2.4, 1.0], atol=1e-12)


def test_draws_are_seeded_resumable_and_shared():
    sizes = [(37, 53), (64, 48)]
    a, b = A(seed=42), A(seed=42)
    d1 = a.draw(sizes, 4)
    assert d1 == b.draw(sizes, 4) and d1 != A(seed=43).draw(sizes, 4)
    assert len(d1) == 2 and all(len(clip) == 4 and clip[0] is None and all(len(w) == 6 for w in clip[1:]) for clip in d1), "keep_first: frame 0 is None"
    assert all(w is not None for clip in A(keep_first=False, seed=1).draw(sizes, 3) for w in clip)
    state = a.state_dict()
    nxt = a.draw(sizes, 4)
    c = A(seed=7)
    c.load_state_dict(state)
    assert c.draw(sizes, 4) == nxt != d1, "state_dict round-trips mid-sequence"
    # the defaults are weak: every drawn motion stays within its ranges
    for clip in A(seed=5).draw([(480, 640)] * 8, 8):
        for w in clip[1:]:
            lin = np.linalg.inv(np.array([[w[0], w[1]], [w[3], w[4]]]))
            assert 0.9 < abs(np.linalg.det(lin)) ** 0.5 < 1.3
    with pytest.raises(ValueError, match="range"):
        A(rotate=(5, -5))
    with pytest.raises(ValueError, match="45"):
        A(shear=(-45, 45))


class _Step(_BatchInput, _ValidIndices):
    """the input-stage half of a TrainStep on the host: its image / target buffers, and a preprocessor that only records what it is given to stage"""

    def __init__(self, x, t, valid=None):
        self.x, self.t, self.valid_indices, self.staged = x, t, valid, []

    def _batch_preprocessor(self):
        return self

    def _stage(self, plan):
        self.staged.append(plan)


@pytest.fixture
def not_capturing(monkeypatch):
    """(stage_batch asks the runtime whether a capture is under way, which needs a device: here the answer is no)"""
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)


def test_step_harness_shares_one_transform_between_a_frame_and_its_mask(not_capturing):
    images, masks, _ = _batch()
    B, T = 2, 3
    step = _Step(torch.zeros(B, T, 3, 32, 40), torch.zeros(B * T, 32, 40, dtype=torch.int64))
    step.stage_batch(images, masks, repeat=T, augment=A(seed=9))
    plan = step.staged[-1]
    want = [w for clip in A(seed=9).draw([a.shape[:2] for a in images], T) for w in clip]
    assert plan.warp_layout.n_image_warps == plan.warp_layout.n_mask_warps == 4
    assert [tuple(w) for w in plan.witems["a"]] == [w for w in want if w is not None] == [tuple(w) for w in plan.wtitems["a"]], "an image and its mask share coefficients"
    # one mask per clip: that of the annotated frame, which set_valid_indices names
    step = _Step(torch.zeros(B, T, 3, 32, 40), torch.zeros(B, 32, 40, dtype=torch.int64), valid=torch.zeros(B, dtype=torch.int32))
    aug = A(seed=9)
    with pytest.raises(ValueError, match="set_valid_indices"):
        step.stage_batch(images, masks, repeat=T, augment=aug)
    assert aug.draw([(5, 5)], 2) == A(seed=9).draw([(5, 5)], 2), "a refused batch draws nothing"
    step.set_valid_indices([2, 0], T)
    step.stage_batch(images, masks, repeat=T, augment=A(seed=9))
    plan = step.staged[-1]
    assert plan.warp_layout.n_mask_warps == 1 and tuple(plan.wtitems["a"][0]) == want[2] and plan.layout.n_targets == 2


# ================================================================================================ refusals
def test_refusals_come_before_any_write(monkeypatch, not_capturing):
    images, masks, out = _batch()
    ok = [None, (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)]
    with pytest.raises(ValueError, match="warps has 3 entries for 2"):
        P.pack_batch(images, masks, out_size=out, warps=[None] * 3)
    with pytest.raises(ValueError, match="target_warps has 1 entries for 2"):
        P.pack_batch(images, masks, out_size=out, target_warps=[None])
    with pytest.raises(ValueError, match="target_warps without targets"):
        P.pack_batch(images, out_size=out, target_warps=ok)
    with pytest.raises(ValueError, match="six coefficients"):
        P.pack_batch(images, out_size=out, warps=[None, (1.0, 0.0, 0.0)])
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite"):
            P.pack_batch(images, masks, out_size=out, warps=[None, (1.0, 0.0, bad, 0.0, 1.0, 0.0)])
    with pytest.raises(ValueError, match="overflow int32"):
        P.pack_batch(images, masks, out_size=out, target_warps=[None, (1.0, 0.01, 1e6, 0.0, 1.0, 0.0)])
    with pytest.raises(TypeError, match=r"FramePreprocessor\.images"):
        P.pack_batch([_Cuda(), _Cuda()], out_size=out, warps=ok)

    # the step harness: nothing reaches the preprocessor
    B, T = 2, 3
    step = _Step(torch.zeros(B, T, 3, 32, 40), torch.zeros(B * T, 32, 40, dtype=torch.int64))
    aug = A(seed=1)
    with pytest.raises(ValueError, match="repeat=T"):
        step.stage_batch(images * 3, masks * 3, augment=aug)
    with pytest.raises(ValueError, match="repeat=T"):
        _Step(torch.zeros(B * T, 3, 32, 40), torch.zeros(B * T, 32, 40, dtype=torch.int64)).stage_batch(images, masks, repeat=T, augment=aug)
    with pytest.raises(ValueError, match="frames"):
        step.stage_batch(images[:1], masks[:1], repeat=T, augment=aug)
    with pytest.raises(ValueError, match="target masks"):
        step.stage_batch(images, masks * 2, repeat=T, augment=aug)
    with pytest.raises(TypeError, match=r"FramePreprocessor\.images"):
        step.stage_batch([_Cuda(), _Cuda()], masks, repeat=T, augment=aug)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="outside the graph capture"):
        step.stage_batch(images, masks, repeat=T, augment=aug)
    with pytest.raises(RuntimeError, match="outside the graph capture"):
        step.load_batch(images, masks, repeat=T, augment=aug)
    pp = P.BatchPreprocessor(out)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)          # (the preprocessor asks about a capture only where there is a GPU)
    for call in (pp.stage, pp.batch):
        with pytest.raises(RuntimeError, match="outside the graph capture"):
            call(images, masks, repeat=T, warps=[None] * 6)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    assert step.staged == [] and aug.draw([(9, 9)], 2) == A(seed=1).draw([(9, 9)], 2), "nothing was staged, nothing was drawn"


class _Cuda(torch.Tensor):
    """a tensor that says it lives on the GPU: what the CUDA-input refusal looks at, on a machine without one"""
    @staticmethod
    def __new__(cls):
        return torch.Tensor._make_subclass(cls, torch.zeros(8, 8, 3, dtype=torch.uint8))

    @property
    def is_cuda(self):
        return True


def test_struct_mirror_has_the_size_of_the_header():
    import ctypes
    import os
    import re
    from lavt_hip import _capi as K
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "lavt_hip.h")).read()
    body = re.search(r"typedef struct lavt_pp_warp \{(.*?)\} lavt_pp_warp_t;", header, re.S).group(1)
    size, names = 0, []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, rest = decl.split(None, 1)
            width = {"int64_t": 8, "int32_t": 4, "double": 8}[ctype]
            for part in rest.split(","):
                m = re.fullmatch(r"(\w+)(?:\[(\d+)\])?", part.strip())
                names.append(m.group(1))
                assert size % width == 0, "a member that the compiler would pad"
                size += width * int(m.group(2) or 1)
    assert size == 128 == ctypes.sizeof(K.PPWarp) == P.WARP_DTYPE.itemsize
    assert names == [f[0] for f in K.PPWarp._fields_] == list(P.WARP_DTYPE.names)
    for name, _ in K.PPWarp._fields_:
        assert getattr(K.PPWarp, name).offset == P.WARP_DTYPE.fields[name][1], name
    assert (K.WARP_FIXED, K.WARP_TABLES) == (P.WARP_FIXED, P.WARP_TABLES) == (0, 1)
    assert re.search(r"#define LAVT_WARP_FIXED 0\b", header) and re.search(r"#define LAVT_WARP_TABLES 1\b", header)
    for name, arity in (("lavt_affine_u8_batch", 8), ("lavt_affine_nearest_u8_batch", 11)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
        assert m and len(m.group(1).split(",")) == arity == len(K._PROTOTYPES[name]) and name in K.EXPORTED
    assert K.lib.lavt_abi_version() == K.EXPECTED_ABI == 7, "new symbols only, under the current ABI version"
