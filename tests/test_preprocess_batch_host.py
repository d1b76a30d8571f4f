"""Host-side checks of the batched input stage (no GPU): lavt_hip.preprocess.pack_batch lays a batch of mixed-size sources out as one blob, and
apply_packed_numpy reads that blob the way the kernels of csrc/preprocess.hip do -- the descriptors and tables of the blob, its offsets, the integer
stage, the three fp32 operations.  Reference: PIL's results in tests/golden/preprocess_batch_cases.npz (generator beside it) and the cases a, b, c, e
of preprocess_cases.npz, which all go to 32 x 32 and form a fourth mixed batch.  Every comparison is exact."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from lavt_hip import preprocess as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = ("m", "n", "v", "abce")
MEAN_T, STD_T = torch.tensor(P.MEAN, dtype=torch.float32).view(-1, 1, 1), torch.tensor(P.STD, dtype=torch.float32).view(-1, 1, 1)


def load_batch(golden, name):
    """-> (sources, PIL's uint8 images, mask sources, PIL's masks, (Ho, Wo)): lists with one entry per source of the batch"""
    if name == "abce":
        g = golden("preprocess_cases")
        return ([g[f"{c}_src"][0] for c in name], [g[f"{c}_pil"][0] for c in name], [g[f"{c}_msrc"][0] for c in name], [g[f"{c}_mpil"][0] for c in name], (32, 32))
    g = golden("preprocess_batch_cases")
    idx = range(int(g[f"{name}_count"]))
    return ([g[f"{name}{i}_src"] for i in idx], [g[f"{name}{i}_pil"] for i in idx], [g[f"{name}{i}_msrc"] for i in idx], [g[f"{name}{i}_mpil"] for i in idx],
            tuple(int(v) for v in g[f"{name}_out"]))


def expected_images(pil_u8):
    """ToTensor + Normalize of the reference (transforms.py:83-87, 106-113) on PIL's uint8 frames, on the CPU, as tests/test_gpu_preprocess.py computes it"""
    t = torch.from_numpy(np.ascontiguousarray(np.stack(pil_u8))).permute(0, 3, 1, 2).to(torch.float32).div(255)
    return (t - MEAN_T) / STD_T


def expected_targets(mpil):
    return torch.from_numpy(np.stack(mpil).astype(np.int64))


def _check(blob, layout, pil, mpil, what):
    u8, tg = P.apply_packed_numpy(blob, layout, integer_stage=True)
    f32, tg2 = P.apply_packed_numpy(blob, layout)
    assert u8.shape == (len(pil),) + layout.out_size + (3,) and np.array_equal(u8, np.stack(pil)), f"{what}: the integer stage differs from PIL"
    assert f32.dtype == np.float32 and torch.equal(torch.from_numpy(f32), expected_images(pil)), f"{what}: the fp32 finish differs from the reference's"
    if mpil is None:
        assert tg is None and tg2 is None
    else:
        assert tg.dtype == np.int64 and np.array_equal(tg, tg2) and torch.equal(torch.from_numpy(tg), expected_targets(mpil)), f"{what}: masks differ from PIL"


@pytest.mark.parametrize("name", BATCHES)
def test_packed_batch_equals_pil(golden, name):
    src, pil, msrc, mpil, out = load_batch(golden, name)
    blob, L = P.pack_batch(src, msrc, out_size=out)
    assert blob.dtype == np.uint8 and blob.ndim == 1 and blob.size == L.nbytes and L.n_frames == L.n_targets == len(src) and L.out_size == out
    _check(blob, L, pil, mpil, f"batch {name}")
    blob, L = P.pack_batch(src, out_size=out)
    assert L.n_targets == 0 and L.mask_bytes == 0
    _check(blob, L, pil, None, f"batch {name} without targets")


def test_fixture_exercises_what_it_claims(golden):
    """batch m: ksize_x 5/3/3/7 and ksize_y 5/7/3/3 in one launch, three x tiles with a 2-pixel last one, an identity item; batch n: a one-row source"""
    src, _, _, _, out = load_batch(golden, "m")
    assert [P.resample_tables(s.shape[1], out[1])[0].shape[1] for s in src] == [5, 3, 3, 7]
    assert [P.resample_tables(s.shape[0], out[0])[0].shape[1] for s in src] == [5, 7, 3, 3]
    assert out[1] == 2 * 64 + 2 and out[0] % 16 != 0 and src[2].shape[:2] == out
    assert min(s.shape[0] for s in load_batch(golden, "n")[0]) == 1


def test_repeat_makes_clips(golden):
    src, pil, msrc, mpil, out = load_batch(golden, "v")
    blob, L = P.pack_batch(src, msrc, out_size=out, repeat=3)
    assert L.n_frames == L.n_targets == 6 and L.pixel_bytes == sum(s.size for s in src), "a repeated source is stored once"
    _check(blob, L, [pil[0]] * 3 + [pil[1]] * 3, [mpil[0]] * 3 + [mpil[1]] * 3, "repeat=3")
    # targets that are one per clip already (valid_indices) are kept one to one by an explicit target_map
    blob, L = P.pack_batch(src, msrc, out_size=out, repeat=3, target_map=[0, 1])
    assert (L.n_frames, L.n_targets) == (6, 2)
    _check(blob, L, [pil[0]] * 3 + [pil[1]] * 3, mpil, "repeat=3, one target per clip")
    with pytest.raises(ValueError, match="repeat"):
        P.pack_batch(src, out_size=out, repeat=3, frame_map=[0, 1])


def test_permuted_map_with_a_source_used_twice_and_fewer_targets(golden):
    src, pil, msrc, mpil, out = load_batch(golden, "n")
    fm, tm = [3, 0, 4, 0, 2, 1], [1, 1, 0]
    blob, L = P.pack_batch(src, msrc[:2], out_size=out, frame_map=fm, target_map=tm)
    assert (L.n_frames, L.n_targets) == (6, 3) and L.mask_bytes == msrc[0].size + msrc[1].size
    _check(blob, L, [pil[i] for i in fm], [mpil[i] for i in tm], "permuted maps")
    items = blob[L.items_off:L.items_off + 64 * L.n_frames].view(P.ITEM_DTYPE)
    assert items["src_off"][1] == items["src_off"][3] == 0 and items["src_off"][0] == sum(s.size for s in src[:3])
    with pytest.raises(ValueError, match="frame_map"):
        P.pack_batch(src, out_size=out, frame_map=[0, 5])
    with pytest.raises(ValueError, match="target_map"):
        P.pack_batch(src, msrc[:2], out_size=out, target_map=[2])
    with pytest.raises(ValueError, match="target_map without targets"):
        P.pack_batch(src, out_size=out, target_map=[0])


@pytest.mark.parametrize("name", BATCHES)
def test_sections_are_aligned_and_ordered(golden, name):
    src, _, msrc, _, out = load_batch(golden, name)
    _, L = P.pack_batch(src, msrc, out_size=out)
    offs = [L.items_off, L.titems_off, L.tables_off, L.pixels_off, L.masks_off, L.nbytes]
    assert all(o % 16 == 0 for o in offs) and offs == sorted(offs) and offs[0] == 0
    ends = [L.items_off + 64 * L.n_frames, L.titems_off + 64 * L.n_targets, L.tables_off + 4 * L.table_elems, L.pixels_off + L.pixel_bytes, L.masks_off + L.mask_bytes]
    assert all(e <= nxt and nxt - e < 16 for e, nxt in zip(ends, offs[1:])), "sections overlap or leave more than the alignment gap"
    assert L.pixel_bytes == sum(s.size for s in src) and L.mask_bytes == sum(m.size for m in msrc), "sources are packed back to back"
    if name == "abce":          # 37 x 53 first: every later source starts at an odd byte
        blob, _ = P.pack_batch(src, msrc, out_size=out)
        for section, n, field in ((L.items_off, L.n_frames, "src_off"), (L.titems_off, L.n_targets, "mask_off")):
            assert any(int(o) % 2 for o in blob[section:section + 64 * n].view(P.ITEM_DTYPE)[field]), "odd offsets are normal: nothing pads a source"


def test_tables_of_equal_size_pairs_are_stored_once(golden):
    src, _, msrc, _, out = load_batch(golden, "n")          # (48,64) (64,48) (43,64) (30,30) (1,5) -> 32 x 32
    blob, L = P.pack_batch(src, msrc, out_size=out)
    keys = [k for k, _ in L.tables]
    assert len(keys) == len(set(keys))
    sizes = {s for a in src for s in a.shape[:2]}          # 48, 64, 43, 30, 1, 5: x and y share a table when size pairs agree
    assert sorted(keys) == sorted([("resample", s, 32) for s in sizes] + [("nearest", s, 32) for s in sizes])
    want = sum(P.resample_tables(s, 32)[0].size + P.resample_tables(s, 32)[1].size + P.nearest_table(s, 32).size for s in sizes)
    assert L.table_elems == want
    items = blob[L.items_off:L.items_off + 64 * L.n_frames].view(P.ITEM_DTYPE)
    assert items["coef_x"][0] == items["coef_y"][1] == items["coef_x"][2] and items["bounds_y"][0] == items["bounds_x"][1]          # 64 -> 32 and 48 -> 32
    # the stored tables are the cached host tables, byte for byte
    tables = blob[L.tables_off:L.tables_off + 4 * L.table_elems].view(np.int32)
    coef, bounds = P.resample_tables(64, 32)
    assert np.array_equal(tables[items["coef_x"][0]:items["coef_x"][0] + coef.size], coef.reshape(-1)) and items["ksize_x"][0] == coef.shape[1]
    assert np.array_equal(tables[items["bounds_x"][0]:items["bounds_x"][0] + bounds.size], bounds.reshape(-1))


def test_input_forms_and_refusals(golden):
    Image = pytest.importorskip("PIL.Image")
    src, pil, msrc, mpil, out = load_batch(golden, "v")
    a, _ = P.pack_batch(src, msrc, out_size=out)
    b, _ = P.pack_batch([Image.fromarray(s, "RGB") for s in src], [Image.fromarray(m, "L") for m in msrc], out_size=out)
    c, _ = P.pack_batch([torch.from_numpy(s) for s in src], tuple(msrc), out_size=out)
    assert np.array_equal(a, b) and np.array_equal(a, c)
    with pytest.raises(TypeError, match="uint8"):
        P.pack_batch([s.astype(np.float32) for s in src], out_size=out)
    with pytest.raises(ValueError, match="RGB"):
        P.pack_batch(msrc, out_size=out)
    with pytest.raises(ValueError, match="no images"):
        P.pack_batch([], out_size=out)
    with pytest.raises(ValueError, match="out_size"):
        P.pack_batch(src, out_size=(0, 4))


def test_struct_mirror_has_the_size_of_the_header():
    from lavt_hip import _capi as K
    header = open(os.path.join(ROOT, "include", "lavt_hip.h")).read()
    body = re.search(r"typedef struct lavt_pp_item \{(.*?)\} lavt_pp_item_t;", header, re.S).group(1)
    size, names = 0, []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, rest = decl.split(None, 1)
            width = {"int64_t": 8, "int32_t": 4}[ctype]
            for part in rest.split(","):
                names.append(part.strip())
                assert size % width == 0, "a member that the compiler would pad"
                size += width
    assert size == 64 == ctypes.sizeof(K.PPItem) == P.ITEM_DTYPE.itemsize
    assert names == [f[0] for f in K.PPItem._fields_] == list(P.ITEM_DTYPE.names)
    for name, _ in K.PPItem._fields_:
        assert getattr(K.PPItem, name).offset == P.ITEM_DTYPE.fields[name][1], name
    src = open(os.path.join(ROOT, "lavt-rs_amd", "csrc", "preprocess.hip")).read()
    assert re.search(r"static_assert\(sizeof\(lavt_pp_item_t\) == 64", src)


def test_new_symbols_are_bound_under_abi_7():
    from lavt_hip import _capi as K
    from lavt_hip import ops
    C = ctypes
    assert K._PROTOTYPES["lavt_resize_norm_u8_batch"] == [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32,
                                                          C.c_int32] + [C.c_float] * 6 + [C.c_void_p]
    assert K._PROTOTYPES["lavt_resize_nearest_u8_batch"] == [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32,
                                                             C.c_int32, C.c_void_p]
    for name in ("lavt_resize_norm_u8_batch", "lavt_resize_nearest_u8_batch"):
        assert name in K.EXPORTED and hasattr(K.lib, name)
    assert K.lib.lavt_abi_version() == K.EXPECTED_ABI == 7
    assert callable(ops.resize_normalize_u8_batch) and callable(ops.resize_nearest_u8_batch)


def test_entries_refuse_bad_descriptors_without_a_gpu(golden):
    """the argument checks run on the host copy before any launch: they can be exercised with host pointers standing in for the device ones"""
    from lavt_hip import _capi as K
    src, _, msrc, _, out = load_batch(golden, "v")
    blob, L = P.pack_batch(src, msrc, out_size=out)

    def norm(b, n=L.n_frames):
        p = b.ctypes.data
        return K.lib.lavt_resize_norm_u8_batch(p + L.items_off, p + L.items_off, n, p + L.tables_off, p + L.tables_off, L.table_elems, p + L.pixels_off, L.pixel_bytes, p, *out,
                                               *P.MEAN, *P.STD, None)

    def near(b):
        p = b.ctypes.data
        return K.lib.lavt_resize_nearest_u8_batch(p + L.titems_off, p + L.titems_off, L.n_targets, p + L.tables_off, p + L.tables_off, L.table_elems, p + L.masks_off, L.mask_bytes,
                                                  p, *out, None)

    def edited(section, field, value, item=1):
        b = blob.copy()
        b[section:section + 64 * 2].view(P.ITEM_DTYPE)[field][item] = value
        return b

    for bad, word in ((edited(L.items_off, "src_off", L.pixel_bytes - 8), b"outside"), (edited(L.items_off, "src_off", -1), b"outside"), (edited(L.items_off, "ksize_y", 0), b"positive"),
                      (edited(L.items_off, "coef_x", L.table_elems - 3), b"table"), (edited(L.items_off, "bounds_y", -4), b"table"), (edited(L.items_off, "Hs", 39), b"row range"),
                      (edited(L.items_off, "Ws", 23), b"column range")):
        assert norm(bad) == -22 and word in K.lib.lavt_last_error(), K.lib.lavt_last_error()
    assert norm(blob, 0) == -22 and norm(blob, 65536) == -22
    swapped = blob.copy()          # bounds_y that is not monotone: two rows of the y table of item 0 exchanged
    it = swapped[L.items_off:L.items_off + 64].view(P.ITEM_DTYPE)[0]
    by = swapped[L.tables_off:L.tables_off + 4 * L.table_elems].view(np.int32)[int(it["bounds_y"]):int(it["bounds_y"]) + 2 * out[0]].reshape(-1, 2)
    by[[2, 9]] = by[[9, 2]]
    assert norm(swapped) == -22 and b"row range" in K.lib.lavt_last_error()
    for bad, word in ((edited(L.titems_off, "mask_off", L.mask_bytes), b"outside"), (edited(L.titems_off, "idx_x", L.table_elems), b"index table"), (edited(L.titems_off, "Hs", 20), b"row of")):
        assert near(bad) == -22 and word in K.lib.lavt_last_error(), K.lib.lavt_last_error()


def test_collate_raw_keeps_ragged_lists(golden):
    src, _, msrc, _, _ = load_batch(golden, "n")
    samples = [(s, m, torch.full((1, 20), i), torch.ones(1, 20, dtype=torch.int64)) for i, (s, m) in enumerate(zip(src, msrc))]
    images, masks, emb, att = P.collate_raw(samples)
    assert isinstance(images, list) and isinstance(masks, list) and len(images) == len(masks) == 5
    assert all(a.dtype == np.uint8 and np.array_equal(a, s) for a, s in zip(images, src)) and all(np.array_equal(a, m) for a, m in zip(masks, msrc))
    assert tuple(emb.shape) == (5, 1, 20) and emb[3, 0, 0] == 3 and tuple(att.shape) == (5, 1, 20)
    assert len(P.collate_raw([s[:2] for s in samples])) == 2
    blob, L = P.pack_batch(images, masks, out_size=(32, 32))
    assert L.n_frames == 5
    # as the collate_fn of a DataLoader
    dl = torch.utils.data.DataLoader(samples, batch_size=3, collate_fn=P.collate_raw)
    first = next(iter(dl))
    assert [a.shape for a in first[0]] == [s.shape for s in src[:3]] and tuple(first[2].shape) == (3, 1, 20)


def test_cuda_input_is_refused_by_type():
    class FakeCuda(torch.Tensor):
        @property
        def is_cuda(self):
            return True
    t = torch.zeros(4, 4, 3, dtype=torch.uint8).as_subclass(FakeCuda)
    with pytest.raises(TypeError, match=r"FramePreprocessor\.images"):
        P.pack_batch([t], out_size=(2, 2))
    with pytest.raises(TypeError, match=r"FramePreprocessor\.images"):
        P.pack_batch(t, out_size=(2, 2))
