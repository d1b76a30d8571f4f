"""The reference's training-log counts, restated literally (train.py:64-76 behind lib/_utils.py:21), and the inputs the I / U tests share.

    output = F.interpolate(logits, (Ho, Wo), mode="bilinear", align_corners=True);  pred = output.argmax(1)
    I = sum(pred * gt);  U = sum(pred + gt) - I                                       -- pooled over the batch

Everything here runs on the CPU; tests/test_train_iu_host.py checks the cases without a GPU, tests/test_gpu_train_iu.py checks lavt_upsample_iu
against them.  Two kinds of cases:

EXACT: logits are randint(-16, 17) / 8 (multiples of 1/8 in [-2, 2]: representable in bf16) and the geometry has a dyadic scale (1/4 or the
identity), so every interpolation weight is a multiple of 1/4, every product and partial sum a multiple of 1/128 below 2^3 -- exact in fp32 in any
evaluation order, with or without fused multiply-adds.  Sample 0 carries a planted block of equal logits (exact ties: argmax picks class 0), the last
sample has class-1 logits = class-0 logits - 1 (an all-background prediction) and an all-zero target (I = U = 0).

MARGIN: a non-dyadic geometry with x = (randn * 2).bfloat16().float() from a seeded generator.  The smallest fp64 |up1 - up0| over all pixels is
asserted >= 1e-4 by the tests as a precondition on their inputs; fp32 interpolation error at these magnitudes is about 1e-6, so the counts of a
correct kernel are exactly the restatement's.
"""
import functools

import torch
import torch.nn.functional as F

# name -> (B, Hi, Wi, Ho, Wo)
EXACT_GEOMETRIES = {"q_3x5x9_17x33": (3, 5, 9, 17, 33), "q_2x4x3_13x9": (2, 4, 3, 13, 9), "id_2x10x9": (2, 10, 9, 10, 9)}
# name -> ((B, Hi, Wi, Ho, Wo), seed)
MARGIN_GEOMETRIES = {"m_2x7x5_23x18": ((2, 7, 5, 23, 18), 0), "m_2x30x30_120x120": ((2, 30, 30, 120, 120), 1)}
MIN_MARGIN = 1e-4


def upsampled(logits, Ho, Wo, dtype=torch.float64):
    """logits [B, 2, Hi, Wi] -> [B, 2, Ho, Wo] in `dtype` on the CPU (lib/_utils.py:21)"""
    return F.interpolate(logits.to(dtype), size=(Ho, Wo), mode="bilinear", align_corners=True)


def train_iu(logits, target, sel=None, dtype=torch.float64):
    """train.py:64-76 -> (I, U) as Python integers.  logits: [B, 2, Hi, Wi] (NCHW, any float dtype), target: int64 [n, Ho, Wo] in {0, 1}.
    sel: the flat frame numbers of train.py:283 -- `index_select(logits, 0, sel)` first; an entry outside [0, B) drops that sample (and its target)."""
    B = logits.shape[0]
    if sel is not None:
        sel = [int(s) for s in sel]
        keep = [j for j, s in enumerate(sel) if 0 <= s < B]
        if not keep:
            return 0, 0
        logits = torch.index_select(logits, 0, torch.tensor([sel[j] for j in keep]))
        target = torch.index_select(target, 0, torch.tensor(keep))
    assert logits.shape[0] == target.shape[0]
    out = upsampled(logits, int(target.shape[-2]), int(target.shape[-1]), dtype)
    pred = out.argmax(1)
    gt = target
    inter = torch.sum(torch.mul(pred, gt))
    union = torch.sum(torch.add(pred, gt)) - inter
    return int(inter), int(union)


def margin(logits, Ho, Wo):
    """the smallest fp64 |up1 - up0| over all pixels"""
    out = upsampled(logits, Ho, Wo)
    return float((out[:, 1] - out[:, 0]).abs().min())


def ties(logits, Ho, Wo):
    """pixels whose two upsampled logits are equal in fp64"""
    out = upsampled(logits, Ho, Wo)
    return int((out[:, 1] == out[:, 0]).sum())


@functools.lru_cache(maxsize=None)
def exact_case(name):
    """-> (logits fp32 [B, 2, Hi, Wi], target int64 [B, Ho, Wo]); do not write into them"""
    B, Hi, Wi, Ho, Wo = EXACT_GEOMETRIES[name]
    g = torch.Generator().manual_seed(1000 + sorted(EXACT_GEOMETRIES).index(name))
    logits = torch.randint(-16, 17, (B, 2, Hi, Wi), generator=g).float() / 8
    target = torch.randint(0, 2, (B, Ho, Wo), generator=g, dtype=torch.int64)
    # a block of equal logits in sample 0: the upsampled pixels inside it are exact ties
    h, w = max(2, Hi // 2), max(2, Wi // 2)
    logits[0, 1, :h, :w] = logits[0, 0, :h, :w]
    # the last sample predicts background everywhere and has no foreground label: I = U = 0
    logits[B - 1, 1] = logits[B - 1, 0] - 1
    target[B - 1] = 0
    return logits, target


@functools.lru_cache(maxsize=None)
def margin_case(name):
    """-> (logits fp32 [B, 2, Hi, Wi] holding bf16-representable values, target int64 [B, Ho, Wo]); do not write into them"""
    (B, Hi, Wi, Ho, Wo), seed = MARGIN_GEOMETRIES[name]
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(B, 2, Hi, Wi, generator=g) * 2).bfloat16().float()
    target = torch.randint(0, 2, (B, Ho, Wo), generator=g, dtype=torch.int64)
    return logits, target


def all_cases():
    """-> [(name, logits, target)] of every exact and margin case"""
    return [(n,) + exact_case(n) for n in EXACT_GEOMETRIES] + [(n,) + margin_case(n) for n in MARGIN_GEOMETRIES]


def nhwc_rows(logits, dtype=torch.float32):
    """[B, 2, Hi, Wi] -> the NHWC rows [B*Hi*Wi, 2] the C ABI reads, in `dtype`"""
    B, C, Hi, Wi = logits.shape
    return logits.permute(0, 2, 3, 1).reshape(B * Hi * Wi, C).contiguous().to(dtype)
