"""The contract of lavt_gather_samples_bwd (include/lavt_hip.h), restated in torch on the CPU for tests/test_pair_train_host.py and
tests/test_gpu_pair_train.py:

    dx[b] = sum over {j : sel[j] == b} of dy[j]      ascending j, fp32 adds from +0.0, ONE rounding to the element type at the end;
    an image nobody names gets zeros; an entry of sel outside [0, B) contributes nothing."""
import torch


def gather_bwd_sequential(dy, sel, B):
    """dy: CPU tensor [nsel, ...] (fp32 or bf16), sel: host integers -> dx [B, ...] of dy's dtype, the kernel's summation order literally"""
    acc = torch.zeros((B,) + tuple(dy.shape[1:]), dtype=torch.float32)
    for j, b in enumerate(int(v) for v in sel):
        if 0 <= b < B:
            acc[b] = acc[b] + dy[j].float()          # one fp32 add per slot, in slot order
    return acc.to(dy.dtype)                          # round-to-nearest-even, once


def gather_bwd_index_add(dy, sel, B):
    """the same sum by torch.index_add_ in fp64 over the in-range entries -> fp64 [B, ...]"""
    live = [j for j, b in enumerate(int(v) for v in sel) if 0 <= b < B]
    out = torch.zeros((B,) + tuple(dy.shape[1:]), dtype=torch.float64)
    if live:
        out.index_add_(0, torch.tensor([int(sel[j]) for j in live], dtype=torch.int64), dy[live].double())
    return out


def bounded_integer_samples(seed, sel, B, per, dtype, bound=248):
    """integer data in [-8, 8] for MANY slots per image: a value that would carry an image's running sum past +-bound has its sign flipped, so every
    partial sum is an integer of magnitude <= 248 -- exact in fp32 and, as an integer below 2^8, in bf16"""
    import numpy as np
    rng = np.random.default_rng(seed)
    v = rng.integers(-8, 9, size=(len(sel), per)).astype(np.int64)
    run = np.zeros((B, per), dtype=np.int64)
    for j, b in enumerate(sel):
        if 0 <= b < B:
            flip = np.abs(run[b] + v[j]) > bound
            v[j] = np.where(flip, -v[j], v[j])
            run[b] += v[j]
    return torch.from_numpy(v).to(dtype)


def integer_samples(seed, nsel, per, dtype):
    """integer-valued data in [-8, 8]: every partial sum of up to 2^13 slots is an integer below 2^16, exact in fp32; bf16 holds integers up to 256
    exactly, so with at most 32 slots per image the rounded result is exact too"""
    g = torch.Generator("cpu").manual_seed(seed)
    return torch.randint(-8, 9, (nsel, per), generator=g).to(dtype)
