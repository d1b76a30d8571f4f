"""Shared by test_meters_host.py and test_gpu_meters.py: the fixture written by tests/golden/make_train_meter_golden.py (the reference's own
SmoothedValue / MetricLogger / IoU on fixed sequences), loaded once, and the field-for-field comparison of two meter snapshots."""
import functools
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PROPS = ("median", "avg", "global_avg", "max", "value")


@functools.lru_cache(maxsize=None)
def cases():
    """{case: {array name: array, 'strings': [str(MetricLogger) after every iteration]}}; never written"""
    z = np.load(os.path.join(GOLDEN, "train_meter_cases.npz"))
    strings = json.load(open(os.path.join(GOLDEN, "train_meter_cases.json")))
    out = {}
    for key in z.files:
        c, k = key.split("/")
        out.setdefault(c, {})[k] = z[key]
    for c in out:
        out[c]["strings"] = strings[c]
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same_block(got, want, skip=()):
    """every header word and every ring field of two lavt_hip.meters.Snapshot equal bit for bit (ring fields named in `skip` left out) -> list of differences"""
    diff = []
    if not np.array_equal(bits(got.header), bits(want.header)):
        diff += [f"header[{i}]: {got.header[i]!r} != {want.header[i]!r}" for i in range(len(want.header)) if bits(got.header)[i] != bits(want.header)[i]]
    for f in want.ring.dtype.names:
        if f not in skip and not np.array_equal(bits(got.ring[f]), bits(want.ring[f])):
            diff.append(f"ring.{f}: {got.ring[f].tolist()} != {want.ring[f].tolist()}")
    return diff
