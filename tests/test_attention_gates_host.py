"""Mutation self-test of the window-attention gates (tests/attn_pairs.py), CPU only.  The GPU tests (test_gpu_attention_pairs.py) compare the kernels with
an fp64 reference through these gate functions; here the "kernel" is the same reference with one fault injected, its P, stored output and dS rounded to
bf16 as a correct bf16 kernel's are.  Every fault must fail at least one gate, and the unmutated rounded reference must pass all of them.

Faults: (a) the corner offsets of the table read / bin into the neighbouring entry; (b) one masked pair of the last window is unmasked; (c) one padded
key column has bias 0 instead of -1e30 (one more visible zero key); (d) one (i, j) pair's dS is binned into r + 1."""
import functools
from types import SimpleNamespace

import pytest
import torch

import attn_pairs as AP
from test_gpu_ops import rnd

CASES = {"w7": ((1, 14, 14), (1, 7, 7)), "w12": ((1, 24, 24), (1, 12, 12)), "video147": ((3, 14, 14), (8, 7, 7))}          # all shifted
HEADS, DIFFUSE_HEADS = 16, 4
BF = torch.bfloat16
K = max(AP.ENTRY_K.values())          # the loosest route's factor: a fault caught at this gate is caught on every route


def _store(x):
    return x.to(torch.float32).to(BF)


@functools.lru_cache(maxsize=None)
def _setup(name):
    cs = AP.make_case(*CASES[name], True)
    tables, rows = AP.probe_tables(cs, HEADS)
    assert len(tables) == 1
    s = SimpleNamespace(cs=cs, table=tables[0], rows=rows[0], pad=AP.padding_table(cs, HEADS), qkv=AP.probe_qkv(cs, HEADS), counts=AP.pair_counts(cs))
    s.y, s.sel = AP.reference(cs, s.qkv, s.table, with_top=True)
    s.y_pad = AP.reference(cs, s.qkv, s.pad)
    s.dq = rnd(cs.Bw * cs.N, 3 * DIFFUSE_HEADS * 32, seed=1).to(BF).float()
    s.dt = rnd(cs.R, DIFFUSE_HEADS, seed=2, scale=0.5).to(BF).float()
    s.go = rnd(cs.Bw * cs.N, DIFFUSE_HEADS * 32, seed=99).to(BF).float()
    s.ref = AP.reference(cs, s.dq, s.dt, s.go)
    s.floor = AP.per_entry_error(AP.reference(cs, s.dq, s.dt, s.go, round_bf16=True)[2], s.ref[2], s.counts)
    return s


def _mutations(s):
    cs = s.cs
    mask = cs.mask.clone()
    # (b): a masked pair of the last window at a probed offset -- a pair at an unprobed offset is outside what the probe can see, and the diffuse
    # gates see one pair at 1e-2 x max (which is why the probe exists)
    at = torch.stack([cs.idx == r for r in s.rows]).any(0) & (cs.mask[-1] < -1)
    i, j = torch.nonzero(at)[0].tolist()
    mask[-1, i, j] = 0.0
    return {"a": dict(idx=AP.idx_corners_to_neighbour(cs)), "b": dict(mask=mask), "c": dict(pad_key=True), "d": dict(bin_idx=AP.idx_one_pair_shifted(cs))}


def _failed_gates(s, **fault):
    """names of the gates that the reference with `fault` injected fails"""
    cs = s.cs
    fwd = {k: v for k, v in fault.items() if k != "bin_idx"}
    y = _store(AP.reference(cs, s.qkv, s.table, round_bf16=True, **fwd))
    y_pad = _store(AP.reference(cs, s.qkv, s.pad, round_bf16=True, **fwd))
    dy, dqkv, dtable = AP.reference(cs, s.dq, s.dt, s.go, round_bf16=True, **fault)
    gates = {
        "probe forward": lambda: AP.gate_forward(y, s.y, BF, "probe"),
        "probe selection": lambda: AP.gate_selection(cs, y, s.qkv, HEADS, s.sel, "probe"),
        "padding probe": lambda: AP.gate_forward(y_pad, s.y_pad, BF, "padding probe"),
        "diffuse forward": lambda: AP.gate_forward(_store(dy), s.ref[0], BF, "diffuse"),
        "diffuse backward": lambda: AP.gate_backward(_store(dqkv), dtable, s.ref, BF, "diffuse"),
        "per-entry dtable": lambda: AP.gate_per_entry(dtable, s.ref[2], s.counts, BF, s.floor, K, "diffuse"),
    }
    failed = []
    for name, gate in gates.items():
        try:
            gate()
        except AssertionError:
            failed.append(name)
    return failed


@pytest.mark.parametrize("name", list(CASES))
def test_rounded_reference_passes_every_gate(name):
    assert _failed_gates(_setup(name)) == []


@pytest.mark.parametrize("fault", ["a", "b", "c", "d"])
@pytest.mark.parametrize("name", list(CASES))
def test_every_fault_fails_a_gate(name, fault):
    s = _setup(name)
    failed = _failed_gates(s, **_mutations(s)[fault])
    print(f"\n[{name} fault ({fault})] fails: {failed}")
    assert failed, f"fault ({fault}) passes every gate on {name}"
    # what each device is for: the probe sees the forward faults pair by pair, the per-entry metric the binning faults
    if fault in "ab":
        assert "probe forward" in failed
    if fault == "a":
        assert "probe selection" in failed and "per-entry dtable" in failed
    if fault == "c":
        assert "padding probe" in failed
    if fault == "d":
        assert failed == ["per-entry dtable"]


@pytest.mark.parametrize("name", list(CASES))
def test_probes_are_not_vacuous(name):
    s = _setup(name)
    AP.assert_probe_bites(s.cs, s.rows, s.sel, name)
    # every probed offset is a distinct reachable table row; corners, centre and centre +-1 lead the list
    assert len(set(s.rows)) == HEADS and all(int(s.counts[r]) > 0 for r in s.rows)
    naxes = sum(w > 1 for w in s.cs.win)
    assert [int(s.counts[r]) for r in s.rows[:2 ** naxes]] == [1] * 2 ** naxes
    assert int(s.counts[s.rows[2 ** naxes]]) == s.cs.N


@pytest.mark.parametrize("name", list(CASES))
def test_per_entry_gate_is_a_third_of_the_binning_faults(name):
    """the hard condition on the bf16 per-entry gate K x floor: at most one third of the smallest per-entry error of the faults that act on the
    table-gradient binning, (a) and (d).  (Faults (b) and (c) touch the forward; the probes carry them.)"""
    s = _setup(name)
    m = _mutations(s)
    errs = {f: AP.per_entry_error(AP.reference(s.cs, s.dq, s.dt, s.go, **m[f])[2], s.ref[2], s.counts) for f in "ad"}
    print(f"\n[{name}] per-entry floor {s.floor:.3e}, gate {K * s.floor:.3e}, faults {errs}")
    assert 5e-4 < s.floor < 6e-3, s.floor          # bf16 rounding of P and dS: 2^-9 per term
    assert K * s.floor <= min(errs.values()) / 3


def test_reference_matches_autograd():
    """the hand-written fp64 backward of attn_pairs.reference against autograd of the statement test_window_attention uses"""
    s = _setup("w7")
    cs = s.cs
    q = s.dq.double().requires_grad_(True)
    t = s.dt.double().requires_grad_(True)
    qq, k, v = q.view(cs.Bw, cs.N, 3, DIFFUSE_HEADS, 32).permute(2, 0, 3, 1, 4)
    a = (qq * 32 ** -0.5) @ k.transpose(-1, -2) + t[cs.idx.reshape(-1)].view(cs.N, cs.N, DIFFUSE_HEADS).permute(2, 0, 1)[None]
    a = (a.view(2, cs.nW, DIFFUSE_HEADS, cs.N, cs.N) + cs.mask[None, :, None]).view(cs.Bw, DIFFUSE_HEADS, cs.N, cs.N)
    y = (a.softmax(-1) @ v).transpose(1, 2).reshape(cs.Bw * cs.N, DIFFUSE_HEADS * 32)
    y.backward(s.go.double())
    for got, ref in zip(s.ref, (y.detach(), q.grad, t.grad)):
        assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
