"""Every result bit of the fused optimizer against tests/golden/optim_bits.json, recorded on the MI355X from the commit named in the file by
tests/golden/make_optim_bits_golden.py: the eight <guard, AMSGrad, EMA> updates over five steps (clip, a skipped step, a held step), both ticks, the
norm's two passes, the per-tensor sums, the fold of gradient accumulation, the swap.  tests/optim_bits_cases.py holds the cases and runs them; the
comparison is equality of sha256 digests of raw bytes -- no tolerance, and a difference names the case, the step and the stream."""
import functools
import json
import os

import pytest

import optim_bits_cases as C

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "optim_bits.json")


@functools.lru_cache(maxsize=None)
def _recorded():
    return json.load(open(GOLDEN))


def test_the_fixture_covers_every_case():
    assert list(_recorded()["cases"]) == C.CASES and len(C.CASES) == 11
    assert all(len(v) > 0 for v in _recorded()["cases"].values())


@pytest.mark.parametrize("name", C.CASES)
def test_every_bit_is_the_recorded_one(name):
    rec = _recorded()
    want, got = rec["cases"][name], C.run_case(name)
    assert list(got) == list(want), "the case writes other streams than the recorded run"
    differ = [k for k in want if got[k] != want[k]]
    assert not differ, f"{name}: {len(differ)} of {len(want)} streams differ from {rec['parent']} ({rec['hipcc']}), first: {differ[:6]}"
