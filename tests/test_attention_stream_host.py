"""Host-side checks of the streaming window-attention entry points (csrc/attention_stream.hip): declared, bound, exported, and their two queries
(coverage, scratch size) answer as documented in include/lavt_hip.h.  No GPU needed."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lavt_window_attn_stream_ok", "lavt_window_attn_stream_fwd", "lavt_window_attn_stream_bwd_ws", "lavt_window_attn_stream_bwd")


def test_stream_symbols_declared_bound_exported():
    from lavt_hip import _capi
    header = open(os.path.join(ROOT, "include", "lavt_hip.h")).read()
    declared = set(re.findall(r"\b(lavt_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared, name
        assert name in _capi.EXPORTED, name
        assert hasattr(_capi._cdll, name), f"liblavt_hip.so does not export {name}"
    assert _capi.lib.lavt_abi_version() == 7


@pytest.mark.parametrize("N", [576, 660, 800, 1008, 1152])
def test_stream_ok_covers_video_window12(N):
    from lavt_hip import _capi as K
    for heads in range(1, 33):
        assert K.lib.lavt_window_attn_stream_ok(K.BF16, N, 8, 12, 12, heads, 32) == 1, (N, heads)
    assert K.lib.lavt_window_attn_stream_ok(K.F32, N, 8, 12, 12, 4, 32) == 0
    for hd in (16, 64):
        assert K.lib.lavt_window_attn_stream_ok(K.BF16, N, 8, 12, 12, 4, hd) == 0


def test_stream_ok_limits():
    from lavt_hip import _capi as K
    assert K.lib.lavt_window_attn_stream_ok(K.BF16, 2048, 8, 16, 16, 8, 32) == 1
    assert K.lib.lavt_window_attn_stream_ok(K.BF16, 2049, 8, 16, 17, 8, 32) == 0
    assert K.lib.lavt_window_attn_stream_ok(K.BF16, 1153, 8, 12, 12, 4, 32) == 0        # more tokens than the window holds
    assert K.lib.lavt_window_attn_stream_ok(K.BF16, 8, 8, 12, 12, 4, 32) == 0


@pytest.mark.parametrize("nwin,N,heads", [(64, 1152, 4), (16, 1152, 8), (4, 1152, 16), (1, 1152, 32), (3, 660, 2), (2, 1008, 1)])
def test_stream_bwd_ws_formula(nwin, N, heads):
    from lavt_hip import _capi as K
    ld = -(-N // 32) * 32
    assert K.lib.lavt_window_attn_stream_bwd_ws(K.BF16, nwin, N, heads, 8, 12, 12) == nwin * heads * N + heads * N * ld
    assert K.lib.lavt_window_attn_stream_bwd_ws(K.F32, nwin, N, heads, 8, 12, 12) == 0
