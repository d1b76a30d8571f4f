"""CPU tests of the captured-train-iteration C ABI: the gradient-norm / guarded-update entry points are declared in include/lavt_hip.h, bound in
lavt_hip._capi and exported by the library, under the unchanged ABI version; the scratch-size query follows its documented formula."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lavt_grad_norm_ws", "lavt_grad_norm", "lavt_adamw_step_chunks_guarded")


def test_guard_entry_points_are_declared_bound_and_exported():
    from lavt_hip import _capi
    header = open(os.path.join(ROOT, "include", "lavt_hip.h")).read()
    declared = set(re.findall(r"\b(lavt_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/lavt_hip.h"
        assert name in _capi.EXPORTED, f"{name} is not bound in lavt_hip/_capi.py"
        assert hasattr(_capi._cdll, name), f"liblavt_hip.so does not export {name}"
    assert _capi.lib.lavt_abi_version() == _capi.EXPECTED_ABI == 7


def test_grad_norm_scratch_follows_its_documented_formula():
    """include/lavt_hip.h: `ws floats = nchunks` (one fp32 partial per chunk of lavt_adamw_chunk_elems() gradient values)"""
    from lavt_hip import _capi
    header = open(os.path.join(ROOT, "include", "lavt_hip.h")).read()
    assert re.search(r"ws floats = nchunks\b", header), "the scratch formula is not documented in the header"
    for n in (1, 2, 7, 255, 256, 257, 14543, 1 << 20):
        assert _capi.lib.lavt_grad_norm_ws(n) == n
    assert _capi.lib.lavt_grad_norm_ws(0) == 0


def test_guard_options_exist_on_the_python_surface():
    import inspect
    from lavt_hip.engine import TrainStep
    from lavt_hip.optim import FusedAdamW
    sig = inspect.signature(FusedAdamW.__init__).parameters
    assert sig["max_grad_norm"].default == 0.0 and sig["skip_nonfinite"].default is False
    for name in ("hold", "last_grad_norm", "skipped_steps"):
        assert callable(getattr(FusedAdamW, name))
    for name in ("make_optimizer", "attach_optimizer"):
        assert callable(getattr(TrainStep, name))
    # TrainStep keeps its positional signature
    assert list(inspect.signature(TrainStep.__init__).parameters)[:12] == ["self", "model", "image", "l_feats", "l_mask", "target", "world", "use_graph", "bucket_mib",
                                                                          "fused_loss", "refresh_weights_in_step", "context"]
