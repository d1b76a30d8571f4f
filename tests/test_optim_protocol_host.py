"""The optimizer's device protocol is written once on each side of the C ABI -- LAVT_CTL_* / LAVT_ADAMW_* in include/lavt_hip.h, CTL_* / DESC_COLS /
HYPER_COLS in lavt_hip/optim.py -- and the two agree.  No GPU needed."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_defs(prefix):
    header = open(os.path.join(ROOT, "include", "lavt_hip.h")).read()
    return {k: int(v) for k, v in re.findall(r"#define (%s\w+) (\d+)\b" % prefix, header)}


def test_control_block_slots_are_the_header_s():
    from lavt_hip import optim as O
    assert _header_defs("LAVT_CTL_") == {"LAVT_CTL_NORM": O.CTL_NORM, "LAVT_CTL_CLIP": O.CTL_CLIP, "LAVT_CTL_SKIP": O.CTL_SKIP, "LAVT_CTL_SKIPPED": O.CTL_SKIPPED,
                                         "LAVT_CTL_HOLD": O.CTL_HOLD, "LAVT_CTL_ACCUMULATING": O.CTL_ACCUMULATING, "LAVT_CTL_MICRO": O.CTL_MICRO,
                                         "LAVT_CTL_FLOATS": O.CTL_FLOATS}
    assert [O.CTL_NORM, O.CTL_CLIP, O.CTL_SKIP, O.CTL_SKIPPED, O.CTL_HOLD, O.CTL_ACCUMULATING, O.CTL_MICRO, O.CTL_FLOATS] == [0, 1, 2, 3, 4, 5, 6, 8]


def test_table_columns_are_the_header_s():
    from lavt_hip import optim as O
    defs = _header_defs("LAVT_ADAMW_")
    assert defs.pop("LAVT_ADAMW_DESC_COLS") == O.DESC_COLS == 6 and defs.pop("LAVT_ADAMW_HYPER_COLS") == O.HYPER_COLS == 5
    # the column names, in the order FusedAdamW._build writes a row and the kernels read it
    assert [k for k, _ in sorted(defs.items(), key=lambda kv: kv[1]) if k.startswith("LAVT_ADAMW_DESC_")] == [
        "LAVT_ADAMW_DESC_" + n for n in ("PARAM", "GRAD", "EXP_AVG", "EXP_AVG_SQ", "NUMEL", "COPY")]
    assert [k for k, _ in sorted(defs.items(), key=lambda kv: kv[1]) if k.startswith("LAVT_ADAMW_HYPER_")] == [
        "LAVT_ADAMW_HYPER_" + n for n in ("LR", "WEIGHT_DECAY", "BETA1", "BETA2", "EPS")]
    assert sorted(v for k, v in defs.items() if "_DESC_" in k) == list(range(O.DESC_COLS))
    assert sorted(v for k, v in defs.items() if "_HYPER_" in k) == list(range(O.HYPER_COLS))


def test_tables_are_a_named_tuple_in_the_positional_order():
    from lavt_hip.optim import _Tables
    assert _Tables._fields == ("key", "desc", "hyper", "count", "chunks", "nchunks", "fused", "vmax", "ema")


def test_initial_control_block():
    """what FusedAdamW._make_guard uploads: zeros, and a clip coefficient of 1 (x * 1.0f is exact)"""
    import inspect

    import torch

    from lavt_hip.optim import FusedAdamW, initial_control_block
    g = initial_control_block()
    assert g.dtype == torch.float32 and g.device.type == "cpu" and g.tolist() == [0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert "initial_control_block().to(" in inspect.getsource(FusedAdamW._make_guard)
