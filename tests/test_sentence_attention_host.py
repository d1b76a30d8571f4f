"""CPU tests of the fused sentence attention's host side: the two entry points are declared, bound with the header's arity and exported; the reference
statement of tests/sentence_attn_ref.py is the attention `torch.nn.functional.scaled_dot_product_attention` computes; BertModel's switch; the geometry
predicate of ops.sentence_attention; the host-side surface of TrainStep(text_encoder=) that needs no device."""
import inspect
import os
import re

import pytest
import torch

import sentence_attn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lavt_sentence_attn_fwd", "lavt_sentence_attn_bwd")


def _declared_arity(header, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
    assert m, f"include/lavt_hip.h does not declare {name}"
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_header_declares_and_capi_binds_the_two_symbols_with_matching_arity():
    from lavt_hip import _capi
    header = open(os.path.join(ROOT, "include", "lavt_hip.h")).read()
    for name in NEW:
        n = _declared_arity(header, name)
        assert name in _capi.EXPORTED, f"{name} is not bound in lavt_hip/_capi.py"
        assert len(_capi._PROTOTYPES[name]) == n, f"{name}: the header declares {n} arguments, _capi binds {len(_capi._PROTOTYPES[name])}"
        assert hasattr(_capi._cdll, name), f"liblavt_hip.so does not export {name}"
    assert _declared_arity(header, NEW[0]) == 11 and _declared_arity(header, NEW[1]) == 12
    assert _capi.lib.lavt_abi_version() == _capi.EXPECTED_ABI == 7


def test_reference_statement_is_scaled_dot_product_attention_with_an_additive_mask():
    B, N, heads = 2, 7, 3
    H = heads * R.HD
    qkv, keybias, dout, _, _ = R.case_inputs(B, N, heads, seed=3, with_keep=False)
    out, dq, dk, dv = R.reference(qkv, keybias, dout, B, N, heads)
    x = qkv.double().requires_grad_(True)
    q, k, v = (x[:, i * H:(i + 1) * H].view(B, N, heads, R.HD).permute(0, 2, 1, 3) for i in range(3))
    sdpa = torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=keybias.double().view(B, 1, 1, N))
    sdpa = sdpa.permute(0, 2, 1, 3).reshape(B * N, H)
    sdpa.backward(dout.double())
    assert float((out - sdpa.detach()).abs().max()) < 1e-12
    for mine, theirs in ((dq, x.grad[:, :H]), (dk, x.grad[:, H:2 * H]), (dv, x.grad[:, 2 * H:])):
        assert float((mine - theirs).abs().max()) < 1e-12
    # the fp32 mode is the same statement, a rounding error away
    out32 = R.reference(qkv, keybias, dout, B, N, heads, dtype=torch.float32)[0]
    assert out32.dtype == torch.float32 and 0 < float((out32.double() - out).abs().max()) < 1e-5
    # an explicit keep mask of ones with scale 1 changes nothing; a dropped probability removes exactly its term
    ones = torch.ones(B, heads, N, N, dtype=torch.uint8)
    assert torch.equal(R.reference(qkv, keybias, dout, B, N, heads, keep=ones, drop_scale=1.0)[0], out)
    mask = R.ragged_mask(3, 9, seed=1)
    assert mask[0].sum() == 9 and mask[-1].sum() == 1 and bool((mask[:, :-1] >= mask[:, 1:]).all())


def test_bert_model_switch_defaults_off_and_is_a_constructor_keyword():
    from bert.modeling_bert import BertConfig, BertModel
    cfg = BertConfig(vocab_size=16, hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=32, max_position_embeddings=8)
    assert BertModel(cfg).fused_attention is False
    assert BertModel(cfg, fused_attention=True).fused_attention is True
    assert "fused_attention" in inspect.signature(BertModel.from_pretrained).parameters
    assert "fused_attention" not in BertModel(cfg).state_dict()          # a plain attribute: the checkpoint keys do not move


def test_geometry_predicate_is_what_the_op_uses():
    from lavt_hip import ops
    for N, hd in ((1, 64), (20, 64), (64, 64), (65, 64), (72, 64), (0, 64), (20, 32), (20, 128)):
        assert ops.sentence_attention_ok(N, hd) == R.sentence_attention_ok(N, hd) == (hd == 64 and 1 <= N <= 64), (N, hd)
    src = inspect.getsource(ops.sentence_attention)
    assert "sentence_attention_ok(" in src and "masked_self_attention(" in src
    assert list(inspect.signature(ops.sentence_attention).parameters) == ["qkv", "keybias", "B", "N", "heads", "p_drop", "keep"]


def test_train_step_surface_for_a_text_encoder():
    from lavt_hip import checkpoint
    from lavt_hip.engine import TrainStep, _StepModules
    assert inspect.signature(TrainStep.__init__).parameters["text_encoder"].default is None
    mk = inspect.signature(TrainStep.make_optimizer).parameters
    assert mk["text_encoder_layers"].default == 10 and mk["lang_enc_params"].default == "encoder-10"
    assert checkpoint.TRAIN_STATE_KEYS == ("model", "optimizer", "lavt_train_state") and checkpoint.TRAIN_STATE_FORMAT == 1
    model, enc = torch.nn.Linear(2, 2), torch.nn.Sequential(torch.nn.Linear(2, 2), torch.nn.LayerNorm(2))
    names = [n for n, _ in _StepModules(model, enc).named_parameters()]
    assert names == ["bert_model.0.weight", "bert_model.0.bias", "bert_model.1.weight", "bert_model.1.bias", "weight", "bias"]
    assert [id(p) for p in _StepModules(model, enc).parameters()] == [id(p) for p in enc.parameters()] + [id(p) for p in model.parameters()]


def test_save_train_state_refuses_bert_model_as_metadata(tmp_path):
    from lavt_hip.checkpoint import save_train_state
    with pytest.raises(ValueError, match="bert_model"):
        save_train_state(tmp_path / "x.pth", object(), bert_model={})
