"""CPU tests of Predictor(text_encoder=) and the fused encoder opening (DESIGN.md "Text encoder in the prediction"): lavt_bert_embed_ln_fwd is declared,
bound with the header's arity and exported while the ABI number stays; the new keywords and their defaults; and the pure id / mask check of
Predictor.set_sentences.  No GPU needed."""
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "lavt_bert_embed_ln_fwd"


def _declaration(header, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
    assert m, f"include/lavt_hip.h does not declare {name}"
    return [a.strip() for a in m.group(1).split(",") if a.strip()]


def test_header_declares_and_capi_binds_the_symbol_with_matching_arity():
    import ctypes as C
    from lavt_hip import _capi
    header = open(os.path.join(ROOT, "include", "lavt_hip.h")).read()
    args = _declaration(header, NAME)
    assert len(args) == 19
    assert NAME in _capi.EXPORTED, f"{NAME} is not bound in lavt_hip/_capi.py"
    proto = _capi._PROTOTYPES[NAME]
    assert len(proto) == len(args), f"{NAME}: the header declares {len(args)} arguments, _capi binds {len(proto)}"
    want = [C.c_void_p if "*" in a else C.c_float if a.startswith("float ") else C.c_int32 for a in args]
    assert proto == want, [(a, p) for a, p, w in zip(args, proto, want) if p is not w]
    assert hasattr(_capi._cdll, NAME), f"liblavt_hip.so does not export {NAME}"
    # the header's comment says what the kernel does with values it cannot refuse
    comment = header[:header.index("int " + NAME)].rsplit("/*", 1)[1]
    for phrase in ("word row 0", "type row 0", "N > n_pos", "E[x^2] - mean^2"):
        assert phrase in comment, phrase


def test_the_abi_version_is_unchanged():
    from lavt_hip import _capi
    assert _capi.lib.lavt_abi_version() == _capi.EXPECTED_ABI == 7


def test_predictor_takes_text_encoder_keyword_only_default_none():
    from lavt_hip.engine import Predictor
    p = inspect.signature(Predictor.__init__).parameters["text_encoder"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    assert callable(Predictor.set_sentences)


def test_bert_model_switch_defaults_off_and_is_a_constructor_keyword():
    from bert.modeling_bert import BertConfig, BertModel
    cfg = BertConfig(vocab_size=16, hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=32, max_position_embeddings=8)
    assert BertModel(cfg).fused_embeddings is False and BertModel(cfg).fused_attention is False
    m = BertModel(cfg, fused_embeddings=True)
    assert m.fused_embeddings is True and m.fused_attention is False
    assert inspect.signature(BertModel.from_pretrained).parameters["fused_embeddings"].default is False
    assert inspect.signature(BertModel.__init__).parameters["fused_embeddings"].default is False
    assert "fused_embeddings" not in m.state_dict()          # a plain attribute: the checkpoint keys do not move
    assert BertModel().fused_embeddings is False


def test_ops_bert_embed_ln_signature_and_grad_refusal():
    from bert.modeling_bert import BertConfig, BertEmbeddings
    from lavt_hip import ops
    assert list(inspect.signature(ops.bert_embed_ln).parameters) == ["ids", "token_type_ids", "attention_mask", "emb_module", "N", "dtype"]
    emb = BertEmbeddings(BertConfig(vocab_size=16, hidden_size=64, num_hidden_layers=1, num_attention_heads=1, intermediate_size=32, max_position_embeddings=8))
    ids = torch.zeros(2, 4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no backward"):          # grad mode on, parameters require grad: refused before any pointer is taken
        ops.bert_embed_ln(ids, None, None, emb, 4, torch.float32)
    with torch.no_grad(), pytest.raises(RuntimeError, match="GPU memory only"):
        ops.bert_embed_ln(ids, None, None, emb, 4, torch.float32)


def test_check_sentences_refuses_each_case_and_passes_a_valid_pair():
    from lavt_hip import ops
    from lavt_hip.engine import check_sentences
    shape, vocab, n_pos = (3, 22), 64, 32
    ids = torch.randint(0, vocab, shape)
    ids[0, 0], ids[2, 21] = 0, vocab - 1          # both ends of the range are inside it
    mask = (torch.arange(22)[None, :] < torch.tensor([22, 9, 0])[:, None]).long()
    assert check_sentences(ids, mask, shape, vocab, n_pos) is None
    assert check_sentences(ids, mask, torch.Size(shape), vocab, 22) is None          # N_l == max_position_embeddings is inside
    with pytest.raises(ValueError, match="ids"):
        check_sentences(ids[:2], mask, shape, vocab, n_pos)
    with pytest.raises(ValueError, match="ids"):
        check_sentences(ids.int(), mask, shape, vocab, n_pos)
    with pytest.raises(ValueError, match="ids"):
        check_sentences(ids.tolist(), mask, shape, vocab, n_pos)
    with pytest.raises(ValueError, match="mask"):
        check_sentences(ids, mask[:, :21], shape, vocab, n_pos)
    with pytest.raises(ValueError, match="mask"):
        check_sentences(ids, mask.float(), shape, vocab, n_pos)
    with pytest.raises(ValueError, match="mask"):
        check_sentences(ids, mask.unsqueeze(-1), shape, vocab, n_pos)
    for bad in (-1, vocab, 2 ** 40):
        wrong = ids.clone()
        wrong[1, 5] = bad
        with pytest.raises(ValueError, match=r"ids.*\(1, 5, %d\).*vocabulary" % bad):
            check_sentences(wrong, mask, shape, vocab, n_pos)
    with pytest.raises(ValueError, match="max_position_embeddings = 21"):
        check_sentences(ids, mask, shape, vocab, 21)
    wide = (2, ops.KV_LD + 1)
    with pytest.raises(ValueError, match="KV_LD"):
        check_sentences(torch.zeros(wide, dtype=torch.int64), torch.ones(wide, dtype=torch.int64), wide, vocab, 512)
    full = (2, ops.KV_LD)
    assert check_sentences(torch.zeros(full, dtype=torch.int64), torch.ones(full, dtype=torch.int64), full, vocab, 512) is None
    # the function is pure: nothing it was given has changed
    assert int(ids[0, 0]) == 0 and int(ids[2, 21]) == vocab - 1 and mask.sum().item() == 31
