"""CPU tests of AMSGrad on the fused AdamW: the C entry point is declared, bound and exported under the unchanged ABI version; the constructor, the
optimizer-wide flag and the checkpoint rules of FusedAdamW(amsgrad=True); the language-encoder groups of lavt_param_groups (--lang_enc_params and the
separate text encoder of --model lavt, train.py:623-686)."""
import os
import re

import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the symbol
def test_amsgrad_entry_point_is_declared_bound_and_exported():
    from lavt_hip import _capi
    header = open(os.path.join(ROOT, "include", "lavt_hip.h")).read()
    declared = set(re.findall(r"\b(lavt_[a-z0-9_]+)\s*\(", header))
    name = "lavt_adamw_step_chunks_amsgrad"
    assert name in declared, f"{name} is not declared in include/lavt_hip.h"
    assert name in _capi.EXPORTED, f"{name} is not bound in lavt_hip/_capi.py"
    assert hasattr(_capi._cdll, name), f"liblavt_hip.so does not export {name}"
    assert len(_capi._PROTOTYPES[name]) == 10
    assert _capi.lib.lavt_abi_version() == _capi.EXPECTED_ABI == 7


# ------------------------------------------------------------------------------------------------ the constructor
def _cpu_params():
    g = torch.Generator().manual_seed(2)
    return [nn.Parameter(torch.randn(4, 3, generator=g)), nn.Parameter(torch.randn(5, generator=g))]


def test_constructor_accepts_amsgrad():
    from lavt_hip.optim import FusedAdamW
    ps = _cpu_params()
    opt = FusedAdamW([ps[0]], amsgrad=True)
    assert opt.param_groups[0]["amsgrad"] is True and opt.defaults["amsgrad"] is True
    opt.add_param_group({"params": [ps[1]], "amsgrad": True})
    assert [g["amsgrad"] for g in opt.param_groups] == [True, True]


def test_amsgrad_is_optimizer_wide():
    from lavt_hip.optim import FusedAdamW
    ps = _cpu_params()
    with pytest.raises(ValueError, match="amsgrad"):
        FusedAdamW([{"params": [ps[0]]}, {"params": [ps[1]], "amsgrad": False}], amsgrad=True)
    opt = FusedAdamW([ps[0]], amsgrad=True)
    with pytest.raises(ValueError, match="amsgrad"):
        opt.add_param_group({"params": [ps[1]], "amsgrad": False})
    assert len(opt.param_groups) == 1
    plain = FusedAdamW([ps[0]])
    assert plain.defaults["amsgrad"] is False and plain.param_groups[0]["amsgrad"] is False
    with pytest.raises(ValueError, match="amsgrad"):
        plain.add_param_group({"params": [ps[1]], "amsgrad": True})


# ------------------------------------------------------------------------------------------------ checkpoints
def _torch_checkpoint(amsgrad):
    ps = _cpu_params()
    ref = torch.optim.AdamW([{"params": ps[:1], "weight_decay": 0.0}, {"params": ps[1:]}], lr=1e-2, weight_decay=0.05, amsgrad=amsgrad)
    g = torch.Generator().manual_seed(3)
    for p in ps:
        p.grad = torch.randn(p.shape, generator=g)
    ref.step()
    return ps, ref


def _clone_groups(ps):
    qs = [nn.Parameter(p.detach().clone()) for p in ps]
    return qs, [{"params": qs[:1], "weight_decay": 0.0}, {"params": qs[1:]}]


def test_torch_amsgrad_checkpoint_loads():
    from lavt_hip.optim import FusedAdamW
    ps, ref = _torch_checkpoint(True)
    qs, groups = _clone_groups(ps)
    ours = FusedAdamW(groups, lr=1e-2, weight_decay=0.05, amsgrad=True)
    ours.load_state_dict(ref.state_dict())
    for p, q in zip(ps, qs):
        for key in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
            assert key in ours.state[q] and torch.equal(ours.state[q][key], ref.state[p][key]), key
        assert bool(ours.state[q]["max_exp_avg_sq"].any())
    assert ours.steps_taken() == 1
    assert all(g["amsgrad"] is True for g in ours.param_groups)
    sd = ours.state_dict()
    assert all("max_exp_avg_sq" in st for st in sd["state"].values()) and len(sd["state"]) == 2


def test_checkpoints_of_the_other_kind_are_refused():
    from lavt_hip.optim import FusedAdamW
    ps, ref = _torch_checkpoint(True)
    _, groups = _clone_groups(ps)
    with pytest.raises(ValueError, match=r"amsgrad=\[True\].*amsgrad=False"):
        FusedAdamW(groups, lr=1e-2, weight_decay=0.05).load_state_dict(ref.state_dict())
    ps, ref = _torch_checkpoint(False)
    _, groups = _clone_groups(ps)
    ours = FusedAdamW(groups, lr=1e-2, weight_decay=0.05, amsgrad=True)
    with pytest.raises(ValueError, match=r"amsgrad=\[False\].*amsgrad=True"):
        ours.load_state_dict(ref.state_dict())
    assert not ours.state, "a refused checkpoint left state behind"


# ------------------------------------------------------------------------------------------------ lavt_param_groups
class _TextEncoder(nn.Module):
    def __init__(self, frozen_layer):
        super().__init__()
        self.embeddings = nn.Linear(3, 2)
        self.encoder = nn.Module()
        self.encoder.layer = nn.ModuleList([nn.Linear(2, 2) for _ in range(12)])
        self.pooler = nn.Linear(2, 2)                     # in no group
        self.encoder.layer[frozen_layer].bias.requires_grad_(False)
        self.embeddings.bias.requires_grad_(False)


class _Model(nn.Module):
    def __init__(self, with_text=True):
        super().__init__()
        self.backbone = nn.Module()
        self.backbone.proj = nn.Linear(2, 2)
        self.backbone.norm1 = nn.LayerNorm(2)
        self.backbone.absolute_pos_embed = nn.Parameter(torch.zeros(2))
        self.backbone.relative_position_bias_table = nn.Parameter(torch.zeros(2))
        self.classifier = nn.Linear(2, 2)
        self.classifier.bias.requires_grad_(False)
        if with_text:
            self.text_encoder = _TextEncoder(frozen_layer=4)


def _expected(model, enc, mode):
    """train.py:615-684 written out for the stand-in"""
    no_decay = [p for n, p in model.backbone.named_parameters() if "norm" in n or "absolute_pos_embed" in n or "relative_position_bias_table" in n]
    decay = [p for n, p in model.backbone.named_parameters() if not ("norm" in n or "absolute_pos_embed" in n or "relative_position_bias_table" in n)]
    groups = [no_decay, decay, [p for p in model.classifier.parameters() if p.requires_grad]]
    first10 = []
    for i in range(10):
        first10 += [p for p in enc.encoder.layer[i].parameters() if p.requires_grad]
    whole = [p for p in enc.encoder.parameters() if p.requires_grad]
    emb = [p for p in enc.embeddings.parameters() if p.requires_grad]
    groups += {"encoder-10": [first10], "encoder-all": [whole], "embeddings+encoder-10": [emb, first10], "embeddings+encoder-all": [emb, whole]}[mode]
    return groups


def _check(groups, want):
    assert len(groups) == len(want)
    for i, (g, w) in enumerate(zip(groups, want)):
        assert len(g["params"]) == len(w) and all(a is b for a, b in zip(g["params"], w)), f"group {i}"
        assert all(p.requires_grad for p in g["params"])
        assert (g.get("weight_decay") == 0.0 and set(g) == {"params", "weight_decay"}) if i == 0 else set(g) == {"params"}


@pytest.mark.parametrize("mode,count", [("encoder-10", 4), ("encoder-all", 4), ("embeddings+encoder-10", 5), ("embeddings+encoder-all", 5)])
def test_lang_enc_params(mode, count):
    from lavt_hip.optim import lavt_param_groups
    model = _Model()
    groups = lavt_param_groups(model, lang_enc_params=mode)
    assert len(groups) == count
    _check(groups, _expected(model, model.text_encoder, mode))
    sizes = {"encoder-10": [19], "encoder-all": [23], "embeddings+encoder-10": [1, 19], "embeddings+encoder-all": [1, 23]}[mode]
    assert [len(g["params"]) for g in groups[3:]] == sizes          # 2 tensors per layer, one of them frozen in layer 4 and in the embeddings


@pytest.mark.parametrize("mode", ["encoder-10", "embeddings+encoder-all"])
def test_external_text_encoder(mode):
    """--model lavt: the fourth group comes from a separate bert_model (train.py:623-632), also when the model carries an encoder of its own"""
    from lavt_hip.optim import lavt_param_groups
    bert = _TextEncoder(frozen_layer=9)
    for model in (_Model(with_text=False), _Model()):
        _check(lavt_param_groups(model, lang_enc_params=mode, text_encoder=bert), _expected(model, bert, mode))


def test_bad_lang_enc_params_raises():
    from lavt_hip.optim import lavt_param_groups
    for bad in ("encoder-12", "embeddings", "", None):
        with pytest.raises(ValueError, match="lang_enc_params"):
            lavt_param_groups(_Model(), lang_enc_params=bad)


def test_default_call_is_the_parents():
    from lavt_hip.optim import lavt_param_groups
    model = _Model()
    _check(lavt_param_groups(model), _expected(model, model.text_encoder, "encoder-10"))
    three = lavt_param_groups(model, 3)                  # positional text_encoder_layers, as existing callers pass it
    assert len(three) == 4 and len(three[3]["params"]) == 6 and three[3]["params"][0] is model.text_encoder.encoder.layer[0].weight
    _check(three[:3], _expected(model, model.text_encoder, "encoder-10")[:3])
    bare = _Model(with_text=False)
    assert len(lavt_param_groups(bare)) == 3             # a model without a text encoder: no language group
