"""TrainStep(text_encoder=): the separate `bert_model` of `--model lavt` trained inside the captured step (DESIGN.md "Text encoder in the step").

Setup: the micro 2-D LAVT of test_gpu_modules._build (embed 32, depths 2-2-2-2, window 7, DropPath off) on 2 images of 64^2 with 22 tokens, and a separate
2-layer BertModel (hidden 768, 12 heads of 64, dropout off unless a test turns it on), everything in fp32.

Gradient parity rule (test_gpu_dice_boundary.test_train_step_dice_boundary): per parameter, relative L2 <= 3 % and no element further than 6 % of the
parameter's scale.  Analytically zero gradients hold rounding noise on both sides (measured: 2.4e-7 against 1e-2 .. 1 elsewhere) and are held to 5 % of
their weight's scale instead, as there: the PWAM biases in front of an InstanceNorm, and -- here -- two of the encoder's: `attention.self.key.bias`, which
shifts every score of a query row by the same q . b and so cancels in the softmax, and the bias of the LAST LayerNorm, which adds the same vector to every
token of l_feats -- the model reads l_feats only through PWAM's f_key / f_value, a Conv1d followed by an InstanceNorm1d over the tokens, which removes it."""
import pytest
import torch
import torch.nn.functional as F

from lavt_hip.detweights import det_inputs, fill_state_dict_

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_L = 22
ZERO_GRAD_BIASES = tuple(f"image_lang_att.{m}.0.bias" for m in ("f_key", "f_value", "f_query", "W")) + ("attention.self.key.bias", "encoder.layer.1.output.LayerNorm.bias")
_REF = {}


@pytest.fixture(autouse=True)
def _fp32():
    import lavt_hip
    with lavt_hip.use_dtype(torch.float32):
        yield


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _model(salt=0):
    from test_gpu_modules import _build
    model = _build(32, [2, 2, 2, 2], [1, 2, 4, 8], 7, dpr=0.0)
    if salt:
        fill_state_dict_(model, salt=salt)
    return model.train()


def _bert(fused=False, p=0.0, salt=0):
    from bert.modeling_bert import BertConfig, BertModel
    enc = BertModel(BertConfig(vocab_size=64, hidden_size=768, num_hidden_layers=2, num_attention_heads=12, intermediate_size=256, max_position_embeddings=32,
                               hidden_dropout_prob=p, attention_probs_dropout_prob=p), fused_attention=fused)
    fill_state_dict_(enc, salt=salt + 1)
    return enc.to(DEV).train()


def _batch(seed=100, n=2):
    """(image, ids, attention mask, target) on the device; n expressions (n != 2: a pair-list batch over the 2 images)"""
    x, _, _, _ = det_inputs(2, 64, N_L, seed=seed)
    _, _, m, tgt = det_inputs(n, 64, N_L, seed=seed + 1)
    mask = m.squeeze(-1).long()
    ids = torch.randint(1, 64, mask.shape, generator=torch.Generator().manual_seed(seed)) * mask
    return tuple(v.to(DEV) for v in (x, ids, mask, tgt))


def _step(fused=False, p=0.0, salt=0, batch=None, **kw):
    from lavt_hip import ops
    from lavt_hip.engine import TrainStep
    model, enc = _model(salt), _bert(fused, p, salt)
    static = tuple(v.clone() for v in (batch or _batch()))
    return TrainStep(model, *static, text_encoder=enc, context=ops.StepContext(), **kw), static


def _enc_grads_nonzero(step):
    torch.cuda.synchronize()
    got = {n: float(p.grad.abs().max()) for n, p in step.text_encoder.named_parameters() if not n.startswith("pooler.")}
    dead = [n for n, g in got.items() if not g > 0 and not n.endswith(ZERO_GRAD_BIASES)]
    assert not dead, f"encoder parameters without gradient: {dead[:6]}"


def _reference_flow():
    """train.py:217-224 written out with the drop-in modules and plain autograd (composed attention) -> (loss, {name: gradient})"""
    if not _REF:
        from lavt_hip import ops
        model, enc = _model(), _bert()
        x, ids, mask, tgt = _batch()
        with ops.use_context(ops.StepContext()):          # a context no harness has touched: ordinary autograd accumulation into .grad
            l = enc(ids, attention_mask=mask)[0].permute(0, 2, 1)
            out = model(x, l, mask.unsqueeze(-1))
            loss = F.cross_entropy(out, tgt, weight=torch.tensor([0.9, 1.1], device=DEV))
            loss.backward()
            torch.cuda.synchronize()
        grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
        grads.update({"bert_model." + n: p.grad.clone() for n, p in enc.named_parameters() if p.grad is not None})
        _REF["loss"], _REF["grads"] = float(loss.detach()), grads
    return _REF["loss"], _REF["grads"]


@pytest.mark.parametrize("fused", (False, True), ids=("composed", "fused"))
def test_parity_with_the_reference_flow(fused):
    ref_loss, ref = _reference_flow()
    assert sum(n.startswith("bert_model.") for n in ref) >= 30 and any(not n.startswith("bert_model.") for n in ref)
    step, _ = _step(fused=fused, use_graph=False)
    step.step()
    torch.cuda.synchronize()
    loss = float(step.loss)
    print(f"\n[text step fused={fused}] loss {loss:.8f}, reference flow {ref_loss:.8f}")
    assert abs(loss - ref_loss) < 1e-5
    bad, worst, seen = [], (0.0, 0.0, ""), 0
    for n, p in step._named_parameters():
        if n not in ref:
            continue
        seen += 1
        scale = float(ref[n].abs().max())
        if n.endswith(ZERO_GRAD_BIASES):
            wscale = float(ref[n[:-4] + "weight"].abs().max())
            assert scale <= 0.05 * wscale and float(p.grad.abs().max()) <= 0.05 * wscale, (n, scale, float(p.grad.abs().max()), wscale)
            continue
        err = float((p.grad - ref[n]).abs().max())
        rel = float((p.grad - ref[n]).norm()) / max(float(ref[n].norm()), scale * ref[n].numel() ** 0.5 * 0.1, 1e-9)
        worst = max(worst, (err / max(scale, 1e-9), rel, n))
        if err > 0.06 * scale + 1e-7 or rel > 0.03:
            bad.append((n, round(err / max(scale, 1e-9), 4), round(rel, 4), scale))
    print(f"[text step fused={fused}] worst (max-abs / scale, relative L2, name): {worst}")
    assert seen == len(ref), "every parameter of both modules that has a reference gradient is compared"
    assert not bad, sorted(bad, key=lambda b: -b[1])[:12]


@pytest.mark.parametrize("fused", (False, True), ids=("composed", "fused"))
def test_capture_replays_the_eager_loss(fused):
    step, _ = _step(fused=fused)
    eager = step.step().clone()
    step.warmup_and_capture(eager_iters=1)
    assert step.captured
    step.step()
    torch.cuda.synchronize()
    assert torch.equal(step.loss, eager), "replay and eager step must agree bit for bit"
    _enc_grads_nonzero(step)


def test_owned_optimizer_updates_the_grouped_encoder_layers_only():
    step, _ = _step(fused=True)
    enc = step.text_encoder
    opt = step.make_optimizer(text_encoder_layers=1, lr=1e-3, weight_decay=1e-2, tensor_norms=True)
    grouped = {id(p) for g in opt.param_groups for p in g["params"]}
    assert all(id(p) in grouped for p in enc.encoder.layer[0].parameters()) and not any(id(p) in grouped for p in enc.encoder.layer[1].parameters())
    before = {n: p.detach().clone() for n, p in enc.named_parameters()}
    model_before = step.model.backbone.layers[0].blocks[0].attn.qkv.weight.detach().clone()
    step.warmup_and_capture(eager_iters=1)
    assert step.captured
    assert all(torch.equal(_bits(before[n]), _bits(p)) for n, p in enc.named_parameters()), "the warm-up holds the optimizer: nothing moves"
    step.step()
    step.step()
    _enc_grads_nonzero(step)
    moved = {n: not torch.equal(_bits(before[n]), _bits(p)) for n, p in enc.named_parameters()}
    for n, m in moved.items():
        if n.startswith("encoder.layer.0."):
            assert m, f"{n} is in the optimizer's group and did not change"
        else:
            assert not m, f"{n} is in no group and changed"
    assert not torch.equal(model_before, step.model.backbone.layers[0].blocks[0].attn.qkv.weight)
    norms = opt.grad_norms()
    mine = [k for k in norms if isinstance(k, str) and k.startswith("bert_model.encoder.layer.0.")]
    assert len(mine) == len(list(enc.encoder.layer[0].parameters())) and not any(isinstance(k, int) for k in norms)
    assert norms["bert_model.encoder.layer.0.attention.self.query.weight"] > 0
    assert opt.last_nonfinite() is None
    names = [e[0] for e in step._acc_layout()]
    assert "bert_model.embeddings.word_embeddings.weight" in names and "backbone.patch_embed.proj.weight" in names
    groups = step._config()["param_groups"]
    assert groups[-1][0][0].startswith("bert_model.encoder.layer.0.") and not any(e[0].startswith("<") for g in groups for e in g)


def _run(n_first, n_last, step, static, batches):
    losses = []
    for i in range(n_first, n_last):
        for dst, src in zip(static, batches[i]):
            dst.copy_(src)
        losses.append(step.step().clone())
    torch.cuda.synchronize()
    return losses


def _owned(salt, seed, **kw):
    torch.manual_seed(seed)
    step, static = _step(fused=True, salt=salt, deterministic=True, **kw)
    step.make_optimizer(text_encoder_layers=1, lr=3e-4, weight_decay=1e-2, max_grad_norm=1.0, total_steps=40)
    step.warmup_and_capture(eager_iters=1)
    assert step.captured
    return step, static


def test_checkpoint_carries_the_encoder_and_resumes_bit_for_bit(tmp_path):
    from lavt_hip import checkpoint, ops
    from lavt_hip.engine import TrainStep
    assert checkpoint.TRAIN_STATE_KEYS == ("model", "optimizer", "lavt_train_state")
    batches = [_batch(seed=200 + 2 * i) for i in range(4)]
    a, sa = _owned(0, 1)
    la = _run(0, 4, a, sa, batches)
    pa = a.model.backbone.layers[0].blocks[0].attn.qkv.weight.detach().clone()
    ea = a.text_encoder.encoder.layer[0].attention.self.query.weight.detach().clone()
    del a
    b, sb = _owned(0, 1)
    lb = _run(0, 2, b, sb, batches)
    state = b.state_dict()
    assert list(state.keys()) == ["model", "optimizer", "lavt_train_state", "bert_model"]
    assert state["bert_model"].keys() == b.text_encoder.state_dict().keys()
    assert all(not v.is_cuda for v in state["bert_model"].values())
    assert any(e[0].startswith("bert_model.") for g in state["lavt_train_state"]["config"]["param_groups"] for e in g)
    path = tmp_path / "run.pth"
    checkpoint.save_train_state(path, b, epoch=3)
    del b
    c, sc = _owned(7, 5)                                        # another salt, another seed: every tensor must come from the file
    extra = checkpoint.load_train_state(path, c)
    assert extra == {"epoch": 3}, "'bert_model' is the step's entry, not user metadata"
    lc = _run(2, 4, c, sc, batches)
    assert all(torch.equal(x, y) for x, y in zip(la[:2], lb)) and all(torch.equal(x, y) for x, y in zip(la[2:], lc)), ([float(v) for v in la], [float(v) for v in lb + lc])
    assert torch.equal(_bits(pa), _bits(c.model.backbone.layers[0].blocks[0].attn.qkv.weight))
    assert torch.equal(_bits(ea), _bits(c.text_encoder.encoder.layer[0].attention.self.query.weight))
    # the file loads into the reference's objects: single_bert_model.load_state_dict(ckpt['bert_model'])
    saved = torch.load(path, map_location="cpu", weights_only=True)["bert_model"]
    fresh = _bert(salt=3)
    fresh.load_state_dict(saved)
    assert torch.equal(fresh.encoder.layer[1].output.dense.weight.cpu(), saved["encoder.layer.1.output.dense.weight"])
    # a checkpoint of a step WITHOUT encoder is refused before any write, and the other way round
    x, _, _, tgt = batches[0]
    _, l, m, _ = det_inputs(2, 64, N_L, seed=3)
    plain = TrainStep(_model(), x.clone(), l.to(DEV), m.to(DEV), tgt.clone(), context=ops.StepContext(), deterministic=True, use_graph=False)
    plain.make_optimizer(lr=3e-4, max_grad_norm=1.0, total_steps=40)
    plain.warmup_and_capture(eager_iters=1)
    torch.cuda.synchronize()
    snap = [p.detach().clone() for p in c._params]
    with pytest.raises(ValueError, match="bert_model"):
        c.load_state_dict(plain.state_dict())
    assert "bert_model" not in plain.state_dict()
    assert all(torch.equal(_bits(s), _bits(p)) for s, p in zip(snap, c._params)), "a refused load has changed nothing"
    psnap = [p.detach().clone() for p in plain._params]
    with pytest.raises(ValueError, match="bert_model"):
        plain.load_state_dict(c.state_dict())
    assert all(torch.equal(_bits(s), _bits(p)) for s, p in zip(psnap, plain._params))


def test_accumulate_two_runs_one_captured_cycle():
    step, _ = _step(fused=True, accumulate=2)
    step.make_optimizer(text_encoder_layers=1, lr=1e-3)
    w = step.text_encoder.encoder.layer[0].output.dense.weight
    before = w.detach().clone()
    step.warmup_and_capture(eager_iters=1)
    assert step.captured and step.acc.numel() == step.buckets.flat.numel() == sum(p.numel() for p in step._params if p.requires_grad)
    l0 = step.step().clone()
    assert step.micro_step() == 1 and torch.equal(_bits(before), _bits(w)), "the first micro-step of a cycle updates nothing"
    l1 = step.step().clone()
    torch.cuda.synchronize()
    assert step.micro_step() == 0 and not torch.equal(_bits(before), _bits(w))
    assert torch.isfinite(l0) and torch.isfinite(l1)
    _enc_grads_nonzero(step)


def test_pair_list_batch_feeds_the_encoder_n_expressions():
    x, ids, mask, tgt = _batch(seed=300, n=3)
    image_of = torch.tensor([0, 1, 1], dtype=torch.int32, device=DEV)
    step, _ = _step(fused=True, batch=(x, ids, mask, tgt), image_of=image_of)
    assert step.l.shape == (3, N_L) and step.t.shape[0] == 3 and step.x.shape[0] == 2
    step.warmup_and_capture(eager_iters=1)
    assert step.captured
    loss = step.step().clone()
    torch.cuda.synchronize()
    assert torch.isfinite(loss)
    _enc_grads_nonzero(step)


def test_dropout_on_follows_torchs_cuda_generator():
    step, _ = _step(fused=True, p=0.1)
    assert step.text_encoder.fused_attention and step.text_encoder.config.attention_probs_dropout_prob == 0.1
    step.warmup_and_capture(eager_iters=1)
    assert step.captured
    torch.cuda.synchronize()
    rng = torch.cuda.get_rng_state(DEV)
    a = step.step().clone()
    torch.cuda.synchronize()
    torch.cuda.set_rng_state(rng, DEV)
    b = step.step().clone()
    c = step.step().clone()          # (the generator has moved on: other masks)
    torch.cuda.synchronize()
    assert torch.isfinite(a) and torch.equal(a, b), (float(a), float(b))
    assert not torch.equal(a, c)


def test_constructor_refusals_name_the_argument():
    from lavt_hip import ops
    from lavt_hip.engine import TrainStep
    model, enc = _model(), _bert()
    x, ids, mask, tgt = _batch()
    kw = dict(context=ops.StepContext())
    with pytest.raises(ValueError, match="l_feats"):
        TrainStep(model, x, torch.randn(2, 768, N_L, device=DEV), mask, tgt, text_encoder=enc, **kw)
    with pytest.raises(ValueError, match="l_mask"):
        TrainStep(model, x, ids, mask.unsqueeze(-1).float(), tgt, text_encoder=enc, **kw)
    with pytest.raises(ValueError, match="text_encoder.*eval"):
        TrainStep(model, x, ids, mask, tgt, text_encoder=_bert().eval(), **kw)
    with pytest.raises(ValueError, match="text_encoder lives on"):
        TrainStep(model, x, ids, mask, tgt, text_encoder=_bert().cpu(), **kw)
    with pytest.raises(ValueError, match="text_encoder.*valid_indices"):
        TrainStep(model, x, ids, mask, tgt, text_encoder=enc, valid_indices=torch.tensor([0, 1], dtype=torch.int32, device=DEV), **kw)
    # an eval-mode model may carry an eval-mode encoder; and the default is the step of before: no encoder, no 'bert_model.' name
    plain = TrainStep(model, x, det_inputs(2, 64, N_L, seed=3)[1].to(DEV), mask.unsqueeze(-1).float(), tgt, **kw)
    assert plain.text_encoder is None and not any(n.startswith("bert_model.") for n, _ in plain._named_parameters())
