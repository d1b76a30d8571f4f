"""Exact checkpoint and resume of a captured training run (DESIGN.md "Checkpoint and resume"): TrainStep.state_dict() / load_state_dict() through
lavt_hip.checkpoint.save_train_state / load_train_state.

Every scenario, on one GPU with TrainStep(deterministic=True), graph replay and bf16:
  run A   N steps without interruption on a fixed list of batches; the loss bits of every step, and at the end parameters, buffers, both moments (and
          max_exp_avg_sq), the bf16 `lin` copies, the step counter, guard[3], guard[5:7], acc, the DropPath state, the fp8 arrays, torch's generator
  run B   as A, writes a file after m steps (B may go on and write a second file at a later m), and is deleted
  run C   a new model filled from another salt under another seed -- every tensor must be overwritten -- in a new context with a new TrainStep and owned
          optimizer: warmup_and_capture(), load_train_state, N - m steps
and everything recorded of C equals A's bit for bit (the comparison is on the bit patterns: after a NaN batch the BatchNorm statistics hold NaN, which
torch.equal on floats would call unequal to itself); the losses of steps m+1 .. N too.  Nothing is run a second time to look for a difference.

The NaN batch of scenario 2 is an ordinary floating-point value in an input image."""
import math
from types import SimpleNamespace

import pytest
import torch

from lavt_hip.detweights import det_inputs, fill_state_dict_

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OKW = dict(lr=3e-4, weight_decay=1e-2, max_grad_norm=1.0, skip_nonfinite=True, total_steps=40, power=0.9)


def _bits(t):
    t = t.detach().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _eq(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _assert_same(a, b, what):
    assert a.keys() == b.keys(), (what, sorted(a.keys() ^ b.keys())[:6])
    bad = [k for k in a if not _eq(a[k], b[k])]
    assert not bad, f"{what}: {len(bad)} of {len(a)} recorded tensors differ, e.g. {bad[:6]}"


# ------------------------------------------------------------------------------------------------ the models and their batches
def _micro2d(salt):
    """test_gpu_modules._build(32, [2,2,2,2], [1,2,4,8], 7, dpr=0.2) -> (model, the static input buffers)"""
    from test_gpu_modules import _build
    model = _build(32, [2, 2, 2, 2], [1, 2, 4, 8], 7, dpr=0.2)
    if salt:
        fill_state_dict_(model, salt=salt)
    return model.train(), tuple(v.to(DEV) for v in det_inputs(2, 64, 20, seed=100))


def _batches2d(n):
    return [tuple(v.to(DEV) for v in det_inputs(2, 64, 20, seed=100 + i)) for i in range(n)]


def _video_bert(salt):
    """the micro Video-Swin of test_gpu_dice_boundary._video_model (2 clips x 4 frames x 64^2) around the micro BERT of
    test_gpu_modules.test_lavt_one_micro_matches_oracle_chain (1 layer, 12 heads, hidden 768) with dropout 0.1, in training mode"""
    from bert.modeling_bert import BertConfig, BertModel
    from test_gpu_dice_boundary import _video_model
    model = _video_model()[0]
    model.text_encoder = BertModel(BertConfig(vocab_size=64, hidden_size=768, num_hidden_layers=1, num_attention_heads=12, intermediate_size=256,
                                              max_position_embeddings=32, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1), add_pooling_layer=False)
    fill_state_dict_(model, salt=salt)
    model.to(DEV).train()
    assert any(isinstance(mod, torch.nn.Dropout) and mod.p > 0 for mod in model.modules())
    return model, _batches_video(1)[0]


def _batches_video(n):
    out = []
    for i in range(n):
        frames, _, m, tgt = det_inputs(2, 64, 22, seed=300 + i, frames=4)
        mask = m.squeeze(-1).long()
        ids = torch.randint(1, 64, mask.shape, generator=torch.Generator().manual_seed(40 + i)) * mask
        out.append((frames.to(DEV), ids.to(DEV), mask.to(DEV), tgt[[2, 5]].contiguous().to(DEV)))
    return out


# ------------------------------------------------------------------------------------------------ one run
def _start(make, salt, seed, opt_kw, **step_kw):
    """a model from `make(salt)` under torch.manual_seed(seed), in a new context, with an owned optimizer, warmed up and captured"""
    from lavt_hip import ops
    from lavt_hip.engine import TrainStep
    torch.manual_seed(seed)
    model, static = make(salt)
    static = tuple(v.clone() for v in static)
    step = TrainStep(model, *static, context=ops.StepContext(), deterministic=True, **step_kw)
    step.make_optimizer([p for p in model.parameters() if p.requires_grad], **dict(OKW, **opt_kw))
    step.warmup_and_capture()
    assert step.captured
    return step, static


def _snapshot(step):
    from lavt_hip.checkpoint import fp8_site_slots
    torch.cuda.synchronize()
    model, opt, ctx = step.model, step.opt, step.context
    names = {id(p): n for n, p in model.named_parameters()}
    out = {}
    for n, p in model.named_parameters():
        out["p|" + n] = p.detach().clone()
        for k, v in opt.state.get(p, {}).items():
            if torch.is_tensor(v) and k != "step":
                out[f"m|{n}|{k}"] = v.clone()
    for n, b in model.named_buffers():
        out["b|" + n] = b.detach().clone()
    for key, ent in ctx.weights.store.items():
        if key[1] == torch.bfloat16 and key[2] == "lin" and ent[2]() is not None:
            out["lin|" + names[key[0]]] = ent[1].clone()
    out["step"], out["guard3"], out["phase"] = opt._step.clone(), opt.guard[3:4].clone(), opt.guard[5:7].clone()
    if step.acc is not None:
        out["acc"] = step.acc.clone()
    for dev, st in ctx.dp_state.items():
        out[f"droppath|{dev}"] = st.clone()
    if ctx.fp8.prev is not None:
        for n, i in fp8_site_slots(ctx.fp8.slots, names).items():
            out["fp8|" + n] = torch.stack([ctx.fp8.prev[i], ctx.fp8.cur[i]])
    out["rng"] = torch.cuda.get_rng_state(DEV)
    return out


def _steps(step, static, batches, first, last, nan_at=None):
    losses = []
    for i in range(first, last):
        for dst, src in zip(static, batches[i]):
            dst.copy_(src)
        if i == nan_at:
            static[0].fill_(math.nan)
        losses.append(step.step().clone())
    torch.cuda.synchronize()
    return losses


def _scenario(tmp_path, make, batches, saves, dtype=torch.bfloat16, opt_kw=None, nan_at=None, **step_kw):
    """A, B (one file per m in `saves`), one C per file -> (A's snapshot, {m: the file's content}); the assertions of the module docstring"""
    import lavt_hip
    from lavt_hip.checkpoint import load_train_state, save_train_state
    N, opt_kw = len(batches), opt_kw or {}
    with lavt_hip.use_dtype(dtype):
        step, static = _start(make, 0, 1234, opt_kw, **step_kw)
        loss_a = _steps(step, static, batches, 0, N, nan_at)
        snap_a = _snapshot(step)
        del step

        step, static = _start(make, 0, 1234, opt_kw, **step_kw)
        done, files = 0, {}
        for m in saves:
            _steps(step, static, batches, done, m, nan_at)
            done = m
            save_train_state(str(tmp_path / f"at{m}.pt"), step, epoch=m, note="mid-epoch")
            files[m] = torch.load(str(tmp_path / f"at{m}.pt"), map_location="cpu", weights_only=True)
        del step

        for m in saves:
            step, static = _start(make, 7, 99, opt_kw, **step_kw)
            extra = load_train_state(str(tmp_path / f"at{m}.pt"), step)
            assert extra == {"epoch": m, "note": "mid-epoch"}
            assert step.micro_step() == m % step.accumulate
            loss_c = _steps(step, static, batches, m, N, nan_at)
            snap_c = _snapshot(step)
            assert all(_eq(a, c) for a, c in zip(loss_a[m:], loss_c)), (m, [float(v) for v in loss_a[m:]], [float(v) for v in loss_c])
            _assert_same(snap_a, snap_c, f"resumed after {m} of {N} steps")
            del step
    return snap_a, files, loss_a


# ------------------------------------------------------------------------------------------------ 1 - 5
@pytest.mark.parametrize("amsgrad", [False, True])
def test_resume_2d_is_exact(tmp_path, amsgrad):
    """1. 2-D micro, ce, clip 1.0, non-finite skip, DropPath 0.2; N = 5, m = 2; plain and amsgrad=True"""
    snap, files, losses = _scenario(tmp_path, _micro2d, _batches2d(5), [2], opt_kw={"amsgrad": amsgrad})
    assert float(snap["step"]) == 5.0 and float(snap["guard3"]) == 0.0 and all(math.isfinite(float(v)) for v in losses)
    assert any(k.startswith("droppath|") for k in snap) and any(k.startswith("lin|") for k in snap)
    assert any(k.endswith("|max_exp_avg_sq") for k in snap) == amsgrad
    train = files[2]["lavt_train_state"]
    assert train["format"] == 1 and "acc" not in train and train["fp8"] == {} and float(train["guard"][4]) == 0.0
    assert train["droppath"] and all(counter > 0 for _, counter in train["droppath"].values())


def test_resume_after_a_skipped_step_is_exact(tmp_path):
    """2. as 1, with a NaN image in step 2: the skipped step lies before the save; its count and the unmoved step counter carry over"""
    snap, files, _ = _scenario(tmp_path, _micro2d, _batches2d(5), [2], nan_at=1)
    sched = files[2]["optimizer"]["lavt_schedule"]
    assert sched["steps_taken"] == 1 and sched["skipped_steps"] == 1 and float(files[2]["lavt_train_state"]["guard"][3]) == 1.0
    assert float(snap["step"]) == 4.0 and float(snap["guard3"]) == 1.0


def test_resume_inside_and_between_accumulation_cycles_is_exact(tmp_path):
    """3. accumulate=3, N = 9 micro-steps.  m = 4 (micro index 1): the file holds acc, and micro_step() == 1 after the load (asserted in _scenario); m = 6,
    a cycle boundary: no acc in the file.  Both resumed runs end on A's bits."""
    snap, files, _ = _scenario(tmp_path, _micro2d, _batches2d(9), [4, 6], accumulate=3)
    assert float(snap["step"]) == 3.0 and snap["phase"].tolist() == [0.0, 0.0]
    inside, boundary = files[4]["lavt_train_state"], files[6]["lavt_train_state"]
    assert inside["guard"][5:7].tolist() == [1.0, 1.0] and inside["acc"].shape == snap["acc"].shape and bool(inside["acc"].any())
    assert boundary["guard"][5:7].tolist() == [0.0, 0.0] and "acc" not in boundary


def test_resume_fp8_is_exact(tmp_path, monkeypatch):
    """4. LAVT_FP8=1's arithmetic, the fill threshold lowered so that the micro decoder takes the e4m3 convolutions (as test_gpu_deterministic's fp8 test
    does): the |max| history travels by site name.  N = 4, m = 2.
    (No run here takes a snapshot between its warm-up and its first step: with fp8 on, such a read-only snapshot was seen to change the bits of the steps
    after it in uninterrupted runs too -- DESIGN.md "Checkpoint and resume", the open point at the end of "Exactness".)"""
    from lavt_hip import ops
    monkeypatch.setattr(ops, "_FP8_CONV_MIN_TILES", 0)
    snap, files, _ = _scenario(tmp_path, _micro2d, _batches2d(4), [2], dtype="fp8")
    saved = files[2]["lavt_train_state"]["fp8"]
    assert saved and all(n.startswith("classifier.") and n.rsplit("|", 1)[1] in ("act", "dy") and tuple(v.shape) == (2,) for n, v in saved.items())
    assert {"fp8|" + n for n in saved} == {k for k in snap if k.startswith("fp8|")}
    assert any(float(v.abs().max()) > 0 for v in saved.values()) and files[2]["lavt_train_state"]["config"]["fp8"] is True


def test_resume_video_with_bert_dropout_is_exact(tmp_path):
    """5. micro Video-Swin, dice_boundary, valid_indices = [2, 5], the micro BERT in training mode with dropout 0.1: its keep masks are drawn from
    torch's CUDA generator inside the graph.  N = 4, m = 2."""
    vi = torch.tensor([2, 5], dtype=torch.int32, device=DEV)
    snap, files, losses = _scenario(tmp_path, _video_bert, _batches_video(4), [2], loss="dice_boundary", valid_indices=vi)
    assert files[2]["lavt_train_state"]["torch_cuda_rng"].dtype == torch.uint8
    assert not _eq(losses[0], losses[1])


# ------------------------------------------------------------------------------------------------ 6 - 8: one captured step for all
@pytest.fixture(scope="module")
def captured():
    """fp8 + accumulate=2 + amsgrad + DropPath 0.2, captured; one step taken -> an early state_dict (micro index 1); two more steps"""
    import lavt_hip
    from lavt_hip import ops
    mp = pytest.MonkeyPatch()
    mp.setattr(ops, "_FP8_CONV_MIN_TILES", 0)
    try:
        with lavt_hip.use_dtype("fp8"):
            batches = _batches2d(3)
            step, static = _start(_micro2d, 0, 1234, {"amsgrad": True}, accumulate=2)
            _steps(step, static, batches, 0, 1)
            early = step.state_dict()
            early_snap = _snapshot(step)
            _steps(step, static, batches, 1, 3)
            yield SimpleNamespace(step=step, early=early, early_snap=early_snap)
    finally:
        mp.undo()


def _addresses(step):
    ctx, opt = step.context, step.opt
    out = {"p|" + n: p.data_ptr() for n, p in step.model.named_parameters()}
    out.update({"b|" + n: b.data_ptr() for n, b in step.model.named_buffers()})
    for n, p in step.model.named_parameters():
        out.update({f"m|{n}|{k}": v.data_ptr() for k, v in opt.state[p].items() if torch.is_tensor(v)})
    out.update({"step": opt._step.data_ptr(), "guard": opt.guard.data_ptr(), "acc": step.acc.data_ptr(), "fp8 prev": ctx.fp8.prev.data_ptr(),
                "fp8 cur": ctx.fp8.cur.data_ptr()})
    out.update({f"droppath|{dev}": st.data_ptr() for dev, st in ctx.dp_state.items()})
    return out


def test_load_keeps_every_address_and_installs_the_state(captured):
    """6. after load_state_dict on a captured step every parameter, buffer, moment (max_exp_avg_sq included), opt._step, opt.guard, acc, the DropPath
    state and fp8 prev / cur live where they lived; and the state is the early one, bit for bit (compute copies re-made)"""
    step = captured.step
    now = _snapshot(step)
    assert step.micro_step() == 1 and not _eq(now["step"], captured.early_snap["step"])
    want = _addresses(step)
    assert any(k.endswith("|max_exp_avg_sq") for k in want) and any(k.startswith("droppath|") for k in want) and step.context.fp8.slots
    ids = (id(step.opt._step), id(step.opt.guard), id(step.acc), id(step.context.fp8.prev), id(step.context.fp8.cur))
    step.load_state_dict(captured.early)
    assert _addresses(step) == want
    assert ids == (id(step.opt._step), id(step.opt.guard), id(step.acc), id(step.context.fp8.prev), id(step.context.fp8.cur))
    assert step.micro_step() == 1 and step.opt.steps_taken() == 0
    _assert_same(captured.early_snap, _snapshot(step), "the state after the load")


def test_refusals_leave_the_state_alone(captured):
    """7. load before warmup_and_capture(): RuntimeError; FusedAdamW.load_state_dict on the captured owned optimizer: RuntimeError; a checkpoint with
    another accumulate, another amsgrad, a renamed parameter, an fp8 site the model does not have: ValueError naming the field -- and after each the
    step's state is bitwise what it was"""
    import copy

    import lavt_hip
    from lavt_hip import ops
    from lavt_hip.engine import TrainStep
    step = captured.step
    before = _snapshot(step)
    with lavt_hip.use_dtype("fp8"):
        model, static = _micro2d(0)
        cold = TrainStep(model, *static, context=ops.StepContext(), deterministic=True, accumulate=2)
        cold.make_optimizer([p for p in model.parameters()], **dict(OKW, amsgrad=True))
        with pytest.raises(RuntimeError, match="warmup_and_capture"):
            cold.load_state_dict(captured.early)
    with pytest.raises(RuntimeError, match="TrainStep.load_state_dict"):
        step.opt.load_state_dict(captured.early["optimizer"])

    def edited(fn):
        sd = copy.deepcopy(captured.early)
        fn(sd["lavt_train_state"])
        return sd

    def rename(train):
        train["config"]["param_groups"][0][3][0] += "_renamed"

    def site(train):
        train["fp8"]["classifier.no_such_conv.weight|act"] = torch.zeros(2)
    cases = [(lambda t: t["config"].update(accumulate=3), "'accumulate'"), (lambda t: t["config"].update(amsgrad=False), "'amsgrad'"),
             (rename, "'param_groups'.*_renamed"), (site, "fp8 site 'classifier.no_such_conv.weight.act'")]
    for fn, match in cases:
        with pytest.raises(ValueError, match=match):
            step.load_state_dict(edited(fn))
        _assert_same(before, _snapshot(step), f"after the refusal of {match}")


def test_file_entries_load_into_torch_adamw_and_a_plain_model(captured, tmp_path):
    """8. the reference's resume lines on the file: model.load_state_dict(ckpt['model']) (train.py:610) and optimizer.load_state_dict(ckpt['optimizer'])
    (train.py:724) with a torch.optim.AdamW"""
    from lavt_hip.checkpoint import save_train_state
    from test_gpu_modules import _build
    path = str(tmp_path / "ckpt.pt")
    save_train_state(path, captured.step, epoch=3)
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    assert set(ckpt) == {"model", "optimizer", "lavt_train_state", "epoch"} and ckpt["epoch"] == 3
    model = _build(32, [2, 2, 2, 2], [1, 2, 4, 8], 7, dpr=0.2)
    fill_state_dict_(model, salt=5)
    res = model.load_state_dict(ckpt["model"])
    assert not res.missing_keys and not res.unexpected_keys
    for (n, p), (_, q) in zip(model.named_parameters(), captured.step.model.named_parameters()):
        assert _eq(p.detach(), q.detach()), n
    ps = [p for p in model.parameters()]
    opt = torch.optim.AdamW(ps, lr=1e-3, amsgrad=True)
    opt.load_state_dict(ckpt["optimizer"])
    mine = captured.step.opt
    assert opt.param_groups[0]["lr"] == OKW["lr"] and opt.param_groups[0]["amsgrad"] is True
    for p, q in zip(ps, [q for q in captured.step.model.parameters()]):
        for k in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
            assert _eq(opt.state[p][k], mine.state[q][k]), k
        assert float(opt.state[p]["step"]) == float(mine.steps_taken())
