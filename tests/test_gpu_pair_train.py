"""GPU checks of pair-list TRAIN batches: lavt_gather_samples_bwd, ops.gather_pairs, MultiModalSwinTransformer.forward(image_of=) in training mode and
TrainStep(image_of=).

The kernel through the C ABI against tests/pair_train_ref.py (exact on integer data; bit for bit on random data: the summation order is part of the
contract).  The step on the micro 2-D geometry of tests/test_gpu_eval_pairs.py (embed_dim 32, depths 2-2-2-2, heads 1-2-4-8, window 7, 64 x 64 images,
20 tokens) against the plain TrainStep on the gathered images `x[image_of]` -- the code path a step without image_of takes, unchanged here.  The fp32
gates are those of tests/test_gpu_modules.py::test_e2e_micro_train_grads_golden, quoted:

    assert abs(float(loss) - float(g["loss"])) < 1e-4
    if not err <= 2e-3 * max(float(ref[0]), 1e-6) + 5e-6:          # ref[0] = the gradient's L2 norm

applied here to max |g_pair - g_plain| of every parameter (that test applies them to a digest of 24 entries).  For mc_dice and dice_boundary the same
2e-3 is asked of the flat gradient's relative L2 error.  No bound below is taken from what the code gives."""
import numpy as np
import pytest
import torch

from lavt_hip.detweights import det_inputs, fill_state_dict_
from pair_train_ref import bounded_integer_samples, gather_bwd_index_add, gather_bwd_sequential, integer_samples
from test_gpu_eval_pairs import ARGS, IMAGE_SEED

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16]
PAIRS = [1, 0, 1, 1, 0]          # unequal multiplicities: image 1 three times, image 0 twice


@pytest.fixture(autouse=True)
def _fp32():
    import lavt_hip
    lavt_hip.set_compute_dtype(torch.float32)
    yield
    lavt_hip.set_compute_dtype(torch.float32)


def _i32(values):
    return torch.tensor(list(values), dtype=torch.int32, device=DEV)


# ================================================================================================ 1-3. the kernel through the C ABI
def _launch(dy, sel, B, per, dx, nsel=None, dtype=None):
    from lavt_hip import _capi as K
    rc = K.lib.lavt_gather_samples_bwd(K.dt(dy.dtype) if dtype is None else dtype, K.ptr(dy), K.ptr(sel), sel.numel() if nsel is None else nsel, B, per, K.ptr(dx), K.stream())
    torch.cuda.synchronize()
    return rc


def _offset_view(n, dtype, off):
    """n elements of NaN whose base is `off` elements past a 256-byte allocation boundary"""
    return torch.full((n + off,), float("nan"), dtype=dtype, device=DEV)[off:]


SEL7 = [2, 0, 2, -1, 2, 7, 0]          # B = 3: image 1 is named by nobody, -1 and 7 are out of range
KERNEL_CASES = [  # (id, B, sel, sample_elems, offset of dy's base, offset of dx's base)
    ("1", 3, SEL7, 1, 0, 0),
    ("7-elementwise", 3, SEL7, 7, 0, 0),
    ("1568-vector", 3, SEL7, 1568, 0, 0),
    ("14400x32", 3, SEL7, 14400 * 32, 0, 0),
    ("1568-dy-misaligned", 3, SEL7, 1568, 1, 0),
    ("1568-dx-misaligned", 3, SEL7, 1568, 0, 1),
    ("one-slot-one-image", 1, [0], 1568, 0, 0),
    # 57 (bf16) / 113 (fp32) tiles of 1024 16-byte chunks against a grid of 2048 // 64 = 32 columns: the grid-stride loop takes a second pass (and a
    # fourth), which 14400 x 32 at B = 3 does not reach
    ("14400x32-64-images-grid-stride", 64, [63, 0, 63], 14400 * 32, 0, 0),
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", KERNEL_CASES, ids=[c[0] for c in KERNEL_CASES])
def test_kernel_is_exact_on_integer_data(case, dtype):
    _, B, sel, per, off_y, off_x = case
    dy_host = integer_samples(per % 1000 + B, len(sel), per, dtype)
    dy = _offset_view(len(sel) * per, dtype, off_y)
    dy.copy_(dy_host.reshape(-1))
    dx = _offset_view(B * per, dtype, off_x)
    assert (dy.data_ptr() % 16 != 0) == bool(off_y) and (dx.data_ptr() % 16 != 0) == bool(off_x)
    assert _launch(dy, _i32(sel), B, per, dx) == 0
    got = dx.cpu().reshape(B, per)
    want = gather_bwd_index_add(dy_host, sel, B)
    assert torch.equal(got.double(), want), f"max |error| {float((got.double() - want).abs().max())}"
    assert torch.equal(got, gather_bwd_sequential(dy_host, sel, B))
    named = {b for b in sel if 0 <= b < B}
    for b in range(B):
        if b not in named:
            assert not got[b].any(), f"image {b} is named by nobody: zeros over the NaN fill"
        else:
            assert got[b].any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_kernel_with_65535_slots(dtype):
    """B = 2, nsel = 65 535, 4 elements per sample: every workgroup walks the whole list.  The data keeps every partial sum an integer of at most 248, so
    fp32 and bf16 are exact all the way"""
    sel = [(j * 7 // 3) % 2 for j in range(65535)]
    dy_host = bounded_integer_samples(9, sel, 2, 4, dtype)
    dx = _offset_view(2 * 4, dtype, 0)
    assert _launch(dy_host.to(DEV).reshape(-1), _i32(sel), 2, 4, dx) == 0
    got, want = dx.cpu().reshape(2, 4), gather_bwd_index_add(dy_host, sel, 2)
    assert torch.equal(got.double(), want) and want.abs().sum() > 0


def test_kernel_order_is_ascending_fp32_and_one_rounding():
    """random data, B = 2, sel = [1, 0, 1, 1, 0, 1], 1568 elements: the bits of the sequential ascending-j fp32 sum; bf16: of that sum rounded once; the
    same bits from a second launch"""
    sel, per = [1, 0, 1, 1, 0, 1], 1568
    host = torch.randn(6, per, generator=torch.Generator("cpu").manual_seed(21))
    for dtype in DTYPES:
        dy_host = host.to(dtype)
        dy, seld = dy_host.to(DEV).reshape(-1), _i32(sel)
        a, b = _offset_view(2 * per, dtype, 0), _offset_view(2 * per, dtype, 0)
        assert _launch(dy, seld, 2, per, a) == 0 and _launch(dy, seld, 2, per, b) == 0
        want = gather_bwd_sequential(dy_host, sel, 2)
        assert torch.equal(a.cpu().reshape(2, per), want), f"{dtype}: not the sequential fp32 sum" + (" rounded once" if dtype == torch.bfloat16 else "")
        assert torch.equal(a, b)


def test_kernel_refuses_bad_arguments():
    from lavt_hip import _capi as K
    per = 8
    dy, sel = torch.ones(4 * per, device=DEV), _i32([0, 1, 0, 1])
    for kw, what in ((dict(nsel=0), "nsel"), (dict(nsel=65536), "nsel"), (dict(dtype=2), "dtype")):
        dx = _offset_view(2 * per, torch.float32, 0)
        assert _launch(dy, sel, 2, per, dx, **kw) == -22
        assert "lavt_gather_samples_bwd" in K.lib.lavt_last_error().decode() and what in K.lib.lavt_last_error().decode()
        assert bool(dx.isnan().all()), "nothing was launched"


# ================================================================================================ 4. the op
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", ["BLC", "NCHW-view-of-NHWC"])
def test_gather_pairs_equals_index_select_and_its_autograd(layout, dtype):
    from lavt_hip import ops
    B, sel = 3, [2, 0, 2, 2, 0]
    g = torch.Generator("cpu").manual_seed(4)
    if layout == "BLC":
        x_host, gy_host = torch.randint(-8, 9, (B, 49, 32), generator=g).to(dtype), torch.randint(-8, 9, (5, 49, 32), generator=g).to(dtype)
        x, gy = x_host.to(DEV).requires_grad_(True), gy_host.to(DEV)
    else:
        x_host, gy_host = torch.randint(-8, 9, (B, 7, 5, 16), generator=g).to(dtype), torch.randint(-8, 9, (5, 7, 5, 16), generator=g).to(dtype)
        x_host, gy_host = x_host.permute(0, 3, 1, 2), gy_host.permute(0, 3, 1, 2)
        x, gy = x_host.to(DEV).requires_grad_(True), gy_host.to(DEV)
        assert not x.is_contiguous() and x.stride() == x_host.stride()
    xr = x_host.double().requires_grad_(True)
    torch.index_select(xr, 0, torch.tensor(sel)).backward(gy_host.double())
    y = ops.gather_pairs(x, _i32(sel))
    assert y.stride()[1:] == x.stride()[1:] and torch.equal(y.detach().cpu(), x_host[sel])
    y.backward(gy)
    torch.cuda.synchronize()
    assert x.grad.shape == x.shape and torch.equal(x.grad.cpu().double(), xr.grad)
    assert not x.grad[1].any(), "image 1 is named by nobody"
    x2 = x.detach().requires_grad_(True)
    ops.gather_pairs(x2, _i32(sel)).backward(gy.contiguous())          # a contiguous gradient for a permuted output is put into the output's layout first
    assert torch.equal(x2.grad.cpu().double(), xr.grad)
    with pytest.raises(RuntimeError, match="GPU memory only"):
        ops.gather_pairs(x_host, _i32(sel))
    with pytest.raises(ValueError):
        ops.gather_pairs(x, _i32(sel).long())
    assert not ops.gather_samples(x, _i32(sel), pairs=True).requires_grad, "gather_samples stays outside autograd"


# ================================================================================================ the step on the micro geometry
def _micro(sd=None, dpr=0.0):
    from lib._utils import LAVT
    from lib.backbone import MultiModalSwinTransformer
    from lib.mask_predictor import SimpleDecoding
    bb = MultiModalSwinTransformer(embed_dim=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8], window_size=7, drop_path_rate=dpr, args=ARGS)
    model = LAVT(bb, SimpleDecoding(256, ARGS))
    fill_state_dict_(model)
    if sd is not None:
        model.load_state_dict(sd)
    return model.to(DEV).train()


class _Batch:
    def __init__(self):
        self.x = det_inputs(2, 64, 20, seed=IMAGE_SEED)[0].to(DEV)
        _, l, m, t = det_inputs(5, 64, 20, seed=77)
        self.l, self.m, self.t = l.to(DEV), m.to(DEV), t.to(DEV)
        self.t2 = det_inputs(5, 64, 20, seed=78)[3].to(DEV)
        self.sd = {k: v.clone() for k, v in _micro().state_dict().items()}


@pytest.fixture(scope="module")
def batch():
    return _Batch()


def _one_step(batch, dtype, loss, pairs):
    """an eager deterministic step from the batch's state dict -> (loss, {name: gradient}, stats); pairs=None: the plain step on x[PAIRS]"""
    import lavt_hip
    from lavt_hip import ops
    from lavt_hip.engine import TrainStep
    with lavt_hip.use_dtype(dtype):
        model = _micro(batch.sd)
        if pairs is None:
            step = TrainStep(model, batch.x[PAIRS].contiguous(), batch.l, batch.m, batch.t, context=ops.StepContext(), use_graph=False, deterministic=True, loss=loss)
        else:
            step = TrainStep(model, batch.x, batch.l, batch.m, batch.t, context=ops.StepContext(), use_graph=False, deterministic=True, loss=loss, image_of=_i32(pairs))
        step.warmup_and_capture(eager_iters=2)          # (eager: no capture; no optimizer: the parameters stay, and train-mode BatchNorm does not read its buffers)
        out = step.step().clone()
        torch.cuda.synchronize()
        grads = {n: (p.grad.detach().float().clone() if p.grad is not None else None) for n, p in model.named_parameters()}
        return float(out), grads, step.stats.clone()


_PLAIN = {}


def _plain(batch, dtype, loss):
    """the reference runs, computed once per (dtype, loss) and shared"""
    key = (dtype, loss)
    if key not in _PLAIN:
        _PLAIN[key] = _one_step(batch, dtype, loss, None)
    return _PLAIN[key]


def _grads(model):
    """every parameter gradient of the last step, flattened in named_parameters order"""
    return torch.cat([p.grad.detach().reshape(-1).clone() for _, p in model.named_parameters() if p.grad is not None])


def _flat(grads, names):
    return torch.cat([grads[n].reshape(-1).double() for n in names])


def _front(name):
    """is the parameter in front of the gather (its gradient passes lavt_gather_samples_bwd)?"""
    return name.startswith("backbone.patch_embed.") or name.startswith("backbone.layers.0.blocks.")


def test_step_parity_fp32_ce(batch):
    loss_ref, g_ref, stats_ref = _plain(batch, torch.float32, "ce")
    loss, g, stats = _one_step(batch, torch.float32, "ce", PAIRS)
    print(f"\nloss pair {loss:.7f} plain {loss_ref:.7f}")
    assert abs(loss - loss_ref) < 1e-4
    assert float(stats_ref[3]) > 0 and float((stats[2:4] - stats_ref[2:4]).abs().max()) <= 2, "I / U over the N samples (a pixel on the decision boundary may flip)"
    bad, same_behind, n_behind, n_front = [], 0, 0, 0
    for n, ref in g_ref.items():
        if ref is None or float(ref.abs().max()) == 0.0:
            assert g[n] is None or float(g[n].abs().max()) == 0.0, f"{n}: the reference leaves it without gradient"
            continue
        err, norm = float((g[n] - ref).abs().max()), float(ref.norm())
        if not err <= 2e-3 * norm + 5e-6:
            bad.append((n, err, norm))
        if _front(n):
            n_front += 1
        else:
            n_behind += 1
            same_behind += int(torch.equal(g[n], ref))
    print(f"parameters behind the gather (stages 1-3, every PWAM / gate, decoder): {same_behind} of {n_behind} gradients bit-identical to the plain step; {n_front} in front")
    assert n_front > 0 and n_behind > 0
    assert not bad, f"{len(bad)} parameter gradients off: {bad[:8]}"


@pytest.mark.parametrize("loss", ["mc_dice", "dice_boundary"])
def test_step_parity_fp32_other_criteria(batch, loss):
    loss_ref, g_ref, _ = _plain(batch, torch.float32, loss)
    out, g, _ = _one_step(batch, torch.float32, loss, PAIRS)
    names = [n for n, r in g_ref.items() if r is not None]
    rel = float((_flat(g, names) - _flat(g_ref, names)).norm() / _flat(g_ref, names).norm())
    print(f"\n{loss}: loss pair {out:.7f} plain {loss_ref:.7f}; flat gradient relative L2 error {rel:.3e}")
    assert abs(out - loss_ref) < 1e-4 and rel <= 2e-3


def test_step_parity_bf16(batch):
    """against the fp32 plain run: in each parameter group the pair run's relative L2 error must not exceed 1.5 x the bf16 plain run's (the pair path sums
    the slot gradients in fp32 and rounds once: it should not be worse; the margin absorbs the noise of a micro model)"""
    _, g32, _ = _plain(batch, torch.float32, "ce")
    _, g_plain, _ = _plain(batch, torch.bfloat16, "ce")
    _, g_pair, _ = _one_step(batch, torch.bfloat16, "ce", PAIRS)
    names = [n for n, r in g32.items() if r is not None and float(r.abs().max()) > 0.0]
    for group, pick in (("in front of the gather", _front), ("all others", lambda n: not _front(n))):
        sel = [n for n in names if pick(n)]
        ref = _flat(g32, sel)
        e_plain, e_pair = float((_flat(g_plain, sel) - ref).norm() / ref.norm()), float((_flat(g_pair, sel) - ref).norm() / ref.norm())
        print(f"\nbf16 against fp32 plain, {group} ({len(sel)} parameters): plain {e_plain:.4e}, pair {e_pair:.4e}, ratio {e_pair / e_plain:.3f}")
        assert e_pair <= 1.5 * e_plain, f"{group}: pair {e_pair:.4e} against plain {e_plain:.4e}"


@pytest.mark.parametrize("dtype", DTYPES)
def test_replay_follows_the_buffer(batch, dtype):
    """captured with [0, 0, 1, 1, 1]; replay; set_image_of([1, 1, 0, 0, 1]) and new targets; replay: each time the bits of the eager pair step on the same
    buffers (deterministic mode; no optimizer: the parameters stay)"""
    import lavt_hip
    from lavt_hip import ops
    from lavt_hip.engine import TrainStep
    first, second = [0, 0, 1, 1, 1], [1, 1, 0, 0, 1]
    with lavt_hip.use_dtype(dtype):
        steps = []
        for use_graph in (True, False):
            step = TrainStep(_micro(batch.sd), batch.x, batch.l, batch.m, batch.t.clone(), context=ops.StepContext(), use_graph=use_graph, deterministic=True,
                             image_of=_i32(first))
            step.warmup_and_capture()
            assert step.captured == use_graph
            steps.append(step)
        seen = []
        for pairs, tgt in ((first, batch.t), (second, batch.t2)):
            out = []
            for step in steps:
                step.set_image_of(pairs)
                step.t.copy_(tgt)
                loss = step.step().clone()
                torch.cuda.synchronize()
                assert step.image_of.tolist() == pairs
                out.append((loss, _grads(step.model)))
            assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]), f"{pairs}: replay and eager differ"
            assert bool(out[0][1].isfinite().all()) and float(out[0][1].abs().max()) > 0
            seen.append(out[0])
        assert not torch.equal(seen[0][1], seen[1][1]), "the second replay followed the buffer"
        with pytest.raises(ValueError):
            steps[0].set_image_of([0, -1, 1, 1, 1])


def test_droppath_draw_in_pair_mode(batch):
    """one launch, one tick: width max(B, N), stage 0's modules take B columns, the others N; the default draw is the draw it was, bit for bit"""
    from lavt_hip import ops
    with ops.use_context(ops.StepContext()):
        bb = _micro(batch.sd, dpr=0.2).backbone
        dev = torch.device(DEV)
        ops.droppath_draw(torch.ones(1, 1, device=dev), 1)          # (creates the generator)
        ops.droppath_reseed(99, dev)
        bb._draw_drop_path(2, dev, slots=5)
        live = [(li, blk.drop_path) for li, layer in enumerate(bb.layers) for blk in layer.blocks if blk.drop_path.drop_prob > 0]
        assert [tuple(f.shape) for li, d in live for f in d._batched] == [((2,) if li == 0 else (5,)) for li, d in live for _ in (0, 1)]
        pair_rows = torch.stack([torch.nn.functional.pad(f, (0, 5 - f.numel())) for _, d in live for f in d._batched])
        assert ops.droppath_state_dict()[str(dev)] == (99, 1), "one tick of the generator"
        ops.droppath_reseed(99, dev)
        want = ops.droppath_draw(bb._dp_keep, 5)
        for r, (row, w) in enumerate(zip(pair_rows, want)):
            n = 2 if live[r // 2][0] == 0 else 5
            assert torch.equal(row[:n], w[:n]), "the leading columns of one draw of width 5"
        ops.droppath_reseed(99, dev)
        bb._draw_drop_path(2, dev)
        default = torch.stack([f for _, d in live for f in d._batched])
        ops.droppath_reseed(99, dev)
        assert torch.equal(default, ops.droppath_draw(bb._dp_keep, 2)) and ops.droppath_state_dict()[str(dev)] == (99, 1)
        for _, d in live:
            d._batched = None


def test_determinism_with_droppath_and_accumulation(batch):
    """drop_path_rate 0.2, deterministic: two steps from the same state (parameters, buffers, DropPath generator) give the same bits; accumulate=2 with an
    owned optimizer completes one cycle with a finite update, and the state dict carries the slot count"""
    from lavt_hip import ops
    from lavt_hip.engine import TrainStep
    dev = torch.device(DEV)
    sd = {k: v.clone() for k, v in _micro(batch.sd, dpr=0.2).state_dict().items()}
    ctx = ops.StepContext()
    model = _micro(sd, dpr=0.2)
    step = TrainStep(model, batch.x, batch.l, batch.m, batch.t, context=ctx, use_graph=False, deterministic=True, image_of=_i32(PAIRS))
    step.warmup_and_capture(eager_iters=2)
    runs = []
    for _ in range(2):
        with ops.use_context(ctx):
            ops.droppath_reseed(4321, dev)
        model.load_state_dict(sd)
        loss = step.step().clone()
        torch.cuda.synchronize()
        runs.append((loss, _grads(model)))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    with ops.use_context(ctx):
        ops.droppath_reseed(1234, dev)
    model.load_state_dict(sd)
    other = step.step().clone()
    torch.cuda.synchronize()
    assert not torch.equal(_grads(model), runs[0][1]), "another seed drops other paths: DropPath is live in pair mode"
    del other

    model = _micro(sd, dpr=0.2)
    step = TrainStep(model, batch.x, batch.l, batch.m, batch.t, context=ops.StepContext(), deterministic=True, accumulate=2, image_of=_i32(PAIRS))
    step.make_optimizer(lr=1e-3, weight_decay=1e-2, max_grad_norm=1.0, skip_nonfinite=True)
    step.warmup_and_capture()
    assert step.captured
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    step.step()
    torch.cuda.synchronize()
    assert all(torch.equal(p, before[n]) for n, p in model.named_parameters()), "the first micro-step of a cycle updates nothing"
    step.set_image_of([0, 1, 0, 0, 1])
    step.step()
    torch.cuda.synchronize()
    assert step.micro_step() == 0
    assert all(bool(p.isfinite().all()) for p in model.parameters())
    moved = [n for n, p in model.named_parameters() if not torch.equal(p, before[n])]
    assert any(n.startswith("backbone.layers.0.blocks.") for n in moved) and any(n.startswith("classifier.") for n in moved)
    state = step.state_dict()
    assert state["lavt_train_state"]["config"]["pair_slots"] == 5
    step.load_state_dict(state)
    plain = dict(state["lavt_train_state"]["config"])
    del plain["pair_slots"]
    state["lavt_train_state"]["config"] = plain
    with pytest.raises(ValueError, match="pair_slots"):
        step.load_state_dict(state)


def test_load_batch_brings_two_images_and_five_masks(batch):
    from lavt_hip import ops, preprocess as P
    from lavt_hip.engine import TrainStep
    rng = np.random.default_rng(3)
    images = [rng.integers(0, 256, (48, 80, 3), dtype=np.uint8), rng.integers(0, 256, (97, 61, 3), dtype=np.uint8)]
    masks = [rng.integers(0, 2, s, dtype=np.uint8) for s in ((48, 80), (97, 61), (97, 61), (48, 80), (97, 61))]
    x, t = torch.full((2, 3, 64, 64), float("nan"), device=DEV), torch.full((5, 64, 64), -1, dtype=torch.int64, device=DEV)
    step = TrainStep(_micro(batch.sd), x, batch.l, batch.m, t, context=ops.StepContext(), use_graph=False, image_of=_i32(PAIRS))
    step.load_batch(images, masks)
    torch.cuda.synchronize()
    pp = P.FramePreprocessor((64, 64))
    assert step.x is x and step.t is t
    assert torch.equal(x, torch.cat([pp.images(a[None]) for a in images])) and torch.equal(t, torch.cat([pp.targets(m[None]) for m in masks]))
    with pytest.raises(ValueError, match="target masks"):
        step.stage_batch(images, masks[:2])
    with pytest.raises(ValueError, match="frames"):
        step.stage_batch(images + images[:1], masks)
