"""Shared by tests/golden/make_optim_bits_golden.py and tests/test_gpu_optim_bits.py: the cases whose every output bit the fused optimizer must keep, and
the one function that runs a case on the GPU and digests what it wrote.  The maker records the digests from a commit known to be good; the test runs
the same function on the code under test and compares for equality.

Data, seeded on the CPU.  Flat state offsets (elements) 0, 8192, 24640, 32833, 41024, 49219, 49220:
  (128, 64)   one whole aligned chunk, with a bf16 'lin' compute copy          (257, 64)  two whole aligned chunks + a tail of 64, with a copy
  (8193,)     an aligned whole chunk + a tail of one                            (8191,)    one element short of a chunk
  (8195,)     a parameter that is a VIEW 4 bytes off 16-byte alignment: a whole chunk taken element by element, + a tail of 3
  (1,), (7,)  single-workgroup tails
Three groups: the defaults; one with its own lr; one with weight decay 0.  total_steps = 10, so the poly schedule moves on every step.  beta2 = 0.95 and
the gradients shrink (SCALES), so that AMSGrad's running maximum binds.  MAX_NORM lies between the smallest and the largest gradient norm of the
applied steps (asserted in inputs()): the clip coefficient is below 1 on some steps and exactly 1 on others.

Only API that the recording commit and the code under test share is used: the FusedAdamW constructor, step(), hold(), swap_ema(), set_grad_source(),
state[p], .guard, last_nonfinite(), the per-tensor sums, ops.weights.get / ops.weights.store and lavt_grad_accumulate."""
import functools
import hashlib

import torch

DEV = "cuda:0"
SHAPES = [(128, 64), (257, 64), (8193,), (8191,), (8195,), (1,), (7,)]
COPIES = (0, 1)                        # tensors with a bf16 'lin' compute copy
OFF16 = 4                              # the tensor whose parameter is a view 4 bytes off 16-byte alignment
SCALES = [1.0, 0.05, 0.05, 1.0, 0.02]  # gradient scale of steps 1..5
MICRO_SCALES = [1.0, 1.0, 1.0, 0.05, 0.05, 0.05]          # accumulation: two cycles of ACC_K micro-batches
MAX_NORM = 10.0
KW = dict(lr=1e-2, weight_decay=0.05, betas=(0.9, 0.95))
T, POWER, DECAY, ACC_K = 10, 0.9, 0.9, 3
INF_AT = (2, 5)                        # guarded cases, step 3: (tensor, element) of the one Inf
STREAMS = ("exp_avg", "exp_avg_sq", "max_exp_avg_sq", "ema")

FORMS = [(g, a, e) for g in (False, True) for a in (False, True) for e in (False, True)]


def form_name(guarded, amsgrad, ema):
    return ("guarded" if guarded else "plain") + ("_amsgrad" if amsgrad else "") + ("_ema" if ema else "")


CASES = [form_name(*f) for f in FORMS] + ["accumulate_guarded_ema", "tensor_norms", "ema_swap"]


@functools.lru_cache(maxsize=None)
def inputs():
    """CPU tensors, computed once, never written: the parameters, five gradient sets, six micro-batch gradient sets, what an earlier cycle left in acc"""
    g = torch.Generator().manual_seed(20261020)
    params = [torch.randn(*s, generator=g) for s in SHAPES]
    grads = [[torch.randn(*s, generator=g) * sc for s in SHAPES] for sc in SCALES]
    micro = [[torch.randn(*s, generator=g) * sc for s in SHAPES] for sc in MICRO_SCALES]
    stale = torch.randn(sum(p.numel() for p in params), generator=g)
    norms = [float(torch.cat([x.double().reshape(-1) for x in gs]).norm()) for gs in grads]
    assert min(norms) < MAX_NORM < max(norms), norms
    cycles = [float(sum(torch.cat([x.double().reshape(-1) for x in gs]) for gs in micro[c:c + ACC_K]).norm()) / ACC_K for c in (0, ACC_K)]
    assert min(cycles) < MAX_NORM < max(cycles), cycles
    return dict(params=params, grads=grads, micro=micro, stale=stale)


def digest(t):
    t = t.detach()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def _groups(ps):
    return [{"params": ps[:3]}, {"params": ps[3:5], "lr": 3e-3}, {"params": ps[5:], "weight_decay": 0.0}]


def _make(**kw):
    """GPU copies of the parameters (the OFF16 one as a misaligned view), the bf16 copies of COPIES, one FusedAdamW over the three groups"""
    from lavt_hip import ops
    from lavt_hip.optim import FusedAdamW
    ps = []
    for i, p in enumerate(inputs()["params"]):
        if i == OFF16:
            q = torch.nn.Parameter(torch.zeros(p.numel() + 8, device=DEV)[1:1 + p.numel()])
            with torch.no_grad():
                q.copy_(p)
            assert q.data_ptr() % 16 == 4 and q.is_contiguous()
        else:
            q = torch.nn.Parameter(p.clone().to(DEV))
        ps.append(q)
    for i in COPIES:
        ops.weights.get(ps[i], torch.bfloat16, "lin")
    return ps, FusedAdamW(_groups(ps), total_steps=T, power=POWER, **KW, **kw)


def _set_grads(ps, gs, inf_at=None):
    for i, (q, gr) in enumerate(zip(ps, gs)):
        gr = gr.clone()
        if inf_at is not None and i == inf_at[0]:
            gr.view(-1)[inf_at[1]] = float("inf")
        q.grad = gr.to(DEV)


def _snapshot(out, tag, opt, ps):
    """one digest per stream and tensor of everything an update may write, so that a difference names the case, the step and the stream"""
    from lavt_hip import ops
    torch.cuda.synchronize()
    for i, p in enumerate(ps):
        out[f"{tag}/param{i}"] = digest(p)
        for key in STREAMS:
            if key in opt.state[p]:
                out[f"{tag}/{key}{i}"] = digest(opt.state[p][key])
    with ops.use_context(opt.context):
        for i in COPIES:
            out[f"{tag}/copy{i}"] = digest(ops.weights.store[(id(ps[i]), torch.bfloat16, "lin")][1])
    out[f"{tag}/step_counter"] = digest(opt.state[ps[0]]["step"])
    if opt.guard is not None:
        out[f"{tag}/ctl"] = digest(opt.guard)


def _five_steps(out, opt, ps, guarded, after_step=None):
    """steps 1, 2 and 5 with ordinary gradients; guarded: step 3 carries one Inf and is skipped, step 4 runs under hold(True), released afterwards"""
    for k, gs in enumerate(inputs()["grads"]):
        _set_grads(ps, gs, INF_AT if guarded and k == 2 else None)
        if guarded and k == 3:
            opt.hold(True)
        opt.step()
        _snapshot(out, f"step{k + 1}", opt, ps)
        if after_step is not None:
            after_step(k)
        if guarded and k == 3:
            opt.hold(False)


def _accumulate(out):
    from lavt_hip import _capi as K
    D = inputs()
    ps, opt = _make(ema_decay=DECAY, max_grad_norm=MAX_NORM, skip_nonfinite=True)
    n = sum(p.numel() for p in ps)
    flat, acc = torch.zeros(n, device=DEV), D["stale"].to(DEV)
    off = 0
    for p in ps:
        p.grad = flat[off:off + p.numel()].view_as(p)
        off += p.numel()
    opt.set_grad_source(flat, acc)
    for c, gs in enumerate(D["micro"]):
        flat.copy_(torch.cat([x.reshape(-1) for x in gs]))
        K.check(K.lib.lavt_grad_accumulate(K.ptr(flat), K.ptr(acc), n, ACC_K, K.ptr(opt.guard), K.stream()))
        opt.step()
        _snapshot(out, f"micro{c + 1}", opt, ps)
        out[f"micro{c + 1}/acc"] = digest(acc)


def _tensor_norms(out):
    ps, opt = _make(max_grad_norm=MAX_NORM, skip_nonfinite=True, tensor_norms=True)

    def sums(k):
        out[f"step{k + 1}/tensor_sums"] = digest(opt._tn[1])
        out[f"step{k + 1}/last_nonfinite"] = repr(opt.last_nonfinite())
    _five_steps(out, opt, ps, True, sums)


def _ema_swap(out):
    ps, opt = _make(ema_decay=DECAY)
    for gs in inputs()["grads"][:2]:
        _set_grads(ps, gs)
        opt.step()
    for tag in ("swap1", "swap2"):
        opt.swap_ema()
        _snapshot(out, tag, opt, ps)


def run_case(name):
    """{label: sha256 of the raw bytes (or, for last_nonfinite, the repr)} of case `name`, in the order written"""
    out = {}
    if name == "accumulate_guarded_ema":
        _accumulate(out)
    elif name == "tensor_norms":
        _tensor_norms(out)
    elif name == "ema_swap":
        _ema_swap(out)
    else:
        guarded, amsgrad, ema = FORMS[CASES.index(name)]
        kw = dict(max_grad_norm=MAX_NORM, skip_nonfinite=True) if guarded else {}
        ps, opt = _make(amsgrad=amsgrad, ema_decay=DECAY if ema else None, **kw)
        assert (opt.guard is not None) == guarded
        _five_steps(out, opt, ps, guarded)
    return out
