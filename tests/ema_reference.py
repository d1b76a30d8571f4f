"""The CPU reference of the weight-EMA tests (test_ema_host.py, test_gpu_ema.py): torch.optim.AdamW + LambdaLR +
torch.optim.swa_utils.AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(0.9)) on the data of tests/test_gpu_amsgrad.py (seed 23, its SHAPES and SCALES,
lr=1e-2, weight_decay=0.05, betas=(0.9, 0.95)).  Pure torch, nothing of the product is run.  Computed once per form, shared, read-only."""
import functools

import torch
from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

from test_gpu_amsgrad import KW, POWER, SCALES, SHAPES, T, _groups

DECAY = 0.9
EMA_GATE = 3e-6          # |e - ref| <= EMA_GATE * max(1, |ref|max): 2e-6, the project's parameter gate (the average is a convex combination of iterates
                         # that each meet it) + 1e-6 for the spread between equivalent fp32 formulations of the rule (lerp / multiply-add / fused
                         # multiply-add differ by at most 2.8e-7 on this data)


class _Bag(torch.nn.Module):
    def __init__(self, params):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(p.clone()) for p in params])


@functools.lru_cache(maxsize=None)
def data():
    g = torch.Generator().manual_seed(23)
    params = [torch.randn(*s, generator=g) for s in SHAPES]
    grads = [[torch.randn(*s, generator=g) * sc for s in SHAPES] for sc in SCALES]
    return params, grads


@functools.lru_cache(maxsize=None)
def reference(amsgrad=False):
    """-> dict(params, grads, after = the parameters after each of the six steps, ema = torch's average after each of them)"""
    params, grads = data()
    bag = _Bag(params)
    ps = list(bag.ps)
    opt = torch.optim.AdamW(_groups(ps), amsgrad=amsgrad, **KW)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda x: (1 - x / T) ** POWER)
    avg = AveragedModel(bag, multi_avg_fn=get_ema_multi_avg_fn(DECAY))
    after, ema = [], []
    for gs in grads:
        for p, gr in zip(ps, gs):
            p.grad = gr.clone()
        opt.step()
        sched.step()
        avg.update_parameters(bag)
        after.append([p.detach().clone() for p in ps])
        ema.append([e.detach().clone() for e in avg.module.ps])
    return dict(params=params, grads=grads, after=after, ema=ema)
