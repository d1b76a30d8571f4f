"""Generator of tests/golden/train_meter_cases.npz (+ .json for the strings): what the reference's own training log gives on the CPU for fixed
sequences of (loss, lr, I, U) -- utils.SmoothedValue and utils.MetricLogger.__str__ (utils.py:16-104), train.IoU (train.py:64-76) and the per-iteration
bookkeeping of train.py:463-500 (acc_ious, cum_I, cum_U, seg_correct, the epoch summary).  The tests need neither the reference nor its environment.

    python tests/golden/make_train_meter_golden.py /path/to/the/reference/checkout

utils.py is imported as it is.  train.py is not importable without its data-set dependencies, so only the `IoU` function's node of the parsed file is
executed.  IoU is driven with real tensors: logits (1, 2, 1, L) and a target (1, 1, L) built to have exactly the wanted intersection and union.

Cases (every loss / lr is an fp32 value, held as the double the reference's `.item()` returns):
  loss6   the issue's sequence [0.5, 0.25, 1.0, 0.75, 0.125, 2.0] at window_size 4
  run19   19 iterations, window_size 5: seeded losses, a poly lr, and the I / U pairs below in turn -- (7, 10) and (9, 10) pass their thresholds only when
          the division is done in double precision, (0, 0) and (0, 57) are the empty cases
Per iteration the file holds iou, seg_correct, cum_I, cum_U, the five SmoothedValue properties of the loss and iou meters, and str(MetricLogger)."""
import ast
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PAIRS = [(0, 0), (0, 57), (1, 2), (3, 5), (4, 5), (7, 10), (9, 10), (4999, 10000), (6, 10)]
PROPS = ("median", "avg", "global_avg", "max", "value")


def load_reference(root):
    spec = importlib.util.spec_from_file_location("reference_utils", os.path.join(root, "utils.py"))
    utils = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(utils)
    path = os.path.join(root, "train.py")
    tree = ast.parse(open(path).read(), path)
    node = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "IoU")
    ns = {"torch": torch}
    exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
    return utils, ns["IoU"]


def masks(I, U):
    """logits (1, 2, 1, L) and target (1, 1, L) with sum(pred * gt) = I and sum(pred + gt) - I = U"""
    L = max(U, 1)
    pred = torch.zeros(L, dtype=torch.int64)
    pred[:U] = 1
    gt = torch.zeros(L, dtype=torch.int64)
    gt[:I] = 1
    logits = torch.stack([1.0 - pred.float(), pred.float()]).view(1, 2, 1, L)
    return logits, gt.view(1, 1, L)


def run(utils, IoU, losses, lrs, pairs, window):
    logger = utils.MetricLogger(delimiter="  ")
    logger.add_meter("lr", utils.SmoothedValue(window_size=1, fmt="{value}"))          # train.py:201
    logger.add_meter("loss", utils.SmoothedValue(window_size=window))
    logger.add_meter("iou", utils.SmoothedValue(window_size=window))
    thresholds = [.5, .6, .7, .8, .9]
    seg_correct = np.zeros(5, dtype=np.int32)
    acc_ious, cum_I, cum_U, total_its = 0, 0, 0, 0
    out = {k: [] for k in ("iou", "seg_correct", "cum_I", "cum_U", "loss_props", "iou_props")}
    strings = []
    for loss, lr, (I, U) in zip(losses, lrs, pairs):
        total_its += 1
        iou, i, u = IoU(*masks(I, U))
        acc_ious += iou
        cum_I += i
        cum_U += u
        for n, t in enumerate(thresholds):
            seg_correct[n] += (iou >= t)
        logger.update(loss=torch.tensor(loss, dtype=torch.float32).item(), lr=lr, iou=iou)
        out["iou"].append(float(iou))
        out["seg_correct"].append(seg_correct.copy())
        out["cum_I"].append(int(cum_I))
        out["cum_U"].append(int(cum_U))
        out["loss_props"].append([float(getattr(logger.loss, p)) for p in PROPS])
        out["iou_props"].append([float(getattr(logger.iou, p)) for p in PROPS])
        strings.append(str(logger))
    arrays = {"iou": np.array(out["iou"], dtype=np.float64), "seg_correct": np.stack(out["seg_correct"]).astype(np.int64),
              "cum_I": np.array(out["cum_I"], dtype=np.int64), "cum_U": np.array(out["cum_U"], dtype=np.int64),
              "loss_props": np.array(out["loss_props"], dtype=np.float64), "iou_props": np.array(out["iou_props"], dtype=np.float64),
              "mean_iou": np.float64(100 * (acc_ious / total_its))}
    if int(cum_U) != 0:
        arrays["overall_iou"] = np.float64(float(100 * cum_I / cum_U))          # train.py:500 (a float32 tensor division in the reference)
    return arrays, strings


def main():
    utils, IoU = load_reference(sys.argv[1])
    cases, strings = {}, {}
    # ---- loss6
    losses = np.array([0.5, 0.25, 1.0, 0.75, 0.125, 2.0], dtype=np.float32)
    arrays, s = run(utils, IoU, losses.tolist(), [0.0] * 6, [(1, 2)] * 6, 4)
    assert arrays["loss_props"][-1].tolist() == [0.75, 0.96875, 4.625 / 6, 2.0, 2.0] and "loss: 0.7500 (0.7708)" in s[-1], (arrays["loss_props"][-1], s[-1])
    cases["loss6"] = dict(arrays, losses=losses, lrs=np.zeros(6, dtype=np.float32), I=np.full(6, 1, dtype=np.int64), U=np.full(6, 2, dtype=np.int64), window=np.int64(4))
    strings["loss6"] = s
    # ---- run19
    rng = np.random.default_rng(20260)
    losses = (0.2 + 1.5 * rng.random(19)).astype(np.float32)
    lrs = (5e-5 * (1.0 - np.arange(1, 20) / 40.0) ** 0.9).astype(np.float32)
    pairs = [PAIRS[i % len(PAIRS)] for i in range(19)]
    arrays, s = run(utils, IoU, losses.tolist(), [float(v) for v in lrs], pairs, 5)
    cases["run19"] = dict(arrays, losses=losses, lrs=lrs, I=np.array([p[0] for p in pairs], dtype=np.int64), U=np.array([p[1] for p in pairs], dtype=np.int64),
                          window=np.int64(5))
    strings["run19"] = s
    # the pairs that tell the precisions apart: an fp32 division misses both thresholds
    assert float(np.float32(7) / np.float32(10)) < 0.7 <= 7 / 10 and float(np.float32(9) / np.float32(10)) < 0.9 <= 9 / 10
    np.savez(os.path.join(HERE, "train_meter_cases.npz"), **{f"{c}/{k}": v for c, d in cases.items() for k, v in d.items()})
    with open(os.path.join(HERE, "train_meter_cases.json"), "w") as f:
        json.dump(strings, f, indent=1)
    print({c: (len(strings[c]), strings[c][-1]) for c in strings})


if __name__ == "__main__":
    main()
