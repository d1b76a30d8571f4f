"""Host-side evaluation metrics of the reference's test loop (test.py:84-108).

EvalMeter accumulates per-sample intersection / union pixel counts -- what `lavt_hip.engine.Predictor.iu` holds after a step -- and reports mean IoU,
precision@{0.5 ... 0.9} and overall IoU in percent.  It runs on the host: `update` copies the counts it is given (a device tensor is read with one
device-to-host copy at that point, never inside Predictor.step()).
"""
import numpy as np

THRESHOLDS = (0.5, 0.6, 0.7, 0.8, 0.9)          # test.py:61 eval_seg_iou_list


class EvalMeter:
    def __init__(self):
        self.reset()

    def reset(self):
        self.cum_I = 0
        self.cum_U = 0
        self.ious = []
        self.correct = [0] * len(THRESHOLDS)
        self.count = 0

    def update(self, iu):
        """iu: per-sample (I, U) counts, shape (n, 2) or (2,): a torch tensor (any device), numpy array or nested sequence of integers."""
        if hasattr(iu, "detach"):
            iu = iu.detach().cpu().numpy()
        iu = np.asarray(iu, dtype=np.int64).reshape(-1, 2)
        for I, U in iu.tolist():
            this_iou = 0.0 if U == 0 else I * 1.0 / U          # test.py:86-89
            self.ious.append(this_iou)
            self.cum_I += I
            self.cum_U += U
            for k, th in enumerate(THRESHOLDS):
                self.correct[k] += this_iou >= th                # test.py:93-95
            self.count += 1

    def summary(self):
        """-> {"mean_iou", "precision@0.5" ... "precision@0.9", "overall_iou"} in percent (test.py:100-108)"""
        if self.count == 0:
            raise RuntimeError("EvalMeter.summary: no samples")
        out = {"mean_iou": float(np.mean(np.array(self.ious)) * 100.0)}
        for k, th in enumerate(THRESHOLDS):
            out[f"precision@{th}"] = self.correct[k] * 100.0 / self.count
        out["overall_iou"] = (self.cum_I * 100.0 / self.cum_U) if self.cum_U else 0.0
        return out

    def __str__(self):
        s = self.summary()
        lines = ["Final results:", "Mean IoU is %.2f" % s["mean_iou"]]
        lines += ["    precision@%s = %.2f" % (th, s[f"precision@{th}"]) for th in THRESHOLDS]
        lines.append("    overall IoU = %.2f" % s["overall_iou"])
        return "\n".join(lines)
