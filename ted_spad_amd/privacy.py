"""The privacy side of TeD-SPAD on MI355X: training and scoring the VISPR privacy classifier fb (privacy_training/train_privacy.py).

    PrivacyTrainStep(fb, fa=None).step(images, labels)     one `train_epoch` batch (:41-56): fa eval (the `anon` flag), fb train forward,
                                                            BCEWithLogitsLoss, backward, Adam
    PrivacyTrainStep.evaluate(images, labels)               one `val_epoch` batch (:78-91): eval forward + the loss
    privacy_metrics(logits, labels, paths)                  the epoch-end numbers of `val_epoch` (:99-134): per-class precision / recall /
                                                            F1 / AP, their macro means (cMAP = macro AP), pred_dict / label_dict

fb is `load_fb_model(arch='r50', ssl=False, num_pa=7)` (resnet50.ResNet50 with a 7-way fc); the step's head is ONE launch (fc, loss and
the three fc gradients: tedspad_bce_head_fwd_bwd). Gradients are scaled by a static `loss_scale` and checked for non-finite values before
the step, as in AnonymizerTrainStep (train_step.py). `privacy_metrics` is host numpy and restates scikit-learn's
`precision_recall_fscore_support` / `average_precision_score` (the reference's imports, :4) -- including the threshold quirk: F1 is
computed on `logits > 0.5`, not on probabilities (DESIGN.md "The privacy classifier").
"""
from __future__ import annotations

import numpy as np
import torch

from . import head
from .train_nets import PredictorTrainer
from .train_step import StepDriver, fused_adam


class PrivacyTrainStep(StepDriver):
    def __init__(self, fb_model, fa_model=None, learning_rate: float = 1e-3, loss_scale: float = 256.0):
        """fb_model: ResNet50 with an fc (cuda). fa_model: the frozen anonymizer in front (`anon = True`, params_privacy.py:6), or None.
        learning_rate: params_privacy.py:18 (the script rewrites it every epoch: `set_lr`)."""
        super().__init__(loss_scale)
        self.fb, self.fa = fb_model, fa_model
        self.fb_tr = PredictorTrainer(fb_model)
        self.opt = fused_adam(fb_model, learning_rate)                # train_privacy.py:172; `set_lr` is :31-32

    def _input(self, images):
        if self.fa is None:
            return images
        self.fa.eval()                                                # :38,71
        with torch.no_grad():
            return self.fa(images)                                    # :49,86

    def step(self, images, labels):
        """images (B,3,H,W) fp32 cuda, labels (B,N) float (0/1). Returns dict(loss=float, skipped=DeviceFlag)."""
        self.fb.train()                                               # :39
        self._begin(images.device, (self.opt,))                       # :42
        x = self._input(images)
        _, loss, tape = self.fb_tr.forward(x, labels, grad_scale=self.loss_scale)     # :49-52: fb forward, fc + BCEWithLogitsLoss fused
        self._post(dict(loss=loss))                                   # :53
        self.fb_tr.backward(tape)                                     # :55
        v, skipped = self._end(self.fb_tr, None, self.opt, self.fb)   # :56
        return dict(loss=v["loss"], skipped=skipped)

    def evaluate(self, images, labels):
        """One `val_epoch` batch (:84-89): fb.eval() forward (after fa when given) and the loss. Returns (logits (B,N) fp32, loss 0-d fp32
        tensor on the device) -- the logits are exactly `fb.eval()(x)`'s; the loss is the loss-only form of the fused head kernel."""
        self.fb.eval()                                                # :72
        x = self._input(images)
        with torch.no_grad():
            logits = self.fb(x)
        _, loss, _, _, _ = head.bce_head(logits, labels, grads=False)
        return logits, loss[0]


def _binary_average_precision(y_true, y_score):
    """scikit-learn's `average_precision_score` for one class: the step integral of the precision-recall curve with tied scores grouped into
    one threshold (sklearn.metrics._ranking._binary_clf_curve / precision_recall_curve, drop_intermediate=False). A class without positives:
    recall is set to 1 at every threshold, which makes its AP 0."""
    order = np.argsort(y_score, kind="mergesort")[::-1]
    score, truth = y_score[order], y_true[order]
    idx = np.r_[np.where(np.diff(score))[0], truth.size - 1]
    tps = np.cumsum(truth, dtype=np.float64)[idx]
    fps = 1 + idx - tps
    ps = tps + fps
    precision = np.zeros_like(tps)
    np.divide(tps, ps, out=precision, where=(ps != 0))
    recall = np.ones_like(tps) if tps[-1] == 0 else tps / tps[-1]
    precision, recall = np.hstack((precision[::-1], 1)), np.hstack((recall[::-1], 0))
    return float(max(0.0, -np.sum(np.diff(recall) * precision[:-1])))


def _div0(a, b):
    out = np.zeros_like(a, dtype=np.float64)
    np.divide(a, b, out=out, where=(b != 0))
    return out


def privacy_metrics(logits, labels, paths=None) -> dict:
    """The scores `val_epoch` prints and returns (train_privacy.py:99-134).

    logits (M,N) raw fb outputs, labels (M,N) in {0,1}, paths: M image paths (optional).
    Returns dict(precision, recall, f1, ap: per class (N,) float64 arrays; macro_precision, macro_recall, macro_f1, macro_ap (cMAP): floats;
    pred_dict: basename -> list of logit rows in input order; label_dict: basename -> the first label row of that name).
    F1 / precision / recall threshold the LOGITS at 0.5 (the reference's `np.array(predictions) > 0.5`, :104), i.e. sigmoid > 0.622; a
    ratio with a zero denominator is 0 (scikit-learn's zero_division default). AP ranks the logits, which is the same as ranking probabilities."""
    raw = np.asarray(logits.detach().cpu() if torch.is_tensor(logits) else logits)
    logits = raw.astype(np.float64)
    labels = np.asarray(labels.detach().cpu() if torch.is_tensor(labels) else labels)
    if logits.ndim != 2 or logits.shape != labels.shape:
        raise ValueError("privacy_metrics: logits %s and labels %s must both be (M, N)" % (logits.shape, labels.shape))
    if not np.isin(labels, (0, 1)).all():
        raise ValueError("privacy_metrics: labels must be 0 / 1 (multi-label indicator matrix)")
    truth = labels.astype(bool)
    pred = logits > 0.5                                               # :104 (logits, not probabilities)
    tp = (pred & truth).sum(0).astype(np.float64)
    fp = (pred & ~truth).sum(0).astype(np.float64)
    fn = (~pred & truth).sum(0).astype(np.float64)
    precision, recall = _div0(tp, tp + fp), _div0(tp, tp + fn)
    f1 = _div0(2 * tp, 2 * tp + fp + fn)
    ap = np.array([_binary_average_precision(truth[:, c].astype(np.float64), logits[:, c]) for c in range(logits.shape[1])])
    pred_dict, label_dict = {}, {}
    if paths is not None:
        if len(paths) != logits.shape[0]:
            raise ValueError("privacy_metrics: %d paths for %d rows" % (len(paths), logits.shape[0]))
        for i, p in enumerate(paths):                                 # :121-130
            key = str(p.split("/")[-1])
            pred_dict.setdefault(key, []).append(raw[i])
            label_dict.setdefault(key, labels[i])
    return dict(precision=precision, recall=recall, f1=f1, ap=ap, macro_precision=float(np.mean(precision)), macro_recall=float(np.mean(recall)),
                macro_f1=float(np.mean(f1)), macro_ap=float(np.mean(ap)), pred_dict=pred_dict, label_dict=label_dict)
