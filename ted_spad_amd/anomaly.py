"""Frame-level anomaly-detection metrics of MGFN's `test()` (anomaly_detection_mgfn/test.py:13-51), host numpy without scikit-learn.

`anomaly_metrics` reproduces, step for step, what test.py computes with scikit-learn (1.7.2): `roc_curve(drop_intermediate=True)` + `auc`
and `precision_recall_curve` + `auc` (sklearn.metrics._ranking: `_binary_clf_curve`, `roc_curve`, `precision_recall_curve`, `auc`), on the
segment scores stretched to frames (Q-M4). `evaluate` chains `MGFN.score` and the metrics as `test()` does."""
from __future__ import annotations

import numpy as np
import torch


def frame_scores(pred_segments, n_frames: int, frames_per_segment: int = 32) -> np.ndarray:
    """Segment scores on the frame axis, as test.py:32-43 builds them (Q-M4): each score repeated `frames_per_segment` times ("skip rate
    2, 16 frames"). When that is not gt's length n, with r = n / (repeated length), repeated score k covers frames [E_k, E_{k+1}) where
    E_k = floor(k r + 1/2) in float64; a frame no score covers is 0. The result is float32, as in test.py."""
    seg = np.repeat(np.asarray(pred_segments, dtype=np.float32).reshape(-1), frames_per_segment)
    if n_frames == seg.size:
        return seg
    r = float(n_frames) / float(seg.size)
    edges = np.floor(np.arange(seg.size + 1, dtype=np.float64) * r + 0.5).astype(np.int64)
    frame = np.arange(n_frames)
    owner = np.searchsorted(edges, frame, side="right") - 1        # the last k with E_k <= frame: later scores win empty ranges
    out = np.zeros(n_frames, dtype=np.float32)
    hit = frame < edges[-1]
    out[hit] = seg[owner[hit]]
    return out


def _binary_clf_curve(y_true, y_score):
    # sklearn.metrics._ranking._binary_clf_curve without sample weights: scores in decreasing order (a stable sort of the ascending order,
    # reversed), one threshold per distinct score, cumulative true positives in float64
    order = np.argsort(y_score, kind="mergesort")[::-1]
    y_score, y_true = y_score[order], y_true[order]
    idx = np.r_[np.where(np.diff(y_score))[0], y_true.size - 1]
    tps = np.cumsum(y_true * 1.0, dtype=np.float64)[idx]
    fps = 1 + idx - tps
    return fps, tps, y_score[idx]


def _auc(x, y):
    # sklearn.metrics.auc: the trapezoid rule (scipy.integrate.trapezoid), negated for a decreasing x
    direction = 1
    dx = np.diff(x)
    if np.any(dx < 0):
        if np.all(dx <= 0):
            direction = -1
        else:
            raise ValueError("x is neither increasing nor decreasing")
    return float(direction * np.add.reduce(dx * (y[1:] + y[:-1]) / 2.0))


def anomaly_metrics(pred_segments, gt, frames_per_segment: int = 32):
    """(rec_auc, pr_auc) of test.py:30-51 for the concatenated per-video segment scores `pred_segments` and the frame-level labels `gt`.

    rec_auc is the area under the ROC curve after scikit-learn's `drop_intermediate` pruning, pr_auc the TRAPEZOID area under the
    precision-recall curve (not average precision). Ties are one threshold. A gt with a single class gives what scikit-learn gives (it
    warns there; this function does not): without positives or without negatives the ROC curve is NaN, so rec_auc is NaN; without positives
    precision is 0 at recall 1 up to the closing point (recall 0, precision 1), so pr_auc is 0.5; without negatives pr_auc is 1."""
    if torch.is_tensor(pred_segments):
        pred_segments = pred_segments.detach().cpu().numpy()
    gt = np.asarray(gt.detach().cpu() if torch.is_tensor(gt) else gt).reshape(-1)
    classes = np.unique(gt)
    if not set(classes.tolist()) <= {0, 1}:
        raise ValueError("anomaly_metrics: gt must hold 0 / 1 frame labels, got %s" % classes[:5])
    score = frame_scores(pred_segments, len(gt), frames_per_segment)
    if not np.isfinite(score).all():
        raise ValueError("anomaly_metrics: scores must be finite")
    truth = gt == 1
    fps, tps, _ = _binary_clf_curve(truth, score)
    # roc_curve(drop_intermediate=True)
    if len(fps) > 2:
        keep = np.where(np.r_[True, np.logical_or(np.diff(fps, 2), np.diff(tps, 2)), True])[0]
        rf, rt = fps[keep], tps[keep]
    else:
        rf, rt = fps, tps
    rf, rt = np.r_[0, rf], np.r_[0, rt]
    fpr = np.repeat(np.nan, rf.shape) if rf[-1] <= 0 else rf / rf[-1]
    tpr = np.repeat(np.nan, rt.shape) if rt[-1] <= 0 else rt / rt[-1]
    rec_auc = _auc(fpr, tpr)
    # precision_recall_curve (drop_intermediate=False)
    ps = tps + fps
    precision = np.zeros_like(tps)
    np.divide(tps, ps, out=precision, where=(ps != 0))
    recall = np.ones_like(tps) if tps[-1] == 0 else tps / tps[-1]
    precision, recall = np.hstack((precision[::-1], 1)), np.hstack((recall[::-1], 0))
    pr_auc = _auc(recall, precision)
    return rec_auc, pr_auc


def evaluate(model, videos, gt, frames_per_segment: int = 32):
    """test.py's `test()`: score every video (`MGFN.score`, one ragged batch), concatenate the per-segment crop means in order, and return
    (rec_auc, pr_auc) against the frame-level `gt`."""
    scores = model.score(videos)
    pred = torch.cat([s.reshape(-1) for s in scores]).cpu().numpy() if scores else np.zeros(0, np.float32)
    return anomaly_metrics(pred, gt, frames_per_segment)
