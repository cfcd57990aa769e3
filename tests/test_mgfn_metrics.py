"""CPU: ted_spad_amd.anomaly.anomaly_metrics against test.py:30-51 computed with scikit-learn (tests/golden/make_mgfn_golden.py's
`sklearn_test_metrics`: roc_curve + auc and precision_recall_curve + auc on the x32-stretched segment scores)."""
import sys

import numpy as np
import pytest

from conftest import GOLDEN_DIR
from ted_spad_amd.anomaly import anomaly_metrics, frame_scores
from ted_spad_amd.synth import synth_tensor

pytest.importorskip("sklearn.metrics")
sys.path.insert(0, GOLDEN_DIR)
from make_mgfn_golden import sklearn_test_metrics as _test_py  # noqa: E402


def _same(a, b):
    return (np.isnan(a) and np.isnan(b)) or a == b


def _case(n_seg, extra, seed=0, levels=None, p=0.6):
    s = synth_tensor(seed, "anom_pred%d" % n_seg, (n_seg,)).numpy()
    if levels:
        s = np.round(s * levels) / levels                        # heavy ties across segments as well
    n = 32 * n_seg + extra
    u = synth_tensor(seed, "anom_gt%d" % n_seg, ((n + 24) // 25,)).numpy()
    gt = (u[np.arange(n) // 25] > p).astype(np.float32)
    return s, gt


@pytest.mark.parametrize("n_seg,extra,levels", [(40, 0, None), (40, 0, 4), (57, 13, None), (57, -21, 5), (300, 1000, None), (9, -100, None)])
def test_matches_test_py(n_seg, extra, levels):
    s, gt = _case(n_seg, extra, levels=levels)
    assert 0 < gt.sum() < len(gt)
    got, ref = anomaly_metrics(s, gt), _test_py(s, gt)
    print(n_seg, extra, levels, got, ref)
    assert got[0] == ref[0] and got[1] == ref[1]


def test_all_tied_scores():
    s, gt = _case(20, 7)
    s[:] = 0.5
    got, ref = anomaly_metrics(s, gt), _test_py(s, gt)
    assert got == ref and got[0] == 0.5


@pytest.mark.parametrize("label", [0.0, 1.0])
def test_single_class_gt(label):
    """Only one class in gt: scikit-learn's ROC curve is NaN (rec_auc NaN); without positives pr_auc = 0.5 (precision 0 at recall 1, then the
    closing point (recall 0, precision 1)), without
    negatives pr_auc = 1."""
    s, gt = _case(30, 5)
    gt[:] = label
    got, ref = anomaly_metrics(s, gt), _test_py(s, gt)
    print(label, got, ref)
    assert _same(got[0], ref[0]) and _same(got[1], ref[1])
    assert np.isnan(got[0]) and got[1] == (1.0 if label else 0.5)


def test_integer_gt_and_int_labels_only():
    s, gt = _case(25, 3)
    assert anomaly_metrics(s, gt.astype(np.int64)) == _test_py(s, gt.astype(np.int64))
    with pytest.raises(ValueError):
        anomaly_metrics(s, gt * 2)


@pytest.mark.parametrize("n_seg,n_frames", [(10, 320), (10, 333), (10, 300), (7, 100), (3, 1000), (50, 1601)])
def test_frame_scores_mapping(n_seg, n_frames):
    """Q-M4 written out frame by frame: repeated score k covers frames int(k r + 0.5) .. int((k + 1) r + 0.5) - 1, uncovered frames are 0."""
    s = synth_tensor(0, "fs%d_%d" % (n_seg, n_frames), (n_seg,)).numpy()
    got = frame_scores(s, n_frames)
    rep = np.repeat(s, 32)
    want = np.zeros(n_frames, np.float32)
    if n_frames == rep.size:
        want = rep
    r = n_frames / rep.size
    for f in range(n_frames if n_frames != rep.size else 0):
        ks = [k for k in range(rep.size) if int(k * r + 0.5) <= f < int((k + 1) * r + 0.5)]
        if ks:
            want[f] = rep[ks[-1]]
    assert got.dtype == np.float32 and np.array_equal(got, want)
