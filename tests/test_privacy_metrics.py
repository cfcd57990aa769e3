"""CPU: privacy.privacy_metrics, the epoch-end scores of privacy_training/train_privacy.py:99-134 restated in numpy, against scikit-learn
(the reference's own metric functions) and against hand-computed values."""
import warnings

import numpy as np
import pytest

from ted_spad_amd.privacy import privacy_metrics


def _sklearn(logits, labels):
    metrics = pytest.importorskip("sklearn.metrics")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        prec, rec, f1, _ = metrics.precision_recall_fscore_support(labels, (np.array(logits) > 0.5).astype(int))     # train_privacy.py:104
        ap = metrics.average_precision_score(labels, logits, average=None)                                           # :113
    return prec, rec, f1, np.asarray(ap)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_matches_sklearn_with_ties_and_a_class_without_positives(seed):
    rng = np.random.default_rng(seed)
    m, n = 97, 7
    labels = (rng.random((m, n)) < 0.35).astype(np.float32)
    labels[:, 3] = 0                                                  # no positive at all: sklearn's AP convention for it
    labels[:, 5] = 1                                                  # only positives
    logits = rng.normal(0.3, 1.5, (m, n)).astype(np.float32)
    logits[:, 1] = np.round(logits[:, 1] * 2) / 2                     # heavy ties: AP groups tied scores into one threshold
    logits[:, 2] = 0.5                                                # every score tied, exactly at the F1 threshold
    logits[::3, 4] = logits[0, 4]
    r = privacy_metrics(logits, labels)
    prec, rec, f1, ap = _sklearn(logits, labels)
    np.testing.assert_allclose(r["precision"], prec, rtol=0, atol=1e-12)
    np.testing.assert_allclose(r["recall"], rec, rtol=0, atol=1e-12)
    np.testing.assert_allclose(r["f1"], f1, rtol=0, atol=1e-12)
    np.testing.assert_allclose(r["ap"], ap, rtol=0, atol=1e-12)
    assert r["macro_ap"] == pytest.approx(float(np.mean(ap)), abs=1e-12)
    assert r["macro_f1"] == pytest.approx(float(np.mean(f1)), abs=1e-12)
    assert r["macro_precision"] == pytest.approx(float(np.mean(prec)), abs=1e-12)
    assert r["macro_recall"] == pytest.approx(float(np.mean(rec)), abs=1e-12)


def test_hand_computed_four_by_two():
    # class 0: scores 2.0 (pos), 1.0 (neg), 0.7 (pos), -1.0 (neg); class 1: 0.9 (neg), 0.9 (pos), 0.2 (pos), 0.1 (neg)
    logits = np.array([[2.0, 0.9], [1.0, 0.9], [0.7, 0.2], [-1.0, 0.1]])
    labels = np.array([[1, 0], [0, 1], [1, 1], [0, 0]])
    r = privacy_metrics(logits, labels)
    # class 0: predicted positive (> 0.5): rows 0,1,2 -> tp 2, fp 1, fn 0; class 1: rows 0,1 -> tp 1, fp 1, fn 1
    np.testing.assert_allclose(r["precision"], [2 / 3, 1 / 2])
    np.testing.assert_allclose(r["recall"], [1.0, 1 / 2])
    np.testing.assert_allclose(r["f1"], [0.8, 0.5])
    # AP class 0: ranks pos, neg, pos -> P@1 = 1 (R 1/2), P@3 = 2/3 (R 1)  -> 1/2 + 1/2 * 2/3
    # AP class 1: the tie at 0.9 is one threshold holding one pos of two -> P = 1/2 at R = 1/2; then 0.2 (pos): P = 2/3 at R = 1
    np.testing.assert_allclose(r["ap"], [0.5 + 1 / 3, 0.25 + 1 / 3])
    assert r["macro_ap"] == pytest.approx((5 / 6 + 7 / 12) / 2)
    assert r["macro_f1"] == pytest.approx(0.65)


def test_f1_thresholds_the_logits_not_the_probabilities():
    """train_privacy.py:104 thresholds the raw fb outputs at 0.5. A logit of 0.3 is sigmoid 0.574 (a positive by probability) but a
    negative here; a logit of 0.6 is a positive."""
    logits = np.array([[0.3], [0.6], [-2.0]])
    labels = np.array([[1], [1], [0]])
    r = privacy_metrics(logits, labels)
    assert r["precision"][0] == 1.0 and r["recall"][0] == 0.5         # by probability (> 0.5) both positives would be found
    assert r["f1"][0] == pytest.approx(2 / 3)
    assert r["ap"][0] == 1.0                                          # the ranking itself is perfect


def test_zero_division_is_zero():
    r = privacy_metrics(np.array([[0.0, 0.0], [0.1, 0.2]]), np.array([[0, 1], [0, 0]]))
    assert list(r["precision"]) == [0.0, 0.0] and list(r["recall"]) == [0.0, 0.0] and list(r["f1"]) == [0.0, 0.0]
    assert r["ap"][0] == 0.0 and r["ap"][1] == 0.5                     # class 0 has no positive (AP 0); class 1: its positive ranks second


def test_basename_grouping():
    """pred_dict / label_dict of train_privacy.py:121-130: keyed by the last path component; predictions of one name are collected in
    input order, the label row is the first one seen."""
    logits = np.array([[0.1, 0.2], [0.3, 0.4], [0.5, 0.6]], dtype=np.float32)
    labels = np.array([[0, 1], [1, 0], [1, 1]], dtype=np.float32)
    r = privacy_metrics(logits, labels, paths=["/a/x/img1.jpg", "/b/y/img2.jpg", "/c/img1.jpg"])
    assert sorted(r["pred_dict"]) == ["img1.jpg", "img2.jpg"] == sorted(r["label_dict"])
    assert [list(v) for v in r["pred_dict"]["img1.jpg"]] == [[np.float32(0.1), np.float32(0.2)], [np.float32(0.5), np.float32(0.6)]]
    assert r["pred_dict"]["img1.jpg"][0].dtype == np.float32
    assert list(r["label_dict"]["img1.jpg"]) == [0, 1]
    assert list(r["label_dict"]["img2.jpg"]) == [1, 0]
    assert privacy_metrics(logits, labels)["pred_dict"] == {}


def test_bad_inputs_raise():
    with pytest.raises(ValueError):
        privacy_metrics(np.zeros((3, 2)), np.zeros((3, 3)))
    with pytest.raises(ValueError):
        privacy_metrics(np.zeros((3, 2)), np.full((3, 2), 0.5))


def test_product_code_does_not_import_sklearn():
    import ast
    import os
    from conftest import ROOT
    pkg = os.path.join(ROOT, "ted_spad_amd")
    for name in os.listdir(pkg):
        if name.endswith(".py"):
            tree = ast.parse(open(os.path.join(pkg, name)).read())
            for node in ast.walk(tree):
                mods = [a.name for a in node.names] if isinstance(node, ast.Import) else [node.module or ""] if isinstance(node, ast.ImportFrom) else []
                assert not any(m.split(".")[0] == "sklearn" for m in mods), name
