"""Writes tests/golden/mgfn_golden.npz and mgfn_golden_meta.json from the reference's MGFN (anomaly_detection_mgfn/models/mgfn.py).

The reference is imported in place on the CPU, one subprocess per config (`option.parse_args()` runs at import, so `sys.argv` carries
the config); only `visdom` is stubbed. MSNSD's eval branch calls `.cuda()`, so the model's own `forward` runs with `MSNSD` swapped for a
function that captures its inputs (the to_logits output and the per-crop scores), and the eval-branch selection (bs = 1) is redone here.
Weights: `synth.synth_mgfn_state_dict`; features: `synth_tensor` U[0, 2) under the names recorded in the meta, so the GPU box rebuilds every
input without the reference.

Stored per case: fp64 crop-mean scores, per-crop logits, per-token magnitudes, the top-3 indices, score_abnormal and abn_feamagnitude, and
the to_logits output h for T = 3. Recorded: the reference's own fp32-vs-fp64 error on the same weights and inputs. Asserted: the logits
are not saturated, the top-3 choice is stable, and the evaluation set's distinct scores are far enough apart that both AUCs are fixed.

    python tests/golden/make_mgfn_golden.py                 # writes the fixture
    python tests/golden/make_mgfn_golden.py --worker JOB OUT  # one config (used by the above and by tests/test_mgfn_golden.py)
"""
import json
import os
import subprocess
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from _refimport import REFERENCE_ROOT, reference_available  # noqa: E402
from ted_spad_amd.synth import synth_mgfn_state_dict, synth_tensor  # noqa: E402

SEED = 0
NCROPS = 10
CONFIGS = {
    "a": dict(feature_size=2048, depths=[3, 3, 2], types=["gb", "fb", "fb"], Ts=[3, 7, 32, 300]),
    "b": dict(feature_size=1024, depths=[3, 3, 2], types=["gb", "fb", "fb"], Ts=[32]),
    "c": dict(feature_size=2048, depths=[1, 1, 1], types=["fb", "gb", "gb"], Ts=[32]),
}
EVAL_TS = [5, 12, 3, 9, 7, 11]                 # set (d): config a's weights
EVAL_GT_EXTRA = 37                           # gt is 37 frames longer than 32 x segments: ratio != 1 (Q-M4)


def video_name(case, T):
    return "mgfn_video/%s/T%d" % (case, T)


def make_video(name, T, F, dtype=torch.float32):
    return synth_tensor(SEED, name, (1, NCROPS, T, F + 1), 0.0, 2.0).to(dtype)


def make_gt(n_segments):
    n = 32 * n_segments + EVAL_GT_EXTRA
    u = synth_tensor(SEED, "mgfn_eval_gt", ((n + 39) // 40,)).numpy()
    return (u[np.arange(n) // 40] > 0.6).astype(np.float32)            # anomalous runs of 40 frames


def sklearn_test_metrics(pred_segments, gt):
    """test.py:30-51 restated, with scikit-learn doing the curves and areas: every segment score spread over 32 frames; when that does
    not give gt's length n, with r = n / (32 x segments), the k-th spread score fills frames int(k r + 0.5) up to int((k + 1) r + 0.5),
    the rest stays 0 (float32); then auc(roc_curve(drop_intermediate=True)) and auc(recall, precision) of precision_recall_curve."""
    import warnings

    from sklearn.metrics import auc, precision_recall_curve, roc_curve
    spread = np.repeat(np.asarray(pred_segments, dtype=np.float32).reshape(-1), 32)
    n = len(gt)
    if n == spread.size:
        frames = spread
    else:
        r = float(n) / float(spread.size)
        edges = [int(k * r + 0.5) for k in range(spread.size + 1)]
        frames = np.zeros(n, dtype=np.float32)
        stop = min(edges[-1], n)
        frames[:stop] = np.repeat(spread, np.diff(edges))[:stop]
    labels, values = list(gt), list(frames)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fpr, tpr, _ = roc_curve(labels, values, drop_intermediate=True)
        precision, recall, _ = precision_recall_curve(labels, values)
        return auc(fpr, tpr), auc(recall, precision)


# ---------------------------------------------------------------------------------------------------------------------------------------
def worker(job_path, out_path):
    """One config inside this process: import the reference, run every video in fp32 and fp64, save the raw outputs."""
    job = json.load(open(job_path))
    cfg = job["cfg"]
    sys.argv = ["mgfn", "--feature_size", str(cfg["feature_size"])] + sum(
        (["--depths%d" % (i + 1), str(d), "--mgfn_type%d" % (i + 1), t] for i, (d, t) in enumerate(zip(cfg["depths"], cfg["types"]))), [])
    sys.modules.setdefault("visdom", types.ModuleType("visdom"))
    sys.dont_write_bytecode = True
    sys.path.insert(0, os.path.join(REFERENCE_ROOT, "anomaly_detection_mgfn"))
    import models.mgfn as ref  # noqa: E402

    captured = {}

    def capture(features, scores, bs, batch_size, drop_out, ncrops, k):
        captured["h"], captured["scores"] = features, scores
        return None, None, None, None, None

    ref.MSNSD = capture
    torch.manual_seed(0)
    model = ref.mgfn().eval()
    sd = synth_mgfn_state_dict(model.state_dict(), SEED)
    model.load_state_dict(sd)
    res = {"keys": json.dumps([[k, list(v.shape)] for k, v in model.state_dict().items()])}
    for dt, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
        m = ref.mgfn().eval()
        m.load_state_dict(sd)
        m = m.to(dt)
        ref.MSNSD = capture
        with torch.no_grad():
            for name, T in job["videos"]:
                m(make_video(name, T, cfg["feature_size"], dt))
                h, s = captured["h"], captured["scores"]                 # (ncrops, T, 1024), (ncrops, T, 1)
                logits = m.fc(h)[..., 0]
                mags = torch.norm(h, p=2, dim=2)
                # MSNSD eval branch, bs = 1 (models/mgfn.py:23-86; dropout is the identity in eval)
                crop_scores = s.view(1, NCROPS, -1).mean(1)
                crop_mags = mags.view(1, NCROPS, -1).mean(1)
                r = dict(logits=logits, crop_scores=crop_scores[0], mags=mags, crop_mags=crop_mags[0])
                if T >= 3:
                    idx = torch.topk(crop_mags, 3, dim=1)[1]
                    r["idx"] = idx[0]
                    r["score_abnormal"] = torch.mean(torch.gather(crop_scores.unsqueeze(2), 1, idx.unsqueeze(2)), dim=1)[0, 0]
                    r["feat"] = torch.cat([torch.gather(hc.unsqueeze(0), 1, idx.unsqueeze(2).expand(-1, -1, h.shape[2])) for hc in h])
                r["h"] = h
                for k, v in r.items():
                    res["%s|%s|%s" % (tag, name, k)] = v.numpy()
    np.savez(out_path, **res)


def run_worker(cfg, videos, tmpdir):
    job = os.path.join(tmpdir, "job.json")
    out = os.path.join(tmpdir, "out.npz")
    json.dump({"cfg": cfg, "videos": videos}, open(job, "w"))
    subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", job, out], check=True)
    return dict(np.load(out))


def _rel(a, b):
    return float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()))


def main():
    import tempfile

    assert reference_available(), "the reference is needed to write the fixture"
    out, meta = {}, {"seed": SEED, "ncrops": NCROPS, "configs": CONFIGS, "cases": {}, "eval": {}}
    errs = {"mags_rel_l2": 0.0, "h_rel_l2": 0.0, "logits_max_abs": 0.0, "scores_max_abs": 0.0}
    with tempfile.TemporaryDirectory() as tmp:
        raw = {}
        for c, cfg in CONFIGS.items():
            vids = [[video_name(c, T), T] for T in cfg["Ts"]]
            if c == "a":
                vids += [[video_name("eval%d" % i, T), T] for i, T in enumerate(EVAL_TS)]
            raw[c] = run_worker(cfg, vids, tmp)
            meta["configs"][c]["state_dict"] = json.loads(str(raw[c]["keys"]))
    for c, cfg in CONFIGS.items():
        R = raw[c]
        for T in cfg["Ts"]:
            name = video_name(c, T)
            g = lambda tag, k: R["%s|%s|%s" % (tag, name, k)]  # noqa: E731
            e = {"mags_rel_l2": _rel(g("f32", "mags"), g("f64", "mags")), "h_rel_l2": _rel(g("f32", "h"), g("f64", "h")),
                 "logits_max_abs": float(np.abs(g("f32", "logits") - g("f64", "logits")).max()),
                 "scores_max_abs": float(np.abs(g("f32", "crop_scores") - g("f64", "crop_scores")).max())}
            for k in errs:
                errs[k] = max(errs[k], e[k])
            z = g("f64", "logits")
            case = "%s_T%d" % (c, T)
            meta["cases"][case] = {"config": c, "T": T, "video": name, "F": cfg["feature_size"], "errors": e,
                                   "logit_std": float(z.std()), "logit_max_abs": float(np.abs(z).max())}
            assert z.std() >= 0.2 and np.abs(z).max() <= 12, (case, z.std(), np.abs(z).max())       # sigmoid not saturated
            for k in ("crop_scores", "logits", "mags", "idx", "score_abnormal"):
                out["%s/%s" % (case, k)] = g("f64", k)
            out["%s/feat" % case] = g("f64", "feat").astype(np.float32)
            if T == 3:
                out["%s/h" % case] = g("f64", "h").astype(np.float32)
    meta["errors"] = errs
    for case, m in meta["cases"].items():                                # top-3 stable: 3rd vs 4th crop-mean magnitude
        if m["T"] > 3:
            cm = np.sort(out["%s/mags" % case].mean(0))[::-1]
            gap, need = float(cm[2] - cm[3]), 100 * errs["mags_rel_l2"] * float(cm[0])
            m["top3_gap"], m["top3_gap_needed"] = gap, need
            assert gap > need, (case, gap, need)
    # ---- evaluation set (d): test.py:30-51 with scikit-learn on the fp32 reference's scores ----
    R = raw["a"]
    pred32 = np.concatenate([R["f32|%s|crop_scores" % video_name("eval%d" % i, T)] for i, T in enumerate(EVAL_TS)])
    pred64 = np.concatenate([R["f64|%s|crop_scores" % video_name("eval%d" % i, T)] for i, T in enumerate(EVAL_TS)])
    gt = make_gt(len(pred32))
    assert len(gt) != 32 * len(pred32)
    rec_auc, pr_auc = sklearn_test_metrics(pred32, gt)
    score_bound = 10 * errs["scores_max_abs"]
    d = np.diff(np.unique(pred64))
    meta["eval"] = {"Ts": EVAL_TS, "videos": [video_name("eval%d" % i, T) for i, T in enumerate(EVAL_TS)], "gt_len": int(len(gt)),
                    "rec_auc": float(rec_auc), "pr_auc": float(pr_auc), "min_score_gap": float(d.min()),
                    "score_bound": score_bound}
    assert len(np.unique(pred64)) == len(pred64) and d.min() > 4 * score_bound, (d.min(), score_bound)
    out["eval/gt"] = gt
    out["eval/scores"] = pred64
    np.savez_compressed(os.path.join(HERE, "mgfn_golden.npz"), **out)
    with open(os.path.join(HERE, "mgfn_golden_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print(json.dumps(errs), meta["eval"])


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--worker":
        worker(sys.argv[2], sys.argv[3])
    else:
        main()
