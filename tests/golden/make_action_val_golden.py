"""Writes tests/golden/action_val_golden.npz and action_val_golden_meta.json from the reference's own validation functions.

The reference is imported in place on the CPU: `val_epoch_video` of anonymization_training/train_anonymizer.py (:216-301) and `val_epoch` of
action_training/train_anonymized_action.py (:115-200) run as written, with a plain list of batches as the data loader and `use_cuda=False`.
Third-party imports the two scripts make at module level and this image lacks are replaced by empty `sys.modules` stubs (tensorboardX, decord,
torchvision and its sub-modules, segmentation_models_pytorch, tkinter.tix); none of them is reached by the two functions. The epoch-end
statements (:475-504 / :352-381) are the scripts' `main` bodies and cannot be called; they are repeated here on the dicts the functions
return: np.mean over each pred_dict entry, np.flip(np.argsort(...)) and the comparison with label_dict.

Models: load_fa_model('unet') and load_ft_model('largei3d', num_classes=102) with `synth_state_dict` weights; videos: `synth_train_video`
(2, 48, 3, 64, 64) under the names in the meta; two passes ("modes") over the same two video names, the second in the opposite order. The
labels are chosen after a first look at the models' own per-video prediction: video 0 gets it, video 1 gets the next class -- one right, one
wrong. Outputs only are stored. ft's logits pass through a forward hook and the two criteria through recording wrappers, so the per-batch
logits, cross entropies and triplet values are the ones the functions computed.

Asserted (conditions on the inputs, so that an fp32 rounding difference cannot change a prediction): every logit is finite, and in every
stored probability row -- per clip and per video -- the two largest probabilities differ by at least 1e-3.

    python tests/golden/make_action_val_golden.py
"""
import importlib.util
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from _refimport import REFERENCE_ROOT, _stub, import_reference, reference_available  # noqa: E402
from ted_spad_amd.synth import synth_state_dict, synth_train_video  # noqa: E402

SEED = 0
SHAPE = (2, 48, 3, 64, 64)
NUM_CLASSES = 102
NAMES = ["v_Walk_g01_c01.avi", "v_Run_g02_c03.avi"]
PASSES = [dict(mode=0, video="action_val/mode0", order=[0, 1], dir="/data/ucf/mode0"),
          dict(mode=1, video="action_val/mode1", order=[1, 0], dir="/data/ucf/mode1")]
PARAMS = SimpleNamespace(num_frames=16, loss="ce", temporal_loss="trip", temporal_loss_weight=0.1, triplet_loss_margin=1, num_classes=NUM_CLASSES)
MIN_GAP = 1e-3


def batch_inputs(ps):
    """The loader's batch of one pass: synth_train_video rows in the pass's video order."""
    return synth_train_video(SEED, ps["video"], SHAPE)[ps["order"]].contiguous()


def import_scripts():
    ml, _ = import_reference()
    _stub("tensorboardX", SummaryWriter=None)
    _stub("decord", bridge=SimpleNamespace(set_bridge=lambda name: None))      # ucf101_dl.py:19 calls it at import
    tv = sys.modules["torchvision"]
    tv.transforms = _stub("torchvision.transforms")
    tv.utils = _stub("torchvision.utils", save_image=None)
    mods = {}
    for name, rel in (("video", "anonymization_training/train_anonymizer.py"), ("action", "action_training/train_anonymized_action.py")):
        spec = importlib.util.spec_from_file_location("tedspad_ref_" + name, os.path.join(REFERENCE_ROOT, rel))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        mods[name] = m
    return ml, mods


class Recorder(nn.Module):
    def __init__(self, inner):
        super().__init__()
        self.inner, self.values = inner, []

    def forward(self, *a):
        v = self.inner(*a)
        self.values.append(float(v))
        return v


def epoch_end(pred_dict, label_dict):
    """train_anonymizer.py:491-504 on the dicts `val_epoch*` filled."""
    predictions = np.zeros((len(list(pred_dict.keys())), NUM_CLASSES))
    ground_truth = []
    for entry, key in enumerate(pred_dict.keys()):
        predictions[entry] = np.mean(pred_dict[key], axis=0)
    for key in label_dict.keys():
        ground_truth.append(label_dict[key])
    pred_array = np.flip(np.argsort(predictions, axis=1), axis=1)
    c_pred = pred_array[:, 0]
    correct_count = np.sum(c_pred == ground_truth)
    return predictions, c_pred, int(correct_count), float(correct_count) / len(c_pred)


def top2_gap(rows):
    s = np.sort(np.asarray(rows, dtype=np.float64), axis=1)
    return float((s[:, -1] - s[:, -2]).min())


def main():
    assert reference_available(), "the reference is needed to write the fixture"
    ml, mods = import_scripts()
    torch.manual_seed(0)
    fa = ml.load_fa_model(arch="unet")
    ft = ml.load_ft_model("largei3d", num_classes=NUM_CLASSES, kin_pretrained=False)
    fa.load_state_dict(synth_state_dict(fa.state_dict(), SEED))
    ft.load_state_dict(synth_state_dict(ft.state_dict(), SEED))
    logits_seen = []
    ft.register_forward_hook(lambda m, i, o: logits_seen.append(o[0].detach().numpy().copy()))

    # first look: the per-video prediction, to fix the labels (video 0 right, video 1 wrong)
    fa.eval(); ft.eval()
    look = {}
    with torch.no_grad():
        for ps in PASSES:
            x = batch_inputs(ps).permute(0, 2, 1, 3, 4)
            shape = x.shape
            anon = fa(x.reshape(-1, shape[1], shape[3], shape[4])).reshape(shape)
            pr = torch.softmax(ft(anon[:, :, :16])[0], dim=1).numpy()
            for row, v in zip(pr, ps["order"]):
                look.setdefault(v, []).append(row)
    top = {v: int(np.argmax(np.mean(rows, axis=0))) for v, rows in look.items()}
    labels_by_video = [top[0], (top[1] + 1) % NUM_CLASSES]
    logits_seen.clear()

    out, meta = {}, {"seed": SEED, "shape": list(SHAPE), "num_classes": NUM_CLASSES, "names": NAMES, "labels": labels_by_video,
                     "passes": PASSES, "params": vars(PARAMS), "min_top2_gap_required": MIN_GAP, "captured_with": "the reference's own val_epoch_video and val_epoch, CPU fp32"}
    gaps = []
    for fn in ("video", "action"):
        crit, crit_t = Recorder(nn.CrossEntropyLoss()), Recorder(nn.TripletMarginLoss(margin=PARAMS.triplet_loss_margin))
        pred_dict, label_dict = {}, {}
        accs, losses, running = [], [], []
        for k, ps in enumerate(PASSES):
            lab = torch.tensor([labels_by_video[v] for v in ps["order"]], dtype=torch.long)
            paths = ["%s/%s" % (ps["dir"], NAMES[v]) for v in ps["order"]]
            loader = [(batch_inputs(ps), lab, paths, None)]
            n0 = len(logits_seen)
            if fn == "video":
                pred_dict, label_dict, acc, loss = mods[fn].val_epoch_video(0, ps["mode"], 1.0, pred_dict, label_dict, loader, ft, fa, crit, crit_t, False, "cpu", PARAMS)
            else:
                pred_dict, label_dict, acc, loss = mods[fn].val_epoch(0, ps["mode"], 1.0, pred_dict, label_dict, loader, fa, ft, crit, crit_t, False, "cpu", PARAMS)
            accs.append(acc); losses.append(float(loss))
            running.append(epoch_end(pred_dict, label_dict)[3])
            lg = logits_seen[n0]                                       # the first ft call of the batch is the one whose logits are used
            assert np.isfinite(lg).all()
            out["%s/pass%d/logits" % (fn, k)] = lg
            out["%s/pass%d/labels" % (fn, k)] = lab.numpy()
            out["%s/pass%d/vid" % (fn, k)] = np.asarray(ps["order"], dtype=np.int32)
        predictions, c_pred, correct_count, accuracy = epoch_end(pred_dict, label_dict)
        assert list(pred_dict.keys()) == NAMES and [int(label_dict[k]) for k in NAMES] == labels_by_video
        for k, ps in enumerate(PASSES):                               # pred_dict rows back in batch order
            rows = np.stack([pred_dict[NAMES[v]][k] for v in ps["order"]])
            out["%s/pass%d/probs" % (fn, k)] = rows
            gaps.append(top2_gap(rows))
        gaps.append(top2_gap(predictions))
        out["%s/ce" % fn] = np.asarray(crit.values, dtype=np.float64)
        out["%s/triplet" % fn] = np.asarray(crit_t.values, dtype=np.float64)
        out["%s/pass_accuracy" % fn] = np.asarray(accs, dtype=np.float64)
        out["%s/pass_loss" % fn] = np.asarray(losses, dtype=np.float64)
        out["%s/running_accuracy" % fn] = np.asarray(running, dtype=np.float64)
        out["%s/mean_probs" % fn] = predictions
        out["%s/predictions" % fn] = c_pred.astype(np.int64)
        out["%s/accuracy" % fn] = np.float64(accuracy)
        out["%s/correct_count" % fn] = np.int64(correct_count)
        out["%s/val_loss" % fn] = np.float64(np.mean(losses))
        assert correct_count == 1 and accuracy == 0.5, (fn, correct_count, accuracy)
        assert len(crit.values) == len(PASSES) and len(crit_t.values) == (len(PASSES) if fn == "action" else 0)
    meta["min_top2_gap"] = min(gaps)
    assert min(gaps) >= MIN_GAP, gaps
    np.savez_compressed(os.path.join(HERE, "action_val_golden.npz"), **out)
    with open(os.path.join(HERE, "action_val_golden_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print(json.dumps({k: (v.tolist() if v.size < 8 else list(v.shape)) for k, v in out.items()}), meta["min_top2_gap"])


if __name__ == "__main__":
    main()
