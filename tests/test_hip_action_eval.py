"""-m gpu: validation of the action classifier on MI355X (ted_spad_amd/action_eval.py, csrc/action_eval.hip) -- the softmax / cross-entropy /
top-1 kernel against fp64 torch, the per-video vote kernels against fp64 numpy and a restatement of the reference's dict logic, the
fixture captured from the reference's own `val_epoch_video` / `val_epoch` (tests/golden/make_action_val_golden.py), and ActionValidator
end to end against the factory's modules composed by hand."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import GOLDEN_DIR, rel_l2
from ted_spad_amd.synth import synth_state_dict, synth_tensor, synth_train_video

pytestmark = pytest.mark.gpu


# ---- softmax / CE / top-1 ------------------------------------------------------------------------------------------------------------
def _logits(B, C):
    """Rows spread over [-80, 80]: the maximum (80) sits at a different column per row, a runner-up 0.1 .. 0.5 below it, one entry is -80
    (C = 2: odd rows are negated instead, [-80, -79.9 ..]). The runner-up keeps every row's loss well above fp64 torch's own resolution:
    with the top class alone at 80, the loss of a row labelled with it is ~e^-100, which `cross_entropy` in fp64 returns as 0."""
    z = synth_tensor(0, "sce_z_%d_%d" % (B, C), (B, C), -80.0, 79.0)
    lab = (synth_tensor(0, "sce_l_%d_%d" % (B, C), (B,)) * C).long().clamp(0, C - 1)
    for r in range(B):
        m = (7 * r + 3) % C
        z[r, m] = 80.0
        z[r, (m + 2) % C if C > 2 else 1 - m] = 80.0 - 0.1 * (1 + r % 5)
        if C > 2:
            z[r, (m + 1) % C] = -80.0
        elif r % 2:
            z[r] = -z[r]
    lab[0] = int(z[0].argmax())                                     # row 0 is labelled with its top class: max - z[label] is exactly 0
    return z, lab


@pytest.mark.parametrize("C", [2, 63, 64, 65, 101, 400, 1024])
@pytest.mark.parametrize("B", [1, 2, 33, 64])
def test_softmax_ce_eval_vs_fp64(B, C):
    from ted_spad_amd.action_eval import softmax_ce_eval
    z, lab = _logits(B, C)
    z64 = z.double()
    assert float(z64.abs().max()) >= 79.9 and bool(torch.isfinite(z64).all())
    p_r = torch.softmax(z64, dim=1)
    rows_r = F.cross_entropy(z64, lab, reduction="none")
    top2 = torch.topk(z64, 2, dim=1).values
    assert float((top2[:, 0] - top2[:, 1]).min()) >= 0.01           # every row: the fp64 argmax is not a rounding matter
    probs, row_loss, loss, pred = softmax_ce_eval(z.cuda(), lab)
    assert probs.dtype == torch.float32 and pred.dtype == torch.int32 and loss.shape == (1,)
    e = {"probs": rel_l2(probs.cpu(), p_r), "row_loss": rel_l2(row_loss.cpu(), rows_r), "loss": rel_l2(loss.cpu(), rows_r.mean().reshape(1))}
    print("B=%d C=%d" % (B, C), " ".join("%s %.2e" % kv for kv in e.items()))
    assert bool(torch.isfinite(probs).all()) and bool(torch.isfinite(row_loss).all())
    assert float((probs.double().sum(1) - 1).abs().max()) <= 1e-5
    for k, v in e.items():
        assert v <= 1e-5, (k, v)
    assert torch.equal(pred.cpu().long(), z64.argmax(dim=1))
    again = softmax_ce_eval(z.cuda(), lab.cuda())                    # device labels: the same launch without the host check
    assert all(torch.equal(a, b) for a, b in zip(again, (probs, row_loss, loss, pred)))


def test_softmax_ce_eval_tie_rule():
    """Among exactly equal maxima the highest index wins: np.flip(np.argsort(p, kind='stable'), axis=1)[:, 0]."""
    from ted_spad_amd.action_eval import softmax_ce_eval
    for C in (2, 64, 101, 400):
        z = torch.zeros(3, C)
        z[1] = -5.0
        if C > 7:
            z[2] = synth_tensor(0, "tie%d" % C, (C,), -3, 1)
            z[2, 3] = z[2, 7] = 2.5
        probs, _, _, pred = softmax_ce_eval(z.cuda(), [0, 1, 1])
        want = np.flip(np.argsort(probs.cpu().numpy(), axis=1, kind="stable"), axis=1)[:, 0]
        assert pred.cpu().tolist()[:2] == [C - 1, C - 1]
        if C > 7:
            assert int(pred[2]) == 7
        assert pred.cpu().tolist() == want.tolist()


def test_softmax_ce_eval_rejects_bad_arguments_and_writes_nothing():
    from ted_spad_amd._lib import TedSpadHipError
    from ted_spad_amd.action_eval import softmax_ce_eval, softmax_ce_eval_into
    z = synth_tensor(0, "sce_bad", (4, 1025), -1, 1).cuda()
    lab_h = np.zeros(4, dtype=np.int64)
    lab = torch.from_numpy(lab_h).cuda()
    outs = [torch.full((4, 1025), -7.0, device="cuda"), torch.full((4,), -7.0, device="cuda"), torch.full((1,), -7.0, device="cuda"),
            torch.full((4,), -7, dtype=torch.int32, device="cuda")]
    bad_label = np.array([0, 101, 0, 0], dtype=np.int64)
    neg_label = np.array([0, 0, -1, 0], dtype=np.int64)
    for kw, host in ((dict(B=0, Cn=101), lab_h), (dict(B=4, Cn=1), lab_h), (dict(B=4, Cn=1025), lab_h), (dict(B=1025, Cn=2), lab_h),
                     (dict(B=4, Cn=101), bad_label), (dict(B=4, Cn=101), neg_label)):
        with pytest.raises(TedSpadHipError):
            softmax_ce_eval_into(z, lab, host, *outs, **kw)
    with pytest.raises(TedSpadHipError):
        softmax_ce_eval(z[:, :101].contiguous(), [0, 0, 0, 101])
    torch.cuda.synchronize()
    assert all(bool((o == -7).all()) for o in outs)


# ---- the vote kernels ----------------------------------------------------------------------------------------------------------------
V, VC = 5, 101
VIDS = [[0, 1, 2, 0, 3, 1, 2], [3, 2, 1, 0, 3, 0, 1], [0, 1, 2, 3, 0, 1, 3]]      # video 4 is never named; <= 6 rows per video
LABELS_V = [11, 5, 77, 0, 9]


def _vote_rows():
    rows = [torch.softmax(synth_tensor(0, "vote%d" % i, (7, VC), -4, 4), dim=1) for i in range(3)]
    labels = list(LABELS_V)
    mean64 = _mean64(rows)
    for k in range(4):                                              # videos 1 and 3 right, 0 and 2 wrong
        top = int(np.argmax(mean64[k]))
        labels[k] = top if k % 2 else (top + 1) % VC
    return rows, labels


def _mean64(rows):
    acc = [[] for _ in range(V)]
    for r, vid in zip(rows, VIDS):
        for row, v in zip(r.numpy(), vid):
            acc[v].append(row.astype(np.float64))
    return [np.mean(a, axis=0) if a else None for a in acc]


def _run_votes(rows, split=None):
    from ted_spad_amd.action_eval import vote_accumulate
    sums = torch.zeros(V, VC, device="cuda")
    counts = torch.zeros(V, dtype=torch.int32, device="cuda")
    for r, vid in zip(rows, VIDS):
        parts = [(0, 7)] if split is None else [(0, split), (split, 7)]
        for a, b in parts:
            vote_accumulate(r[a:b].contiguous().cuda(), vid[a:b], sums, counts)
    return sums, counts


def test_vote_kernels_vs_fp64_and_the_dict_logic():
    from ted_spad_amd.action_eval import vote_finalize
    rows, labels = _vote_rows()
    mean64 = _mean64(rows)
    sums, counts = _run_votes(rows)
    lab_t = torch.tensor(labels, dtype=torch.int64).cuda()
    mean, pred, correct = vote_finalize(sums, counts, lab_t)
    want_counts = [sum(v.count(k) for v in VIDS) for k in range(V)]
    assert max(want_counts) <= 8 and want_counts[4] == 0 and any(len(set(v)) < len(v) for v in VIDS)
    assert counts.cpu().tolist() == want_counts
    worst = max(float(np.max(np.abs(mean[k].cpu().numpy().astype(np.float64) - mean64[k]) / mean64[k])) for k in range(4))
    print("vote mean: max relative error %.2e" % worst)
    assert worst <= 1e-6                                             # sequential fp32 sum of k <= 8 terms + one division: <= 8 x 2^-24
    assert int(pred[4]) == -1 and int(correct[4]) == 0 and bool((mean[4] == 0).all())
    # the reference's dict logic (train_anonymizer.py:285-294,475-487) in numpy, on names
    names = ["vid%d.avi" % k for k in range(V)]
    pred_dict, label_dict = {}, {}
    for r, vid in zip(rows, VIDS):
        for row, v in zip(r.numpy(), vid):
            pred_dict.setdefault(names[v], []).append(row)
            label_dict.setdefault(names[v], labels[v])
    predictions = np.stack([np.mean(pred_dict[k], axis=0) for k in pred_dict])
    s = np.sort(predictions.astype(np.float64), axis=1)
    assert float((s[:, -1] - s[:, -2]).min()) > 1e-5                 # the restatement's own top-1 is not a rounding matter
    c_pred = np.flip(np.argsort(predictions, axis=1, kind="stable"), axis=1)[:, 0]
    truth = np.asarray([label_dict[k] for k in pred_dict])
    order = [names.index(k) for k in pred_dict]
    assert pred.cpu().numpy()[order].tolist() == c_pred.tolist()
    assert correct.cpu().numpy()[order].tolist() == (c_pred == truth).astype(np.uint8).tolist()
    assert int(correct.sum()) == 2 and int((counts > 0).sum()) == 4
    # bit-identical on repeat, and with each batch's rows in the same order under two launches (4 + 3 rows)
    sums2, counts2 = _run_votes(rows)
    sums3, counts3 = _run_votes(rows, split=4)
    assert torch.equal(sums2, sums) and torch.equal(sums3, sums) and torch.equal(counts2, counts) and torch.equal(counts3, counts)
    mean2, pred2, correct2 = vote_finalize(sums3, counts3, lab_t)
    assert torch.equal(mean2, mean) and torch.equal(pred2, pred) and torch.equal(correct2, correct)


def test_vote_finalize_tie_rule_and_division():
    from ted_spad_amd.action_eval import vote_finalize
    sums = synth_tensor(0, "votetie", (3, 70), 0, 1)
    sums[0, 3] = sums[0, 7] = 1.5
    sums[1] = 0.25
    counts = torch.tensor([3, 7, 1], dtype=torch.int32)
    mean, pred, correct = vote_finalize(sums.cuda(), counts.cuda(), torch.tensor([7, 69, 0]).cuda())
    assert pred.cpu().tolist()[:2] == [7, 69] and correct.cpu().tolist()[:2] == [1, 1]
    assert np.array_equal(mean.cpu().numpy(), sums.numpy() / counts.numpy().astype(np.float32)[:, None])    # IEEE division, not a reciprocal


def test_vote_accumulate_rejects_out_of_range_before_any_launch():
    from ted_spad_amd._lib import TedSpadHipError
    from ted_spad_amd.action_eval import vote_accumulate
    probs = torch.full((3, VC), 0.5, device="cuda")
    sums = torch.full((V, VC), -7.0, device="cuda")
    counts = torch.full((V,), -7, dtype=torch.int32, device="cuda")
    for vid in ([0, V, 1], [0, 1, -1]):
        with pytest.raises(TedSpadHipError):
            vote_accumulate(probs, vid, sums, counts)
    torch.cuda.synchronize()
    assert bool((sums == -7).all()) and bool((counts == -7).all())


# ---- the fixture captured from the reference's val_epoch_video / val_epoch ---------------------------------------------------------------
@pytest.fixture(scope="module")
def action_golden():
    with open(os.path.join(GOLDEN_DIR, "action_val_golden_meta.json")) as f:
        meta = json.load(f)
    return dict(np.load(os.path.join(GOLDEN_DIR, "action_val_golden.npz"))), meta


@pytest.mark.parametrize("fn", ["video", "action"])
def test_golden_logits_through_the_kernels(action_golden, fn):
    from ted_spad_amd.action_eval import softmax_ce_eval, vote_accumulate, vote_finalize
    g, meta = action_golden
    nv, nc = len(meta["names"]), meta["num_classes"]
    sums = torch.zeros(nv, nc, device="cuda")
    counts = torch.zeros(nv, dtype=torch.int32, device="cuda")
    labels_v = torch.tensor(meta["labels"], dtype=torch.int64).cuda()
    for k in range(len(meta["passes"])):
        z, lab, vid = (g["%s/pass%d/%s" % (fn, k, n)] for n in ("logits", "labels", "vid"))
        probs, _, loss, pred = softmax_ce_eval(torch.from_numpy(z).cuda(), lab)
        assert rel_l2(probs.cpu(), g["%s/pass%d/probs" % (fn, k)]) <= 1e-5
        assert rel_l2(loss.cpu(), g["%s/ce" % fn][k:k + 1]) <= 1e-5
        trip = g["%s/triplet" % fn]
        total = float(loss) + (meta["params"]["temporal_loss_weight"] * trip[k] if len(trip) else 0.0)
        assert abs(total - g["%s/pass_loss" % fn][k]) <= 1e-5 * g["%s/pass_loss" % fn][k]
        want = np.flip(np.argsort(g["%s/pass%d/probs" % (fn, k)], axis=1), axis=1)[:, 0]
        assert pred.cpu().tolist() == want.tolist()
        assert float(np.sum(pred.cpu().numpy() == lab)) / len(lab) == g["%s/pass_accuracy" % fn][k]
        vote_accumulate(probs, vid, sums, counts)
        mean, pred_v, correct = vote_finalize(sums, counts, labels_v)
        assert float(correct.sum()) / nv == g["%s/running_accuracy" % fn][k]
    assert rel_l2(mean.cpu(), g["%s/mean_probs" % fn]) <= 1e-5
    assert pred_v.cpu().tolist() == g["%s/predictions" % fn].tolist()
    assert int(correct.sum()) == int(g["%s/correct_count" % fn]) and float(correct.sum()) / nv == float(g["%s/accuracy" % fn])
    assert counts.cpu().tolist() == [len(meta["passes"])] * nv


# ---- ActionValidator end to end ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nets():
    from ted_spad_amd.model_loaders import load_fa_model, load_ft_model
    fa = load_fa_model(arch="unet")
    ft = load_ft_model("largei3d", num_classes=102)
    fa.load_state_dict(synth_state_dict(fa.state_dict(), 0))
    ft.load_state_dict(synth_state_dict(ft.state_dict(), 0))
    fa, ft = fa.cuda(), ft.cuda()
    x = synth_train_video(0, "action_val/mode0", (2, 48, 3, 64, 64)).cuda()
    fa.eval(); ft.eval()
    with torch.no_grad():                                            # the reference's statements over the factory's modules (:232,240-251)
        v = x.permute(0, 2, 1, 3, 4)
        anon = fa(v.reshape(-1, v.shape[1], v.shape[3], v.shape[4])).reshape(v.shape)
        heads = [ft(c) for c in torch.split(anon, [16, 16, 16], dim=2)]
        raw = ft(v[:, :, :16])[0]
    return fa, ft, x, heads, raw


PATHS = ["/data/ucf/mode0/v_Walk_g01_c01.avi", "/data/ucf/mode0/v_Run_g02_c03.avi"]


def _state(m):
    return {k: v.clone() for k, v in m.state_dict().items()}


def test_action_validator_end_to_end(nets):
    from ted_spad_amd.action_eval import ActionValidator
    from ted_spad_amd.losses import TripletMarginLoss
    fa, ft, x, heads, _ = nets
    logits_r = heads[0][0]
    labels = [int(logits_r[0].argmax()), (int(logits_r[1].argmax()) + 1) % 102]
    before = _state(fa), _state(ft)
    fa.train(); ft.train()
    val = ActionValidator(ft, fa)
    out = val.evaluate(x, labels, PATHS)
    assert not fa.training and not ft.training                       # left in eval, as val_epoch* leaves them (:220-221)
    assert all(v.is_cuda for v in out.values())
    assert torch.equal(out["logits"], logits_r)
    ce_r = float(nn.CrossEntropyLoss()(logits_r.double().cpu(), torch.tensor(labels)))
    assert abs(float(out["loss"]) - ce_r) <= 1e-5 * ce_r
    assert rel_l2(out["probs"].cpu(), torch.softmax(logits_r.double().cpu(), dim=1)) <= 1e-5
    assert out["pred"].cpu().tolist() == logits_r.argmax(1).cpu().tolist()
    p1 = val.end_pass()
    assert p1["accuracy"] == 0.5 and abs(p1["loss"] - ce_r) <= 1e-5 * ce_r and p1["running_accuracy"] == 0.5
    assert val.counts.cpu().tolist() == [1, 1]
    val.evaluate(x.flip(0), labels[::-1], ["/other/dir/" + p.split("/")[-1] for p in PATHS[::-1]])     # second pass: same names, other order
    p2 = val.end_pass()
    assert val.counts.cpu().tolist() == [2, 2] and p2["num_videos"] == 2
    res = val.result()
    assert res["names"] == [p.split("/")[-1] for p in PATHS] and res["labels"].tolist() == labels
    assert res["num_videos"] == 2 and res["correct_count"] == 1 and res["accuracy"] == 0.5
    assert abs(res["val_loss"] - np.mean([p1["loss"], p2["loss"]])) <= 1e-12
    assert res["mean_probs"].shape == (2, 102) and res["predictions"].tolist() == [labels[0], (labels[1] - 1) % 102]
    assert [len(res["pred_dict"][n]) for n in res["names"]] == [2, 2] and res["label_dict"] == dict(zip(res["names"], labels))
    assert np.array_equal(res["pred_dict"][res["names"][0]][0], out["probs"][0].cpu().numpy())
    for a, b in zip(before, (_state(fa), _state(ft))):               # parameters and buffers untouched
        assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    val.reset()
    assert val.counts.numel() == 0 and val.val_losses == []
    with pytest.raises(RuntimeError):
        val.result()
    # temporal_loss: CE + weight x triplet on the three eval features (train_anonymized_action.py:158-165)
    val_t = ActionValidator(ft, fa, temporal_loss=True)
    out_t = val_t.evaluate(x, labels, PATHS)
    assert torch.equal(out_t["logits"], logits_r)
    trip = float(TripletMarginLoss(margin=1)(heads[0][1], heads[1][1], heads[2][1]))
    trip64 = float(nn.TripletMarginLoss(margin=1)(*(h[1].double().cpu() for h in heads)))
    assert abs(trip - trip64) <= 1e-5 * trip64
    assert abs(float(out_t["loss"]) - (ce_r + 0.1 * trip)) <= 1e-5 * (ce_r + 0.1 * trip)
    with pytest.raises(ValueError):
        val_t.evaluate(x[:, :16], labels, PATHS)                     # the triplet needs three clips


def test_action_validator_without_anonymizer(nets):
    from ted_spad_amd.action_eval import ActionValidator
    _, ft, x, _, raw = nets
    val = ActionValidator(ft)
    out = val.evaluate(x, torch.tensor([3, 4]), PATHS)
    assert torch.equal(out["logits"], raw)
    out16 = val.evaluate(x[:, :16].contiguous(), np.array([3, 4]), PATHS)           # a single-clip loader (single_val_dataloader)
    assert torch.equal(out16["logits"], raw)
    assert val.end_pass()["num_videos"] == 2 and val.counts.cpu().tolist() == [2, 2]
