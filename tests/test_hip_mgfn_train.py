"""-m gpu: MGFN training on MI355X (ted_spad_amd.mgfn.MGFNTrainStep). One iteration against the reference's recorded losses, selections,
gradients and BatchNorm buffers (tests/golden/mgfn_train_golden.npz) and against the fp64 restatement, each within 10x the reference's own
fp32-vs-fp64 error for that quantity (the largest over the fixture's cases: the rule of tests/test_hip_mgfn.py); determinism bit for bit; five Adam steps against the restatement's
fp64 trajectory; the eval path after training; the full-width model once; the refused shapes."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, rel_l2
from ted_spad_amd.mgfn import MGFN, MGFNTrainStep
from ted_spad_amd.synth import synth_mgfn_state_dict, synth_tensor

import mgfn_train_restate as R

sys.path.insert(0, GOLDEN_DIR)
import make_mgfn_train_golden as G  # noqa: E402

pytestmark = pytest.mark.gpu

BUFFERS = ("running_mean", "running_var", "num_batches_tracked")
_cache = {}


def _meta():
    if "meta" not in _cache:
        with open(os.path.join(GOLDEN_DIR, "mgfn_train_golden_meta.json")) as f:
            _cache["meta"] = json.load(f)
        _cache["gold"] = dict(np.load(os.path.join(GOLDEN_DIR, "mgfn_train_golden.npz")))
    return _cache["meta"], _cache["gold"]


def _cfg(meta, case):
    c = meta["cases"][case]
    return (meta["feature_size"], tuple(c["depths"]), tuple(c["types"]), meta["mag_ratio"])


def _model(meta, case):
    c = meta["cases"][case]
    m = MGFN(feature_size=meta["feature_size"], depths=tuple(c["depths"]), mgfn_types=tuple(c["types"]))
    m.load_state_dict(synth_mgfn_state_dict(m.state_dict(), meta["seed"]))
    return m.cuda()


def _inputs(meta, gold, case, dtype=torch.float32):
    return G.make_inputs(case, dtype, (gold[case + "/mask_abn"], gold[case + "/mask_nor"]), meta["cases"][case]["salt"])


def _restatement(meta, gold, case):
    """The fp64 restatement of the case, computed once: (result, gradients, BatchNorm buffers)."""
    key = "restate/" + case
    if key not in _cache:
        m = _model(meta, case)
        sd = {k: (v.cpu().double() if v.is_floating_point() else v.cpu()) for k, v in m.state_dict().items()}
        _cache[key] = R.grads(sd, *_inputs(meta, gold, case, torch.float64), _cfg(meta, case), k=meta["k"])
    return _cache[key]


def _run(meta, gold, case, model=None):
    model = model or _model(meta, case)
    ni, ai, nl, al, masks = _inputs(meta, gold, case)
    drv = MGFNTrainStep(model, meta["batch_size"], dropout_rate=meta["dropout_rate"], k=meta["k"])
    out = drv.forward_backward(ni.cuda(), ai.cuda(), nl.cuda(), al.cuda(), tuple(m.cuda() for m in masks))
    return model, drv, out


@pytest.mark.parametrize("case", ["a", "b", "c", "d"])
def test_gradients_vs_reference_fixture(case):
    meta, gold = _meta()
    E = meta["errors"]                                             # per quantity, the largest over the fixture's cases
    model, _, out = _run(meta, gold, case)
    r64, g64, bn64 = _restatement(meta, gold, case)
    for name in G.LOSSES:
        want = float(gold["%s/loss/%s" % (case, name)])
        got, bound = out[name], 10 * E["loss_rel"][name] * abs(want)
        print("%s %-12s %.9g  reference %.9g  |diff| %.2e  bound %.2e" % (case, name, got, want, abs(got - want), bound))
        assert abs(got - want) <= bound, (name, got, want, bound)
    assert torch.equal(out["idx_normal"].cpu(), torch.from_numpy(gold[case + "/idx_normal"]))
    assert torch.equal(out["idx_abnormal"].cpu(), torch.from_numpy(gold[case + "/idx_abnormal"]))
    for name in ("score_normal", "score_abnormal", "scores"):
        e = float(np.abs(out[name].cpu().double().numpy() - gold["%s/%s" % (case, name)]).max())
        print("%s %-14s max abs %.2e  bound %.2e" % (case, name, e, 10 * E["scores_max_abs"]))
        assert out[name].shape == gold["%s/%s" % (case, name)].shape and e <= 10 * E["scores_max_abs"], name
    sd = model.state_dict()
    for k in sd:
        if k.endswith("num_batches_tracked"):
            assert int(sd[k]) == int(gold["%s/bn/%s" % (case, k)]) == 1
        elif k.endswith(BUFFERS):
            e = rel_l2(sd[k].cpu().double().numpy(), gold["%s/bn/%s" % (case, k)])
            print("%s %-44s rel-L2 %.2e  bound %.2e" % (case, k, e, 10 * E["bn_rel_l2"][k]))
            assert e <= 10 * E["bn_rel_l2"][k], k
    worst = 0.0
    for k, p in model.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape and p.grad.dtype == torch.float32, k
        g = p.grad.cpu().double()
        gn, bound = float(gold["%s/gnorm/%s" % (case, k)]), 10 * E["grad_rel_l2"][k]
        e_norm = abs(float(g.norm()) - gn) / gn
        e_32 = float(np.abs(g.reshape(-1)[:32].numpy() - gold["%s/g32/%s" % (case, k)]).max()) / gn       # on the scale of the whole gradient
        e_full = rel_l2(g.numpy(), g64[k].numpy())
        worst = max(worst, e_full / bound)
        print("%s %-44s norm %.2e  sample %.2e  full vs fp64 restatement %.2e  bound %.2e" % (case, k, e_norm, e_32, e_full, bound))
        assert e_norm <= bound and e_32 <= bound and e_full <= bound, k
        if g.numel() < G.FULL_BELOW:
            assert rel_l2(g.numpy(), gold["%s/gfull/%s" % (case, k)]) <= bound, k
    print("%s worst gradient error / bound %.3f" % (case, worst))


def test_forward_backward_is_deterministic():
    meta, gold = _meta()
    runs = []
    for _ in range(2):
        model, _, out = _run(meta, gold, "a")
        runs.append((out, [p.grad.clone() for p in model.parameters()], [b.clone() for b in model.buffers()]))
    (o1, g1, b1), (o2, g2, b2) = runs
    assert all(o1[k] == o2[k] for k in G.LOSSES)
    assert all(torch.equal(o1[k], o2[k]) for k in ("score_normal", "score_abnormal", "scores", "idx_normal", "idx_abnormal"))
    assert all(torch.equal(p, q) for p, q in zip(g1, g2)) and all(torch.equal(p, q) for p, q in zip(b1, b2))


def _restate_trajectory(sd, inputs, cfg, k, steps, dtype):
    """`steps` costs of the restatement stepped with torch.optim.Adam(lr=1e-3, weight_decay=5e-4) (main.py:72-73) on the CPU."""
    prm = {key: (v.to(dtype).clone().requires_grad_(True) if not key.endswith(BUFFERS) else v.clone()) for key, v in sd.items()}
    opt = torch.optim.Adam([v for v in prm.values() if v.requires_grad], lr=1e-3, weight_decay=5e-4)
    ni, ai, nl, al, masks = inputs
    costs = []
    for _ in range(steps):
        bn_out = {}
        opt.zero_grad()
        r = R.train_cost(prm, ni, ai, nl, al, masks, cfg, k, bn_out)
        r["cost"].backward()
        opt.step()
        prm.update(bn_out)
        costs.append(float(r["cost"]))
    return costs


def test_five_steps_then_eval_path():
    meta, gold = _meta()
    case, steps = "a", 5
    model = _model(meta, case)
    sd0 = {k: v.cpu().clone() for k, v in model.state_dict().items()}
    cfg = _cfg(meta, case)
    c64 = _restate_trajectory({k: (v.double() if v.is_floating_point() else v) for k, v in sd0.items()}, _inputs(meta, gold, case, torch.float64),
                              cfg, meta["k"], steps, torch.float64)
    c32 = _restate_trajectory(sd0, _inputs(meta, gold, case, torch.float32), cfg, meta["k"], steps, torch.float32)
    ni, ai, nl, al, masks = _inputs(meta, gold, case)
    args = (ni.cuda(), ai.cuda(), nl.cuda(), al.cuda(), tuple(m.cuda() for m in masks))
    drv = MGFNTrainStep(model, meta["batch_size"], lr=1e-3, weight_decay=5e-4, dropout_rate=meta["dropout_rate"], k=meta["k"])
    drv.set_lr(1e-3)
    costs = [drv.step(*args)["cost"] for _ in range(steps)]
    for i in range(steps):
        own = abs(c32[i] - c64[i])
        print("step %d cost %.9g  fp64 restatement %.9g  |diff| %.2e  restatement fp32-vs-fp64 %.2e" % (i, costs[i], c64[i], abs(costs[i] - c64[i]), own))
    for i in range(steps):
        assert abs(costs[i] - c64[i]) <= 10 * abs(c32[i] - c64[i]), (i, costs[i], c64[i], c32[i])
    assert costs[-1] < costs[0]
    # ---- the eval path after training: packed weights are rebuilt, the running statistics are used ----
    keys = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    assert keys == meta["cases"][case]["state_dict"]
    assert all(int(v) == steps for k, v in model.state_dict().items() if k.endswith("num_batches_tracked"))
    v = synth_tensor(3, "mgfn_train_eval_video", (7, 10, meta["feature_size"] + 1), 0.0, 2.0).cuda()
    model.eval()
    s_trained = model.score([v])[0]
    fresh = MGFN(feature_size=meta["feature_size"], depths=cfg[1], mgfn_types=cfg[2])
    fresh.load_state_dict(model.state_dict())
    fresh = fresh.cuda().eval()
    assert torch.equal(s_trained, fresh.score([v])[0])
    untrained = _model(meta, case).eval()
    assert not torch.equal(s_trained, untrained.score([v])[0])
    model.train()
    with pytest.raises(NotImplementedError, match="MGFNTrainStep"):
        model(v.permute(1, 0, 2).unsqueeze(0))


def test_full_width_once():
    F_, n, nc, T = 2048, 2, 10, 32
    m = MGFN()                                                        # F = 2048, depths 3 / 3 / 2
    m.load_state_dict(synth_mgfn_state_dict(m.state_dict(), 0))
    m = m.cuda()
    x = synth_tensor(4, "mgfn_train_full", (2 * n, nc, T, F_ + 1), 0.0, 2.0).cuda()
    masks = tuple((synth_tensor(4, "mgfn_train_full_mask%d" % i, (n, T)) >= 0.5).float().cuda() / 0.3 for i in range(2))
    out = MGFNTrainStep(m, n).forward_backward(x[:n], x[n:], torch.zeros(n).cuda(), torch.ones(n).cuda(), masks)
    for name in G.LOSSES:
        assert np.isfinite(out[name]), (name, out[name])
    total = out["loss_cls"] + (0.001 * out["loss_con"] + out["loss_con_a"] + out["loss_con_n"]) * 0.001
    assert abs(out["loss_total"] - total) <= 1e-6 * abs(total)
    assert abs(out["cost"] - (out["loss_total"] + out["loss_smooth"] + out["loss_sparse"])) <= 1e-6 * abs(out["cost"])
    for k, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, k


def test_refused_shapes_raise():
    F_ = 64
    m = MGFN(feature_size=F_, depths=(1, 1, 1)).cuda()
    with pytest.raises(ValueError, match="batch_size == 1"):
        MGFNTrainStep(m, 1)
    z, o = torch.zeros(3).cuda(), torch.ones(3).cuda()
    x = torch.rand(3, 1, 8, F_ + 1).cuda()
    with pytest.raises(ValueError, match="odd"):
        MGFNTrainStep(m, 3).forward_backward(x, x, z, o)
    x = torch.rand(2, 2, 2, F_ + 1).cuda()
    with pytest.raises(ValueError, match="segments < k"):
        MGFNTrainStep(m, 2).forward_backward(x, x, z[:2], o[:2])
    x = torch.rand(2, 2, 8, F_ + 1).cuda()
    with pytest.raises(ValueError, match="masks"):
        MGFNTrainStep(m, 2).forward_backward(x, x, z[:2], o[:2], masks=(torch.ones(2, 7).cuda(), torch.ones(2, 8).cuda()))
    out = MGFNTrainStep(m, 2).forward_backward(x, x, z[:2], o[:2])              # masks drawn on the device
    assert np.isfinite(out["cost"]) and m.training
