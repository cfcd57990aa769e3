"""CPU: the fp64 restatement of one MGFN training iteration (tests/mgfn_train_restate.py) against the reference's recorded losses,
selections, gradients and BatchNorm buffers (tests/golden/mgfn_train_golden.npz, written by tests/golden/make_mgfn_train_golden.py from
the reference's own train-mode forward, mgfn_loss, smooth, sparsity and backward); the refused shapes; the top-k tie rule."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR
from ted_spad_amd.mgfn import MGFN
from ted_spad_amd.synth import synth_mgfn_state_dict

import mgfn_train_restate as R

sys.path.insert(0, GOLDEN_DIR)
import make_mgfn_train_golden as G  # noqa: E402

REL = 1e-9


def _meta():
    with open(os.path.join(GOLDEN_DIR, "mgfn_train_golden_meta.json")) as f:
        return json.load(f)


def _golden():
    return dict(np.load(os.path.join(GOLDEN_DIR, "mgfn_train_golden.npz")))


def state_dict_of(meta, case, dtype=torch.float64):
    c = meta["cases"][case]
    m = MGFN(feature_size=meta["feature_size"], depths=tuple(c["depths"]), mgfn_types=tuple(c["types"]))
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in synth_mgfn_state_dict(m.state_dict(), meta["seed"]).items()}


def inputs_of(meta, gold, case, dtype):
    return G.make_inputs(case, dtype, (gold[case + "/mask_abn"], gold[case + "/mask_nor"]), meta["cases"][case]["salt"])


def _close(name, got, want, rel=REL):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    e = np.linalg.norm((got - want).ravel()) / max(np.linalg.norm(want.ravel()), 1e-300)
    assert got.shape == want.shape and e <= rel, (name, e)


@pytest.mark.parametrize("case", ["a", "b", "c", "d"])
def test_fp64_restatement_matches_fixture(case):
    meta, gold = _meta(), _golden()
    c = meta["cases"][case]
    cfg = (meta["feature_size"], tuple(c["depths"]), tuple(c["types"]), meta["mag_ratio"])
    r, g, bn = R.grads(state_dict_of(meta, case), *inputs_of(meta, gold, case, torch.float64), cfg, k=meta["k"])
    for name in G.LOSSES:
        _close(name, r[name].numpy(), gold["%s/loss/%s" % (case, name)])
    assert abs(float(r["cost"]) - float(r["loss_total"] + r["loss_smooth"] + r["loss_sparse"])) <= 1e-12 * abs(float(r["cost"]))
    for name in ("score_normal", "score_abnormal", "scores"):
        _close(name, r[name].numpy(), gold["%s/%s" % (case, name)])
    assert (r["idx_normal"].numpy() == gold[case + "/idx_normal"]).all() and (r["idx_abnormal"].numpy() == gold[case + "/idx_abnormal"]).all()
    keys = [k for k, _ in c["state_dict"]]
    assert sorted(g) == sorted(k for k in keys if not k.endswith(("running_mean", "running_var", "num_batches_tracked")))
    for k, v in g.items():
        _close("gnorm " + k, float(v.norm()), gold["%s/gnorm/%s" % (case, k)])
        # a sample of 32 elements is compared on the scale of the whole gradient
        d = np.abs(v.reshape(-1)[:32].numpy() - gold["%s/g32/%s" % (case, k)]).max()
        assert d <= REL * float(gold["%s/gnorm/%s" % (case, k)]), (k, d)
        if v.numel() < G.FULL_BELOW:
            _close("gfull " + k, v.numpy(), gold["%s/gfull/%s" % (case, k)])
    for k, v in bn.items():
        _close("bn " + k, v.numpy(), gold["%s/bn/%s" % (case, k)])
    assert len(bn) == sum(1 for k in keys if k.endswith(("running_mean", "running_var", "num_batches_tracked")))


def test_refused_shapes():
    with pytest.raises(ValueError, match="batch_size == 1"):
        R.check_shapes(1, 10, 32, 3)
    with pytest.raises(ValueError, match="even"):
        R.check_shapes(3, 1, 32, 3)
    with pytest.raises(ValueError, match="segments < k"):
        R.check_shapes(2, 10, 2, 3)
    R.check_shapes(2, 1, 3, 3)


def test_topk_tie_rule_lowest_index_wins():
    x = torch.tensor([[0.0, 5.0, 0.0, 0.0, 7.0, 0.0],            # two survivors: the third pick is the first zero
                      [2.0, 2.0, 2.0, 2.0, 2.0, 2.0],
                      [0.0, 0.0, 0.0, 1.0, 0.0, 0.0]], dtype=torch.float64)
    assert R.topk_lowest_index(x, 3).tolist() == [[4, 1, 0], [0, 1, 2], [3, 0, 1]]
    # the whole cost with a row that has fewer than k survivors: the selection is the rule's, and gradients reach only those rows
    n, nc, T, C = 2, 2, 6, 8
    gen = torch.Generator().manual_seed(3)
    h = torch.randn(2 * n * nc, T, C, generator=gen, dtype=torch.float64).requires_grad_(True)
    s = torch.rand(2 * n * nc, T, generator=gen, dtype=torch.float64)
    m_abn = torch.ones(n, T, dtype=torch.float64)
    m_abn[0] = 0
    m_abn[0, 4] = 1
    r = R.msnsd_cost(h, s, n, nc, (m_abn, torch.ones(n, T, dtype=torch.float64)), torch.zeros(n), torch.ones(n))
    assert r["idx_abnormal"][0].tolist() == [4, 0, 1]
    r["cost"].backward()
    rows = h.grad.view(2 * n, nc, T, C)[n].abs().sum((0, 2))     # abnormal video 0
    assert (rows[[4, 0, 1]] > 0).all() and (rows[[2, 3, 5]] == 0).all()
