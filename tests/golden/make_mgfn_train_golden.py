"""Writes tests/golden/mgfn_train_golden.npz and mgfn_train_golden_meta.json: one training iteration of the reference's MGFN
(anomaly_detection_mgfn/models/mgfn.py in train mode, train.py's mgfn_loss / smooth / sparsity, cost.backward()).

The reference is imported in place on the CPU, one subprocess per case (`option.parse_args()` runs at import, so `sys.argv` carries the
config). `visdom` (and `tqdm` where absent) are stubbed; `torch.set_default_tensor_type` and `Tensor.cuda` are made no-ops for train.py:3 and
the `.cuda()` calls of MSNSD and mgfn_loss; `model.drop_out` is replaced by a module that returns the supplied masks (first call:
select_idx, second: select_idx_normal). train.py:88-91 hard-codes 32 segments; the same lines run here with the case's T.
Weights: `synth.synth_mgfn_state_dict` (with torch's default init every to_logits row has nearly the same norm and the top-k choice is a
coin toss); inputs: `synth_tensor` U[0, 2) under recorded names; labels 0 (normal) and 1 (abnormal). The masks are built from the reference's
fp64 magnitudes (build_masks) and stored.

Stored per case (fp64): every loss term, score_normal / score_abnormal / scores, the selected indices, per-parameter gradient norms, the
first 32 elements of every gradient, full gradients of tensors under 4096 elements, the BatchNorm buffers after the forward. Recorded in
the meta: the reference's own fp32-vs-fp64 error per quantity, per case and (`errors`, what the tests use) the largest over the cases; for
the loss scalars never less than 2^-23 of the value. Asserted: the masked magnitudes that decide the top-k choice and its order
are at least 100x the reference's fp32-vs-fp64 magnitude error apart.

    python tests/golden/make_mgfn_train_golden.py                   # writes the fixture
    python tests/golden/make_mgfn_train_golden.py --worker JOB OUT  # one case
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
F_SIZE, BATCH, K, DROP = 64, 2, 3, 0.7
CASES = {
    "a": dict(depths=[1, 1, 1], types=["gb", "fb", "fb"], T=32, ncrops=10),
    "b": dict(depths=[1, 1, 1], types=["gb", "fb", "fb"], T=5, ncrops=2),
    "c": dict(depths=[1, 1, 1], types=["gb", "fb", "fb"], T=3, ncrops=1),
    "d": dict(depths=[1, 1, 1], types=["fb", "gb", "gb"], T=32, ncrops=2),
}
LOSSES = ("cost", "loss_smooth", "loss_sparse", "loss_cls", "loss_con", "loss_con_n", "loss_con_a", "loss_total")
FULL_BELOW = 4096


def make_inputs(case, dtype=torch.float32, masks=None, salt=0):
    """(ninput, ainput, nlabel, alabel, masks) of a case; `masks` = (select_idx, select_idx_normal) as the fixture stores them (the
    generator builds them from the reference's magnitudes: build_masks)."""
    c = CASES[case]
    T, nc = c["T"], c["ncrops"]
    x = synth_tensor(SEED, "mgfn_train/%s/x%d" % (case, salt), (2 * BATCH, nc, T, F_SIZE + 1), 0.0, 2.0).to(dtype)
    if masks is not None:
        masks = tuple(torch.as_tensor(np.asarray(m)).to(dtype) for m in masks)
    return x[:BATCH], x[BATCH:], torch.zeros(BATCH, dtype=dtype), torch.ones(BATCH, dtype=dtype), masks


def build_masks(case, mags, req):
    """Dropout-like masks (0 or 1/(1-p)) under which the k + 1 largest surviving magnitudes of every row are at least `req` apart: per row,
    the chain of segments by falling magnitude with that spacing gives the k + 1 largest survivors (all T when T == k); the segments a
    Bernoulli(1-p) draw keeps are kept too where they lie at least `req` below the chain. None when a row has no such chain."""
    c = CASES[case]
    T = c["T"]
    need = min(T, K + 1)
    masks = []
    for which, rows in (("abn", mags[BATCH:]), ("nor", mags[:BATCH])):
        u = synth_tensor(SEED, "mgfn_train/%s/mask_%s" % (case, which), (BATCH, T)).numpy()
        keep = np.zeros((BATCH, T), dtype=bool)
        for r in range(BATCH):
            m = rows[r]
            chain = []
            for s in np.argsort(-m, kind="stable"):
                if not chain or m[chain[-1]] - m[s] >= req:
                    chain.append(int(s))
                if len(chain) == need:
                    break
            if len(chain) < need:
                return None
            keep[r, chain] = True
            keep[r] |= (u[r] >= DROP) & (m <= m[chain[-1]] - req)
        masks.append(keep.astype(np.float64) / (1.0 - DROP))
    return tuple(masks)


class _Masks(torch.nn.Module):
    def __init__(self, masks):
        super().__init__()
        self.masks, self.calls = masks, 0

    def forward(self, ones):
        m = self.masks[self.calls % 2]
        self.calls += 1
        assert m.shape == ones.shape
        return m.to(ones.dtype)


def worker(job_path, out_path):
    job = json.load(open(job_path))
    case = job["case"]
    c = CASES[case]
    sys.argv = ["mgfn", "--feature_size", str(F_SIZE), "--batch_size", str(BATCH)] + sum(
        (["--depths%d" % (i + 1), str(d), "--mgfn_type%d" % (i + 1), t] for i, (d, t) in enumerate(zip(c["depths"], c["types"]))), [])
    sys.modules.setdefault("visdom", types.ModuleType("visdom"))
    try:
        import tqdm  # noqa: F401
    except ImportError:
        sys.modules["tqdm"] = types.SimpleNamespace(tqdm=lambda it, **kw: it)
    sys.dont_write_bytecode = True
    torch.set_default_tensor_type = lambda *a, **k: None
    torch.Tensor.cuda = lambda self, *a, **k: self
    sys.path.insert(0, os.path.join(REFERENCE_ROOT, "anomaly_detection_mgfn"))
    import models.mgfn as ref  # noqa: E402
    import train as ref_train  # noqa: E402

    torch.manual_seed(0)
    sd = synth_mgfn_state_dict(ref.mgfn().state_dict(), SEED)
    res = {"keys": json.dumps([[k, list(v.shape)] for k, v in sd.items()])}
    salt = job["salt"]

    def magnitudes(m, video):
        # the crop-mean magnitudes MSNSD selects on (models/mgfn.py:32-33), from the to_logits output of a forward that leaves the buffers alone
        with torch.no_grad():
            keep_drop, m.drop_out = m.drop_out, _Masks((torch.ones(BATCH, c["T"]), torch.ones(BATCH, c["T"])))
            cap = {}
            hook = m.to_logits.register_forward_hook(lambda mod, i, o: cap.__setitem__("h", o))
            bns = [mod for mod in m.modules() if isinstance(mod, torch.nn.BatchNorm1d)]
            saved = [(b.momentum, b.num_batches_tracked.clone()) for b in bns]
            for b in bns:
                b.momentum = 0.0
            m(video)
            for b, (mom, nbt) in zip(bns, saved):
                b.momentum = mom
                b.num_batches_tracked.copy_(nbt)
            hook.remove()
            m.drop_out = keep_drop
            return torch.norm(cap["h"], p=2, dim=2).view(2 * BATCH, c["ncrops"], -1).mean(1).double().numpy()

    mg = {}
    for dt, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
        m = ref.mgfn()
        m.load_state_dict(sd)
        x = make_inputs(case, dt, salt=salt)
        mg[tag] = magnitudes(m.to(dt).train(), torch.cat((x[0], x[1]), 0))
    mag_err = float(np.abs(mg["f32"] - mg["f64"]).max())
    masks_np = build_masks(case, mg["f64"], 150 * mag_err)
    if masks_np is None:
        np.savez(out_path, infeasible=np.int64(1))
        return
    res["mask_abn"], res["mask_nor"], res["mag_err"] = masks_np[0], masks_np[1], np.float64(mag_err)
    for dt, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
        m = ref.mgfn()
        m.load_state_dict(sd)
        m = m.to(dt).train()
        ninput, ainput, nlabel, alabel, masks = make_inputs(case, dt, masks_np, salt)
        m.drop_out = _Masks(masks)
        T = c["T"]
        score_abnormal, score_normal, abn_feat, nor_feat, scores = m(torch.cat((ninput, ainput), 0))          # train.py:85-87
        flat = scores.view(BATCH * T * 2, -1).squeeze()                                                         # :88-90, T for 32
        abn_scores = flat[BATCH * T:]                                                                           # :91
        loss_criterion = ref_train.mgfn_loss(0.0001)                                                            # :96
        loss_sparse = ref_train.sparsity(abn_scores, BATCH, 8e-3)                                               # :97
        loss_smooth = ref_train.smooth(abn_scores, 8e-4)                                                        # :98
        loss_total = loss_criterion(score_normal, score_abnormal, nlabel, alabel, nor_feat, abn_feat)
        cost = loss_total + loss_smooth + loss_sparse                                                           # :100
        cost.backward()                                                                                         # :104
        # the parts of mgfn_loss, from its own classes on the same tensors (train.py:64-73)
        sep = int(len(abn_feat) / 2)
        la, ln_ = torch.norm(abn_feat, p=1, dim=2), torch.norm(nor_feat, p=1, dim=2)
        parts = dict(cost=cost, loss_smooth=loss_smooth, loss_sparse=loss_sparse, loss_total=loss_total,
                     loss_cls=loss_criterion.criterion(torch.cat((score_normal, score_abnormal), 0).squeeze(), torch.cat((nlabel, alabel), 0)),
                     loss_con=loss_criterion.contrastive(la, ln_, 1), loss_con_n=loss_criterion.contrastive(ln_[sep:], ln_[:sep], 0),
                     loss_con_a=loss_criterion.contrastive(la[sep:], la[:sep], 0))
        for k, v in parts.items():
            res["%s|loss|%s" % (tag, k)] = v.detach().double().numpy()
        res["%s|score_normal" % tag] = score_normal.detach().numpy()
        res["%s|score_abnormal" % tag] = score_abnormal.detach().numpy()
        res["%s|scores" % tag] = scores.detach().numpy()
        res["%s|abn_l1" % tag], res["%s|nor_l1" % tag] = la.detach().numpy(), ln_.detach().numpy()
        for k, p in m.named_parameters():
            assert p.grad is not None, k
            res["%s|grad|%s" % (tag, k)] = p.grad.numpy()
        for k, b in m.named_buffers():
            res["%s|bn|%s" % (tag, k)] = b.detach().numpy()
        mags = torch.from_numpy(mg[tag]).to(dt)
        res["%s|masked_mags_abn" % tag] = (mags[BATCH:] * masks[0]).numpy()
        res["%s|masked_mags_nor" % tag] = (mags[:BATCH] * masks[1]).numpy()
    np.savez(out_path, **res)


def run_worker(case, tmpdir):
    """The case with the first input salt for which build_masks finds masks. Returns (worker output, salt)."""
    job, out = os.path.join(tmpdir, "job_%s.json" % case), os.path.join(tmpdir, "out_%s.npz" % case)
    for salt in range(8):
        json.dump({"case": case, "salt": salt}, open(job, "w"))
        subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", job, out], check=True)
        R = dict(np.load(out))
        if "infeasible" not in R:
            return R, salt
    raise AssertionError("no input of case %s has well separated magnitudes" % case)


def _rel(a, b):
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300))


def topk_lowest_index_np(x, k):
    return np.argsort(-x, axis=1, kind="stable")[:, :k]


def main():
    import tempfile

    assert reference_available(), "the reference is needed to write the fixture"
    out, meta = {}, {"seed": SEED, "feature_size": F_SIZE, "batch_size": BATCH, "k": K, "dropout_rate": DROP, "mag_ratio": 0.1,
                     "cases": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for case, c in CASES.items():
            R, salt = run_worker(case, tmp)
            g = lambda tag, key: R["%s|%s" % (tag, key)]  # noqa: E731
            out["%s/mask_abn" % case], out["%s/mask_nor" % case] = R["mask_abn"], R["mask_nor"]
            cm = dict(c, salt=salt, state_dict=json.loads(str(R["keys"])), errors={"loss": {}, "grad_rel_l2": {}, "bn_rel_l2": {}})
            E = cm["errors"]
            for name in LOSSES:
                out["%s/loss/%s" % (case, name)] = g("f64", "loss|" + name)
                # at least one unit of fp32 resolution: a smaller difference is a coincidence of rounding (case d's loss_smooth came out 0.06
                # ulp from the fp64 value), not a measure of what fp32 arithmetic reaches
                E["loss"][name] = max(float(abs(g("f32", "loss|" + name) - g("f64", "loss|" + name))),
                                      2.0 ** -23 * float(abs(g("f64", "loss|" + name))))
            for name in ("score_normal", "score_abnormal", "scores"):
                out["%s/%s" % (case, name)] = g("f64", name)
            E["scores_max_abs"] = float(np.abs(g("f32", "scores") - g("f64", "scores")).max())
            E["l1_rel_l2"] = max(_rel(g("f32", "abn_l1"), g("f64", "abn_l1")), _rel(g("f32", "nor_l1"), g("f64", "nor_l1")))
            # ---- the top-k choice and its order are stable ----
            k_eff = min(c["T"], K + 1)
            gaps = {}
            for half in ("abn", "nor"):
                m64, m32 = g("f64", "masked_mags_" + half), g("f32", "masked_mags_" + half)
                err = float(np.abs(m32 - m64).max())
                top = -np.sort(-m64, axis=1)[:, :k_eff]
                gap = float(np.min(top[:, :-1] - top[:, 1:]))
                gaps[half] = {"gap": gap, "needed": 100 * err}
                assert gap >= 100 * err and gap > 0, (case, half, gap, err)
                idx = topk_lowest_index_np(m64, K)
                assert (idx == topk_lowest_index_np(m32.astype(np.float64), K)).all(), (case, half)
                assert (m64[np.arange(BATCH)[:, None], idx] > 0).all(), (case, half)            # every selected segment survived its mask
                out["%s/idx_%s" % (case, "abnormal" if half == "abn" else "normal")] = idx.astype(np.int64)
            cm["topk_gaps"] = gaps
            for key in R:
                if key.startswith("f64|grad|"):
                    name = key[len("f64|grad|"):]
                    g64, g32 = R[key], R["f32|grad|" + name]
                    assert np.linalg.norm(g64.ravel()) > 0, (case, name)
                    E["grad_rel_l2"][name] = _rel(g32, g64)
                    out["%s/gnorm/%s" % (case, name)] = np.float64(np.linalg.norm(g64.ravel()))
                    out["%s/g32/%s" % (case, name)] = g64.ravel()[:32].copy()
                    if g64.size < FULL_BELOW:
                        out["%s/gfull/%s" % (case, name)] = g64
                elif key.startswith("f64|bn|"):
                    name = key[len("f64|bn|"):]
                    out["%s/bn/%s" % (case, name)] = R[key]
                    if not name.endswith("num_batches_tracked"):
                        E["bn_rel_l2"][name] = _rel(R["f32|bn|" + name], R[key])
            meta["cases"][case] = cm
            v = sorted(E["grad_rel_l2"].values())
            print(case, "cost err %.2e  grad rel-L2 median %.2e worst %.2e  gaps %s" % (E["loss"]["cost"], v[len(v) // 2], v[-1], gaps))
    # The bound of the GPU tests is 10x meta["errors"]: per quantity the LARGEST error over the cases, as mgfn_golden_meta.json records it
    # (losses relative to their value). One case's own figure is a single draw of rounding noise: case d's fc.bias gradient, one number
    # summed over all tokens with mixed signs, came out 4.5e-8 from fp64 where the same quantity is 1.9e-6 off in case c.
    errs = {"loss_rel": {}, "grad_rel_l2": {}, "bn_rel_l2": {}, "scores_max_abs": 0.0}
    for case, cm in meta["cases"].items():
        E = cm["errors"]
        for name, e in E["loss"].items():
            errs["loss_rel"][name] = max(errs["loss_rel"].get(name, 0.0), e / abs(float(out["%s/loss/%s" % (case, name)])))
        for group in ("grad_rel_l2", "bn_rel_l2"):
            for name, e in E[group].items():
                errs[group][name] = max(errs[group].get(name, 0.0), e)
        errs["scores_max_abs"] = max(errs["scores_max_abs"], E["scores_max_abs"])
    meta["errors"] = errs
    path = os.path.join(HERE, "mgfn_train_golden.npz")
    np.savez_compressed(path, **out)
    with open(os.path.join(HERE, "mgfn_train_golden_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--worker":
        worker(sys.argv[2], sys.argv[3])
    else:
        main()
