"""CPU: the fp64 MGFN restatement (tests/mgfn_restate.py) against the reference's recorded outputs (tests/golden/mgfn_golden.npz), against
the reference model itself on a config the fixture does not hold (skipped without the reference), and the state_dict layout of
ted_spad_amd.mgfn.MGFN against the reference's."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, rel_l2
from ted_spad_amd.mgfn import MGFN
from ted_spad_amd.synth import synth_mgfn_state_dict, synth_tensor

import mgfn_restate

sys.path.insert(0, GOLDEN_DIR)
from _refimport import reference_available  # noqa: E402


def _meta():
    with open(os.path.join(GOLDEN_DIR, "mgfn_golden_meta.json")) as f:
        return json.load(f)


def _golden():
    return dict(np.load(os.path.join(GOLDEN_DIR, "mgfn_golden.npz")))


def _cfg(c):
    return (c["feature_size"], tuple(c["depths"]), tuple(c["types"]), 0.1)


def _model(c, seed):
    m = MGFN(feature_size=c["feature_size"], depths=tuple(c["depths"]), mgfn_types=tuple(c["types"])).eval()
    m.load_state_dict(synth_mgfn_state_dict(m.state_dict(), seed))
    return m


def test_state_dict_matches_reference_layout():
    meta = _meta()
    for c in ("a", "b", "c"):
        cfg = meta["configs"][c]
        ours = [[k, list(v.shape)] for k, v in _model(cfg, meta["seed"]).state_dict().items()]
        assert ours == cfg["state_dict"], c
    d = MGFN().state_dict()
    assert len(d) == 145
    assert tuple(d["stages.0.0.layers.0.1.norm.g"].shape) == (1, 64, 1) and "to_logits.0.weight" in d


@pytest.mark.parametrize("case", ["a_T3", "a_T7", "a_T32", "a_T300", "b_T32", "c_T32"])
def test_fp64_restatement_matches_fixture(case):
    meta, gold = _meta(), _golden()
    m = meta["cases"][case]
    cfg = meta["configs"][m["config"]]
    sd = {k: v.double() for k, v in _model(cfg, meta["seed"]).state_dict().items()}
    video = synth_tensor(meta["seed"], m["video"], (1, meta["ncrops"], m["T"], m["F"] + 1), 0.0, 2.0).double()
    with torch.no_grad():
        r = mgfn_restate.forward(sd, video, _cfg(cfg))
    for k in ("crop_scores", "logits", "mags"):
        e = rel_l2(r[k].numpy(), gold["%s/%s" % (case, k)])
        print(case, k, "rel-L2 %.2e" % e)
        assert e < 1e-10, (k, e)                              # fp64 against fp64: only the summation order differs
    idx = torch.topk(r["crop_mags"], 3)[1].numpy()
    assert (idx == gold["%s/idx" % case]).all()
    assert rel_l2(r["h"][:, idx].numpy(), gold["%s/feat" % case]) < 1e-6   # the fixture keeps features in fp32


@pytest.mark.skipif(not reference_available(), reason="the reference is not on this machine")
def test_fp64_restatement_matches_reference_model():
    """A config that is not in the fixture: F = 1024, depths (2, 1, 1), types (gb, gb, fb), T = 5, run by the fixture generator's worker."""
    cfg = dict(feature_size=1024, depths=[2, 1, 1], types=["gb", "gb", "fb"])
    name, T = "mgfn_video/extra/T5", 5
    with tempfile.TemporaryDirectory() as tmp:
        job, out = os.path.join(tmp, "job.json"), os.path.join(tmp, "out.npz")
        json.dump({"cfg": cfg, "videos": [[name, T]]}, open(job, "w"))
        subprocess.run([sys.executable, os.path.join(GOLDEN_DIR, "make_mgfn_golden.py"), "--worker", job, out], check=True)
        ref = dict(np.load(out))
    sd = {k: v.double() for k, v in _model(cfg, 0).state_dict().items()}
    video = synth_tensor(0, name, (1, 10, T, 1025), 0.0, 2.0).double()
    with torch.no_grad():
        r = mgfn_restate.forward(sd, video, _cfg(cfg))
    for k in ("crop_scores", "logits", "mags", "h"):
        e = rel_l2(r[k].numpy(), ref["f64|%s|%s" % (name, k)])
        print(k, "rel-L2 %.2e" % e)
        assert e < 1e-10, (k, e)
