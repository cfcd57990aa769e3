"""CPU: the training side of the non-local block -- the float64 restatement (tests/nl_grad_ref.py) against the reference's recorded train-mode
results, its closed-form attention gradients against autograd, and the new entries' declarations and argument checks."""
import json
import os
import re
from collections import OrderedDict

import numpy as np
import pytest
import torch

import nl_grad_ref
import nl_ref
from conftest import GOLDEN_DIR, ROOT
from ted_spad_amd.synth import synth_tensor

NEW = ("tedspad_nl_attention_fwd_lse", "tedspad_nl_attention_bwd_workspace", "tedspad_nl_attention_bwd")


@pytest.fixture(scope="module")
def train_golden():
    return dict(np.load(os.path.join(GOLDEN_DIR, "nl_train_golden.npz")))


@pytest.fixture(scope="module")
def train_meta():
    with open(os.path.join(GOLDEN_DIR, "nl_train_golden_meta.json")) as f:
        return json.load(f)


def train_case(name, meta):
    """(x, state_dict, prefix, dy) of a stored case, rebuilt from synth and the stored gain."""
    from ted_spad_amd.i3res50 import NonLocalBlock
    b = meta["cases"][name]
    p = name + ".nl."
    tmpl = OrderedDict((p + k, v) for k, v in NonLocalBlock(*b["dims"]).state_dict().items())
    sd = nl_ref.nl_state_dict(tmpl, meta["seed"], {p: b["gain"]})
    x = synth_tensor(meta["seed"], name + "/in", tuple(b["input"]), -1.0, 1.0)
    return x, sd, p, synth_tensor(meta["seed"], name + "/dy", tuple(b["input"]), -1.0, 1.0)


@pytest.mark.parametrize("name", ["nl_block512", "nl_block1024"])
def test_train_restatement_matches_the_reference(name, train_golden, train_meta):
    """Output, d(input), running statistics and the ten parameter gradients at rel-L2 < 1e-4 (the reference ran in fp32: test_nl_host.py's tolerance);
    out.bias.grad is analytically 0 (bn removes the mean) and is compared absolutely, by the rule of tests/test_hip_train_ops.py:139 -- and so are
    g.bias.grad and phi.bias.grad, which are analytically 0 as well (nl_grad_ref.ZERO_GRADS): the reference's own values of the three are its fp32
    rounding noise (1e-5 against 4 for theta.bias.grad), which no relative comparison can be held to."""
    x, sd, p, dy = train_case(name, train_meta)
    c = train_meta["cases"][name]
    r = nl_grad_ref.block_train(x, sd, p, dy, "train", eps=c["eps"], momentum=c["momentum"])
    keys = ["out", "dx", "running_mean", "running_var"] + ["grad/" + k for k in nl_grad_ref.PARAMS]
    assert sorted(k for k in r if k != "branch_dx") == sorted(keys)
    for k in keys:
        if k[5:] in nl_grad_ref.ZERO_GRADS["train"]:
            # the tolerances of this test at the scale of theta.bias.grad, the one bias gradient that is not zero (a sum of the same kind over the same
            # pixels): 1e-4 of its norm for the fp32 reference's rounding noise, 1e-12 (the closed form's tolerance below) for the float64 restatement
            scale = float(train_golden[name + "/grad/theta.bias/norm"])
            noise = float(np.abs(train_golden[name + "/" + k + "/sample"]).max())
            print("%s %s (analytically 0): restatement %.2e, reference %.2e, scale %.2e" % (name, k, float(r[k].abs().max()), noise, scale))
            assert float(r[k].abs().max()) < 1e-12 * scale and noise < 1e-4 * scale < 2e-2 * c["dy_abs_sum"] ** 0.5
            continue
        e, dn = nl_grad_ref.vs_fixture(r[k], train_golden, name + "/" + k)
        print("%s %s: rel-L2 on the sample %.2e, norm off by %.2e" % (name, k, e, dn))
        assert e < 1e-4 and dn < 1e-4, (name, k)


def test_fixture_is_small_and_samples_are_fixed(train_golden):
    size = sum(os.path.getsize(os.path.join(GOLDEN_DIR, f)) for f in ("nl_train_golden.npz", "nl_train_golden_meta.json"))
    assert size <= 1000000
    assert len(train_golden["nl_block512/out/sample"]) == len(nl_grad_ref.sample_index(2 * 512 * 2 * 7 * 7))
    idx = nl_grad_ref.sample_index(2 * 512 * 2 * 7 * 7)
    assert len(set((idx % 49).tolist())) == 49 and len(set((idx // 49 % 512).tolist())) == 512      # every pixel of the 7 x 7 frame, every channel


@pytest.mark.parametrize("n,q,k,d", [(2, 12, 3, 16), (1, 7, 1, 8), (1, 33, 40, 32)])
def test_closed_form_attention_gradients_match_autograd(n, q, k, d):
    th, ph, g, dt = (synth_tensor(11, "%s/%d/%d" % (t, q, k), s, -1.0, 1.0).double() for t, s in
                     (("th", (n, q, d)), ("ph", (n, k, d)), ("g", (n, k, d)), ("dt", (n, q, d))))
    scale = float(d) ** -0.5
    r = nl_grad_ref.attention_grads(th * 3, ph * 3, g, dt, scale)
    a = nl_grad_ref.attention_autograd(th * 3, ph * 3, g, dt, scale)
    for got, ref in zip((r["dtheta"], r["dphi"], r["dg"]), a):
        assert float((got - ref).abs().max()) < 1e-12
    assert float((r["t"] - nl_ref.attention(th * 3, ph * 3, g, scale)).abs().max()) < 1e-12
    s = torch.einsum("nqd,nkd->nqk", th * 3, ph * 3) * scale
    assert float((r["lse"] - torch.log(torch.exp(s).sum(dim=2))).abs().max()) < 1e-12
    if k == 1:
        assert float(r["dtheta"].abs().max()) == 0.0 and float(r["dphi"].abs().max()) < 1e-15


def test_frozen_mode_of_the_restatement():
    """'frozen': the running statistics are a fixed affine -- they do not move, gamma / beta get no gradient, and the output is nl_ref.block's."""
    from ted_spad_amd.i3res50 import NonLocalBlock
    p = "b."
    tmpl = OrderedDict((p + k, v) for k, v in NonLocalBlock(16, 16, 8).state_dict().items())
    sd = nl_ref.nl_state_dict(tmpl, 3)
    x, dy = synth_tensor(3, "x", (2, 16, 1, 5, 4), -1.0, 1.0), synth_tensor(3, "dy", (2, 16, 1, 5, 4), -1.0, 1.0)
    r = nl_grad_ref.block_train(x, sd, p, dy, "frozen")
    assert "grad/bn.weight" not in r and "grad/bn.bias" not in r and "grad/out.bias" in r
    assert torch.equal(r["running_mean"], sd[p + "bn.running_mean"].double()) and torch.equal(r["running_var"], sd[p + "bn.running_var"].double())
    assert float((r["out"] - nl_ref.block(x, sd, p)).abs().max()) < 1e-12
    assert torch.equal(r["branch_dx"], r["dx"] - dy.double())


def test_given_values_equal_to_the_forwards_own_reproduce_the_gradients():
    """block_train(given=...) evaluates the backward AT given intermediates with the float64 derivative rules: given the float64 forward's own theta,
    phi, g, T and batch statistics it must return the ungiven results; given perturbed ones it must not."""
    from ted_spad_amd.i3res50 import NonLocalBlock
    p = "b."
    tmpl = OrderedDict((p + k, v) for k, v in NonLocalBlock(16, 16, 8).state_dict().items())
    sd = nl_ref.nl_state_dict(tmpl, 5)
    x, dy = synth_tensor(5, "x", (2, 16, 2, 5, 4), -1.0, 1.0), synth_tensor(5, "dy", (2, 16, 2, 5, 4), -1.0, 1.0)
    plain = nl_grad_ref.block_train(x, sd, p, dy, "train")
    th, ph, g = nl_ref.block_parts(x, sd, p)
    t = nl_ref.attention(th, ph, g, 8.0 ** -0.5)
    o = nl_ref._pw(t.transpose(1, 2).reshape(2, 8, 2, 5, 4), sd[p + "out.weight"], sd[p + "out.bias"])
    own = dict(theta=th, phi=ph, g=g, t=t, mean=o.mean(dim=(0, 2, 3, 4)), var=o.var(dim=(0, 2, 3, 4), unbiased=False))
    same = nl_grad_ref.block_train(x, sd, p, dy, "train", given=own)
    assert list(same) == list(plain)
    for k in plain:
        assert float((same[k] - plain[k]).abs().max()) < 1e-12 * max(1.0, float(plain[k].abs().max())), k
    moved = nl_grad_ref.block_train(x, sd, p, dy, "train", given=dict(own, t=t * 1.01))
    assert float((moved["grad/out.weight"] - plain["grad/out.weight"]).abs().max()) > 1e-6
    assert float((moved["grad/theta.weight"] - plain["grad/theta.weight"]).abs().max()) > 1e-9


def test_new_symbols_are_declared_everywhere():
    from ted_spad_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "tedspad_hip.h")).read()
    lib = _lib.lib()
    for s in NEW:
        assert re.search(r"int32_t\s+%s\s*\(" % s, hdr), s
        assert s in _lib.SYMBOLS and hasattr(lib, s), s
    assert re.search(r"#define\s+TEDSPAD_ABI_VERSION\s+5\b", hdr) and _lib.ABI_VERSION == 5 and lib.tedspad_abi_version() == 5
    src = open(os.path.join(ROOT, "ted_spad_amd", "csrc", "nonlocal.hip")).read()
    assert src.count("launch_lds<") >= 4 and "atomicAdd" not in src


def test_unsupported_width_is_the_librarys_error_in_both_new_entries():
    """d = 128: TEDSPAD_EINVAL with a message from tedspad_nl_attention_fwd_lse and tedspad_nl_attention_bwd, before anything touches a device."""
    import ctypes as C
    from ted_spad_amd import _lib
    lib = _lib.lib()
    rc = lib.tedspad_nl_attention_fwd_lse(16, 128, 16, 128, 16, 128, 32, 128, 64, 1, 4, 4, 128, 1.0, _lib.F16, None)
    assert rc != 0 and b"tedspad_nl_attention_fwd_lse" in lib.tedspad_last_error() and b"d = 128" in lib.tedspad_last_error()
    rc = lib.tedspad_nl_attention_bwd(16, 128, 32, 128, 48, 128, 64, 128, 80, 128, 96, 112, 128, 128, 128, 144, 128, 160, 1, 4, 4, 128, 1.0, _lib.F16, None)
    assert rc != 0 and b"tedspad_nl_attention_bwd" in lib.tedspad_last_error() and b"d = 128" in lib.tedspad_last_error()
    with pytest.raises(_lib.TedSpadHipError):
        _lib.check(rc, "tedspad_nl_attention_bwd")
    nbytes = C.c_int64(0)
    assert lib.tedspad_nl_attention_bwd_workspace(3, 392, C.byref(nbytes)) == 0 and nbytes.value == 3 * 392 * 4
    assert lib.tedspad_nl_attention_bwd_workspace(0, 392, C.byref(nbytes)) != 0
