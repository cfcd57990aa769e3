"""CPU: the non-local variant of I3Res50 -- the float64 restatement against the reference's stored block outputs, the parameter layout against the
reference's key list, the training refusals, and the new symbol's three declarations."""
import json
import os
import re
from collections import OrderedDict

import numpy as np
import pytest
import torch

import nl_ref
from conftest import GOLDEN_DIR, ROOT, rel_l2
from ted_spad_amd.synth import synth_tensor


@pytest.fixture(scope="module")
def nl_golden():
    return dict(np.load(os.path.join(GOLDEN_DIR, "nl_golden.npz")))


@pytest.fixture(scope="module")
def nl_meta():
    with open(os.path.join(GOLDEN_DIR, "nl_golden_meta.json")) as f:
        return json.load(f)


def block_case(name, nl_meta):
    """(input, state_dict, prefix) of a stored block case, rebuilt from synth and the stored gain."""
    from ted_spad_amd.i3res50 import NonLocalBlock
    b = nl_meta["blocks"][name]
    p = name + ".nl."
    tmpl = OrderedDict((p + k, v) for k, v in NonLocalBlock(*b["dims"]).state_dict().items())
    return synth_tensor(nl_meta["seed"], name + "/in", tuple(b["input"]), -1.0, 1.0), nl_ref.nl_state_dict(tmpl, nl_meta["seed"], {p: b["gain"]}), p


@pytest.mark.parametrize("name", ["nl_block512", "nl_block1024"])
def test_restatement_matches_the_reference_block(name, nl_golden, nl_meta):
    x, sd, p = block_case(name, nl_meta)
    y = nl_ref.block(x, sd, p)
    assert tuple(y.shape) == tuple(nl_golden[name + "_out"].shape)
    assert rel_l2(y, nl_golden[name + "_out"]) < 1e-4          # the feature tolerance of test_oracle_golden.py (the reference ran in fp32)
    std, pmax = nl_ref.logit_stats(x, sd, p)
    assert abs(std - nl_meta["blocks"][name]["logit_std"]) < 1e-3 and abs(pmax - nl_meta["blocks"][name]["mean_max_prob"]) < 1e-4


def test_pool_drops_the_odd_row_and_column():
    x = torch.arange(2 * 7 * 7, dtype=torch.float64).reshape(1, 1, 2, 7, 7)
    assert torch.equal(nl_ref.pool_hw2(x), torch.nn.functional.max_pool3d(x, (1, 2, 2), (1, 2, 2)))
    assert nl_ref.pool_hw2(x).shape == (1, 1, 2, 3, 3)


def test_state_dict_matches_the_reference_list(nl_meta):
    from ted_spad_amd.i3res50 import I3Res50, NonLocalBlock
    m = I3Res50(num_classes=102, use_nl=True)
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == nl_meta["state_dict"]
    placed = sorted(n[:-3] for n, mod in m.named_modules() if isinstance(mod, NonLocalBlock))
    assert placed == sorted(nl_meta["nl_blocks"]) == sorted(nl_ref.NL_BLOCKS)
    for li in (1, 2, 3, 4):
        for i, blk in enumerate(getattr(m, "layer%d" % li)):
            assert (blk.nl is not None) == ("layer%d.%d" % (li, i) in nl_ref.NL_BLOCKS)
    assert m.layer2[1].nl.dim_inner == 256 and m.layer3[1].nl.dim_inner == 512
    assert m.layer2[1].nl.theta.bias is not None and m.layer2[1].conv1.bias is None


def test_params_signature_covers_the_nl_parameters():
    from ted_spad_amd.i3res50 import I3Res50
    from ted_spad_amd.params import params_signature
    m = I3Res50(num_classes=4, use_nl=True)
    s0 = params_signature(m)
    with torch.no_grad():
        m.layer3[5].nl.phi.bias.add_(1.0)
    s1 = params_signature(m)
    assert s0 != s1
    m.layer2[3].nl.bn.running_var.mul_(2.0)
    assert params_signature(m) != s1


def test_default_keys_are_unchanged(nl_meta):
    from ted_spad_amd.i3res50 import I3Res50
    from ted_spad_amd.model_loaders import wrapper_i3d
    plain = [k for k, _ in nl_meta["state_dict"] if ".nl." not in k]
    assert list(I3Res50(num_classes=102).state_dict().keys()) == plain
    assert list(I3Res50(num_classes=102, use_nl=False).state_dict().keys()) == plain
    w = wrapper_i3d(num_classes=102)
    assert [k[4:] for k in w.state_dict() if k.startswith("i3d.")] == plain
    assert not any(".nl." in k for k in w.state_dict())


def test_factory_switch_builds_and_loads_nl_keys(tmp_path, nl_meta, capsys):
    from ted_spad_amd.model_loaders import load_ft_model
    ft = load_ft_model("largei3d", num_classes=102, use_nl=True)
    assert [k[4:] for k in ft.state_dict() if k.startswith("i3d.")] == [k for k, _ in nl_meta["state_dict"]]
    sd = nl_ref.nl_state_dict(ft.state_dict(), 0, nl_meta["gains"])
    path = str(tmp_path / "nl.pth")
    torch.save({"ft_model_state_dict": sd}, path)
    with pytest.raises(Exception):
        load_ft_model("largei3d", saved_model_file=path, num_classes=102)          # the default network has no place for the nl keys
    ft2 = load_ft_model("largei3d", saved_model_file=path, num_classes=102, use_nl=True)
    for k, v in ft2.state_dict().items():
        assert torch.equal(v, sd[k]), k
    with pytest.raises(NotImplementedError):
        load_ft_model("i3d", num_classes=102, use_nl=True)


def test_training_entry_points_refuse_a_nonlocal_network():
    from ted_spad_amd import autograd
    from ted_spad_amd.model_loaders import wrapper_i3d
    from ted_spad_amd.train_nets import I3DTrainer
    from ted_spad_amd.train_step import ActionTrainStep, AnonymizerTrainStep
    w = wrapper_i3d(num_classes=4, use_nl=True)
    x = torch.zeros(2, 3, 16, 32, 32)
    calls = {
        "train-mode forward": lambda: w.train()(x),
        "eval forward with an input gradient": lambda: w.eval()(x.clone().requires_grad_()),
        "wrapper_forward": lambda: autograd.wrapper_forward(w, x),
        "I3DTrainer": lambda: I3DTrainer(w),
        "freeze_bn": lambda: autograd.freeze_bn(w),
        "ActionTrainStep": lambda: ActionTrainStep(w),
        "AnonymizerTrainStep": lambda: AnonymizerTrainStep(None, w),
    }
    for name, fn in calls.items():
        with pytest.raises(NotImplementedError, match="backward is not built"):
            fn()
    assert not getattr(w, "frozen_bn", False) and "_hip_trainer" not in w.__dict__
    autograd.freeze_bn(wrapper_i3d(num_classes=4))                                  # the default network is still accepted


def test_symbol_is_declared_everywhere():
    from ted_spad_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "tedspad_hip.h")).read()
    assert re.search(r"int32_t\s+tedspad_nl_attention_fwd\s*\(", hdr) and "large_i3d.py:112-119" in hdr
    assert re.search(r"#define\s+TEDSPAD_ABI_VERSION\s+5\b", hdr) and _lib.ABI_VERSION == 5
    assert "tedspad_nl_attention_fwd" in _lib.SYMBOLS
    lib = _lib.lib()                                                               # resolves every declared symbol in the built library
    assert lib.tedspad_abi_version() == 5 and hasattr(lib, "tedspad_nl_attention_fwd")
    src = open(os.path.join(ROOT, "ted_spad_amd", "csrc", "nonlocal.hip")).read()
    assert "launch_lds<" in src                                                   # launched through the library's one launch path (csrc/launch.h)


def test_unsupported_width_is_the_librarys_error():
    """d outside {256, 512}: TEDSPAD_EINVAL with a message, before anything touches a device."""
    from ted_spad_amd import _lib
    lib = _lib.lib()
    rc = lib.tedspad_nl_attention_fwd(16, 128, 16, 128, 16, 128, 32, 128, 1, 4, 4, 128, 1.0, _lib.F16, None)
    assert rc != 0 and b"d = 128" in lib.tedspad_last_error()
    with pytest.raises(_lib.TedSpadHipError):
        _lib.check(rc, "tedspad_nl_attention_fwd")
