"""CPU: the host side of the resume tests (tests/test_hip_resume.py) -- the condition under which bit equality of a resumed Adam trajectory is a fair demand,
the load paths of optim.FusedOptimizer / optim.DynamicLossScale that run before any device state exists, the checkpoint writers' corners those tests lean
on, and the comparison code itself (a planted difference is reported by name)."""
import numpy as np
import pytest
import torch

import optim_ref as R
import resume_helpers as H
from ted_spad_amd.optim import DynamicLossScale, FusedOptimizer


def test_bias_correction_words_do_not_depend_on_how_the_powers_were_formed():
    """A running FusedOptimizer forms beta^(t+1) by repeated double multiplication (optim_finish_kernel), a loaded one as `beta ** (t + 1)`
    (FusedOptimizer._write_state). For betas (0.9, 0.999) the doubles differ from t = 3 on -- which is why words 4..7 of the device state are left out of the
    resume comparison -- and the two fp32 words the update kernel reads (1 - beta1^(t+1), sqrt(1 - beta2^(t+1))) are the same bits for every t in 0..64: a run
    resumed at any of these steps continues with the corrections of the run that never stopped."""
    differ = []
    for t in range(65):
        (l1, l2), lw = H.bias_words_loaded(t)
        (r1, r2), rw = H.bias_words_running(t)
        assert lw == rw, (t, lw, rw)
        if (l1, l2) != (r1, r2):
            differ.append(t)
        assert abs(l1 - r1) <= 64 * np.spacing(l1) and abs(l2 - r2) <= 64 * np.spacing(l2), t     # (last bits only)
    assert differ[0] == 3 and len(differ) > 48, differ               # (a few later t round to the same double again)


def _loaded_state(opt_type, params, kw):
    """A torch.optim state after two real steps on the CPU: non-trivial moments, step = 2, a learning rate of its own."""
    twin = R.torch_twin(opt_type, params, 7e-4, **kw)
    for t in range(2):
        for i, (p, g) in enumerate(zip(params, R.make_grads(t))):
            p.grad = None if i == R.EXCLUDED else g.clone()
        twin.step()
    return twin.state_dict()


def _same_optimizer_state(a, b):
    assert a["param_groups"] == b["param_groups"]
    assert set(a["state"]) == set(b["state"])
    for i in a["state"]:
        assert set(a["state"][i]) == set(b["state"][i]), i
        for k, v in a["state"][i].items():
            w = b["state"][i][k]
            assert (v is None and w is None) or (v.dtype == w.dtype and torch.equal(v, w)), (i, k)


@pytest.mark.parametrize("name", sorted(R.CONFIGS))
def test_fused_optimizer_load_before_any_step_is_idempotent(name):
    """state_dict() -> load_state_dict -> state_dict() on CPU parameters, where the state flats do not exist yet (the `_pending` path a restart takes before the
    model moves to the device): a fresh optimizer's own state, then a torch state with two steps in it. Same `step`, same tensors, same `param_groups`; loading
    the result again changes nothing."""
    opt_type, kw = R.CONFIGS[name]
    params = [torch.nn.Parameter(p) for p in R.make_params()]
    opt = FusedOptimizer(params, opt_type, lr=3e-3, exclude=[params[R.EXCLUDED]], **kw)
    sd0 = opt.state_dict()
    opt.load_state_dict(sd0)
    assert opt._state is None and opt.steps_applied() == 0
    _same_optimizer_state(opt.state_dict(), sd0)
    theirs = _loaded_state(opt_type, params, kw)
    opt.load_state_dict(theirs)
    sd1 = opt.state_dict()
    assert sd1["param_groups"][0]["lr"] == 7e-4 and opt.steps_applied() == (0 if opt_type == "sgd" else 2)
    for i, st in theirs["state"].items():
        for k, v in st.items():
            if torch.is_tensor(v):
                assert torch.equal(sd1["state"][i][k], v.float()), (i, k)                  # 'step' included
    opt.load_state_dict(sd1)
    _same_optimizer_state(opt.state_dict(), sd1)
    opt.load_state_dict(opt.state_dict())
    _same_optimizer_state(opt.state_dict(), sd1)


def test_dynamic_loss_scale_round_trip_without_a_device_state():
    a = DynamicLossScale(init_scale=4096.0, growth_factor=4.0, backoff_factor=0.25, growth_interval=3)
    sd = {"scale": 512.0, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 3, "_growth_tracker": 2}
    a.load_state_dict(sd)
    assert a._dev is None and a.state_dict() == sd and a.get_scale() == 512.0
    b = DynamicLossScale()
    b.load_state_dict(a.state_dict())
    assert b.state_dict() == sd
    b.load_state_dict(b.state_dict())
    assert b.state_dict() == sd and b._dev is None


def test_a_schedules_numpy_learning_rate_is_stored_as_a_float(tmp_path):
    """ReconstructionSchedule's warm-up rates are numpy doubles; through `set_lr` they reach `optimizer.state_dict()`, and a numpy scalar there makes a file that
    `torch.load` (weights only: what model_loaders.load_fa_model uses) refuses. `set_lr` stores a Python float; the checkpoint reads back."""
    from ted_spad_amd.checkpoint import save_reconstruction_checkpoint
    from ted_spad_amd.pretrain import ReconstructionSchedule
    from ted_spad_amd.train_step import StepDriver
    lin = torch.nn.Linear(3, 2)
    drv = StepDriver(env=False)
    drv.opt = torch.optim.Adam(lin.parameters(), lr=1e-3)
    sched = ReconstructionSchedule()
    lr = sched.lr_for_epoch(2)
    assert isinstance(lr, np.floating)
    drv.set_lr(lr)
    assert all(type(g["lr"]) is float and g["lr"] == float(lr) for g in drv.opt.param_groups)
    path = str(tmp_path / "model_temp.pth")
    save_reconstruction_checkpoint(path, 2, sched.lr_counter, lin, drv.opt)
    got = torch.load(path, weights_only=True)
    assert got["optimizer"]["param_groups"][0]["lr"] == float(lr) and got["lr_counter"] == 0 and got["epoch"] == 3


def test_anonymizer_checkpoint_without_a_privacy_branch(tmp_path):
    """AnonymizerTrainStep(fb_model=None) has no fb and no opt_fb: the writer leaves those keys out and writes the rest as it always did."""
    from ted_spad_amd.checkpoint import save_anonymizer_checkpoint
    fa, fb, ft = torch.nn.Linear(3, 2), torch.nn.Linear(2, 2), torch.nn.Linear(2, 4)
    opts = [torch.optim.Adam(m.parameters()) for m in (fa, fb, ft)]
    path = str(tmp_path / "model.pth")
    full = save_anonymizer_checkpoint(path, 4, fa, fb, ft, optimizers=tuple(opts))
    assert list(full) == ["epoch", "fa_model_state_dict", "fb_model_state_dict", "ft_model_state_dict", "optimizer_fa", "optimizer_fb", "optimizer_ft"]
    save_anonymizer_checkpoint(path, 4, fa, None, ft, optimizers=(opts[0], None, opts[2]))
    got = torch.load(path, weights_only=True)
    assert list(got) == ["epoch", "fa_model_state_dict", "ft_model_state_dict", "optimizer_fa", "optimizer_ft"] and got["epoch"] == 5
    assert torch.equal(got["ft_model_state_dict"]["weight"], ft.weight.detach())


# ---- the helpers' own code ----------------------------------------------------------------------------------------------------------------
def _tiny_run(seed=0):
    """A BatchNorm net, one Adam step on the CPU: parameters, running statistics, num_batches_tracked, exp_avg / exp_avg_sq / step."""
    torch.manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.BatchNorm1d(3))
    opt = torch.optim.Adam(net.parameters(), lr=1e-2)
    net(torch.arange(24.0).view(6, 4) / 24).square().sum().backward()
    opt.step()
    return net, opt


def test_snapshot_names_everything_and_equal_runs_compare_equal():
    net, opt = _tiny_run()
    snap = H.snapshot({"net": net}, {"opt": (opt, net)})
    assert {"net/param/0.weight", "net/param/1.bias", "net/buffer/1.running_mean", "net/buffer/1.running_var", "net/buffer/1.num_batches_tracked",
            "opt/lr", "opt/state/0.weight/exp_avg", "opt/state/1.weight/exp_avg_sq", "opt/state/0.bias/step"} <= set(snap)
    assert len(snap) == 4 + 3 + 1 + 3 * 4
    assert snap["opt/lr"] == 1e-2 and int(snap["net/buffer/1.num_batches_tracked"]) == 1 and float(snap["opt/state/0.bias/step"]) == 1.0
    net2, opt2 = _tiny_run()
    assert H.differences(H.snapshot({"net": net2}, {"opt": (opt2, net2)}), snap) == []
    H.assert_same(H.snapshot({"net": net2}, {"opt": (opt2, net2)}), snap, "two equal runs")
    with torch.no_grad():                                             # a snapshot is a copy: the run going on does not change it
        net[0].weight.add_(1.0)
    assert torch.equal(snap["net/param/0.weight"], net2[0].weight.detach())


def test_a_planted_difference_in_a_buffer_is_reported_by_name():
    net, opt = _tiny_run()
    want = H.snapshot({"net": net}, {"opt": (opt, net)})
    with torch.no_grad():
        net[1].running_var[2] += 2.0 ** -20                           # one element, a few last bits
    got = H.snapshot({"net": net}, {"opt": (opt, net)})
    msgs = H.differences(got, want)
    assert len(msgs) == 1 and msgs[0].startswith("net/buffer/1.running_var: 1 of 3 differ; first at (2,)"), msgs
    with pytest.raises(AssertionError, match=r"1 of 20 items differ\n  net/buffer/1\.running_var"):
        H.assert_same(got, want, "planted")
    H.assert_differs(got, want, "planted", "/buffer/")
    with pytest.raises(AssertionError, match="does not exercise"):
        H.assert_differs(got, want, "planted", "/param/")
    with torch.no_grad():
        net[1].num_batches_tracked += 1
    msgs = H.differences(H.snapshot({"net": net}, {"opt": (opt, net)}), want)
    assert [m.split(":")[0] for m in msgs] == ["net/buffer/1.running_var", "net/buffer/1.num_batches_tracked"], msgs


def test_a_planted_difference_in_an_optimizer_step_is_reported_by_name():
    net, opt = _tiny_run()
    want = H.snapshot({"net": net}, {"opt": (opt, net)})
    opt.state[net[1].weight]["step"] += 1
    msgs = H.differences(H.snapshot({"net": net}, {"opt": (opt, net)}), want)
    assert len(msgs) == 1 and msgs[0].startswith("opt/state/1.weight/step: 1 of 1 differ"), msgs
    # the same through FusedOptimizer's layout on CPU parameters (pending state): the step count restarted at 0
    params = [torch.nn.Parameter(p) for p in R.make_params()]
    holder = torch.nn.ParameterList(params)
    fused = FusedOptimizer(params, "adam", lr=1e-3, exclude=[params[R.EXCLUDED]])
    fused.load_state_dict(_loaded_state("adam", params, {}))
    want = H.snapshot({}, {"opt": (fused, holder)})
    assert want["opt/steps_applied"] == 2 and want["opt/words[0:4]"] is None and "opt/state/%d/exp_avg" % R.EXCLUDED not in want
    fused._steps0 = 0
    msgs = H.differences(H.snapshot({}, {"opt": (fused, holder)}), want)
    names = [m.split(":")[0] for m in msgs]
    assert "opt/steps_applied" in names and "opt/state/0/step" in names and all(n.endswith("/step") or n == "opt/steps_applied" for n in names), msgs


def test_losses_and_missing_entries_are_reported():
    a = H.losses([H.step_record({"loss": 1.5, "skipped": False, "pred": torch.tensor([1, 2]), "grad_scale": torch.tensor(256.0), "none": None})], first=2)
    assert a == {"loss/step2/loss": 1.5, "loss/step2/skipped": False, "loss/step2/pred": (1, 2), "loss/step2/grad_scale": 256.0, "loss/step2/none": None}
    b = dict(a, **{"loss/step2/loss": 1.5000001})
    del b["loss/step2/none"]
    b["extra"] = 0
    assert H.differences(b, a) == ["loss/step2/loss: got 1.5000001, want 1.5", "loss/step2/none: only in the reference run", "extra: only in this run"]
    assert H.differences({"x": torch.zeros(2)}, {"x": torch.zeros(3)})[0].startswith("x: got torch.float32 (2,), want torch.float32 (3,)")
    assert H.differences({"x": torch.tensor([float("nan")])}, {"x": torch.tensor([float("nan")])}) == ["x: not torch.equal"]
