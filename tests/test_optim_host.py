"""CPU: the host side of ted_spad_amd.optim -- torch.optim's / GradScaler's state_dict layout, the refusal of CPU tensors, and that the inputs of the GPU kernel
test (tests/optim_ref.py) can see the mistakes its tolerance has to exclude."""
import pytest
import torch

import optim_ref as R
from ted_spad_amd._lib import TedSpadHipError
from ted_spad_amd.optim import DynamicLossScale, FusedOptimizer


def _cpu_params():
    return [torch.nn.Parameter(p) for p in R.make_params()]


@pytest.mark.parametrize("name", sorted(R.CONFIGS))
def test_fresh_state_dict_loads_into_the_torch_class(name):
    opt_type, kw = R.CONFIGS[name]
    params = _cpu_params()
    opt = FusedOptimizer(params, opt_type, lr=3e-3, exclude=[params[R.EXCLUDED]], **kw)
    sd = opt.state_dict()
    twin = R.torch_twin(opt_type, params, 1.0, **{k: 0.5 if k == "momentum" and v else v * 0 for k, v in kw.items()})     # other hyper-parameters: the load brings ours
    assert set(sd["param_groups"][0]) == set(twin.state_dict()["param_groups"][0]) and len(sd["param_groups"]) == 1
    assert sd["param_groups"][0]["params"] == list(range(len(params)))
    assert set(sd["state"]) == set(range(len(params))) - {R.EXCLUDED}, "no state entry for the excluded parameter"
    twin.load_state_dict(sd)
    g = twin.param_groups[0]
    assert g["lr"] == 3e-3 and g["weight_decay"] == kw.get("weight_decay", 0.0)
    if opt_type == "sgd":
        assert g["momentum"] == kw["momentum"] and g["dampening"] == 0 and g["nesterov"] is False
        bufs = [twin.state[p].get("momentum_buffer") for i, p in enumerate(params) if i != R.EXCLUDED]
        assert all((b is None) if kw["momentum"] == 0 else (b.shape == p.shape and not b.any()) for b, p in zip(bufs, [q for i, q in enumerate(params) if i != R.EXCLUDED]))
    else:
        assert g["betas"] == (0.9, 0.999) and g["eps"] == 1e-8 and not g["amsgrad"] and not g["maximize"]
        for i, p in enumerate(params):
            if i != R.EXCLUDED:
                st = twin.state[p]
                assert float(st["step"]) == 0 and st["exp_avg"].shape == p.shape == st["exp_avg_sq"].shape and not st["exp_avg"].any()
    assert params[R.EXCLUDED] not in twin.state
    # ... and the twin steps from it (an excluded parameter has no gradient there either)
    for i, p in enumerate(params):
        p.grad = None if i == R.EXCLUDED else torch.ones_like(p)
    before = params[R.EXCLUDED].detach().clone()
    twin.step()
    assert torch.equal(params[R.EXCLUDED].detach(), before)
    # the way back: a torch state loads, and comes out again as it went in
    opt.load_state_dict(twin.state_dict())
    back = opt.state_dict()
    assert set(back["state"]) == set(sd["state"])
    if opt_type != "sgd":
        assert float(back["state"][0]["step"]) == 1.0 and torch.equal(back["state"][2]["exp_avg"], twin.state[params[2]]["exp_avg"])
    elif kw["momentum"]:
        assert torch.equal(back["state"][2]["momentum_buffer"], twin.state[params[2]]["momentum_buffer"])


def test_dynamic_loss_scale_has_gradscalers_keys_and_defaults():
    ours, theirs = DynamicLossScale().state_dict(), torch.amp.GradScaler("cpu", enabled=True).state_dict()
    assert ours == {"scale": 65536.0, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 2000, "_growth_tracker": 0}
    assert set(ours) == set(theirs) and all(ours[k] == theirs[k] for k in ("growth_factor", "backoff_factor", "growth_interval"))
    s = DynamicLossScale()
    s.load_state_dict({"scale": 128.0, "growth_factor": 4.0, "backoff_factor": 0.25, "growth_interval": 7, "_growth_tracker": 5})
    assert s.state_dict() == {"scale": 128.0, "growth_factor": 4.0, "backoff_factor": 0.25, "growth_interval": 7, "_growth_tracker": 5}
    assert DynamicLossScale.static(256.0).get_scale() == 256.0 and not DynamicLossScale.static(256.0).dynamic


def test_cpu_tensors_are_refused():
    params = _cpu_params()
    opt = FusedOptimizer(params, "adam", lr=1e-3)
    opt.zero_grad()
    with pytest.raises(TedSpadHipError):
        opt.step()
    with pytest.raises(TedSpadHipError):
        DynamicLossScale().device_state("cpu")
    with pytest.raises(NotImplementedError):
        FusedOptimizer(params, "rmsprop")


def _five_steps():
    return [R.make_grads(t) for t in range(len(R.LRS))]


@pytest.mark.parametrize("name", sorted(R.CONFIGS))
def test_the_restated_update_is_torchs(name):
    """float64 against float64: the arithmetic csrc/optim.hip implements (restated in optim_ref.restated) is that of the torch.optim class, to rounding."""
    opt_type, kw = R.CONFIGS[name]
    p0, grads = R.make_params(), _five_steps()
    p64 = R.twin_params(p0)
    twin = R.torch_twin(opt_type, p64, R.LRS[0], **kw)
    for g, lr in zip(grads, R.LRS):
        R.twin_step(twin, p64, g, 1.0, lr)
    ps, ms, vs = R.restated(opt_type, p0, grads, R.LRS, **kw)
    for i in range(len(p0)):
        assert R.rel_l2(ps[i], p64[i]) < 1e-13, (i, R.rel_l2(ps[i], p64[i]))
        m, v = R.twin_state(twin, p64[i], opt_type)
        if i != R.EXCLUDED and m is not None:
            assert R.rel_l2(ms[i], m) < 1e-13
        if i != R.EXCLUDED and v is not None:
            assert R.rel_l2(vs[i], v) < 1e-13


@pytest.mark.parametrize("name,mistake", [("adam", "eps_inside"), ("adam", "no_bias_correction"), ("adam_wd", "swap_decay"), ("adamw", "swap_decay"),
                                          ("adamw", "eps_inside"), ("adamw", "no_bias_correction")])
def test_the_inputs_show_each_mistake_above_the_tolerance(name, mistake):
    """The GPU test holds the parameters to 1e-5 rel-L2 per tensor at most. At its inputs a misplaced eps, a missing bias correction and coupled-for-decoupled
    weight decay each move the float64 result by far more than that, in every tensor of 100 elements or more (the smaller ones may hold no element with a
    gradient of eps's size)."""
    opt_type, kw = R.CONFIGS[name]
    p0, grads = R.make_params(), _five_steps()
    good, _, _ = R.restated(opt_type, p0, grads, R.LRS, **kw)
    bad, _, _ = R.restated(opt_type, p0, grads, R.LRS, mistake=mistake, **kw)
    for i, n in enumerate(R.SIZES):
        if n >= 100 and i != R.EXCLUDED:
            assert R.rel_l2(bad[i], good[i]) > 1e-4, (i, n, R.rel_l2(bad[i], good[i]))


def test_action_checkpoint_with_a_scaler_holds_what_the_reference_resumes_from(tmp_path):
    """'amp_scaler' = GradScaler.state_dict()'s keys, 'optimizer' = torch's layout: the file loads with weights_only=True and into torch's own classes. Without the
    keyword the states are what they were."""
    from ted_spad_amd.checkpoint import save_action_checkpoint
    ft = torch.nn.Linear(5, 3)
    opt = FusedOptimizer(list(ft.parameters()), "adamw", lr=1e-4, weight_decay=1e-4)
    scaler = DynamicLossScale(init_scale=1024.0)
    path = str(tmp_path / "model_temp.pth")
    save_action_checkpoint(path, 7, ft, opt, None, scaler=scaler)
    got = torch.load(path, weights_only=True)
    assert got["epoch"] == 8 and got["amp_scaler"] == scaler.state_dict() and got["amp_scaler"]["scale"] == 1024.0
    theirs = torch.amp.GradScaler("cpu", enabled=True)
    theirs.load_state_dict(got["amp_scaler"])
    assert theirs.state_dict()["growth_interval"] == 2000 and theirs.state_dict()["growth_factor"] == 2.0
    torch.optim.AdamW(ft.parameters()).load_state_dict(got["optimizer"])
    old = save_action_checkpoint(path, 7, ft, torch.optim.Adam(ft.parameters()), 256.0)
    assert old["amp_scaler"] == {"scale": 256.0} and list(old) == ["epoch", "amp_scaler", "ft_model_state_dict", "optimizer"]
