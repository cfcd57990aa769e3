"""-m gpu: ActionTrainStep -- `train_epoch` of action_training/train_action.py (clips straight into ft) and train_anonymized_action.py (a frozen fa in front) with the
optimizer and the loss scale on the HIP path (optim.FusedOptimizer, optim.DynamicLossScale). Shapes and synthetic weights are those of
tests/test_hip_train_step.py::test_action_training_step_frozen_bn_vs_oracle; `_models` and `_report` are copies of that file's helpers."""
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import rel_l2
from ted_spad_amd.synth import synth_state_dict, synth_tensor, synth_train_video
from optim_ref import BOUND_P

pytestmark = pytest.mark.gpu

LABELS = [5, 77, 101, 1]


def _models(beta=None):
    from ted_spad_amd.model_loaders import load_fa_model, load_ft_model
    fa, ft = load_fa_model(arch="unet"), load_ft_model("largei3d", num_classes=102)
    sd_u, sd_l = synth_state_dict(fa.state_dict(), 0), synth_state_dict(ft.state_dict(), 0)
    if beta is not None:
        for sd in (sd_u, sd_l):
            for k in sd:
                if k.rsplit(".", 1)[0] + ".running_mean" in sd and k.endswith(".bias"):
                    sd[k] = torch.full_like(sd[k], beta)
    fa.load_state_dict(sd_u); ft.load_state_dict(sd_l)
    ft.i3d.drop_p = 0.0       # Q13: dropout is stochastic; parity runs with p = 0
    return fa.cuda(), ft.cuda(), sd_u, sd_l


def _report(name, got, ref, min_cos=0.93, med_cos=0.97, tiny=1e-4, abs_tol=5e-3):
    errs, cos = {}, {}
    for k in ref:
        g, r = got[k].detach().cpu().double().flatten(), ref[k].double().flatten()
        if float(r.norm()) > tiny:
            errs[k] = rel_l2(g, r)
            cos[k] = float(g @ r / (g.norm() * r.norm()))
        else:
            assert float((g - r).norm()) <= abs_tol, (k, float((g - r).norm()), float(r.norm()))
    if os.environ.get("TEDSPAD_VERBOSE"):
        for k in errs:
            print("   %-50s rel %.3e cos %.5f |g| %.3e" % (k, errs[k], cos[k], float(ref[k].norm())))
    worst = sorted(errs.items(), key=lambda kv: -kv[1])[:3]
    print(name, "median rel-L2 %.3e, min cosine %.4f, worst %s" % (float(np.median(list(errs.values()))), min(cos.values()), worst))
    assert min(cos.values()) > min_cos and float(np.median(list(cos.values()))) > med_cos
    return errs


def _params(**kw):
    from ted_spad_amd.train_step import DEFAULT_ACTION_PARAMS
    return SimpleNamespace(**{**vars(DEFAULT_ACTION_PARAMS), **kw})


def _frozen_names(ft):
    return [k for k, _ in ft.named_parameters() if k.startswith("i3d.") and (".bn" in k or k.startswith("i3d.bn") or ".downsample.1." in k)]


@functools.lru_cache(maxsize=None)
def _video48():
    return synth_train_video(0, "train_video64", (4, 48, 3, 64, 64))


@functools.lru_cache(maxsize=None)
def _video16():
    return _video48()[:, :16].contiguous()


@functools.lru_cache(maxsize=None)
def _trip_reference():
    """computed once, never written to: the oracle's three-clip action step at the synthetic weights"""
    from oracle import train_step_ref
    _, _, sd_u, sd_l = _cpu_sds()
    return train_step_ref.action_step(_video48(), torch.tensor(LABELS), sd_u, sd_l)


@functools.lru_cache(maxsize=None)
def _cpu_sds():
    from ted_spad_amd.model_loaders import load_fa_model, load_ft_model
    fa, ft = load_fa_model(arch="unet"), load_ft_model("largei3d", num_classes=102)
    return None, None, synth_state_dict(fa.state_dict(), 0), synth_state_dict(ft.state_dict(), 0)


def test_raw_single_clip_adamw_step_vs_oracle_and_the_excluded_parameters():
    """train_action.py's default: no anonymizer, one clip per sample, plain cross-entropy. Loss and gradients against the fp32 oracle; with AdamW at lr 1e-2 and
    weight decay 0.1 a parameter without a gradient must not move at all (the reference's optimizer skips `.grad is None`: a zero-gradient slot that is decayed
    anyway fails here), the others must."""
    from oracle import i3res50_ref, losses_ref, train_step_ref
    from ted_spad_amd.train_step import ActionTrainStep
    _, ft, _, sd_l = _models()
    video, labels = _video16(), torch.tensor(LABELS)
    ref_sd = train_step_ref._grad_sd(sd_l)
    ref_loss = losses_ref.cross_entropy_torch(i3res50_ref.wrapper_forward(video.permute(0, 2, 1, 3, 4), ref_sd, train=True, frozen_bn=True)[0], labels)
    ref_loss.backward()
    ref_loss = float(ref_loss.detach())
    frozen = _frozen_names(ft)
    ref_g = {k: p.grad for k, p in ref_sd.items() if torch.is_tensor(p) and p.requires_grad and p.grad is not None and k not in frozen}
    assert ref_g and not any(k.startswith("mlp.") for k in ref_g), "feat1 never reaches the loss: the oracle has no mlp gradient either"
    step = ActionTrainStep(ft, None, params=_params(opt_type="adamw", learning_rate=1e-2, weight_decay=0.1), loss_scale=256.0)
    before = {k: v.detach().clone() for k, v in ft.state_dict().items()}
    out = step.step(video.cuda(), labels.cuda())
    assert out["phase"] == "action" and out["loss_temporal"] is None and not out["skipped"]
    print("raw one-clip loss %.6f, oracle %.6f" % (out["loss"], ref_loss))
    assert abs(out["loss"] - ref_loss) < 5e-3 * abs(ref_loss) and out["loss_ce"] == out["loss"]
    assert out["pred"].shape == (4,) and out["pred"].dtype == torch.int64 and out["pred"].is_cuda and float(out["grad_scale"]) == 256.0
    got = {k: p.grad / out["grad_scale"] for k, p in ft.named_parameters() if p.grad is not None}      # .grad still carries the scale
    assert frozen and all(k not in got for k in frozen) and not any(k.startswith("mlp.") for k in got)
    assert set(ref_g) == set(got), sorted(set(ref_g) ^ set(got))[:5]
    errs = _report("raw action step ft grads", got, ref_g, min_cos=0.9, med_cos=0.97)
    assert float(np.median(list(errs.values()))) < 0.25
    after = ft.state_dict()
    names = dict(ft.named_parameters())
    still = [k for k in names if k.startswith("mlp.") or k in frozen]
    assert all(torch.equal(after[k], before[k]) for k in still), [k for k in still if not torch.equal(after[k], before[k])][:5]
    moved = [k for k in names if k not in still]
    assert "i3d.fc.weight" in moved and "i3d.fc.bias" in moved and all(not torch.equal(after[k], before[k]) for k in moved)
    assert all(torch.equal(after[k], before[k]) for k in after if k.startswith("i3d.") and ("running_" in k or "num_batches" in k))
    assert int(after["mlp.bn1.num_batches_tracked"]) == 1 and not torch.equal(after["mlp.bn1.running_mean"], before["mlp.bn1.running_mean"])
    assert set(step.opt.state_dict()["state"]) == {i for i, (k, _) in enumerate(ft.named_parameters()) if k in moved}


def test_anonymised_triplet_adam_step_is_torchs_update_on_every_tensor(deterministic):
    """train_anonymized_action.py with `temporal_loss='trip'`, Adam, static scale 256: losses as the existing step_action test holds them; then the update itself --
    the float64 torch.optim.Adam step computed on the CPU from the parameters before the step and the gradients in `.grad` divided by `grad_scale` equals the
    parameters after it, under the kernel test's bound, for all 168 tensors (pointers, exclusion and lr wiring on the real network)."""
    from ted_spad_amd.train_step import ActionTrainStep
    fa, ft, _, _ = _models()
    ref_l, _ = _trip_reference()
    lr = 3e-3
    step = ActionTrainStep(ft, fa, params=_params(temporal_loss="trip"), loss_scale=256.0)
    fa_before = {k: v.detach().clone() for k, v in fa.state_dict().items()}
    before = {k: p.detach().double().cpu().clone() for k, p in ft.named_parameters()}
    out = step.step(_video48().cuda(), torch.tensor(LABELS).cuda(), lr=lr)
    assert not out["skipped"] and float(out["grad_scale"]) == 256.0
    assert abs(out["loss"] - ref_l["loss"]) < 5e-3 * abs(ref_l["loss"])
    assert abs(out["loss_temporal"] - ref_l["loss_temporal"]) < 2e-2 * abs(ref_l["loss_temporal"])
    names = [k for k, _ in ft.named_parameters()]
    assert len(names) == 168
    twin_p = {k: torch.nn.Parameter(before[k].clone()) for k in names}
    for k, p in ft.named_parameters():
        twin_p[k].grad = None if p.grad is None else p.grad.detach().double().cpu() / 256.0
    frozen = _frozen_names(ft)
    assert all((twin_p[k].grad is None) == (k in frozen) for k in names)
    torch.optim.Adam(list(twin_p.values()), lr=lr).step()
    worst = max((rel_l2(p.detach().cpu().double(), twin_p[k].detach()), k) for k, p in ft.named_parameters())
    print("action step: worst rel-L2 of the updated parameters against float64 torch.optim.Adam: %.3e (%s)" % worst)
    assert worst[0] < BOUND_P
    assert all(torch.equal(p.detach().double().cpu(), before[k]) for k, p in ft.named_parameters() if k in frozen)
    assert all(not torch.equal(p.detach().double().cpu(), before[k]) for k, p in ft.named_parameters() if p.grad is not None and bool(p.grad.any()))
    assert all(k in frozen or bool(p.grad.any()) for k, p in ft.named_parameters() if "conv" in k or k.startswith(("i3d.fc", "mlp.fc")))
    assert all(torch.equal(v, fa_before[k]) for k, v in fa.state_dict().items()), "fa is not trained here"


def test_an_overflowing_scale_skips_the_step():
    from ted_spad_amd.train_step import ActionTrainStep
    _, ft, _, _ = _models()
    step = ActionTrainStep(ft, None, params=_params(), loss_scale=2.0 ** 60)
    before = {k: p.detach().clone() for k, p in ft.named_parameters()}
    out = step.step(_video16().cuda(), torch.tensor(LABELS).cuda())
    assert bool(out["skipped"]) is True and out["skipped"] == True
    assert all(torch.equal(p.detach(), before[k]) for k, p in ft.named_parameters()), "a skipped step must leave the parameters alone"
    assert step.opt.steps_applied() == 0 and step.scaler.get_scale() == 2.0 ** 60, "a static scale does not back off"


def test_the_dynamic_scale_backs_off_until_a_step_is_applied():
    """GradScaler() starts at 65536; a static 256 is known to work at these weights, so at most eight halvings are needed. Every scale is a power of two and
    halves exactly after a skipped step."""
    from ted_spad_amd.train_step import ActionTrainStep
    _, ft, _, _ = _models()
    step = ActionTrainStep(ft, None, params=_params())            # loss_scale="dynamic"
    assert step.scaler.state_dict() == {"scale": 65536.0, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 2000, "_growth_tracker": 0}
    video, labels = _video16().cuda(), torch.tensor(LABELS).cuda()
    scales, skipped = [], []
    for _ in range(12):
        out = step.step(video, labels)
        scales.append(float(out["grad_scale"]))
        skipped.append(bool(out["skipped"]))
        if not skipped[-1]:
            break
    scales.append(step.scaler.get_scale())
    print("dynamic scale:", scales, skipped)
    assert scales[0] == 65536.0 and all(s > 0 and np.log2(s) == int(np.log2(s)) for s in scales)
    assert all(scales[t + 1] == (scales[t] / 2 if skipped[t] else scales[t]) for t in range(len(skipped)))
    assert not all(skipped) and sum(skipped) <= 8 and step.opt.steps_applied() == skipped.count(False)


def test_eval_after_a_step_sees_the_new_weights():
    """tests/test_hip_train_step.py::test_eval_forward_after_a_fused_optimizer_step_sees_the_new_weights through the new driver: the update kernel writes the
    parameters through raw pointers, the eval-mode weight images must still notice (TE.mark_updated)."""
    from ted_spad_amd.model_loaders import load_ft_model
    from ted_spad_amd.train_step import ActionTrainStep
    _, ft, _, _ = _models()
    clips = synth_tensor(3, "evalclips", (2, 3, 16, 64, 64), 0, 1).cuda()
    ft.eval()
    before = ft.i3d.extract_features(clips).clone()
    step = ActionTrainStep(ft, None, params=_params(learning_rate=1e-3), loss_scale=256.0)
    out = step.step(_video16().cuda(), torch.tensor(LABELS).cuda())
    assert not out["skipped"]
    ft.eval()
    after = ft.i3d.extract_features(clips)
    fresh = load_ft_model("largei3d", num_classes=102)
    fresh.load_state_dict({k: v.detach().cpu().clone() for k, v in ft.state_dict().items()}, strict=True)
    want = fresh.cuda().eval().i3d.extract_features(clips)
    assert rel_l2(after.cpu(), want.cpu()) < 1e-6, "stale weight images after the optimizer kernel's step"
    assert rel_l2(after.cpu(), before.cpu()) > 1e-4, "the step did not move the feature: the test would not see a stale image"


def test_sgd_runs_a_step_and_con_is_refused():
    from ted_spad_amd.train_step import ActionTrainStep
    _, ft, _, _ = _models()
    with pytest.raises(NotImplementedError):
        ActionTrainStep(ft, None, params=_params(loss="con"))
    with pytest.raises(NotImplementedError):
        ActionTrainStep(ft, None, params=_params(arch="r3d"))
    with pytest.raises(NotImplementedError):
        ActionTrainStep(ft, None, params=_params(opt_type="rmsprop"))
    step = ActionTrainStep(ft, None, params=_params(opt_type="sgd", learning_rate=1e-3), loss_scale=256.0)
    before = ft.i3d.fc.weight.detach().clone()
    out = step.step(_video16().cuda(), torch.tensor(LABELS).cuda())
    assert not out["skipped"] and not torch.equal(ft.i3d.fc.weight.detach(), before)
    sd = step.opt.state_dict()
    assert sd["param_groups"][0]["momentum"] == 0.9 and sd["param_groups"][0]["weight_decay"] == 1e-4 and "momentum_buffer" in sd["state"][0]
