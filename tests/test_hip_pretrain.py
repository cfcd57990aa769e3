"""-m gpu: the reconstruction pre-training step (ted_spad_amd/pretrain.py; fa_pretraining/train_reconstruction.py) on MI355X against the path that
existed before it (fp32 ends, torch's sign on the device) and against the fp32 CPU oracle (oracle/unetpp_ref.py + torch.nn.L1Loss + torch.optim.Adam).
6 x 3 x 64 x 64 and the smooth weights of test_unetpp_backward_chain_tight_on_a_smooth_network unless a test says otherwise."""
import numpy as np
import pytest
import torch

from conftest import rel_l2
from test_hip_train_step import _grad_sd, _smooth
from ted_spad_amd.synth import synth_state_dict, synth_tensor

pytestmark = pytest.mark.gpu
SHAPE = (6, 3, 64, 64)
NUMEL = 6 * 3 * 64 * 64


def _fa(beta=4.0):
    from ted_spad_amd.model_loaders import load_fa_model
    fa = load_fa_model()
    sd = synth_state_dict(fa.state_dict(), 0)
    if beta is not None:
        sd = _smooth(sd, beta)
    fa.load_state_dict(sd)
    return fa.cuda(), sd


def _x():
    return synth_tensor(0, "recon", SHAPE)          # in [0, 1): images


def _fused_backward(fa, x, scale):
    """forward(nchw=False) -> kernel -> backward(dl=) -> flush. Returns (loss 0-d, yy fp32 NCHW)."""
    from ted_spad_amd.losses import l1_train
    from ted_spad_amd.train_nets import UNetPPTrainer
    from ted_spad_amd.train_step import StepDriver
    StepDriver()._begin(x.device)
    tr = UNetPPTrainer(fa.train())
    y, tape = tr.forward(x, nchw=False)
    assert y.dims == (SHAPE[0], 1, SHAPE[2], SHAPE[3]) and y.c == 8
    loss, dl, yy = l1_train(y, x, scale, want_y32=True)
    tr.backward(tape, dl=dl)
    tr.flush_grads()
    return loss, yy


@pytest.fixture(scope="module")
def oracle():
    """The fp32 oracle's train-mode forward on the shared batch, its graph kept for one backward pass."""
    from oracle import unetpp_ref
    _, sd = _fa()
    sdg = _grad_sd(sd)
    x = _x()
    y = unetpp_ref.forward(x, sdg, train=True)
    return dict(x=x, y=y, sdg=sdg, loss=float((y.detach() - x).abs().mean()))


@pytest.fixture(scope="module")
def device_run():
    """One fused forward / loss / backward with the automatic scale: loss, output and the UNSCALED parameter gradients."""
    from ted_spad_amd.pretrain import auto_loss_scale
    fa, _ = _fa()
    scale = auto_loss_scale(NUMEL, "f16")
    loss, yy = _fused_backward(fa, _x().cuda(), scale)
    grads = {k: (None if p.grad is None else (p.grad / scale).cpu()) for k, p in fa.named_parameters()}
    return dict(loss=float(loss), yy=yy.cpu(), grads=grads, scale=scale)


def test_fused_path_is_bit_equal_to_the_fp32_ended_path(deterministic):
    """The main correctness statement, no tolerance: forward(nchw=False) -> tedspad_l1_loss_grad_cl -> backward(dl=) gives every parameter the bits of
    forward(x) -> sign(yy - x) * g in fp32 on the device -> backward(tape, dy) (deterministic mode, same weights)."""
    from ted_spad_amd.train_nets import UNetPPTrainer
    from ted_spad_amd.train_step import StepDriver
    x = _x().cuda()
    scale = 256.0
    fa_a, _ = _fa()
    loss, yy_a = _fused_backward(fa_a, x, scale)
    fa_b, _ = _fa()
    StepDriver()._begin(x.device)
    tr = UNetPPTrainer(fa_b.train())
    yy, tape = tr.forward(x)
    assert torch.equal(yy, yy_a)
    g32 = torch.tensor(np.float32(scale) / np.float32(NUMEL), device="cuda")
    tr.backward(tape, torch.sign(yy - x) * g32)
    tr.flush_grads()
    ga, gb = dict(fa_a.named_parameters()), dict(fa_b.named_parameters())
    none = [k for k, p in ga.items() if p.grad is None]
    assert none and all(k.startswith("encoder.layer4.") for k in none) and none == [k for k, p in gb.items() if p.grad is None]
    assert len(none) == len([k for k in ga if k.startswith("encoder.layer4.")])
    diff = [k for k, p in ga.items() if p.grad is not None and not torch.equal(p.grad, gb[k].grad)]
    assert not diff, diff
    assert all(bool((p.grad != 0).any()) for p in ga.values() if p.grad is not None)
    with pytest.raises(ValueError):
        tr.backward(tape)                                             # neither dy nor dl


def test_loss_vs_the_oracle(oracle, device_run):
    yy, y_ref, x = device_run["yy"], oracle["y"].detach(), oracle["x"]
    e = rel_l2(yy, y_ref)
    slack = float((yy.double() - y_ref.double()).abs().mean())        # triangle inequality: | mean|yy - x| - mean|y_ref - x| | <= mean|yy - y_ref|
    print("loss %.7f oracle %.7f (|diff| %.3e <= %.3e), output rel-L2 %.3e" % (device_run["loss"], oracle["loss"], abs(device_run["loss"] - oracle["loss"]), slack, e))
    assert e < 3e-3
    assert abs(device_run["loss"] - oracle["loss"]) <= slack + 1e-6 * oracle["loss"]      # (+ the fp32 sums of both sides)


def _errs(got, ref, tiny=1e-4, abs_tol=5e-3):
    """Per-tensor rel-L2 as test_hip_train_step._report takes it: a tensor whose reference norm is below `tiny` is analytically ~0 and is held to an
    absolute error norm instead."""
    errs = {}
    for k, r in ref.items():
        g, r = got[k].double().flatten(), r.double().flatten()
        if float(r.norm()) > tiny:
            errs[k] = rel_l2(g, r)
        else:
            assert float((g - r).norm()) <= abs_tol, (k, float((g - r).norm()), float(r.norm()))
    return errs


def test_gradients_vs_autograd_at_the_devices_forward_point(oracle, device_run):
    """dy = sign(yy - x) / numel -- the device's own signs -- back-propagated through the fp32 oracle, against the step's unscaled gradients. Bounds of
    test_unetpp_backward_chain_tight_on_a_smooth_network (this chain at this shape)."""
    dy = torch.sign(device_run["yy"] - oracle["x"]) / NUMEL
    oracle["y"].backward(dy)
    ref = {k: v.grad for k, v in oracle["sdg"].items() if v.requires_grad and v.grad is not None}
    got = device_run["grads"]
    assert all((got[k] is None) == (k not in ref) for k in got)
    errs = _errs(got, ref)
    worst, med = max(errs.items(), key=lambda kv: kv[1]), float(np.median(list(errs.values())))
    print("reconstruction backward at the device's forward point (scale %g): median rel-L2 %.3e, worst %.3e (%s)" % (device_run["scale"], med, worst[1], worst[0]))
    assert worst[1] < 8e-2 and med < 1.2e-2


def test_ten_step_trajectory_vs_the_oracle(deterministic):
    """Ten ReconstructionTrainStep.step calls on one fixed batch at lr 1e-3 beside unetpp_ref + nn.L1Loss + Adam(lr 1e-3) from the same weights. No step is
    skipped; the first loss is at the same weights (the triangle bound); loss[9] / loss[0] agrees with the oracle's ratio within 6.5 %, the spread DESIGN.md
    section 10 documents for lr-1e-3 Adam trajectories (the fp32 oracle against itself under an f16-level input change)."""
    from oracle import unetpp_ref
    from ted_spad_amd.pretrain import ReconstructionTrainStep
    from ted_spad_amd.train_nets import UNetPPTrainer
    fa, sd = _fa()
    x = _x()
    sdg = _grad_sd(sd)
    opt = torch.optim.Adam([v for v in sdg.values() if v.requires_grad], lr=1e-3)
    crit = torch.nn.L1Loss()
    step = ReconstructionTrainStep(fa, learning_rate=1e-3)
    xc = x.cuda()
    yy0 = UNetPPTrainer(_fa()[0].train()).forward(xc)[0].cpu()       # the first step's output (deterministic mode: the same bits from the same weights)
    dev, ref = [], []
    for i in range(10):
        opt.zero_grad()
        y = unetpp_ref.forward(x, sdg, train=True)
        loss = crit(y, x)
        loss.backward()
        opt.step()
        ref.append(loss.item())
        if i == 0:
            y0 = y.detach()
        out = step.step(xc)
        assert not out["skipped"], i
        dev.append(out["loss"])
    print("device", ["%.5f" % v for v in dev])
    print("oracle", ["%.5f" % v for v in ref])
    assert step.iteration == 10 and int(fa.encoder.bn1.num_batches_tracked) == 10
    assert all(np.isfinite(dev)) and dev[9] < dev[0]
    slack = float((yy0.double() - y0.double()).abs().mean())
    print("first step: device %.7f oracle %.7f, |diff| %.3e <= mean|yy - y_ref| %.3e" % (dev[0], ref[0], abs(dev[0] - ref[0]), slack))
    assert abs(dev[0] - ref[0]) <= slack + 1e-6 * ref[0]                        # the bound of test_loss_vs_the_oracle
    rd, rr = dev[9] / dev[0], ref[9] / ref[0]
    print("loss[9]/loss[0]: device %.5f oracle %.5f (%.2f %%)" % (rd, rr, 100 * abs(rd / rr - 1)))
    assert abs(rd - rr) <= 0.065 * rr
    step.set_lr(2e-4)
    assert all(g["lr"] == 2e-4 for g in step.opt.param_groups)


def test_evaluate(deterministic):
    from ted_spad_amd.losses import l1_flat
    from ted_spad_amd.pretrain import ReconstructionTrainStep
    fa, _ = _fa()
    step = ReconstructionTrainStep(fa)
    x = _x().cuda()
    step.step(x)                                                      # running statistics that differ from the initial ones
    before = {k: v.detach().clone() for k, v in fa.state_dict().items()}
    out, loss = step.evaluate(x)
    assert not fa.training and out.shape == SHAPE and out.dtype == torch.float32 and loss.dim() == 0
    assert all(torch.equal(v, before[k]) for k, v in fa.state_dict().items()), "evaluate leaves parameters and running statistics alone"
    with torch.no_grad():
        ref = fa.eval()(x)
    assert torch.equal(out, ref)
    assert torch.equal(loss, l1_flat(ref, x))
    ref64 = float((ref.double() - x.double()).abs().mean())
    assert abs(float(loss) - ref64) <= 1e-5 * ref64


def test_bridge_agrees_with_the_driver(deterministic):
    """The reference's own statements (train_reconstruction.py:35-48) through the autograd bridge with losses.L1Loss, against the driver at the bridge's
    scale (TE.GRAD_SCALE = 256): the same forward, the same loss bits (the flat form adds an (n,3,h,w) pair in the train form's order); gradients within
    the bound of test_autograd_path_agrees_with_the_step_driver."""
    from ted_spad_amd import train_engine as TE
    from ted_spad_amd.losses import L1Loss
    from ted_spad_amd.pretrain import ReconstructionTrainStep
    assert TE.GRAD_SCALE == 256.0
    x = _x().cuda()
    fa, _ = _fa()
    step = ReconstructionTrainStep(fa, loss_scale=256.0)
    step.opt = torch.optim.SGD(fa.parameters(), lr=0.0)               # keep the gradients, do not move the weights
    out = step.step(x)
    g_drv = {k: p.grad.detach().clone() for k, p in fa.named_parameters() if p.grad is not None}
    fa2, _ = _fa()
    criterion = L1Loss()
    optimizer = torch.optim.SGD(fa2.parameters(), lr=0.0)
    fa2.train()                                                       # :35
    optimizer.zero_grad()                                             # :43
    output = fa2(x)                                                   # :45
    loss = criterion(output, x)                                       # :46
    loss.backward()                                                   # :47
    optimizer.step()                                                  # :48
    assert np.float32(loss.item()) == np.float32(out["loss"]), (loss.item(), out["loss"])
    cos = []
    for k, p in fa2.named_parameters():
        assert (p.grad is None) == (k not in g_drv), k
        if p.grad is not None:
            a_, b_ = p.grad.flatten().double(), g_drv[k].flatten().double()
            if float(b_.norm()) > 1e-3:
                cos.append(float(a_ @ b_ / (a_.norm() * b_.norm())))
    print("bridge vs driver: median cosine %.6f, min %.6f over %d tensors" % (float(np.median(cos)), min(cos), len(cos)))
    assert float(np.median(cos)) > 0.9 and min(cos) > 0.5


def test_full_batch_step_trains_every_parameter():
    """One step at the script's batch, 32 x 3 x 224 x 224, with the default (automatic) loss scale: not skipped, a finite loss, and no on-path parameter
    whose gradient is identically zero. With the constant scale 256 the gradient entering the head would be 5.3e-5, an f16 subnormal that the matrix cores
    read as 0 (pretrain.py)."""
    from ted_spad_amd.pretrain import ReconstructionTrainStep, auto_loss_scale
    fa, _ = _fa(beta=None)
    step = ReconstructionTrainStep(fa)
    gain = (torch.arange(1, 33).float() / 32).view(-1, 1, 1, 1)
    x = (synth_tensor(0, "recon224", (32, 3, 224, 224)) * gain).cuda()
    assert step.scale_for(x) == auto_loss_scale(4816896, "f16") and step.scale_for(x) / 4816896 >= 2.0 ** -14
    before = {k: p.detach().clone() for k, p in fa.named_parameters()}
    out = step.step(x)
    assert bool(out["skipped"]) is False and np.isfinite(out["loss"]) and out["loss"] > 0
    off = {id(p) for p in step.fa_tr.off_path_params()}
    dead = [k for k, p in fa.named_parameters() if id(p) not in off and (p.grad is None or not bool((p.grad != 0).any()))]
    assert not dead, dead
    assert all(p.grad is None for p in step.fa_tr.off_path_params())
    assert all(not torch.equal(p.detach(), before[k]) for k, p in fa.named_parameters() if id(p) not in off), "Adam moved every on-path parameter"


def test_another_module_is_refused():
    from ted_spad_amd.model_loaders import load_fa_model
    from ted_spad_amd.pretrain import ReconstructionTrainStep
    with pytest.raises(TypeError, match="UnetPlusPlus"):
        ReconstructionTrainStep(load_fa_model(arch="unet"))
