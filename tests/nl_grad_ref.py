"""Host restatement of the TRAINING side of I3Res50's non-local block in float64 (the reference: aux_code/models/large_i3d.py:86-125 under autograd),
built on nl_ref:

    attention_grads(theta, phi, g, dt, scale)   the closed-form gradients of nl_ref.attention that tedspad_nl_attention_bwd computes, with lse and T
    attention_autograd(theta, phi, g, dt, scale)   the same gradients from torch autograd through nl_ref.attention
    block_train(x, sd, prefix, dy, mode)        the block in 'train' (batch statistics, unbiased running-var update) or 'frozen' (running statistics as a
                                                fixed affine) mode, gradients from torch autograd in float64; every intermediate may be replaced (`given`)
    PARAMS                                      the ten parameters, in state_dict order
"""
import math
from collections import OrderedDict

import torch

import nl_ref

PARAMS = ("theta.weight", "theta.bias", "phi.weight", "phi.bias", "g.weight", "g.bias", "out.weight", "out.bias", "bn.weight", "bn.bias")


# Analytically zero in train mode, so compared absolutely (the rule of tests/test_hip_train_ops.py:139), never relatively: out.bias and g.bias shift every
# pixel of a channel in front of bn, which removes the batch mean; phi.bias adds theta_i . b to every logit of row i, which the softmax does not see.
# (In 'frozen' mode only phi.bias stays zero.)
ZERO_GRADS = {"train": ("out.bias", "g.bias", "phi.bias"), "frozen": ("phi.bias",)}


def sample_index(numel, target=2048):
    """The fixed strided sample the training fixture stores of a tensor: flat indices 0, s, 2s, ... with the first stride s >= numel / target that is
    coprime to numel (so that it walks every axis of the power-of-two and 7 x 7 shapes instead of staying on one channel or one pixel)."""
    s = max(1, numel // target)
    while math.gcd(s, numel) != 1:
        s += 1
    return torch.arange(0, numel, s)


def vs_fixture(got, golden, key):
    """(rel-L2 of `got` on the stored sample, relative difference of the L2 norms) against fixture entries `<key>/sample`, `<key>/norm`."""
    got = torch.as_tensor(got).double().flatten()
    ref = torch.as_tensor(golden[key + "/sample"]).double()
    s = got[sample_index(got.numel())]
    norm = float(golden[key + "/norm"])
    return float((s - ref).norm() / ref.norm().clamp_min(1e-300)), abs(float(got.norm()) - norm) / max(norm, 1e-300)


def attention_grads(theta, phi, g, dt, scale):
    """S = scale theta phi^T, P = softmax_j S, T = P g. Returns dict(t, lse, p, dtheta, dphi, dg), float64:
       dg = P^T dT, dP = dT g^T, D_i = sum_c dT[i,c] T[i,c], dS = P o (dP - D), dtheta = scale dS phi, dphi = scale dS^T theta."""
    theta, phi, g, dt = (torch.as_tensor(t).double() for t in (theta, phi, g, dt))
    s = torch.einsum("nqd,nkd->nqk", theta, phi) * float(scale)
    lse = torch.logsumexp(s, dim=2)
    p = torch.exp(s - lse.unsqueeze(2))
    t = torch.einsum("nqk,nkd->nqd", p, g)
    dg = torch.einsum("nqk,nqd->nkd", p, dt)
    dp = torch.einsum("nqd,nkd->nqk", dt, g)
    dd = (dt * t).sum(dim=2, keepdim=True)
    ds = p * (dp - dd)
    return dict(t=t, lse=lse, p=p, dtheta=torch.einsum("nqk,nkd->nqd", ds, phi) * float(scale), dphi=torch.einsum("nqk,nqd->nkd", ds, theta) * float(scale), dg=dg)


def attention_autograd(theta, phi, g, dt, scale):
    th, ph, gg = (torch.as_tensor(t).double().clone().requires_grad_() for t in (theta, phi, g))
    nl_ref.attention(th, ph, gg, scale).backward(torch.as_tensor(dt).double())
    return th.grad, ph.grad, gg.grad


def block_train(x, sd, prefix, dy, mode="train", eps=1e-5, momentum=0.1, given=None):
    """The block on (n, c, t, h, w) input `x` with upstream gradient `dy`, float64. Returns an OrderedDict: out, dx, branch_dx (= dx - dy: what the
    branch alone sends back), running_mean, running_var (after the forward), and one gradient per name of PARAMS ('grad/<name>'; bn.weight / bn.bias are
    missing in 'frozen' mode). given: {"theta" | "phi" | "g" | "t": rows (n, positions, d), "mean" | "var": (c,)} -- values the backward is evaluated AT
    instead of the float64 forward's own (a device's stored 16-bit intermediates and batch statistics); the derivative rules stay the float64 ones."""
    assert mode in ("train", "frozen")
    given = given or {}
    x = torch.as_tensor(x).double().clone().requires_grad_()
    P = OrderedDict((k, sd[prefix + k].double().clone().requires_grad_()) for k in PARAMS)
    psd = {prefix + k: v for k, v in P.items()}
    th, ph, g = nl_ref.block_parts(x, psd, prefix)

    def at(name, v):            # forward value replaced, derivative kept: v + (given - v).detach()
        return v + (torch.as_tensor(given[name]).double() - v).detach() if name in given else v
    th, ph, g = at("theta", th), at("phi", ph), at("g", g)
    d = th.shape[2]
    t = at("t", nl_ref.attention(th, ph, g, float(d) ** -0.5))
    t5 = t.transpose(1, 2).reshape(x.shape[0], d, *x.shape[2:])
    o = nl_ref._pw(t5, P["out.weight"], P["out.bias"])
    v = lambda a: a.view(1, -1, 1, 1, 1)
    rm, rv = sd[prefix + "bn.running_mean"].double(), sd[prefix + "bn.running_var"].double()
    if mode == "train":
        cnt = o.numel() // o.shape[1]
        mean, var = at("mean", o.mean(dim=(0, 2, 3, 4))), at("var", o.var(dim=(0, 2, 3, 4), unbiased=False))
        rm = (1 - momentum) * rm + momentum * mean.detach()
        rv = (1 - momentum) * rv + momentum * var.detach() * cnt / (cnt - 1)
        y = (o - v(mean)) / torch.sqrt(v(var) + eps) * v(P["bn.weight"]) + v(P["bn.bias"]) + x
    else:
        y = (o - v(rm)) / torch.sqrt(v(rv) + eps) * v(P["bn.weight"].detach()) + v(P["bn.bias"].detach()) + x
    dy = torch.as_tensor(dy).double()
    y.backward(dy)
    res = OrderedDict(out=y.detach(), dx=x.grad, branch_dx=x.grad - dy, running_mean=rm, running_var=rv)
    for k, p in P.items():
        if p.grad is not None:
            res["grad/" + k] = p.grad
    return res
