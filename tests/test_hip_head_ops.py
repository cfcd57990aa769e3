"""-m gpu: the fp32 head ops of the training step (csrc/head.hip: BatchNorm1d in train mode, row L2 normalisation, the dropout product) through the C ABI,
against float64 torch (tests/kernel_refs.py). Bounds: (chain length + 8) * 2^-24 times the sum of the absolute terms of each quantity -- the worst case of
a sequential (bn1d: B terms per thread) or strided (normalize: N / 64 terms per lane, then a 6-step butterfly) fp32 sum, plus the few roundings around it."""
import ctypes as Ct

import pytest
import torch

import kernel_refs as R

pytestmark = pytest.mark.gpu
D = torch.float64
F32 = R.F32_EPS
EPS, MOM = 1e-5, 0.1


def L():
    from ted_spad_amd import _lib
    return _lib.lib()


def S():
    return Ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def ok(rc):
    from ted_spad_amd import _lib
    assert rc == 0, _lib.last_error()


def within(got, ref, bound, what):
    err = (got.to(D) - ref).abs()
    bound = torch.as_tensor(bound, dtype=D).expand_as(err)
    bad = err > bound
    assert not bool(bad.any()), "%s: %d elements out of bound, worst error %.3e at bound %.3e" % (
        what, int(bad.sum()), float(err[bad].max()), float(bound[bad][err[bad].argmax()]))


def guarded(rows, cols):
    """a (rows, cols) device matrix with two sentinel rows behind it"""
    return torch.full((rows + 2, cols), 1024.0, device="cuda")


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("C", [1, 255, 257, 2048])
@pytest.mark.parametrize("B", [1, 2, 3, 24])
def test_bn1d_train_fwd_bwd(B, C, relu):
    x = R.synth_tensor(31, "x", (B, C), -2, 2)
    if B > 1:
        x[0, 0] = x[1, 0]                       # a channel with (almost) no variance
    gamma = R.synth_tensor(31, "g", (C,), 0.5, 1.5) * torch.where(R.synth_tensor(31, "gs", (C,)) < 0.25, -1.0, 1.0)
    beta, dy = R.synth_tensor(31, "b", (C,), -0.5, 0.5), R.synth_tensor(31, "dy", (B, C), -1, 1)
    rm, rv = R.synth_tensor(31, "rm", (C,), -0.1, 0.1), R.synth_tensor(31, "rv", (C,), 0.5, 1.5)
    xd, gd, bd, rmd, rvd = x.cuda(), gamma.cuda(), beta.cuda(), rm.cuda(), rv.cuda()
    y, mean, invstd = guarded(B, C), guarded(1, C), guarded(1, C)
    ok(L().tedspad_bn1d_train_fwd(xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), EPS, MOM, rmd.data_ptr(), rvd.data_ptr(), y.data_ptr(), mean.data_ptr(),
                                  invstd.data_ptr(), B, C, relu, S()))
    f = R.bn1d_train_ref(x, gamma, beta, EPS, bool(relu))
    x64, g64, b64 = x.to(D), gamma.to(D), beta.to(D)
    k = (B + 8) * F32
    absx = x64.abs().sum(0) / B + f["mean"].abs()                      # |terms| of mean, and of x - mean
    assert bool((y[B:] == 1024.0).all()) and bool((mean[1:] == 1024.0).all()) and bool((invstd[1:] == 1024.0).all())
    within(mean[0].cpu(), f["mean"], k * x64.abs().sum(0) / B, "mean")
    # var = sum (x - mean)^2 / B: every term carries the error of x - mean twice
    dvar = k * ((x64 - f["mean"]) ** 2).sum(0) / B + 2 * ((x64 - f["mean"]).abs().sum(0) / B) * k * absx
    var = 1 / f["invstd"] ** 2
    within(invstd[0].cpu(), f["invstd"], f["invstd"] * (0.5 * dvar / var + k), "invstd")
    xh = (x64 - f["mean"]) * f["invstd"]
    dxh = k * absx * f["invstd"] + xh.abs() * (0.5 * dvar / var + k)     # error of xhat, per element
    ypre = xh * g64 + b64
    within(y[:B].cpu(), f["y"], g64.abs() * dxh + k * (ypre.abs() + (xh * g64).abs() + b64.abs()), "y")
    within(rmd.cpu(), (1 - MOM) * rm.to(D) + MOM * f["mean"], k * ((1 - MOM) * rm.to(D).abs() + MOM * x64.abs().sum(0) / B), "running_mean")
    # unbiased variance; B = 1: the kernel's documented rule, the biased variance (0) -- torch refuses a one-value batch
    within(rvd.cpu(), (1 - MOM) * rv.to(D) + MOM * f["var_run"], k * (1 - MOM) * rv.to(D) + MOM * (B / max(B - 1, 1)) * (dvar + k * var), "running_var")
    ok(L().tedspad_bn1d_train_fwd(xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), EPS, MOM, None, None, y.data_ptr(), mean.data_ptr(),
                                  invstd.data_ptr(), B, C, relu, S()))              # running statistics not tracked
    # backward, from the forward's own fp32 y / mean / invstd; gradients kept away from the ReLU edge of the stored y
    yk, mk, ik = y[:B].cpu().to(D), mean[0].cpu().to(D), invstd[0].cpu().to(D)
    if relu:
        dy = dy * ((f["y"] > 0) == (yk > 0))
    dyd = dy.cuda()
    dx, dg, db = guarded(B, C), guarded(1, C), guarded(1, C)
    ok(L().tedspad_bn1d_train_bwd(dyd.data_ptr(), xd.data_ptr(), y.data_ptr(), mean.data_ptr(), invstd.data_ptr(), gd.data_ptr(), dx.data_ptr(),
                                  dg.data_ptr(), db.data_ptr(), B, C, relu, S()))
    assert bool((dx[B:] == 1024.0).all()) and bool((dg[1:] == 1024.0).all()) and bool((db[1:] == 1024.0).all())
    gm = dy.to(D) * (yk > 0) if relu else dy.to(D)
    xk = (x64 - mk) * ik                                                # the definition, at the mean / invstd the kernel is handed
    sb, sg = gm.sum(0), (gm * xk).sum(0)
    want = g64 * ik * (gm - sb / B - xk * sg / B)
    within(db[0].cpu(), sb, k * gm.abs().sum(0), "dbeta")
    within(dg[0].cpu(), sg, k * (gm * xk).abs().sum(0) + 2 * F32 * (gm.abs() * (x64.abs() + mk.abs()) * ik).sum(0), "dgamma")
    terms = gm.abs() + gm.abs().sum(0) / B + xk.abs() * (gm * xk).abs().sum(0) / B + (x64.abs() + mk.abs()) * ik * (2 * F32 / k) * (gm * xk).abs().sum(0) / B
    within(dx[:B].cpu(), want, k * (g64 * ik).abs() * terms, "dx")


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("N", [1, 63, 65, 130, 2048])
def test_l2_normalize_rows_fwd_bwd(N, B):
    eps = 1e-12
    x = R.synth_tensor(32, "x", (B, N), -1, 1)
    dy = R.synth_tensor(32, "dy", (B, N), -1, 1)
    if B > 1:
        x[1] = 0.0                                          # an all-zero row
        x[3] = 0.0
        x[3, N // 2] = 1e-14                                # norm 1e-14 < eps
    y, dx = guarded(B, N), guarded(B, N)
    xd, dyd = x.cuda(), dy.cuda()
    ok(L().tedspad_l2_normalize_rows(xd.data_ptr(), y.data_ptr(), B, N, eps, S()))
    ok(L().tedspad_l2_normalize_rows_bwd(xd.data_ptr(), dyd.data_ptr(), dx.data_ptr(), B, N, eps, S()))
    ry, rdx = R.l2_normalize_ref(x, eps, dy)
    assert bool((y[B:] == 1024.0).all()) and bool((dx[B:] == 1024.0).all())
    k = (N / 64 + 8) * F32
    x64, d64 = x.to(D), dy.to(D)
    nr = x64.norm(dim=1, keepdim=True).clamp_min(eps)
    within(y[:B].cpu(), ry, k * ry.abs(), "y")                                  # one positive sum: relative to the value itself
    # dx = (dy - y (y . dy)) / |x|: terms |dy|, |y| sum |y dy|
    terms = (d64.abs() + ry.abs() * (ry * d64).abs().sum(1, keepdim=True)) / nr
    within(dx[:B].cpu(), rdx, k * terms, "dx")
    if B > 1:
        assert float(y[1].abs().max()) == 0.0 and torch.equal(dx[1].cpu(), (dy[1] / torch.tensor(eps, dtype=torch.float32)))       # |x| < eps: dx = dy / eps
        assert bool(torch.isfinite(dx[:B]).all()) and bool(torch.isfinite(y[:B]).all())


@pytest.mark.parametrize("n", [1, 255, 4096 * 256 + 5])
def test_mul_f32(n):
    a, b = R.synth_tensor(33, "a", (n,), -2, 2), R.synth_tensor(33, "b", (n,), -2, 2)
    scale = torch.tensor(1.0 / 0.7, dtype=torch.float32)                        # a dropout keep-probability
    out = torch.full((n + 64,), 1024.0, device="cuda")
    ad, bd = a.cuda(), b.cuda()
    ok(L().tedspad_mul_f32(ad.data_ptr(), bd.data_ptr(), out.data_ptr(), n, float(scale), S()))
    assert torch.equal(out[:n].cpu(), a * b * scale) and bool((out[n:] == 1024.0).all())          # the same association, exact
