"""CPU: the float64 references of tests/kernel_refs.py against float64 torch (autograd) at the shapes the -m gpu op tests use, to 1e-12 relative, and the
properties of the two value generators those tests rely on (ties in the max-pool windows, exactness of dyadic sums). Last, the MGFN references: equal to float64
torch, torch's fp32 evaluation inside every per-element bound, a list of wrong references outside. Then the same for the fp32 head, BCE and vote kernels
(tests/test_hip_head_exact.py): the case tables reach every kernel form, their inputs meet the conditions of exactness, every `wrong=` mutant is caught."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import kernel_refs as R
from oracle import losses_ref
from ted_spad_amd.synth import synth_tensor

D = torch.float64
EPS = 1e-5


def close(a, b, rel=1e-12):
    a, b = torch.as_tensor(a).to(D), torch.as_tensor(b).to(D)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max()) <= rel * max(float(b.abs().max()), 1e-300)


@pytest.mark.parametrize("C,Cz", R.BN_CHANNELS)
@pytest.mark.parametrize("pixels", [7, 255, 257, 1000])          # (1 pixel: torch refuses a one-value batch; the formulas are the same)
def test_bn_refs_vs_torch_autograd(C, Cz, pixels):
    for relu, with_res, y_mask in ((True, True, True), (True, False, False), (False, False, False)):
        z, gamma, beta = R.bn_inputs(5, pixels, C, Cz, 1, torch.float32)
        z = z[0, :, :C].clone().requires_grad_()
        gamma, beta = gamma.to(D).requires_grad_(), beta.to(D).requires_grad_()
        res = synth_tensor(5, "res", (pixels, C), -1, 1).to(D).requires_grad_() if with_res else None
        rm, rv = synth_tensor(5, "rm", (C,), -0.1, 0.1).to(D), synth_tensor(5, "rv", (C,), 0.5, 1.5).to(D)
        rm_t, rv_t = rm.clone(), rv.clone()
        u = F.batch_norm(z, rm_t, rv_t, gamma, beta, training=True, momentum=0.1, eps=EPS)
        y = u + res if with_res else u
        y = F.relu(y) if relu else y
        dy = R.dyadic(5, "dy", (pixels, C))
        y.backward(dy)
        zd = z.detach()
        f = R.bn_train_ref(zd, zd.sum(0), (zd * zd).sum(0), pixels, gamma.detach(), beta.detach(), EPS, res.detach() if with_res else None, relu,
                           momentum=0.1, running_mean=rm, running_var=rv)
        assert close(f["y"], y.detach()) and close(f["running_mean"], rm_t) and close(f["running_var"], rv_t)
        assert close(f["mean"], zd.mean(0)) and close(f["invstd"], 1 / torch.sqrt(zd.var(0, unbiased=False) + EPS))
        assert bool((f["M"] >= f["y"].abs() * (1 - 1e-12)).all())
        b = R.bn_bwd_ref(dy, f["y"] if y_mask else None, zd, f["mean"], f["invstd"], gamma.detach(), beta.detach(), relu)
        scale = max(float(z.grad.abs().max()), float(dy.abs().max()))
        assert float((b["dz"] - z.grad).abs().max()) <= 1e-12 * scale
        assert close(b["sum_g"], beta.grad) and float((b["sum_gx"] - gamma.grad).abs().max()) <= 1e-12 * float(b["abs_gx"].max())
        assert close(b["sum_dz"], b["dz"].sum(0)) and bool((b["abs_gx"] >= b["sum_gx"].abs() * (1 - 1e-12)).all())
        if with_res:
            assert close(b["dres"], res.grad)


def test_bn_mask_recomputed_from_z_equals_mask_from_y():
    z, gamma, beta = R.bn_inputs(6, 257, 40, 40, 1, torch.float32)
    f = R.bn_train_ref(z[0], z[0].sum(0), (z[0] ** 2).sum(0), 257, gamma, beta, EPS, None, True)
    dy = R.dyadic(6, "dy", (257, 40))
    a = R.bn_bwd_ref(dy, f["y"], z[0], f["mean"], f["invstd"], gamma, beta, True)
    b = R.bn_bwd_ref(dy, None, z[0], f["mean"], f["invstd"], gamma, beta, True)
    assert torch.equal(a["g"], b["g"]) and 0.2 < float((a["g"] != 0).double().mean()) < 0.8


@pytest.mark.parametrize("case", R.POOL_CASES, ids=[c[0] for c in R.POOL_CASES])
@pytest.mark.parametrize("c", R.POOL_C)
def test_maxpool_refs_vs_torch(case, c):
    _, k, s, p, thw = case
    x = R.tie_values(7, "px", (2,) + thw + (c,))
    share = R.maxpool_tie_share(x, k, s, p)
    assert share >= 0.30, share           # otherwise the GPU test would not be testing ties
    y, idx = R.maxpool_fwd_ref(x, k, s, p)
    xt = x.permute(0, 4, 1, 2, 3).contiguous().requires_grad_()
    yt, it = F.max_pool3d(xt, k, s, p, return_indices=True)
    assert torch.equal(y, yt.detach().permute(0, 2, 3, 4, 1))
    assert torch.equal(R.local_to_flat_index(idx, thw, k, s, p), it.permute(0, 2, 3, 4, 1))
    dy = R.dyadic(7, "pdy", tuple(y.shape))
    yt.backward(dy.permute(0, 4, 1, 2, 3))
    add = R.dyadic(7, "padd", tuple(x.shape))
    assert torch.equal(R.maxpool_bwd_ref(x, idx, dy, k, s, p), xt.grad.permute(0, 2, 3, 4, 1))
    assert torch.equal(R.maxpool_bwd_ref(x, idx, dy, k, s, p, add=add, relu_mask=True), (xt.grad.permute(0, 2, 3, 4, 1) + add) * (x > 0))


def test_maxpool_ref_nonfinite_follows_torch():
    k, s, p, thw = (1, 3, 3), (1, 2, 2), (0, 1, 1), (1, 6, 6)
    x = R.tie_values(8, "nf", (1,) + thw + (8,))
    x[0, 0, 0, 0, :] = float("inf")
    x[0, 0, 2, 3, 0], x[0, 0, 3, 3, 0] = float("nan"), float("nan")        # two NaNs in one window: the last one keeps the index
    x[0, 0, 5, 5, :] = float("-inf")
    y, idx = R.maxpool_fwd_ref(x, k, s, p)
    yt, it = F.max_pool3d(x.permute(0, 4, 1, 2, 3).contiguous(), k, s, p, return_indices=True)
    yt = yt.permute(0, 2, 3, 4, 1)
    assert torch.equal(torch.isnan(y), torch.isnan(yt)) and torch.equal(torch.nan_to_num(y, 7.0), torch.nan_to_num(yt, 7.0))
    assert torch.equal(R.local_to_flat_index(idx, thw, k, s, p), it.permute(0, 2, 3, 4, 1))
    assert bool(torch.isinf(y[0, 0, 0, 0]).all()) and int(torch.isnan(y).sum()) >= 2


def test_generators():
    t = R.tie_values(1, "t", (4096,))
    assert set(t.tolist()) == {0.0, 0.5, 1.0} and 0.45 < float((t == 0).double().mean()) < 0.55
    for dt in (torch.float16, torch.bfloat16):
        assert torch.equal(t.to(dt).to(D), t)
    d = R.dyadic(1, "d", (2000, 8))
    assert float(d.min()) == -2.0 and float(d.max()) == 2.0 and torch.equal(d * 16, (d * 16).round())
    assert torch.equal(d.float().sum(0).double(), d.sum(0))               # exact in fp32, in any order
    for dt in (torch.float16, torch.bfloat16):
        assert torch.equal(d.to(dt).to(D), d)


@pytest.mark.parametrize("h,w,ho,wo", R.BILINEAR_CASES)
def test_resize_refs(h, w, ho, wo):
    x = synth_tensor(9, "bx", (2, h, w, 8), -1, 1).to(D)
    up, taps = R.bilinear2x_ref(x, ho, wo)
    pt, pl = R.bilinear_pad(h, w, ho, wo)
    inner = torch.zeros(ho, wo, dtype=torch.bool)
    inner[pt:pt + 2 * h, pl:pl + 2 * w] = True
    assert float(up[:, ~inner].abs().max() if (~inner).any() else 0.0) == 0.0
    assert bool((taps + 1e-15 >= up.abs()).all())                         # a convex combination of the four taps
    g = R.dyadic(9, "bg", (2, ho, wo, 8))
    dx = R.bilinear2x_bwd_ref(g, h, w)
    assert close((dx * x).sum(), (up * g).sum())                   # the adjoint of a linear map
    n2 = R.nearest2x_ref(x)
    assert torch.equal(n2[:, 1::2, 0::2], x) and torch.equal(n2[:, 0::2, 1::2], x)
    assert close((R.nearest2x_bwd_ref(g[:, :2 * h, :2 * w]) * x).sum(), (n2 * g[:, :2 * h, :2 * w]).sum())


@pytest.mark.parametrize("B", [1, 2, 3, 24])
def test_bn1d_and_normalize_refs(B):
    C = 255
    x, g, b = synth_tensor(3, "x", (B, C), -2, 2), synth_tensor(3, "g", (C,), 0.5, 1.5), synth_tensor(3, "b", (C,), -0.5, 0.5)
    dy = synth_tensor(3, "dy", (B, C), -1, 1)
    f = R.bn1d_train_ref(x, g, b, EPS, True, dy)
    xd = x.to(D)
    xh = (xd - f["mean"]) * f["invstd"]
    assert close(f["y"], (xh * g + b).clamp_min(0))
    gm = dy.to(D) * (f["y"] > 0)
    assert close(f["dbeta"], gm.sum(0)) and float((f["dgamma"] - (gm * xh).sum(0)).abs().max()) < 1e-12 * float((gm * xh).abs().sum(0).max() + 1)
    want = g.to(D) * f["invstd"] * (gm - gm.mean(0) - xh * (gm * xh).mean(0))
    assert float((f["dx"] - want).abs().max()) < 1e-12 * float(want.abs().max() + gm.abs().max() * float((g.to(D) * f["invstd"]).max()))
    y, dx = R.l2_normalize_ref(x, 1e-12, dy)
    nr = xd.norm(dim=1, keepdim=True)
    assert close(y, xd / nr) and close(dx, (dy.to(D) - y * (y * dy.to(D)).sum(1, keepdim=True)) / nr)
    z = torch.zeros(2, 5)
    z[1] = 1e-14 / 5 ** 0.5
    y, dx = R.l2_normalize_ref(z, 1e-12, torch.ones(2, 5))
    assert close(y, z.to(D) / 1e-12) and close(dx, torch.ones(2, 5, dtype=D) / 1e-12)      # below eps: y = x / eps, dx = dy / eps


def test_loss_refs_vs_numpy_restatements():
    lg, lab = synth_tensor(2, "lg", (5, 65), -3, 3), torch.tensor([0, 64, 3, 3, 17])
    assert abs(float(R.cross_entropy_ref(lg, lab)[0]) - losses_ref.cross_entropy_np(lg.numpy(), lab.numpy())) < 1e-12
    a, p, n = (synth_tensor(2, s, (6, 65), -1, 1) for s in "apn")
    assert abs(float(R.triplet_ref(a, p, n)[0]) - losses_ref.triplet_np(a.numpy(), p.numpy(), n.numpy())) < 1e-12
    zi, zj = synth_tensor(2, "zi", (12, 64), -1, 1) * 0.3, synth_tensor(2, "zj", (12, 64), -1, 1) * 0.3
    for cos in (False, True):
        assert abs(float(R.ntxent_ref(zi, zj, 0.1, cos)[0]) - losses_ref.nt_xent_np(zi.numpy(), zj.numpy(), 0.1, use_cosine=cos)) < 1e-12 * max(1.0, abs(float(R.ntxent_ref(zi, zj, 0.1, cos)[0])))


# ---- the exact-arithmetic conv references and the case tables of tests/test_hip_conv_exact.py ----------------------------------------------------------
def _conv_taps(x, w, stride, pf, pb):
    """conv3d as an explicit sum over taps of strided slices of the padded input: shares no code with F.conv3d."""
    xp = F.pad(x, [pf[2], pb[2], pf[1], pb[1], pf[0], pb[0]])
    co, ci, kt, kh, kw = w.shape
    to, ho, wo = ((xp.shape[2 + i] - w.shape[2 + i]) // stride[i] + 1 for i in range(3))
    y = torch.zeros((x.shape[0], co, to, ho, wo), dtype=D)
    for dt in range(kt):
        for dh in range(kh):
            for dw in range(kw):
                sl = xp[:, :, dt:dt + (to - 1) * stride[0] + 1:stride[0], dh:dh + (ho - 1) * stride[1] + 1:stride[1], dw:dw + (wo - 1) * stride[2] + 1:stride[2]]
                y += torch.einsum("ncthw,oc->nothw", sl, w[:, :, dt, dh, dw])
    return y


CONV_REF_GEOS = [      # k, stride, front pad, back pad, (t, h, w)
    ((1, 3, 3), (1, 1, 1), (0, 1, 1), (0, 1, 1), (2, 6, 7)),
    ((3, 3, 3), (2, 2, 2), (0, 1, 1), (1, 1, 1), (4, 9, 9)),
    ((1, 1, 1), (1, 2, 2), (0, 0, 0), (0, 0, 0), (2, 7, 6)),
    ((5, 7, 7), (2, 2, 2), (2, 3, 3), (2, 3, 3), (4, 12, 10)),
    ((3, 1, 1), (1, 1, 1), (1, 0, 0), (1, 0, 0), (3, 4, 5)),
]


@pytest.mark.parametrize("geo", CONV_REF_GEOS, ids=[str(g[0]) + str(g[1]) for g in CONV_REF_GEOS])
def test_conv_refs_vs_float64_autograd(geo):
    k, stride, pf, pb, thw = geo
    n, ci, co = 2, 5, 6
    x = synth_tensor(21, "x", (n, ci) + thw, -1, 1).to(D).requires_grad_()
    w = synth_tensor(21, "w", (co, ci) + k, -1, 1).to(D).requires_grad_()
    scale, shift = synth_tensor(21, "s", (co,), 0.5, 1.5).to(D), synth_tensor(21, "b", (co,), -1, 1).to(D)
    z = _conv_taps(x, w * scale.view(-1, 1, 1, 1, 1), stride, pf, pb) + shift.view(1, -1, 1, 1, 1)
    assert tuple(z.shape[2:]) == R.conv_out_dims(thw, k, stride, pf, pb)
    res = synth_tensor(21, "r", tuple(z.shape), -1, 1).to(D)
    mask = R.signed_zero_mask(21, "m", tuple(z.shape))
    assert {float(v) for v in mask.unique()} == {-1.0, 0.0, 1.0} and bool(torch.signbit(mask[mask == 0]).any()) and not bool(torch.signbit(mask[mask == 0]).all())
    y_ref, z_ref = R.conv_fwd_ref64(x.detach(), w.detach(), stride, pf, pb, scale=scale, shift=shift, residual=res, mask=mask, relu=True)
    assert close(z_ref, z.detach()) and close(y_ref, (z.detach() + res).clamp_min(0) * (mask > 0))
    dy = synth_tensor(21, "dy", tuple(z.shape), -1, 1).to(D)
    z.backward(dy)
    xres, xmask = synth_tensor(21, "xr", tuple(x.shape), -1, 1).to(D), R.signed_zero_mask(21, "xm", tuple(x.shape))
    assert close(R.conv_dgrad_ref64(dy, w.detach(), x.shape, stride, pf, pb, scale=scale), x.grad)
    assert close(R.conv_dgrad_ref64(dy, w.detach(), x.shape, stride, pf, pb, scale=scale, residual=xres, mask=xmask), (x.grad + xres) * (xmask > 0))
    assert close(R.conv_wgrad_ref64(x.detach(), dy * scale.view(1, -1, 1, 1, 1), w.shape, stride, pf, pb), w.grad)
    st = R.conv_stats_ref64(z.detach(), 2)
    assert close(st[1, 0], z.detach()[1].sum((1, 2, 3))) and close(st[0, 1], (z.detach()[0] ** 2).sum((1, 2, 3))) and close(st.sum(0), R.conv_stats_ref64(z.detach())[0])


def test_small_ints_round_once_and_the_gate():
    v = R.small_ints(3, "v", (4096,), density=0.5)
    assert set(v.tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0} and 0.55 < float((v == 0).double().mean()) < 0.65          # 0.5 + 0.5 / 5
    for dt in (torch.float16, torch.bfloat16):
        assert torch.equal(v.to(dt).to(D), v)
    t = torch.tensor([257.0, 259.0, 2049.0, 131072.0, -3.0], dtype=D)
    assert R.round_once(t, "bf16").tolist() == [256.0, 260.0, 2048.0, 131072.0, -3.0]                                # ties to even
    assert R.round_once(t, "f16").tolist() == [257.0, 259.0, 2048.0, float("inf"), -3.0]
    with pytest.raises(AssertionError):
        R.round_once(torch.tensor([2.0 ** 24 + 1], dtype=D), "f16")
    assert R.exact_in_fp32(torch.tensor([2.0 ** 24 - 1]))
    for bad in (torch.tensor([2.0 ** 24]), torch.tensor([0.5])):
        with pytest.raises(AssertionError):
            R.exact_in_fp32(bad)
    with pytest.raises(AssertionError):
        R.exact_in_fp32(torch.tensor([1.0]), stats_z=torch.tensor([4096.0]))
    assert R.first_mismatch(torch.tensor([1.0, 2.0]), torch.tensor([1.0, 2.0])) == "" and "first at (1,)" in R.first_mismatch(torch.tensor([1.0, 2.0]), torch.tensor([1.0, 3.0]))


@pytest.mark.parametrize("case", R.WGRAD_CASES, ids=[c.name for c in R.WGRAD_CASES])
def test_wgrad_case_table_reaches_its_form_and_passes_the_gate(case):
    form, splits = case.launch_form()
    assert form == case.form, (form, splits)
    M = case.dims[0] * case.out[0] * case.out[1] * case.out[2]
    if case.multi_split:
        assert splits >= 3 and M % 64 != 0 and (M % (((M + splits - 1) // splits + 63) // 64 * 64)) % 64 != 0        # the last split ends inside a 64-pixel step
    x, w, dy = case.tensors()
    assert R.exact_in_fp32(R.conv_wgrad_ref64(x.abs(), dy.abs(), w.shape, case.stride, case.pf, case.pb) * 2)        # * 2: two accumulating calls
    assert float(R.conv_wgrad_ref64(x, dy, w.shape, case.stride, case.pf, case.pb).abs().max()) > 0


@pytest.mark.parametrize("case", R.DGRAD_CASES, ids=[c.name for c in R.DGRAD_CASES])
def test_dgrad_case_table_passes_the_gate(case):
    x, w, dy = case.tensors()
    res = R.small_ints(11, case.name + "res", tuple(x.shape), lo=-8, hi=8, density=1.0)
    assert R.exact_in_fp32(R.conv_dgrad_ref64(dy.abs(), w.abs(), x.shape, case.stride, case.pf, case.pb, scale=torch.full((case.cout,), 8.0)) + res.abs())
    unread = R.conv_dgrad_ref64(torch.ones_like(dy), torch.ones_like(w), x.shape, case.stride, case.pf, case.pb) == 0
    assert bool(unread.any()) == (case.name in ("pw_s2",)), case.name       # input positions the forward conv never reads


@pytest.mark.parametrize("case,must", R.EPILOGUE_CASES, ids=[c.name for c, _ in R.EPILOGUE_CASES])
def test_epilogue_case_table_passes_the_gate(case, must):
    x, w, bias, res, mask = R.epilogue_tensors(case)
    _, zabs = R.conv_fwd_ref64(x.abs(), w.abs(), case.stride, case.pf, case.pb, shift=bias.abs())
    _, z = R.conv_fwd_ref64(x, w, case.stride, case.pf, case.pb, shift=bias)
    st = R.conv_stats_ref64(z.abs(), 1)
    assert R.exact_in_fp32(zabs + res.abs(), st[0, 0], st[0, 1], stats_z=zabs)
    rows = case.dims[0] // R.EPILOGUE_GROUPS * case.out[0] * case.out[1] * case.out[2]
    assert case.dims[0] % R.EPILOGUE_GROUPS == 0 and rows >= 256 and rows % 256 != 0              # group boundaries inside the 256-row tiles ...
    assert rows % 64 != 0 or case.k == (1, 1, 1)                                                                  # ... and, for the 3 x 3 cases, inside the 64-row ones
    assert 0.2 < float((mask > 0).double().mean()) < 0.8 and float(z.abs().max()) > 16


def test_patch_cases_cover_one_split_and_several():
    splits = {c.name: c.launch_form()[1] for c in R.WGRAD_PATCH}
    assert min(splits.values()) == 1 and max(splits.values()) >= 3, splits


# ---- the exact-arithmetic references and case tables of tests/test_hip_fused_exact.py -----------------------------------------------------------------------
DT16 = ("f16", "bf16")


def test_fused_reference_helpers():
    assert R.pow2_scales(5).tolist() == [0.5, 0.25, 0.5, 0.25, 0.5]
    v = R.nonzero_ints(3, "nz", (4096,))
    assert bool((v != 0).all()) and float(v.min()) == -8 and float(v.max()) == 8 and bool((R.negative_ints(3, "ng", (512,)) < 0).all())
    assert R.exact_in_fp32_steps(torch.tensor([0.25 * (2 ** 24 - 1)]), 0.25)
    for bad, step in ((torch.tensor([0.25 * 2 ** 24]), 0.25), (torch.tensor([0.125]), 0.25), (torch.tensor([1.0]), 0.3)):
        with pytest.raises(AssertionError):
            R.exact_in_fp32_steps(bad, step)
    # bf16 keeps 8 bits: 257 -> 256 (a tie, to even, TOWARDS zero), 259 -> 260 (a tie away from zero), 258.5 -> 258 (no tie), 256 stays
    share, ties = R.rounding_stats(torch.tensor([257.0, 259.0, 258.5, 256.0], dtype=D), "bf16")
    assert share == 0.75 and ties == 1
    assert R.rounding_stats(torch.tensor([2049.0, 2051.0, 2048.5, 3.0], dtype=D), "f16") == (0.75, 1)      # 2048.5 is not on the f16 grid, not a tie either
    y = torch.arange(2 * 3 * 5 * 2 * 2, dtype=D).reshape(2, 3, 5, 2, 2)
    assert torch.equal(R.pair_max_t(y), y[:, :, [1, 3]]) and R.upsample2x_nchw(y).shape == (2, 3, 5, 4, 4)
    assert torch.equal(R.upsample2x_nchw(y)[0, 0, 0], torch.tensor([[0.0, 0, 1, 1], [0, 0, 1, 1], [2, 2, 3, 3], [2, 2, 3, 3]], dtype=D))
    assert torch.equal(R.max_pool_ref64(y, (1, 2, 2), (1, 2, 2))[..., 0, 0], y[..., 1, 1])
    assert R.bn_is_telling(R.pow2_scales(8), R.nonzero_ints(3, "b", (8,)))
    for s, b in ((torch.ones(8), torch.ones(8)), (R.pow2_scales(8) * 3, torch.ones(8)), (R.pow2_scales(8), torch.zeros(8)), (R.pow2_scales(8), torch.full((8,), 0.5))):
        with pytest.raises(AssertionError):
            R.bn_is_telling(s, b)


def test_chain_and_dual_references_vs_explicit_taps():
    """chain_ref64 against the tap-by-tap conv with the rounding done by hand; dual_ref64 against two such convs; the step of each stage."""
    x = R.small_ints(5, "cx", (2, 6, 2, 5, 6), lo=-8, hi=8, density=1.0)
    w1, w2 = R.small_ints(5, "cw1", (4, 6, 1, 3, 3), lo=-16, hi=16, density=1.0), R.small_ints(5, "cw2", (6, 4, 1, 1, 1))
    s1, b1, s2, b2 = R.pow2_scales(4), R.nonzero_ints(5, "cb1", (4,)), R.pow2_scales(6), R.nonzero_ints(5, "cb2", (6,))
    st = R.chain_ref64(x, [(w1, R.ONE, R.P011, s1, b1, None, True), (w2, R.ONE, R.P0, s2, b2, x, True)], "bf16")
    ch = lambda v: v.view(1, -1, 1, 1, 1)
    m = (_conv_taps(x, w1, (1, 1, 1), (0, 1, 1), (0, 1, 1)) * ch(s1) + ch(b1)).clamp_min(0)
    assert torch.equal(st[0]["raw"], m) and st[0]["step"] == 0.25 and st[1]["step"] == 0.0625
    m16 = m.to(torch.bfloat16).to(D)
    assert not torch.equal(m16, m) and torch.equal(st[0]["y"], m16)
    out = (_conv_taps(m16, w2, (1, 1, 1), (0, 0, 0), (0, 0, 0)) * ch(s2) + ch(b2) + x).clamp_min(0)
    assert torch.equal(st[1]["raw"], out) and torch.equal(st[1]["y"], out.to(torch.bfloat16).to(D))
    assert torch.equal(st[1]["abs"], _conv_taps(m16, w2.abs(), (1, 1, 1), (0, 0, 0), (0, 0, 0)) * ch(s2) + ch(b2.abs()) + x.abs())
    fp = R.chain_ref64(x, [(w1, R.ONE, R.P011, s1, b1, None, False)], "bf16", fp32_out=True)[0]
    assert torch.equal(fp["y"], fp["raw"]) and bool((fp["y"] < 0).any()) and not fp["stored16"]
    x2 = R.small_ints(5, "cx2", (2, 4, 2, 9, 11))
    wd = R.small_ints(5, "cwd", (4, 4, 1, 1, 1))
    raw, a = R.dual_ref64(x, w1[:, :, :, 1:2, 1:2], s1, b1, x2, wd, s1.flip(0), b1, stride2=2, relu=True)
    want = _conv_taps(x, w1[:, :, :, 1:2, 1:2], (1, 1, 1), (0, 0, 0), (0, 0, 0)) * ch(s1) + ch(b1) + _conv_taps(x2[:, :, :, ::2, ::2], wd, (1, 1, 1), (0, 0, 0), (0, 0, 0)) * ch(s1.flip(0)) + ch(b1)
    assert torch.equal(raw, want.clamp_min(0)) and bool((a >= want.abs()).all())


def _table_rounds(results, table_name):
    """Condition 4 over a table: for each type, a case whose every intermediate is rounded (>= 1 %, ties to even towards zero among them)."""
    for dt in DT16:
        assert any(ok for d, ok in results if d == dt), "%s: no %s case rounds every intermediate" % (table_name, dt)


def _mix_promise(mix, stats, dt, n_inter):
    ok = all(R.rounding_happens(stats, i) for i in range(n_inter))
    assert ok or dt not in mix.rounds
    return ok


def test_bneck_frame_case_table_meets_the_conditions():
    assert [(c.temporal, c.n, c.t) for c in R.BNECK_FRAME_CASES] == [(False, 1, 3), (False, 3, 2), (True, 2, 2), (True, 1, 2)]
    results = []
    for c in R.BNECK_FRAME_CASES:
        x, ws, bn = c.tensors()
        assert all(R.bn_is_telling(s, b) for s, b in bn) and float(x.abs().max()) == c.mix.x_hi and torch.equal(x, x.round())
        for dt in DT16:
            stats = R.fused_conditions(R.chain_ref64(x, c.stages(x, ws, bn), dt), dt, "bneck_frame " + c.name, c.mix)
            results.append((dt, _mix_promise(c.mix, stats, dt, 2)))
    _table_rounds(results, "BNECK_FRAME_CASES")


@pytest.mark.parametrize("table", ["BNECK_TAIL64_CASES", "BNECK_TAIL128_CASES"])
def test_bneck_tail_case_tables_meet_the_conditions(table):
    cases = getattr(R, table)
    want = [(2, 3, 7, 9), (1, 1, 16, 16), (3, 6, 9, 11), (1, 2, 20, 55)] if table.endswith("64_CASES") else [(2, 3, 7, 9), (1, 1, 16, 16), (4, 2, 14, 30)]
    assert [c.dims for c in cases] == want
    forms, results = set(), []
    for c in cases:
        d = c.tensors()
        assert R.bn_is_telling(d["s2"], d["b2"]) and R.bn_is_telling(d["s3"], d["b3"]) and bool((d["res"] != 0).all())
        if c.cmid == 64:
            assert R.bn_is_telling(d["sd"], d["bd"]) and not torch.equal(d["sd"], d["s3"])
        forms |= set(c.forms)
        for dt in DT16:
            for form, st in c.reference(d, dt).items():
                stats = R.fused_conditions(st, dt, "bneck_tail %s %s" % (c.name, form), c.mix)
                results.append((dt, _mix_promise(c.mix, stats, dt, 1)))
    assert forms == ({"residual", "dual", "pool"} if table.endswith("64_CASES") else {"residual"})
    _table_rounds(results, table)


def test_unetpp_tail_case_table_meets_the_conditions():
    assert [(c.h, c.w) for c in R.UPP_TAIL_CASES[:4]] == [(16, 16), (18, 34), (48, 80), (2, 2)] and R.UPP_TAIL_CASES[2].n == 3
    assert R.UPP_TAIL_CASES[0].npatch == 1 and all(c.npatch > 2 * 256 for c in R.UPP_TAIL_CASES if c.walk) and any(c.walk for c in R.UPP_TAIL_CASES)
    results = []
    for c in R.UPP_TAIL_CASES:
        d = c.tensors()
        assert R.bn_is_telling(d["s1"], d["b1"]) and R.bn_is_telling(d["s2"], d["b2"]) and R.bn_is_telling(None, d["bias"])
        for dt in DT16:
            st = c.reference(d, dt)
            assert tuple(st[2]["y"].shape) == (c.n, 3, 1, c.h, c.w) and not st[2]["stored16"]
            stats = R.fused_conditions(st, dt, "unetpp_tail " + c.name, c.mix)
            results.append((dt, _mix_promise(c.mix, stats, dt, 2)))
    _table_rounds(results, "UPP_TAIL_CASES")


@pytest.mark.parametrize("fn,table", [("tpair_reference", "TPAIR_CASES"), ("dual_reference", "DUAL_CASES"), ("dual_p8_reference", "DUAL_P8_CASES"),
                                      ("pool_t2_reference", "POOL_T2_CASES"), ("stem_reference", "STEM_CASES")])
def test_single_stage_case_tables_meet_the_conditions(fn, table):
    """No 16-bit intermediate: conditions 1, 2, 3 and 5 on every stage, the pair max and the pooled stem output included."""
    for c in getattr(R, table):
        for dt in DT16:
            d, st = getattr(R, fn)(c, dt)
            R.fused_conditions(st, dt, "%s %s" % (table, c))
            assert all(x["relu"] for x in st)
            for s, b in (("s", "b"), ("s1", "b1"), ("s2", "b2")):
                if s in d:
                    assert R.bn_is_telling(d[s], d[b])


# ---- the forward conv under every tile configuration: the case table of tests/test_hip_conv_fwd_exact.py ------------------------------------------------------------
@pytest.mark.parametrize("dtype", R.BOTH)
@pytest.mark.parametrize("fc", R.FWD_CASES, ids=[c.name for c in R.FWD_CASES])
def test_fwd_case_table_meets_the_conditions(fc, dtype):
    """Conditions 1-3 and bn_is_telling on every row; every (input channel, tap) of every row has a non-zero weight, so a dropped tap shows; every 'big' row really
    rounds in bf16 (>= 1 % of its stores changed, exact ties resolved towards zero among them), rows t3_2048_512, 3x3_256_256, k333_64_192 and 3x3_64_40_res in f16 too."""
    d, ref = R.fwd_reference(fc, dtype)
    assert R.bn_is_telling(d["s"], d["b"])
    stats = R.fused_conditions(ref, dtype, "fwd " + fc.name)
    assert bool((d["w"] != 0).any(0).all()), "a tap of an input channel has no weight"
    assert fc.big == ("bf16" in fc.rounds) and set(fc.rounds) <= set(R.BOTH)
    if dtype in fc.rounds:
        assert R.rounding_happens(stats, 0), (fc.name, dtype, stats)
    assert (fc.residual, d["res"] is not None) in ((True, True), (False, False))
    if fc.stem:
        R.fwd_stats_reference(fc, d)            # the gate on the statistics' absolute sums and on |z| < 4096 steps


def test_fwd_rows_that_must_round_in_f16_too():
    both = sorted(c.name for c in R.FWD_CASES if c.rounds == R.BOTH)
    assert both == sorted(["t3_2048_512", "3x3_256_256", "k333_64_192", "3x3_64_40_res"])
    assert sorted(c.name for c in R.FWD_CASES if c.big) == sorted(both + ["t3_T2_128_512_res", "k333_144_288"])


@pytest.mark.parametrize("dtype", R.BOTH)
@pytest.mark.parametrize("row", R.GATHER_FWD_CASES, ids=[R.gather_conv_case(r).name for r in R.GATHER_FWD_CASES])
def test_gather_fwd_case_table_meets_the_conditions(row, dtype):
    d, ref = R.gather_fwd_reference(row, dtype)
    assert R.bn_is_telling(d["s"], d["b"])
    R.fused_conditions(ref, dtype, "fwd " + R.gather_conv_case(row).name)
    assert bool((d["w"] != 0).any(0).all())
    assert all(v.shape[1] % 64 == 0 for v in d["srcs"]) and d["srcs"][0].shape[3:] == (row[0][2] // 2, row[0][3] // 2)


def test_fwd_accepts_covers_every_live_tile_and_every_refusing_branch():
    """From the predicate alone: every id in 1 .. NUM_TILE_CFGS other than the retired ones is accepted by at least two rows of different kernel shape or stride
    class -- tiles 19, 38 and 40, whose launchers admit a single (kernel, stride), by at least two rows of different channels or frame size --, the retired ids
    by none, and every refusing clause of the restated rule is hit by a row; the clauses no row of the table can reach (the LDS and halo limits need frames wider
    than any here) by a geometry of their own, on the predicate only."""
    rows = [c.conv for c in R.FWD_CASES]
    assert R.NUM_TILE_CFGS == 40 and len(R.LIVE_CFGS) == 36
    hit = set()
    for cfg in range(1, R.NUM_TILE_CFGS + 1):
        took = [c for c in rows if R.fwd_accepts(cfg, c)]
        for c in rows:
            hit.update(R.fwd_refusals(cfg, c))
        if cfg in R.RETIRED_CFGS:
            assert not took
            continue
        classes = {(c.k, c.stride) for c in took}
        if cfg in R.SINGLE_CLASS_TILES:
            assert classes == {R.SINGLE_CLASS_TILES[cfg]} and len({(c.cin, c.cout, c.dims) for c in took}) >= 2, (cfg, [c.name for c in took])
        else:
            assert len(classes) >= 2, (cfg, [c.name for c in took])
    by_rows = {"retired", "generic:cin%64", "generic:kpad>1024", "stem:cin!=8", "stem:cout>64", "stem:sw!=1", "pw:geometry", "p8:cin%64", "p8:nk<2", "p8:cout%256",
               "flat:geometry", "flat:cout>64", "temporal:geometry", "temporal:T>4", "temporal:cout", "patch:geometry", "patch2:geometry", "patch3:cout"}
    assert by_rows <= hit, sorted(by_rows - hit)
    # the extras' clauses: on rows of the table
    stem, e33, pw = (R.case_by_name(rows, n) for n in ("stem_large", "e_3x3_64_64", "e_1x1_64_128"))
    px = stem.out[0] * stem.out[1] * stem.out[2]
    for cfg, c, extras, clause in ((9, stem, ("mask",), "stem:extras"), (30, stem, ("y32",), "stem:extras"), (20, stem, (("stats_rows", px + 256),), "stem:stats_rows"),
                                   (5, stem, (("stats_rows", 128),), "stats_rows<256"), (19, pw, ("stats",), "pw:extras"), (27, e33, ("mask",), "flat:extras"),
                                   (32, e33, ("ostrided",), "patch:extras"), (38, e33, ("ostrided",), "patch2:extras"), (5, e33, ("gathered",), "gathered:tile"),
                                   (40, e33, ("gathered",), "patch3:gathered"), (28, R.case_by_name(rows, "t3_T4_256_64"), ("y32",), "temporal:extras"),
                                   (25, R.case_by_name(rows, "3x3_256_256"), ("stats",), "p8:extras"),
                                   (32, R.case_by_name(rows, "k333_64_192"), ("gathered",), "gathered:geometry")):
        assert R.fwd_refusals(cfg, c, extras) == [clause], (cfg, c.name, extras, R.fwd_refusals(cfg, c, extras))
    for cfg in (9, 20, 29):
        assert R.fwd_accepts(cfg, stem, ("stats",)) and R.fwd_accepts(cfg, stem, (("stats_rows", px),))
    for cfg in (5, 32, 38, 40):
        assert R.fwd_accepts(cfg, e33, ("mask", "y32", "stats"))
    # the limits no row reaches: a frame 64 wide leaves the flat chunk-major tile's 384-position halo, one 415 wide the flat tile's LDS; a stem with a stride of 7 along h the stem halo's
    assert R.fwd_refusals(33, R.ConvCase("wide", (1, 1, 4, 64), 64, 64, (1, 3, 3))) == ["patch:halo>384"] and R.fwd_accepts(33, R.ConvCase("w62", (1, 1, 4, 62), 64, 64, (1, 3, 3)))
    assert R.fwd_refusals(27, R.ConvCase("wider", (1, 1, 2, 415), 64, 64, (1, 3, 3))) == ["flat:lds"] and R.fwd_accepts(27, R.ConvCase("w414", (1, 1, 2, 414), 64, 64, (1, 3, 3)))
    assert R.fwd_refusals(20, R.ConvCase("stem_s7", (1, 16, 64, 64), 3, 64, (7, 7, 7), (2, 7, 2), pf=(3, 3, 3), pair_w=3)) == ["stem:lds"]
    # the head / tail split: a 128-wide tile with a sibling splits cout = 136 and 288, not 208 (r = 80) nor anything under a tile without one
    c136, c288, c208 = (R.case_by_name(rows, n) for n in ("pw_64_136_res", "k333_144_288", "k333_96_208_res"))
    assert all(R.fwd_is_split(cfg, c136) for cfg in R.NARROW_SIBLING) and not R.fwd_is_split(5, c136) and not R.fwd_is_split(19, c136)
    assert [cfg for cfg in R.LIVE_CFGS if R.fwd_is_split(cfg, c288) and R.fwd_accepts(cfg, c288)] == [1, 3, 11, 13, 22, 24]       # 6: Kpad > 1024; 18, 23, 35, 36: cin % 64
    assert not any(R.fwd_is_split(cfg, c208) for cfg in R.LIVE_CFGS)
    # the ambiguous one, settled from the kernel (conv_igemm_kernel, KS = 2: each wave set multiplies its half of the k16 sub-steps of EVERY K tile, the first included)
    assert all(R.fwd_accepts(cfg, c136) for cfg in R.SPLIT_K_TILES) and R.FwdGeo(c136).nk == 1


# ---- the inference max-pool forms and the clip layouts -------------------------------------------------------------------------------------------------------
IP_IDS = [c.name for c in R.INFER_POOL_CASES]
_ip_refs = {}


def ip_refs(case):
    if case.name not in _ip_refs:
        x = case.x()
        _ip_refs[case.name] = (x, R.maxpool_infer_ref(x, case.k, case.s, case.pf, case.out, False), R.maxpool_infer_ref(x, case.k, case.s, case.pf, case.out, True))
    return _ip_refs[case.name]


@pytest.mark.parametrize("case", R.INFER_POOL_CASES, ids=IP_IDS)
def test_infer_pool_ref_vs_torch_and_the_input_conditions(case):
    x, skip, zero = ip_refs(case)
    pad = [v for f, b in zip(reversed(case.pf), reversed(case.pb)) for v in (f, b)]          # F.pad: last dimension first
    for ref, fill in ((skip, float("-inf")), (zero, 0.0)):
        want = F.max_pool3d(F.pad(x.permute(0, 4, 1, 2, 3), pad, value=fill), case.k, case.s).permute(0, 2, 3, 4, 1)
        assert tuple(want.shape[1:4]) == case.out and torch.equal(ref, want)
    assert float(x.min()) >= -1.125 and float(x.max()) <= 0.125 and torch.equal(x * 64, torch.round(x * 64))
    assert torch.equal(x.to(torch.float16).to(D), x) and torch.equal(x.to(torch.bfloat16).to(D), x)
    assert x.numel() < 4096 or 0.85 < float((x < 0).double().mean()) < 0.93          # 72 of the 81 values
    border = R.pool_border(case.thw, case.k, case.s, case.pf, case.out)
    assert torch.equal(skip[:, ~border], zero[:, ~border]), "zero padding changed an interior output"
    if int(border.sum()) * case.n * case.c >= 100:
        differ = float((skip[:, border] != zero[:, border]).double().mean())
        positive = float((skip > 0).double().mean())
        assert differ >= 0.10 and positive >= 0.25, (differ, positive)


def test_infer_pool_table_reaches_every_form_and_solver_branch():
    forms = {c.name: R.maxpool_form(c.desc()) for c in R.INFER_POOL_CASES}
    for c in R.INFER_POOL_CASES:
        assert forms[c.name][0] == c.form, (c.name, forms[c.name])
        assert R.maxpool_form(c.desc(), idx=True) == ("idx",)
        assert R.maxpool_form(c.desc(), no_lds=True)[0] == ("generic" if c.form == "generic" else "walk")
        assert c.n >= 2 and c.n * c.thw[0] * c.thw[1] * c.thw[2] * c.c * 2 < 64 << 20
    lds = [(c, forms[c.name][1]) for c in R.INFER_POOL_CASES if c.form == "lds"]
    C8 = lambda c: c.c // 8
    assert any(g["CG"] >= 32 for _, g in lds)                                                                  # (a) CG doubled at least twice
    assert any(g["CG"] < 8 and g["CG"] == C8(c) for c, g in lds) and any(C8(c) == 1 and c.thw[2] > 32 for c, g in lds)         # (b)
    assert any(g["rp_host"] == 1 and g["bands"] >= 3 and g["last_band_rows"] < g["HB"] for _, g in lds)       # (c)
    assert any(g["rp_host"] >= 2 and g["bands"] >= 2 for _, g in lds)                                          # (d)
    d = [g for c, g in lds if c.thw[1:] == (30, 9)]
    assert d and all(g["HB"] == 24 for g in d)
    ragged = [g for c, g in lds if C8(c) % g["CG"] and g["rp_last_group"] != g["rp_host"]]
    assert len(ragged) >= 3 and any(g["live_last_group"] < 256 for g in ragged) and any(g["live_last_group"] == 256 for g in ragged)          # (e)
    assert any(c.thw[2] == 32 and C8(c) >= 8 for c, _ in lds)                                                  # (f)
    assert any(c.thw[2] == 33 and C8(c) >= 8 and c.form == "walk" for c in R.INFER_POOL_CASES)                # (g)
    assert {c.thw[0] for c, g in lds if g["bands"] >= 2} >= {1, 2, 3, 4}                                       # (h)
    assert max(g["lds_bytes"] for _, g in lds) == 147456          # the largest request the solver can make and be granted (see below)
    walk = [(c, forms[c.name][1]) for c in R.INFER_POOL_CASES if c.form == "walk"]
    assert len({g["seglen"] for _, g in walk}) >= 3 and any(g["seglen"] > 4 and g["segs"] * g["seglen"] - c.thw[2] >= g["seglen"] for c, g in walk)      # ... a run that starts past the row
    assert any(c.thw[1] % 2 == 1 and c.thw[1] > 1 for c, _ in walk) and any(c.thw[1] == 1 for c, _ in walk)
    assert any(c.thw[2] % g["segs"] for c, g in walk) and any(c.thw[2] % g["segs"] == 0 for c, g in walk)
    assert any(g["refused"] == ["lds"] for _, g in walk) and any("rp" in g["refused"] for _, g in walk)
    assert len({g["seglen"] for c in R.INFER_POOL_CASES if c.form == "lds" for g in [R.maxpool_form(c.desc(), no_lds=True)[1]]}) >= 3          # the child process's walk
    gen = {(c.k, c.s, c.pf, c.pb) for c in R.INFER_POOL_CASES if c.form == "generic"}
    assert {((2, 3, 3), (2, 2, 2), (0, 0, 0), (0, 0, 0)), ((2, 1, 1), (2, 1, 1), (0, 0, 0), (0, 0, 0)), ((1, 3, 3), (1, 2, 2), (0, 0, 0), (0, 1, 1)),
            ((3, 3, 3), (2, 2, 2), (0, 0, 0), (1, 1, 1)), ((2, 2, 2), (2, 2, 2), (0, 0, 0), (0, 1, 1)), ((1, 2, 2), (1, 2, 2), (0, 0, 0), (0, 0, 0))} <= gen
    assert any(c.k == (3, 3, 3) and c.s == (1, 1, 1) and c.pf[0] == 0 and c.out == c.thw for c in R.INFER_POOL_CASES if c.form == "generic")


def test_infer_pool_solver_clauses_no_shape_can_refuse():
    """Of the LDS form's `fits` test, over every frame up to 64 x 300 and every channel count: the row budgets and `hb >= 4 || hb == h` never refuse once
    rp >= 1 (the shrink loop ends at hb = min(h, 8 rp) >= 8 or h), and the 150 KB bound refuses only frames of width 1 with CG = 128 (16 rows, 1024 channels
    and up), which the table has. A seglen above 4 needs rows * segs >= 2^19 at more than 4 columns per run: 2^24 elements or more (H = 1; the table's one such row)."""
    from types import SimpleNamespace
    refused = set()
    for h in range(1, 65):
        for w in range(1, 301):
            for C8 in (1, 2, 3, 5, 8, 9, 16, 17, 32, 64, 128, 129, 256):
                d = SimpleNamespace(n=2, t=2, h=h, w=w, c=8 * C8, ldx=8 * C8, ldy=8 * C8, kt=3, kh=3, kw=3, st=1, sh=1, sw=1, pt=1, ph=1, pw=1, to=2, ho=h, wo=w)
                f = R.maxpool_form(d)
                if f[0] == "walk":
                    r = f[1]["refused"]
                    refused.add((("rp",), 0) if "rp" in r else (tuple(r), w))          # without a row per pass (W * CG > 256) the other clauses say nothing
                    assert f[1]["seglen"] <= 4 or d.n * d.t * h * w * d.c >= 1 << 24
    assert refused == {(("rp",), 0), (("lds",), 1)}, refused


@pytest.mark.parametrize("name", R.INFER_POOL_SPECIAL)
def test_infer_pool_special_values_hold_every_class(name):
    case = R.case_by_name(R.INFER_POOL_CASES, name)
    x = R.special_values(case.x())
    skip, zero = (R.maxpool_infer_ref(x, case.k, case.s, case.pf, case.out, pz) for pz in (False, True))
    has_nan = R.maxpool_infer_ref(torch.isnan(x).to(D), case.k, case.s, case.pf, case.out, False) > 0
    nan_s, nan_z = int(torch.isnan(skip).sum()), int(torch.isnan(zero).sum())
    assert nan_s > nan_z >= 1                                   # windows of NaNs alone: NaN, but 0 where zero padding reaches them
    assert bool((zero[torch.isnan(skip) & ~torch.isnan(zero)] == 0).all())
    assert int((has_nan & torch.isfinite(skip)).sum()) >= 100        # NaNs beside numbers are dropped
    ninf_s, ninf_z = int((skip == float("-inf")).sum()), int((zero == float("-inf")).sum())
    assert ninf_s > ninf_z >= 1 and int((skip == float("inf")).sum()) >= 2 and torch.equal(skip == float("inf"), zero == float("inf"))


def test_layout_table_and_reference():
    rows = {c.name: c for c in R.LAYOUT_CASES}
    assert len(rows) == len(R.LAYOUT_CASES)
    for c in R.LAYOUT_CASES:
        ch, w, strides, pm = c.geometry()
        assert R.clip_layout_form(ch, w, c.cpad, strides, pm) == c.form, (c.name, c.refusals())
        assert ch <= c.cpad and (c.cpad == 8 or w % 2 == 0)
    for cpad in (4, 8):
        sub = [c for c in R.LAYOUT_CASES if c.cpad == cpad]
        for form in ("w8", "generic"):
            assert {c.geometry()[0] for c in sub if c.form == form} >= {1, 2, 3, 4}, (cpad, form)
        assert {c.geometry()[1] for c in sub if c.form == "w8"} >= {8, 72}
        assert any(c.geometry()[2] != torch.empty(c.sl[0][1], c.sl[1][1], c.sl[2][1], c.sl[3][1], c.sl[4][1]).stride() for c in sub if c.form == "w8")
    assert {c.geometry()[0] for c in R.LAYOUT_CASES if c.cpad == 8 and c.form == "generic"} >= {5, 8}
    alone = {tuple(c.refusals()) for c in R.LAYOUT_CASES}
    assert {("sw",), ("w8",), ("ptr",), ("stride",), ("c",)} <= alone                  # each refusing clause of the dispatch, by itself
    x = synth_tensor(73, "lay", (2, 3, 2, 3, 4)).to(D)
    for cpad in (4, 8):
        y = R.clip_layout_ref(x, cpad)
        assert y.shape == (2, 2, 3, 4, cpad) and float(y[..., 3:].abs().max()) == 0.0
        for ch in range(3):
            assert torch.equal(y[..., ch], x[:, ch])
        assert torch.equal(y.reshape(2, 2, 3, 2, 2 * cpad)[..., cpad:cpad + 3], x.permute(0, 2, 3, 4, 1)[:, :, :, 1::2])        # cpad 4: the pair's second pixel


# ---- the weight-image references of tests/test_hip_pack_exact.py ------------------------------------------------------------------------------------------------
PACK_SEED = 3
PACK_IDS = [c.name for c in R.PACK_CASES]


@pytest.mark.parametrize("dtype", R.BOTH)
def test_round16_bits_equals_torchs_conversion(dtype):
    """round16_bits (numpy float16 / integer arithmetic on the fp32 bits) against torch's fp32 -> 16-bit cast: random values over the whole range of the type,
    every planted value, every tie of a binade, subnormals and both zeros."""
    u = synth_tensor(7, "r16", (200000,), -1, 1).numpy().astype(np.float32)
    e = synth_tensor(7, "r16e", (200000,), -30, 15.9).numpy()
    step = 2.0 ** -11 if dtype == "f16" else 2.0 ** -8
    ties = (1.0 + step * np.arange(1, 2 ** 12, 2)).astype(np.float32)
    v = np.concatenate([u, (u * 2.0 ** e).astype(np.float32), R.PACK_PLANTS, -R.PACK_PLANTS, ties, -ties, np.array([0.0, -0.0, 65504.0, -65504.0], dtype=np.float32)])
    t = torch.from_numpy(v)
    want = (t.clamp(-R.F16_MAX, R.F16_MAX) if dtype == "f16" else t).to(R.TDT[dtype]).view(torch.int16).numpy()
    assert np.array_equal(R.round16_bits(v, dtype), want)
    assert np.array_equal(R._once_from_exact(v.astype(np.float64), dtype), want)        # an fp32 value rounded "from exact" is the same single rounding


def _host_packed(w5, case, dtype):
    from ted_spad_amd import engine as E
    return E.PackedConv(torch.from_numpy(w5), None, None, stride=case.stride, dtype=dtype, device="cpu", pair_w=case.pair_w)


@pytest.mark.parametrize("dtype", R.BOTH)
@pytest.mark.parametrize("case", R.PACK_CASES, ids=PACK_IDS)
def test_pack_fwd_image_equals_the_host_packing(case, dtype):
    """pack_image_ref mode 0 == the bits of engine.PackedConv(..., device="cpu").w (torch permute / stem_pair_form, written independently), padded as the library
    pads, with weights that round (ties, subnormals, -0.0). The host packing neither takes a scale nor saturates f16: it gets the fp32 product, clamped to +-65504."""
    w, s = R.pack_weights(case.shape, PACK_SEED)
    for scale in (None, s):
        p = w if scale is None else w * scale.reshape(-1, 1, 1, 1, 1)
        pc = _host_packed(np.clip(p, -R.F16_MAX, R.F16_MAX) if dtype == "f16" else p, case, dtype)
        a = case.pack_args(0)
        assert (pc.cpad, pc.kpad) == (a["rows_pad"], a["kpad"]) and (pc.cin, pc.k) == (case.cink, case.k_k)
        img = R.pack_image_ref(w, scale, dtype=dtype, **a)
        assert img.shape == (pc.cpad, pc.kpad) and img.dtype == np.int16
        assert np.array_equal(img, pc.w.view(torch.int16).numpy())


@pytest.mark.parametrize("dtype", R.BOTH)
@pytest.mark.parametrize("case", R.PACK_CASES, ids=PACK_IDS)
def test_pack_dgrad_image_equals_the_flipped_transposed_forward_image(case, dtype):
    """pack_image_ref mode 1 against a second formulation: the parity class (ct, ch, cw) of strides (st, sh, sw) is the kernel-form weight sub-sampled
    [ct::st, ch::sh, cw::sw], its three tap axes flipped and co exchanged with ci -- whose FORWARD image over co8 channels is the data-gradient image
    (stride 1: the textbook flipped, transposed kernel). The per-co scale is multiplied in first (one fp32 multiply either way)."""
    from ted_spad_amd import engine as E
    w, s = R.pack_weights(case.shape, PACK_SEED)
    classes = case.classes()
    assert sorted(g[0] * g[1] * g[2] for g in classes) == sorted(case.class_taps)
    assert sum(g[0] * g[1] * g[2] for g in classes) == case.k_k[0] * case.k_k[1] * case.k_k[2]            # every kernel-form tap in exactly one class
    for scale in (None, s):
        p = w if scale is None else w * scale.reshape(-1, 1, 1, 1, 1)
        wkf = E.stem_pair_form(torch.from_numpy(p), case.pair_w)[0].numpy() if case.pair_w is not None else p
        for geo in classes:
            Et, Eh, Ew, ct, ch, cw, st, sh, sw = geo
            sub = np.ascontiguousarray(wkf[:, :, ct::st, ch::sh, cw::sw][:, :, ::-1, ::-1, ::-1].swapaxes(0, 1))
            assert sub.shape[2:] == (Et, Eh, Ew)
            a = case.pack_args(1, geo)
            want = R.pack_image_ref(sub, None, cink=case.co8, kwk=Ew, pair_shift=-1, mode=0, rows=sub.shape[0], rows_pad=a["rows_pad"], kpad=a["kpad"], geo=None, dtype=dtype)
            assert np.array_equal(R.pack_image_ref(w, scale, dtype=dtype, **a), want), geo


@pytest.mark.parametrize("case", R.PACK_CASES, ids=PACK_IDS)
def test_pack_cases_take_the_path_named_in_their_row(case):
    """pk_plan_ref per case: LDS tiles or pack_body, rows / channels per tile, more tiles than a job's 256 workgroups, chunks of the last co tile."""
    a = case.pack_args(0)
    q = case.plan(0)
    assert (q.tiled, q.per_tile, q.tiled and q.tiles > R.PK_MAX_BLOCKS) == case.fwd
    assert q.blocks(a["rows_pad"], a["kpad"]) == (min(q.tiles, 256) if q.tiled else min(256, (a["rows_pad"] * a["kpad"] // 8 + 1023) // 1024))
    for geo in case.classes():
        q = case.plan(1, geo)
        assert (q.tiled, q.per_tile, q.tiled and q.tiles > R.PK_MAX_BLOCKS) == case.dgrad
        if q.tiled:
            assert (case.co8 - 1) % 64 // 8 + 1 == case.last_chunks
            a = case.pack_args(1, geo)
            assert a["kpad"] >= geo[0] * geo[1] * geo[2] * case.co8 and a["rows_pad"] > a["rows"]             # rows above `rows` exist: the tiles' zero rows are checked


def test_pack_table_reaches_every_branch_of_the_plan():
    by = {c.name: c for c in R.PACK_CASES}
    co, ci, kt, kh, kw = by["longest_tiled_row"].shape
    assert ci * kt * kh * kw == R.PK_FLOATS - 1 and ci % 8 != 0
    co, ci, kt, kh, kw = by["row_too_long"].shape
    assert R.PK_FLOATS < ci * kt * kh * kw <= R.PK_FLOATS + 8
    co, ci, kt, kh, kw = by[R.PACK_BIG].shape
    assert ci * kt * kh * kw > R.PK_FWD_FLOATS and by[R.PACK_BIG].plan(0).blocks(*by[R.PACK_BIG].image_dims(0)[1:]) == 256
    assert {c.fwd for c in R.PACK_CASES} >= {R.BODY, (True, 1, True), (True, 1, False), (True, 64, True), (True, 64, False), (True, 11, False)}
    assert {c.dgrad for c in R.PACK_CASES} >= {R.BODY, (True, 8, False), (True, 8, True), (True, 16, False), (True, 32, False), (True, 32, True)}
    assert any(c.dgrad == R.BODY and c.pair_w is None for c in R.PACK_CASES) and any(c.pair_w is not None for c in R.PACK_CASES)
    assert {c.last_chunks for c in R.PACK_CASES if c.co8 > 64} >= {1, 2, 4, 6}                             # a last co tile with fewer than 8 chunks
    assert any(c.dgrad[0] and c.shape[1] < c.dgrad[1] for c in R.PACK_CASES)                                # ci below the channels of one tile
    assert any(c.dgrad[0] and c.shape[1] % c.dgrad[1] and c.shape[1] > c.dgrad[1] for c in R.PACK_CASES)    # a last channel tile partly filled
    assert [R.find_job_rounds(n) for n in R.FIND_JOB_SIZES] == [0, 1, 1, 1, 2, 2, 2, 3]


@pytest.mark.parametrize("dtype", R.BOTH)
def test_pack_weights_hold_every_rounding_ingredient(dtype):
    """Per case, with and without the scale: a tie above an even and above an odd mantissa, an f16-subnormal value, -0.0, a value above 65504, nothing non-finite.
    A product w * scale whose fp32 rounding changes the 16-bit result (a pack that rounded once would differ) needs ~2^13 (f16) / 2^16 (bf16) products to occur:
    asserted for the largest case, which both entry points and the find_job tables pack."""
    for case in R.PACK_CASES:
        w, s = R.pack_weights(case.shape, PACK_SEED)
        assert bool(np.isfinite(w).all() and np.isfinite(s).all()) and int((s == 1).sum()) >= 2 and int((s < 0).sum()) >= 1
        for scale in (None, s):
            got = R.rounding_ingredients(w, scale, dtype)
            for key in ("tie_even", "tie_odd", "f16_subnormal", "neg_zero", "above_f16_max"):
                assert got[key] >= 1, (case.name, key)
            assert (got["double_rounding"] == 0) if scale is None else (got["double_rounding"] >= 1 or case.name != R.PACK_BIG), case.name
    # the planted ties round as round-to-nearest-even says, and differently under truncation or round-half-up
    tie = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}[dtype]
    v = np.array([1 + tie, 1 + 3 * tie], dtype=np.float32)
    assert np.array_equal(R.round16_bits(v, dtype), R.round16_bits(np.array([1.0, 1 + 4 * tie], dtype=np.float32), dtype))
    big = R.round16_bits(np.array([70000.0, 65520.0], dtype=np.float32), dtype).view(np.uint16)
    assert list(big) == ([0x7BFF, 0x7BFF] if dtype == "f16" else [0x4789, 0x4780])


def test_fold_and_unpack_refs_equal_the_host_formulas():
    """fold_ref64 == engine.fold_bn's host branch (torch float64), bit for bit after the fp32 rounding; wgrad_unpack_ref == the view ConvLayer.flush_grad takes."""
    from ted_spad_amd import engine as E
    for C in R.FOLD_C:
        g, be, m, v, cb = R.fold_inputs(C, 11)
        assert int((g < 0).sum()) >= (C > 1) and int((v == 0).sum()) >= 1
        for bias in (None, cb):
            for eps in (1e-5, 1e-3):
                sc, sh = R.fold_ref64(g, be, m, v, eps, bias)
                ts, tb = E.fold_bn(*(torch.from_numpy(t) for t in (g, be, m, v)), eps, conv_bias=None if bias is None else torch.from_numpy(bias))
                assert np.array_equal(sc.astype(np.float32), ts.numpy()) and np.array_equal(sh.astype(np.float32), tb.numpy())
                assert bool((np.abs(sh.astype(np.float32).astype(np.float64) - sh) <= R.fold_shift_bound(sh, be, m, sc, bias)).all())
    sc, sh = R.fold_ref64(None, None, None, None, 0.0, cb)
    assert np.array_equal(sc, np.ones(len(cb))) and np.array_equal(sh, cb.astype(np.float64))
    sc, sh = R.fold_ref64(None, None, None, None, 0.0, None, n=5)
    assert np.array_equal(sc, np.ones(5)) and np.array_equal(sh, np.zeros(5))
    assert list(R.ulp32(np.array([1.0, 1.5, 2.0, 0.75, 0.0, 1e-46]))) == [2.0 ** -23, 2.0 ** -23, 2.0 ** -22, 2.0 ** -24, 2.0 ** -149, 2.0 ** -149]
    co, ci, k, cink = 5, 3, (1, 3, 3), 8
    kpad = 128
    dw = torch.from_numpy(R.small_ints(13, "dwp", (128, kpad), -8, 8, density=1.0).numpy().astype(np.float32))
    rs = np.array([0.5, 2.0, 1.0, 4.0, 0.25])
    view = dw[:co, :9 * cink].view(co, 1, 3, 3, cink).permute(0, 4, 1, 2, 3)[:, :ci] * torch.from_numpy(rs).float().view(-1, 1, 1, 1, 1)
    g0 = np.arange(co * ci * 9, dtype=np.float64).reshape(co, ci, 1, 3, 3)
    assert np.array_equal(R.wgrad_unpack_ref(dw.numpy(), co, ci, k, cink, kpad, rs, g0), view.double().numpy() + g0)


# ---- the MGFN references and their per-element bounds (tests/test_hip_mgfn_edges.py) -------------------------------------------------------------------------
# (a) every reference equals float64 torch (autograd / F.conv1d / F.layer_norm / nn.BatchNorm1d / softmax attention); (b) torch's own fp32 evaluation of the same
# operation stays inside every bound, and each deliberately wrong reference leaves it in at least one element. Where a kernel is handed fp32 statistics, the fp32
# evaluation is handed the same ones.
U = R.U
F32T = torch.float32


def inside(got, ref_bound, what):
    ref, bound = ref_bound
    msg = R.worst(got, ref, bound)
    assert not msg, "%s: %s" % (what, msg)


def outside(wrong_value, ref_bound, what):
    ref, bound = ref_bound
    assert R.worst(wrong_value, ref, bound), "%s: the wrong reference stays inside the bound" % what


def not_vacuous(ref_bound, what, rel=1e-3):
    """a bound far above fp32 rounding would accept anything: no element's bound exceeds rel * (the tensor's largest magnitude + 1)"""
    ref, bound = ref_bound
    assert float(bound.max()) <= rel * (float(ref.abs().max()) + 1.0), (what, float(bound.max()), float(ref.abs().max()))


def test_mgfn_transcendental_constants():
    """The worst per-element ratio |fp32 - float64| / (2^-24 |float64|) of torch's CPU expf, erff, logf, sqrtf on the same fp32 inputs (2 M points each);
    measured 1.04 (exp on [-80, 80]), 1.05 (erf on [-6, 6] and on [-1e-3, 1e-3]), 1.03 (log on [1, 1e4]), 1.07 (sqrt). K_* = 11 >= 10x each."""
    g = torch.Generator().manual_seed(0)
    x = torch.rand(2000000, generator=g) * 2 - 1

    def ratio(f, v):
        a, b = f(v).double(), f(v.double())
        return float(((a - b).abs() / (b.abs() * U))[b != 0].max())
    got = {"exp": ratio(torch.exp, x * 80), "erf": max(ratio(torch.erf, x * 6), ratio(torch.erf, x * 1e-3)), "log": ratio(torch.log, 1 + x.abs() * 1e4),
           "sqrt": ratio(torch.sqrt, x.abs() * 1e3 + 1e-6)}
    print(got)
    for name, K in (("exp", R.K_EXP), ("erf", R.K_ERF), ("log", R.K_LOG), ("sqrt", R.K_SQRT)):
        assert 0.5 <= got[name] and 10 * got[name] <= K <= 15 * got[name], (name, got[name], K)


_conv_tokens = R.mgfn_conv_tokens


@pytest.mark.parametrize("taps,cin", R.MGFN_GEMM_TAPS_CIN)
@pytest.mark.parametrize("M", [65, 257])
def test_mgfn_gemm_ref(M, taps, cin):
    N = 64
    off, bounds = R.mgfn_ragged(R.gemm_lengths(M))
    tag = "%d_%d_%d" % (M, taps, cin)
    x = synth_tensor(41, "gx" + tag, (M, cin), -2, 2)
    w3 = synth_tensor(41, "gw" + tag, (N, taps, cin), -1, 1) / (taps * cin) ** 0.5
    bias, res = synth_tensor(41, "gb" + tag, (N,), -0.5, 0.5), synth_tensor(41, "gr" + tag, (M, N), -1, 1)
    for gelu, with_res, with_bias in ((0, 0, 0), (1, 1, 1), (0, 1, 1), (1, 0, 0)):
        def run(dt):
            y = _conv_tokens(x.to(dt), off, w3.to(dt), bias.to(dt) if with_bias else None, taps)
            y = F.gelu(y) if gelu else y
            return y + res.to(dt) if with_res else y
        rb = R.mgfn_gemm_ref(x, bounds, taps, w3.reshape(N, -1), bias if with_bias else None, gelu, res if with_res else None)
        assert close(rb[0], run(D))
        inside(run(F32T), rb, "gemm " + tag)
        not_vacuous(rb, "gemm " + tag)
        if taps > 1:
            for wrong in ("leak", "reversed"):
                outside(R.mgfn_gemm_ref(x, bounds, taps, w3.reshape(N, -1), bias if with_bias else None, gelu, res if with_res else None, wrong=wrong)[0], rb, wrong)
    if taps == 1:                                                       # the LayerNorm prologue (MGFN flavour), statistics handed in fp32
        mu, var = x.mean(1), x.var(1, unbiased=False)
        st32 = torch.stack([mu, 1 / (var.sqrt() + 1e-5)], 1)
        xd = x.to(D)
        st64 = torch.stack([xd.mean(1), 1 / (xd.var(1, unbiased=False).sqrt() + 1e-5)], 1)
        want = _conv_tokens((xd - st64[:, :1]) * st64[:, 1:], off, w3.to(D), bias.to(D), 1)
        assert close(R.mgfn_gemm_ref(x, None, 1, w3.reshape(N, -1), bias, stats=st64)[0], want)
        rb = R.mgfn_gemm_ref(x, None, 1, w3.reshape(N, -1), bias, True, res, stats=st32)
        inside(F.gelu(_conv_tokens((x - st32[:, :1]) * st32[:, 1:], off, w3, bias, 1)) + res, rb, "gemm ln " + tag)
        not_vacuous(rb, "gemm ln " + tag)


_attention_torch = R.mgfn_attention_torch


@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("scale", [2.0, 25.0], ids=["plain", "logits200"])
def test_mgfn_attention_refs(heads, scale):
    off, _ = R.mgfn_ragged(R.MGFN_ATT_LENGTHS)
    M, inner = off[-1], 64 * heads
    qkv = synth_tensor(42, "att%d" % heads, (M, 3 * inner), -1, 1)
    qkv[:, :2 * inner] *= scale                                         # 25: |q . k| / 8 up to 64 * 625 / 8, logits of a few hundred
    do = synth_tensor(42, "attdo%d" % heads, (M, inner), -1, 1)
    o64, g64 = _attention_torch(qkv, off, heads, D, do)
    o32, g32 = _attention_torch(qkv, off, heads, F32T, do)
    fwd = R.mgfn_attention_ref(qkv, off, heads)
    assert close(fwd[0], o64)
    inside(o32, fwd, "attention")
    not_vacuous(fwd, "attention", 1e-2 if scale > 2 else 1e-3)
    bwd, lse = R.mgfn_attention_bwd_ref(qkv, o64, do, off, heads)
    assert close(bwd[0], g64, 1e-10) and bool(torch.isfinite(bwd[1]).all()) and bool(torch.isfinite(lse[1]).all())
    inside(g32, bwd, "attention bwd")
    not_vacuous(bwd, "attention bwd", 0.05 if scale > 2 else 1e-3)
    if scale == 2.0:
        off33, _ = R.mgfn_ragged([33])
        q33 = qkv[:33]
        rb = R.mgfn_attention_ref(q33, off33, heads)
        outside(R.mgfn_attention_ref(q33, off33, heads, wrong="drop_block")[0], rb, "a key block dropped for T = 33")
        outside(R.mgfn_attention_ref(qkv, off, heads, wrong="no_scale")[0], fwd, "a softmax without the 1/8 scale")


@pytest.mark.parametrize("heads,C", [(1, 64), (3, 192), (16, 1024)])
def test_mgfn_relpos_refs(heads, C):
    lengths = [1, 2, 3, 4, 5, 6, 110, 7]
    off, bounds = R.mgfn_ragged(lengths)
    M = off[-1]
    v, do = synth_tensor(43, "rpv%d" % heads, (M, C), -1, 1), synth_tensor(43, "rpd%d" % heads, (M, C), -1, 1)
    w, b = synth_tensor(43, "rpw%d" % heads, (heads, 5), -1, 1), synth_tensor(43, "rpb%d" % heads, (heads,), -0.5, 0.5)

    run = lambda dt: R.mgfn_relpos_torch(v, w, b, off, heads, dt, do)          # noqa: E731
    y64, dv64, dw64, db64 = run(D)
    y32, dv32, dw32, db32 = run(F32T)
    fwd = R.mgfn_relpos_ref(v, bounds, heads, w, b)
    rdv, rdw, rdb = R.mgfn_relpos_bwd_ref(do, v, bounds, heads, w)
    assert close(fwd[0], y64) and close(rdv[0], dv64) and close(rdw[0], dw64, 1e-10) and close(rdb[0], db64, 1e-10)
    for got, rb, what in ((y32, fwd, "relpos"), (dv32, rdv, "relpos dv"), (dw32, rdw, "relpos dw"), (db32, rdb, "relpos db")):
        inside(got, rb, what)
        not_vacuous(rb, what, 1e-2 if what[-2:] in ("dw", "db") else 1e-3)          # dw, db: thousands of terms of mixed sign behind a small sum
    outside(R.mgfn_relpos_ref(v, bounds, heads, w, b, wrong="leak")[0], fwd, "a tap read across a sequence end")
    if heads > 1:
        outside(R.mgfn_relpos_ref(v, bounds, heads, w, b, wrong="head_block")[0], fwd, "the filter of head ch / (C / heads)")


def _hard_rows(x):
    """row 1 (where there is one): 1000 + noise of 1e-2; row 2: constant 3"""
    if x.shape[0] > 2:
        x[1] = 1000.0 + 0.01 * x[1]
        x[2] = 3.0
    return x


@pytest.mark.parametrize("torch_ln", [0, 1])
@pytest.mark.parametrize("C", R.MGFN_ROW_C)
def test_mgfn_layernorm_refs(C, torch_ln):
    M, eps = 5, 1e-5
    x = _hard_rows(synth_tensor(44, "lnx%d" % C, (M, C), -3, 5))
    g, b = synth_tensor(44, "lng%d" % C, (C,), 0.5, 1.5), synth_tensor(44, "lnb%d" % C, (C,), -0.5, 0.5)
    dy, add = synth_tensor(44, "lnd%d" % C, (M, C), -1, 1), synth_tensor(44, "lna%d" % C, (M, C), -1, 1)
    xd = x.to(D)
    mu, rs, dmu, drs = R.mgfn_ln_stats_ref(x, eps, torch_ln)
    e32 = R.f32(eps)
    var = xd.var(1, unbiased=False)
    assert close(mu, xd.mean(1)) and close(rs, 1 / (var + e32).sqrt() if torch_ln else 1 / (var.sqrt() + e32))
    assert float(rs[2]) == (1 / e32 ** 0.5 if torch_ln else 1 / e32)                       # the constant row
    mu32, var32 = x.mean(1), x.var(1, unbiased=False)
    rs32 = 1 / (var32 + eps).sqrt() if torch_ln else 1 / (var32.sqrt() + eps)
    inside(mu32, (mu, dmu), "ln mean")
    inside(rs32, (rs, drs), "ln rs")
    # plain rows: 1e-5 of rs; 1000 + 1e-2 noise: a few per cent; the constant row: nothing says that a sum of equal values is exact, so the MGFN flavour's
    # bound there is dmean against eps (the GPU test asserts the exact value instead)
    assert bool((drs[[0, 3, 4]] <= 1e-5 * rs[[0, 3, 4]]).all()) and float(drs[1]) <= 0.05 * float(rs[1]) and (not torch_ln or float(drs[2]) <= 1e-5 * float(rs[2]))
    onepass = (xd * xd).mean(1).float().double() - mu32.double() ** 2                                      # E[x^2] - mean^2 with one fp32 rounding of E[x^2]
    bad = 1 / (onepass.clamp_min(0) + e32).sqrt() if torch_ln else 1 / (onepass.clamp_min(0).sqrt() + e32)
    assert abs(float(bad[1] - rs[1])) > float(drs[1]), "a one-pass variance meets the bound of the 1000 + noise row"
    outside(1 / (var + e32).sqrt() if not torch_ln else 1 / (var.sqrt() + e32), (rs, drs), "sqrt(var + eps) in place of std + eps")
    # apply and backward, statistics handed in fp32
    keep = [0, 1, 3, 4] if not torch_ln else [0, 1, 2, 3, 4]                                               # MGFN flavour: the constant row divides by zero
    st64, st32 = torch.stack([mu, rs], 1), torch.stack([mu32, rs32], 1)
    xa = xd.clone().requires_grad_()
    if torch_ln:
        ya = F.layer_norm(xa, (C,), g.to(D), b.to(D), e32)
    else:
        ma = xa.mean(1, keepdim=True)
        ya = (xa - ma) / (((xa - ma) ** 2).mean(1, keepdim=True).sqrt() + e32) * g.to(D) + b.to(D)
    (ya * dy.to(D)).sum().backward()
    y = R.mgfn_ln_apply_ref(x, st64, g, b)
    dx = R.mgfn_ln_bwd_ref(dy, x, st64, g, torch_ln, eps, add)
    plain = [0, 3, 4]                              # torch's own float64 LayerNorm loses digits on the 1000 + noise row (its variance cancels): 1e-5 there
    assert close(y[0][plain], ya.detach()[plain]) and close(y[0][1], ya.detach()[1], 1e-5)
    assert close((dx[0] - add.to(D))[plain], xa.grad[plain], 1e-9) and close((dx[0] - add.to(D))[1], xa.grad[1], 1e-4)
    assert torch.equal(y[0][2], b.to(D)), "constant row: y == b"
    y = R.mgfn_ln_apply_ref(x, st32, g, b)
    inside((x - st32[:, :1]) * st32[:, 1:] * g + b, y, "ln apply")
    dx = R.mgfn_ln_bwd_ref(dy, x, st32, g, torch_ln, eps, add)
    d32, xh32 = dy * g, (x - st32[:, :1]) * st32[:, 1:]
    k32 = st32[:, 1:] if torch_ln else 1 / (1 / st32[:, 1:] - eps)
    got = (d32 - d32.mean(1, keepdim=True)) * st32[:, 1:] - xh32 * ((d32 * xh32).mean(1, keepdim=True) * k32) + add
    inside(got[keep], (dx[0][keep], dx[1][keep]), "ln bwd")
    not_vacuous((dx[0][[0, 3, 4]], dx[1][[0, 3, 4]]), "ln bwd")
    if torch_ln:
        assert bool(torch.isfinite(dx[0]).all()) and bool(torch.isfinite(dx[1]).all())


@pytest.mark.parametrize("M", [2, 129])
@pytest.mark.parametrize("C", [4, 260])
def test_mgfn_batchnorm_refs(M, C):
    eps, mom = 1e-5, 0.1
    x = synth_tensor(45, "bnx%d_%d" % (M, C), (M, C), -3, 5)
    x[:, 1] = 2.5                                                       # a constant channel
    g, b = synth_tensor(45, "bng", (C,), 0.5, 1.5), synth_tensor(45, "bnb", (C,), -0.2, 0.2)
    rm, rv = synth_tensor(45, "bnrm", (C,), -0.1, 0.1), synth_tensor(45, "bnrv", (C,), 0.5, 1.5)
    dy, add = synth_tensor(45, "bndy%d" % M, (M, C), -1, 1), synth_tensor(45, "bnad%d" % M, (M, C), -1, 1)

    def run(dt):
        bn = torch.nn.BatchNorm1d(C, eps=R.f32(eps), momentum=R.f32(mom)).to(dt).train()
        with torch.no_grad():
            bn.weight.copy_(g), bn.bias.copy_(b), bn.running_mean.copy_(rm), bn.running_var.copy_(rv)
        xa = x.to(dt).clone().requires_grad_()
        y = bn(xa)
        (y * dy.to(dt)).sum().backward()
        return y.detach(), bn.running_mean, bn.running_var, xa.grad, bn.weight.grad, bn.bias.grad
    t64, t32 = run(D), run(F32T)
    f = R.mgfn_bn_fwd_ref(x, g, b, eps, mom, rm, rv)
    xd = x.to(D)
    assert close(f["y"][0], t64[0]) and close(f["running_mean"][0], t64[1]) and close(f["running_var"][0], t64[2])
    assert close(f["mean"][0], xd.mean(0)) and close(f["invstd"][0], 1 / (xd.var(0, unbiased=False) + R.f32(eps)).sqrt())
    for key, got in (("y", t32[0]), ("running_mean", t32[1]), ("running_var", t32[2])):
        inside(got, f[key], "bn " + key)
        cols = f["invstd"][0] < 10                 # not the constant channel (nor, at M = 2, two close values): an invstd of up to 316 multiplies the error of the mean
        assert int(cols.sum()) >= C // 2 and not bool(cols[1])
        not_vacuous((f[key][0][..., cols], f[key][1][..., cols]), "bn " + key)
    outside(R.mgfn_bn_fwd_ref(x, g, b, eps, mom, rm, rv, wrong="biased_running_var")["running_var"][0], f["running_var"], "a biased running_var")
    assert R.mgfn_bn_fwd_ref(x, g, b, eps, mom)["running_var"] is None
    one = R.mgfn_bn_fwd_ref(x[:1], g, b, eps, mom, rm, rv)               # M = 1: the biased variance, 0
    assert close(one["running_var"][0], (1 - R.f32(mom)) * rv.to(D)) and close(one["y"][0], b.to(D).expand(1, C))
    stat64 = torch.cat([f["mean"][0], f["invstd"][0]])
    bw = R.mgfn_bn_bwd_ref(dy, x, stat64, g, add)
    assert float((bw["dx"][0] - add.to(D) - t64[3]).abs().max()) <= 1e-9 * float(t64[3].abs().max() + 1)
    assert float((bw["dgamma"][0] - t64[4]).abs().max()) <= 1e-9 * float(t64[4].abs().max() + 1) and close(bw["dbeta"][0], t64[5])
    mean32 = x.mean(0)
    stat32 = torch.cat([mean32, 1 / (x.var(0, unbiased=False) + eps).sqrt()])
    bw = R.mgfn_bn_bwd_ref(dy, x, stat32, g, add)
    xh = (x - stat32[:C]) * stat32[C:]
    dbe, dga = dy.sum(0), (dy * xh).sum(0)
    inside(dbe, bw["dbeta"], "bn dbeta")
    inside(dga, bw["dgamma"], "bn dgamma")
    inside(g * stat32[C:] * (dy - dbe / M - xh * dga / M) + add, bw["dx"], "bn dx")
    not_vacuous(bw["dx"], "bn dx", 1e-2)                                 # the constant channel: invstd = 316, the bound grows with it


@pytest.mark.parametrize("C", R.MGFN_ROW_C)
def test_mgfn_head_refs(C):
    M, eps = 5, 1e-5
    x = _hard_rows(synth_tensor(46, "hx%d" % C, (M, C), -3, 5))
    lw, lb = synth_tensor(46, "hlw%d" % C, (C,), 0.5, 1.5), synth_tensor(46, "hlb%d" % C, (C,), -0.1, 0.1)
    fw = synth_tensor(46, "hfw%d" % C, (C,), -0.5, 0.5)
    dsc, dh = synth_tensor(46, "hds%d" % C, (M,), -1, 1), synth_tensor(46, "hdh%d" % C, (M, C), -1, 1)
    for fb in (0.05, 100.0, -100.0):
        def run(dt):
            h = F.layer_norm(x.to(dt), (C,), lw.to(dt), lb.to(dt), R.f32(eps)).requires_grad_()
            z = h @ fw.to(dt) + R.f32(fb)
            s = torch.sigmoid(z)
            (s * dsc.to(dt)).sum().backward()
            return h.detach(), z.detach(), s.detach(), h.detach().norm(dim=1), h.grad
        t64, t32 = run(D), run(F32T)
        r = R.mgfn_head_ref(x, lw, lb, fw, fb, eps)
        for i, key in enumerate(("h", "logit", "score", "mag")):
            assert close(r[key][0], t64[i]), key
            inside(t32[i], r[key], "head " + key)
        not_vacuous((r["h"][0][[0, 3, 4]], r["h"][1][[0, 3, 4]]), "head h")
        (o64, _), (z64, _) = R.mgfn_head_bwd_ref(t64[2], dsc, fw, dh)
        assert float((o64 - dh.to(D) - t64[4]).abs().max()) <= 1e-12
        if abs(fb) == 100.0 and C > 4:             # saturated: float64 gives exactly 1, or a value below the smallest normal fp32 (the kernel's expf overflows: exactly 0)
            assert bool(((r["score"][0] == 1.0) | (r["score"][0] < R.FLOOR32)).all())
        ob, zb = R.mgfn_head_bwd_ref(t32[2], dsc, fw, dh)
        z32 = dsc * t32[2] * (1 - t32[2])
        inside(z32, zb, "head_bwd dz")
        inside(dh + fw * z32[:, None], ob, "head_bwd dh")
        not_vacuous(ob, "head_bwd dh")


def test_mgfn_gelu_refs():
    hard = torch.tensor([0.0, -0.0, 2.0 ** -140, -2.0 ** -140, 1e-3, -1e-3, 0.7, -0.7, 3, -3, 6, -6, 10, -10, 40, -40], dtype=F32T)
    x = torch.cat([hard, synth_tensor(47, "gelux", (1012,), -6, 6)])
    dy = synth_tensor(47, "geludy", (1028,), -1, 1)

    def run(dt):
        xa = x.to(dt).clone().requires_grad_()
        y = F.gelu(xa)
        (y * dy.to(dt)).sum().backward()
        return y.detach(), xa.grad
    t64, t32 = run(D), run(F32T)
    y, dx = R.mgfn_gelu_ref(x), R.mgfn_gelu_bwd_ref(x, dy)
    assert close(y[0], t64[0]) and close(dx[0], t64[1])
    inside(t32[0], y, "gelu")
    # backward: the formula in fp32 torch ops (torch.erf, torch.exp: the functions the constants were measured on). torch's own fp32 GELU backward on the CPU
    # uses a vectorised erf with an ABSOLUTE error of a few 2^-24 (5.4 * 2^-24 of the result at x = 0.006), which no relative constant describes
    xf = x.clone()
    inside(dy * (0.5 * (1 + torch.erf(xf * 0.70710678118654752440)) + xf * 0.39894228040143267794 * torch.exp(-0.5 * xf * xf)), dx, "gelu bwd")
    assert float((t32[1].double() - dx[0]).abs().max()) <= 8 * U
    not_vacuous(y, "gelu", 1e-5)
    not_vacuous(dx, "gelu bwd", 1e-5)
    assert float(y[0][15]) == 0.0 and bool(torch.signbit(y[0][15])) and float(y[0][12]) == 10.0 and float(y[0][14]) == 40.0       # the tails float64 rounds to 0 / x
    assert float(dx[0][15]) == 0.0 and float(dx[0][14]) == float(dy[14])


def test_mgfn_reduction_refs():
    C = 65
    for M in (127, 129, 385):
        a, x = synth_tensor(48, "cra%d" % M, (M, C), -1, 1), synth_tensor(48, "crx%d" % M, (M, C), -3, 5)
        st_row = torch.stack([x.mean(1), 1 / (x.var(1, unbiased=False) + 1e-5).sqrt()], 1)
        st_col = torch.cat([x.mean(0), 1 / (x.var(0, unbiased=False) + 1e-5).sqrt()])
        rowf = synth_tensor(48, "crr%d" % M, (M,), -1, 1)
        cases = {0: (None, None), 1: (x, st_row), 2: (x, st_col), 3: (None, st_col), 4: (None, rowf)}
        for mode, (xx, st) in cases.items():
            for dt in (D, F32T):
                ad = a.to(dt)
                if mode == 0:
                    o0, o1 = ad.sum(0), torch.zeros(C, dtype=dt)
                elif mode == 1:
                    o0, o1 = ad.sum(0), (ad * ((xx.to(dt) - st[:, :1].to(dt)) * st[:, 1:].to(dt))).sum(0)
                elif mode == 2:
                    o0, o1 = ad.sum(0), (ad * ((xx.to(dt) - st[:C].to(dt)) * st[C:].to(dt))).sum(0)
                elif mode == 3:
                    o0, o1 = ((ad - st[:C].to(dt)) ** 2).sum(0), torch.zeros(C, dtype=dt)
                else:
                    o0, o1 = (st.to(dt)[:, None] * ad).sum(0), st.to(dt).sum().expand(C)
                r0, r1 = R.mgfn_col_reduce_ref(a, mode, 0.5, xx, st)
                if dt == D:
                    assert float((r0[0] - 0.5 * o0).abs().max()) <= 1e-12 * M and float((r1[0] - 0.5 * o1).abs().max()) <= 1e-12 * M
                else:
                    inside(0.5 * o0, r0, "col_reduce mode %d out0" % mode)
                    inside(0.5 * o1, r1, "col_reduce mode %d out1" % mode)
                    assert float(r0[1].max()) <= 1e-3 * M and float(r1[1].max()) <= 1e-3 * M
            if M % R.MT_CHUNK:
                w0, w1 = R.mgfn_col_reduce_ref(a, mode, 0.5, xx, st, wrong="skip_last_chunk")
                outside(w0[0], r0, "a column reduction that skips the last partial chunk (mode %d)" % mode)
        m0, _ = R.mgfn_col_reduce_ref(a, 3, 1.0, None, None)
        assert torch.equal(m0[0], R.mgfn_col_reduce_ref(a, 0, 1.0)[0][0])          # mode 3 with st == NULL is mode 0
    sc = synth_tensor(48, "cm", (10 * (1 + 256 + 257),), 0, 1)
    seg = [0, 1, 257, 514]
    cm = R.mgfn_crop_mean_ref(sc, seg, 10)
    want = torch.cat([sc[10 * seg[v]:10 * seg[v + 1]].view(10, -1).to(D).mean(0) for v in range(3)])
    assert close(cm[0], want)
    inside(torch.cat([sc[10 * seg[v]:10 * seg[v + 1]].view(10, -1).mean(0) for v in range(3)]), cm, "crop_mean")
    not_vacuous(cm, "crop_mean", 1e-5)


@pytest.mark.parametrize("M", [17, 129, 300])
def test_mgfn_transpose_and_wgrad_refs(M):
    taps, C, N = 3, 16, 64
    lengths = R.gemm_lengths(M)
    off, bounds = R.mgfn_ragged(lengths)
    ldk = (M + 15) // 16 * 16
    x, dy = synth_tensor(49, "wgx%d" % M, (M, C), -2, 2), synth_tensor(49, "wgd%d" % M, (M, N), -1, 1)
    at, dyt = R.mgfn_transpose_ref(x, bounds, taps, ldk), R.mgfn_transpose_ref(dy, None, 1, ldk)
    assert at.shape == (taps * C, ldk) and float(at[:, M:].abs().max() if ldk > M else 0) == 0 and torch.equal(dyt[:, :M], dy.to(D).t())
    for m in (0, M // 2, M - 1):
        for t in range(taps):
            src = m + t - 1
            want = x[src].to(D) if bounds[m, 0] <= src < bounds[m, 1] else torch.zeros(C, dtype=D)
            assert torch.equal(at[t * C:(t + 1) * C, m], want)
    w = torch.zeros((N, taps, C), dtype=D, requires_grad=True)
    (_conv_tokens(x.to(D), off, w, None, taps) * dy.to(D)).sum().backward()
    rb = R.mgfn_wgrad_ref(at, dyt)
    assert close(rb[0], w.grad.reshape(N, taps * C).t(), 1e-10)
    inside(at.float() @ dyt.float().t(), rb, "wgrad")
    not_vacuous(rb, "wgrad")
    assert R.mgfn_wgrad_slices(ldk, taps * C, N)[1] == (1 if M <= 128 else 2 if M == 129 else 3)


# ---- the fp32 head, BCE and vote kernels: the conditions of tests/test_hip_head_exact.py and its sensitivity, on the references alone --------------------------
def _lin_ep(scale, shift, sc, sh):
    return (scale if sc else None), (shift if sh else None)


def test_linear_table_reaches_every_form():
    """Every row reaches the kernel it names, and the table reaches every kernel on both of its paths (a later change of the launcher's thresholds cannot
    silently empty one); the boundaries the dispatch turns on are all present, from both sides."""
    seen = set()
    for form, B, K, N in R.LINEAR_CASES:
        got = R.linear_form(B, K, N)
        assert got[0] == form, (form, B, K, N, got)
        seen.add(got)
    assert seen == R.LINEAR_FORMS, seen ^ R.LINEAR_FORMS
    shapes = {c[1:] for c in R.LINEAR_CASES}
    assert len(shapes) == len(R.LINEAR_CASES)
    assert {B for B, _, _ in shapes} >= {1, 8, 9, 16, 17, 63, 64, 65} and {K for _, K, _ in shapes} >= {16, 17, 32, 33, 255, 256}
    assert any(B >= 64 and B % 32 for B, K, N in shapes if K <= 32) and {N for B, K, N in shapes if K <= 32 and B >= 64} >= {255, 256, 257}
    assert R.linear_form(63, 16, 9)[0] == R.linear_form(64, 33, 9)[0] == R.linear_form(17, 256, 5)[0] == R.linear_form(16, 255, 5)[0] == "wave"
    assert R.linear_chain(8, 2048, 3) == 38 and R.linear_chain(8, 2050, 3) == 39 and R.linear_chain(64, 24, 3) == 24


@pytest.mark.parametrize("form,B,K,N", R.LINEAR_CASES)
def test_linear_exact_inputs_meet_the_conditions(form, B, K, N):
    """Ranges; sum |x||w| an integer below 2^24 (so is every partial sum, in any order; the epilogue's grid of 2^-2 keeps it exact); telling scales and
    shifts; no pre-activation exactly 0 under any epilogue; the reference equals float64 torch. The ReLU's share of zeros: per row with 16 outputs or more
    between 20 % and 80 % (fewer outputs cannot hold a share: they count in the table's total, below)."""
    x, w, scale, shift = R.linear_exact_inputs(B, K, N)
    assert float(x.abs().max()) <= 8 and float(w.abs().max()) <= 4 and bool((x == x.round()).all()) and bool((w == w.round()).all())
    assert R.bn_is_telling(scale, shift) and (N == 1 or float(scale.min()) < float(scale.max()))
    for sc, sh, relu in R.LINEAR_EPILOGUES:
        s, b = _lin_ep(scale, shift, sc, sh)
        r = R.linear_ref(x, w, s, b, relu)
        assert R.exact_in_fp32(r["abs"]) and R.exact_in_fp32(r["abs"] + 3.0)
        assert torch.equal(r["y"].float().to(D), r["y"]) and bool((r["pre"] * 4 == (r["pre"] * 4).round()).all())
        assert bool((r["pre"] != 0).all())
        want = F.linear(x, w * (s[:, None] if sc else 1.0), b)
        assert torch.equal(r["y"], F.relu(want) if relu else want)
        if relu and B * N >= 16:
            zero = float((r["y"] == 0).double().mean())
            assert 0.2 <= zero <= 0.8, (sc, sh, zero)


def test_linear_relu_share_over_the_table_and_mutants_are_caught():
    """Over the whole table the ReLU zeroes 20 .. 80 % of the outputs under every epilogue; every wrong kernel of LINEAR_WRONG is unequal to the exact reference
    on at least one row (and the rows that catch it are printed)."""
    zero, total = {}, {}
    caught = {m: [] for m in R.LINEAR_WRONG}
    for form, B, K, N in R.LINEAR_CASES:
        x, w, scale, shift = R.linear_exact_inputs(B, K, N)
        for sc, sh, relu in R.LINEAR_EPILOGUES:
            s, b = _lin_ep(scale, shift, sc, sh)
            y = R.linear_ref(x, w, s, b, relu)["y"]
            if relu:
                zero[sc, sh] = zero.get((sc, sh), 0) + int((y == 0).sum())
                total[sc, sh] = total.get((sc, sh), 0) + y.numel()
            for m in R.LINEAR_WRONG:
                if not torch.equal(R.linear_ref(x, w, s, b, relu, wrong=m)["y"], y):
                    caught[m].append((B, K, N, sc, sh, relu))
    for k in zero:
        assert 0.2 <= zero[k] / total[k] <= 0.8, (k, zero[k] / total[k])
    for m, rows in caught.items():
        print(m, len(rows))
        assert rows, "%s equals the reference on every row" % m
        assert len({r[:3] for r in rows}) >= 10, (m, "caught on few shapes only")


@pytest.mark.parametrize("form,B,K,N", R.LINEAR_CASES)
def test_linear_real_bound_holds_torch_fp32_and_rejects_the_mutants(form, B, K, N):
    x, w, scale, shift = R.linear_real_inputs(B, K, N)
    assert x.dtype == w.dtype == scale.dtype == shift.dtype == F32T
    chain = R.linear_chain(B, K, N)
    for sc, sh, relu in ((1, 1, 1), (0, 1, 0)):
        s, b = _lin_ep(scale, shift, sc, sh)
        r = R.linear_ref(x, w, s, b, relu, chain=chain)
        want = F.linear(x.to(D), w.to(D)) * (s.to(D) if sc else 1.0) + b.to(D)
        assert close(r["y"], F.relu(want) if relu else want)
        v32 = F.linear(x, w) * (s if sc else 1.0) + b
        inside(F.relu(v32) if relu else v32, (r["y"], r["bound"]), "linear")
        not_vacuous((r["y"], r["bound"]), "linear", 1e-4)
        for m in R.LINEAR_WRONG:
            moved = not torch.equal(R.linear_ref(x, w, s, b, relu, wrong=m)["y"], r["y"])
            if moved:
                outside(R.linear_ref(x, w, s, b, relu, wrong=m)["y"], (r["y"], r["bound"]), m)


def _bce_autograd(f, W, bias, y, gs):
    f, W, bias = (t.to(D).clone().requires_grad_() for t in (f, W, bias))
    z = f @ W.t() + bias
    loss = F.binary_cross_entropy_with_logits(z, y.to(D))
    (loss * gs).backward()
    return z.detach(), loss.detach(), f.grad, W.grad, bias.grad


def _representable(t):
    return torch.equal(t.float().to(D), t)


@pytest.mark.parametrize("B,K,N", R.BCE_CASES)
def test_bce_exact_inputs_meet_the_conditions(B, K, N):
    """The logits are 0 or at least 40 in magnitude, all three classes present where there are 16 logits; the kernel's formulas in torch's fp32 give g exactly
    (the float64 g is its own fp32 rounding to 2^-50); df, dW, db are fp32 numbers; at least 30 % of df and of dW are non-zero; the reference equals float64
    autograd where sigmoid is not saturated beyond float64 (everywhere: 1e-12)."""
    assert (B * N) & (B * N - 1) == 0 and K % 4 == 0 and B <= 128 and N <= 64
    f, W, bias, y = R.bce_exact_inputs(B, K, N)
    assert bool((W % 40 == 0).all()) and bool((f == f.round()).all()) and set(bias.tolist()) <= {0.0, 40.0, -40.0} and set(y.flatten().tolist()) <= {0.25, 0.5, 1.0}
    r = R.bce_head_ref(f, W, bias, y, R.BCE_EXACT_SCALE)
    z = r["logits"][0]
    n, only = R.bce_logit_classes(z)
    assert only and (B * N < 16 or min(n) >= 1), n
    assert R.exact_in_fp32(f.abs() @ W.abs().t() + bias.abs())
    g = r["g"][0]
    g32 = R.bce_kernel_g32(z, y).to(D)
    assert float((g - g32).abs().max()) <= 2.0 ** -50 and float((g - g.float().to(D)).abs().max()) <= 2.0 ** -50
    gd = g32                                                               # the dyadic g: sums of its products are exact in float64 too
    df, dW, db = R.BCE_EXACT_SCALE * (gd @ W), R.BCE_EXACT_SCALE * (gd.t() @ f), R.BCE_EXACT_SCALE * gd.sum(0)
    for name, v in (("df", df), ("dW", dW), ("db", db)):
        assert _representable(v), name
        assert torch.equal(r[name][0].float().to(D), v), name               # what the GPU test compares with: the reference, rounded to fp32, IS the dyadic value
        unit = 2.0 ** -2 / (B * N)                                          # every term is a multiple of this; the sum of the magnitudes in units of it stays below 2^24
    assert R.exact_in_fp32((gd.abs() @ W.abs()) / unit) and R.exact_in_fp32((gd.abs().t() @ f.abs()) / unit) and R.exact_in_fp32(gd.abs().sum(0) / unit)
    assert float((df != 0).double().mean()) >= 0.3 and float((dW != 0).double().mean()) >= 0.3, (float((df != 0).double().mean()), float((dW != 0).double().mean()))
    assert bool((g32 != 0).any())
    za, la, dfa, dWa, dba = _bce_autograd(f, W, bias, y, R.BCE_EXACT_SCALE)
    assert torch.equal(za, z) and close(r["loss"][0], la.reshape(1)) and close(r["df"][0], dfa, 1e-10) and close(r["dW"][0], dWa, 1e-10) and close(r["db"][0], dba, 1e-10)


@pytest.mark.parametrize("B,K,N", R.BCE_CASES)
def test_bce_dense_bounds_hold_torch_fp32(B, K, N):
    """The dense table: integer logits that are exact in fp32, |z| from 0 to beyond 80 over the table, targets inside (0, 1); the reference equals float64
    autograd, torch's fp32 evaluation of the same formulas lies inside every bound, no bound is vacuous."""
    f, W, bias, y = R.bce_dense_inputs(B, K, N)
    assert R.exact_in_fp32(f.abs() @ W.abs().t() + bias.abs()) and _representable(y)
    assert bool((f[f != 0] % 40 != 0).all()) and bool((W[W != 0] % 40 != 0).all()) and float((f != 0).double().mean()) > 0.5
    for k0 in range(0, K, 256):                                             # every workgroup's slice of columns holds weights: no df / dW slice is all zeros
        assert bool((W[:, k0:k0 + 256] != 0).any()) and bool((f[:, k0:k0 + 256] != 0).any())
    gs = R.BCE_DENSE_SCALE
    r = R.bce_head_ref(f, W, bias, y, gs)
    z = r["logits"][0]
    za, la, dfa, dWa, dba = _bce_autograd(f, W, bias, y, gs)
    assert torch.equal(za, z) and close(r["loss"][0], la.reshape(1)) and close(r["df"][0], dfa, 1e-10) and close(r["dW"][0], dWa, 1e-10) and close(r["db"][0], dba, 1e-10)
    f32_, W32, b32, y32 = (t.float().requires_grad_(i < 3) for i, t in enumerate((f, W, bias, y)))
    z32 = f32_ @ W32.t() + b32
    l32 = F.binary_cross_entropy_with_logits(z32, y32)
    (l32 * gs).backward()
    r2 = R.bce_head_ref(f, W, bias, y, gs, logits=z32.detach())
    inside(l32.detach().reshape(1), r2["loss"], "loss")
    inside(f32_.grad, r2["df"], "df")
    inside(W32.grad, r2["dW"], "dW")
    inside(b32.grad, r2["db"], "db")
    inside(R.bce_kernel_g32(z, y), r2["g"], "g")
    for k, rel in (("loss", 1e-4), ("df", 1e-4), ("dW", 1e-4), ("db", 1e-4)):
        not_vacuous(r2[k], k, rel)


def test_bce_tables_cover_the_logit_range_and_catch_every_mutant():
    zs, ys = [], []
    caught = {m: set() for m in R.BCE_WRONG}
    for B, K, N in R.BCE_CASES:
        fx, Wx, bx, yx = R.bce_exact_inputs(B, K, N)
        ex = R.bce_head_ref(fx, Wx, bx, yx, R.BCE_EXACT_SCALE)
        fd, Wd, bd, yd = R.bce_dense_inputs(B, K, N)
        de = R.bce_head_ref(fd, Wd, bd, yd, R.BCE_DENSE_SCALE)
        zs.append(de["logits"][0].flatten())
        ys.append(yd.flatten())
        for m in R.BCE_WRONG:
            wx = R.bce_head_ref(fx, Wx, bx, yx, R.BCE_EXACT_SCALE, wrong=m)
            if any(not torch.equal(wx[k][0], ex[k][0]) for k in ("logits", "df", "dW", "db")):
                caught[m].add(("exact", B, K, N))
            # the dense test hands the reference the kernel's logits: a wrong kernel's own
            wd = R.bce_head_ref(fd, Wd, bd, yd, R.BCE_DENSE_SCALE, wrong=m)
            rd = R.bce_head_ref(fd, Wd, bd, yd, R.BCE_DENSE_SCALE, logits=wd["logits"][0])
            if not torch.equal(wd["logits"][0], de["logits"][0]) or any(R.worst(wd[k][0], *rd[k]) for k in ("loss", "df", "dW", "db")):
                caught[m].add(("dense", B, K, N))
    z, y = torch.cat(zs), torch.cat(ys)
    assert float(z.abs().max()) >= 80 and float((z.abs() < 5).double().mean()) > 0.02 and bool(((y > 0) & (y < 1)).any()) and bool((y == 0).any()) and bool((y == 1).any())
    for m, rows in caught.items():
        print(m, sorted(rows))
        assert rows, "%s is caught on no row" % m
    assert any(r[0] == "dense" for r in caught["loss_scaled"])              # only the loss moves: the exact table does not compare it exactly


@pytest.mark.parametrize("N", [1, 64])
def test_bce_logits_mode_reference(N):
    """logits mode at (128, 64) and (1, 1): f holds logits from {0, +-40 m}; g is exact as in the exact table and df = g * grad_scale."""
    B = 128 if N == 64 else 1
    z = 40.0 * (R._draw(79, "bcel%d" % N, (B, N), 5) - 2)
    y = torch.tensor([0.25, 0.5, 1.0], dtype=D)[R._draw(79, "bcely%d" % N, (B, N), 3).long()]
    r = R.bce_head_ref(z, None, None, y, R.BCE_EXACT_SCALE)
    g32 = R.bce_kernel_g32(z, y).to(D)
    assert float((r["g"][0] - g32).abs().max()) <= 2.0 ** -50 and _representable(g32 * R.BCE_EXACT_SCALE) and r["dW"] is None
    assert torch.equal(r["df"][0].float().to(D), g32 * R.BCE_EXACT_SCALE)
    assert N == 1 or min(R.bce_logit_classes(z)[0]) >= 1
    zz = z.clone().requires_grad_()
    F.binary_cross_entropy_with_logits(zz, y).backward()
    assert close(r["df"][0], zz.grad * R.BCE_EXACT_SCALE, 1e-10)


@pytest.mark.parametrize("B", R.VOTE_B)
@pytest.mark.parametrize("C", R.VOTE_C)
def test_vote_accumulate_ref_and_its_sensitivity(B, C):
    """The host walk against float64 (at most B + 1 roundings per sum), two launches over a split batch equal to one, the last video untouched; and the order matters: the rows in reverse change at least one bit (B > 1: one row has one order), a miscounted reloaded run changes
    the counts (B > 1)."""
    probs, vid, sums, counts, V = R.vote_inputs(B, C)
    assert probs.dtype == sums.dtype == np.float32 and bool((sums != 0).all()) and bool((counts > 0).all()) and max(vid) == V - 2 and min(vid) == 0
    s, c = R.vote_accumulate_ref(probs, vid, sums, counts)
    want = sums.astype(np.float64)
    for b, v in enumerate(vid):
        want[v] += probs[b].astype(np.float64)
    assert np.abs(s - want).max() <= (B + 1) * 2.0 ** -24 * want.max()
    assert c.tolist() == [int(counts[v]) + vid.count(v) for v in range(V)]
    assert np.array_equal(s[V - 1], sums[V - 1]) and c[V - 1] == counts[V - 1]
    if B > 1:
        h = B // 2 + 1
        s2, c2 = R.vote_accumulate_ref(probs[h:], vid[h:], *R.vote_accumulate_ref(probs[:h], vid[:h], sums, counts))
        assert np.array_equal(s2.view(np.int32), s.view(np.int32)) and np.array_equal(c2, c)
        runs = [v for i, v in enumerate(vid) if i == 0 or vid[i - 1] != v]
        assert len(runs) > len(set(runs)), "no video is reloaded after a flush"
        sr, cr = R.vote_accumulate_ref(probs, vid, sums, counts, wrong="reverse")
        assert np.array_equal(cr, c) and not np.array_equal(sr.view(np.int32), s.view(np.int32)), "the reverse order changes no bit"
        sc_, cc = R.vote_accumulate_ref(probs, vid, sums, counts, wrong="count_reload")
        assert np.array_equal(sc_, s) and not np.array_equal(cc, c)
    if B == 1024:
        alt = sum(1 for i in range(2, B) if vid[i] == vid[i - 2] != vid[i - 1])
        assert alt >= 300 and max(len(list(g)) for _, g in itertools.groupby(vid)) >= 200


@pytest.mark.parametrize("V", R.VOTE_FINAL_V)
@pytest.mark.parametrize("C", R.VOTE_C)
def test_vote_finalize_ref_and_the_tie_rule(V, C):
    sums, counts, labels, want = R.vote_finalize_inputs(V, C)
    mean, pred, correct = R.vote_finalize_ref(sums, counts, labels)
    assert mean.dtype == np.float32 and pred.dtype == np.int32 and correct.dtype == np.uint8
    for v in range(V):
        if counts[v] > 0:
            assert np.abs(mean[v] - sums[v].astype(np.float64) / counts[v]).max() <= 2.0 ** -24 * 1.5
            assert pred[v] == np.flip(np.argsort(mean[v], kind="stable"))[0] and correct[v] == (pred[v] == labels[v])
        else:
            assert not mean[v].any() and pred[v] == -1 and correct[v] == 0
    assert [int(p) for p, w in zip(pred, want) if w != -2] == [w for w in want if w != -2]
    assert correct[0] == 1 and (V == 1 or (0 in correct.tolist() and int(counts[3]) == 0))
    _, p1, c1 = R.vote_finalize_ref(sums, counts, labels, wrong="first_tie")
    assert not np.array_equal(p1, pred) and not np.array_equal(c1, correct)
    if C == 1024 and V >= 4:
        assert sums[2, 0] == sums[2, 1023] == sums[2].max() and pred[2] == 1023
    if C > 70 and V >= 4:
        assert sums[1, 6] == sums[1, 70] == sums[1].max() and pred[1] == 70           # the same lane, 64 apart
    assert sums[0, pred[0]] == sums[0, pred[0] - 1] == sums[0].max()                    # two neighbouring lanes


@pytest.mark.parametrize("C", [2, 65])
def test_softmax_ce_ref_at_the_batch_limit(C):
    """B = 1024: the reference equals float64 torch, torch's fp32 softmax / cross entropy lies inside every bound, the bounds are not vacuous, the float64
    top-1 is no rounding matter, and a row loss taken at the wrong label or a mean over B - 1 rows is outside."""
    B = 1024
    z, lab = R.sce_logits(B, C)
    assert z.dtype == F32T and float(z.abs().max()) == 80.0
    r = R.softmax_ce_ref(z, lab)
    z64 = z.to(D)
    top2 = torch.topk(z64, 2, dim=1).values
    assert float((top2[:, 0] - top2[:, 1]).min()) >= 0.05 and torch.equal(r["pred"], z64.argmax(1))
    rows64 = F.cross_entropy(z64, lab, reduction="none")
    assert close(r["probs"][0], torch.softmax(z64, 1)) and close(r["row_loss"][0], rows64, 1e-9) and close(r["loss"][0], rows64.mean().reshape(1), 1e-9)
    rows32 = F.cross_entropy(z, lab, reduction="none")
    inside(torch.softmax(z, 1), r["probs"], "probs")
    inside(rows32, r["row_loss"], "row loss")
    inside(rows32.mean().reshape(1), r["loss"], "loss")
    not_vacuous(r["probs"], "probs", 1e-4)
    not_vacuous(r["row_loss"], "row loss", 1e-4)
    not_vacuous(r["loss"], "loss", 1e-4)
    outside(F.cross_entropy(z64, (lab + 1) % C, reduction="none"), r["row_loss"], "the loss of the next label")
    outside((rows64.sum() / (B - 1)).reshape(1), r["loss"], "a mean over B - 1 rows")
    outside(torch.softmax(z64 * (1 + 2.0 ** -17), 1), r["probs"], "logits off by 2^-17 relative")
