"""-m gpu: the training side of the non-local block -- tedspad_nl_attention_fwd_lse / tedspad_nl_attention_bwd through the C ABI against the float64
closed form (tests/nl_grad_ref.py), and NonLocalBlock as a differentiable module against the reference's recorded train-mode results.

Bounds. theta and phi are on a 2^-4 grid (test_hip_nl.case), so the logits are exact in fp32.
  lse      |lse - ref| <= 2^-15 + 2^-20 |ref|: k 2^-24 for the sum of at most 392 terms, four roundings of a value of size |lse|.
  dg       = P^T dT with P rounded to the storage type (relative u) and the result rounded once: |err| <= u P^T|dT| + u |dg|; asserted at twice that,
           2 u (P^T|dT| + |dg|), computed from the float64 reference alone.
  dtheta, dphi   a worst-case elementwise bound is vacuous (the D term dominates it), so: rel-L2 against float64 <= 2 max(rel-L2 of torch's own 16-bit
           bmm -> softmax -> bmm autograd on the GPU from the same tensors, u); the 2 is for the one rounding the fused path has more, D from the stored T.
"""
import ctypes as C
import functools
import json
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

import nl_grad_ref
import nl_ref
from conftest import GOLDEN_DIR, rel_l2
from test_hip_nl import GUARD_ROWS, SENTINEL, SHAPES, U, case, qk
from ted_spad_amd.synth import synth_tensor

pytestmark = pytest.mark.gpu
GENERAL = ["rect", "odd7", "layer3", "layer2"]          # partial tile (q 60, k 15), odd7 (sliced phi | g), layer3, layer2; k1 has its own exact test
LSE_GUARD = 12345.0


def tdt_of(dtype):
    return torch.float16 if dtype == "f16" else torch.bfloat16


def upstream(name, variant, dtype):
    n, t, h, w, d, _ = SHAPES[name]
    return synth_tensor(7, "%s/%s/dt" % (name, variant), (n, qk(SHAPES[name])[0], d), -1.0, 1.0).to(tdt_of(dtype)).float()


QUIET_NAN = {"f16": 0x7E00, "bf16": 0x7FC0}


def run(theta, phi, g, dt, dtype, sliced, scale=None, ld=None, poison=False, tape=None):
    """tedspad_nl_attention_fwd, _fwd_lse and _bwd on fresh buffers. Every buffer has GUARD_ROWS rows in front of its first and behind its last row; every
    output row is padded (ld = d + 8, or the 2 d + 8 of a shared dphi | dg buffer). The outputs' padding, the channels of a shared output buffer that belong
    to neither slice and the guards -- the guard floats around lse and the workspace too -- must come back untouched. Returns raw 16-bit images
    (n * rows, d) and float64 copies.
      scale    the softmax scale (default d ** -0.5)
      ld       every operand's row stride, overriding the defaults: {"theta", "dt", "t", "dtheta": ld}, {"phi", "g": ld} or {"pg": (ld, g's channel offset)}
               for phi and g as slices of one buffer, {"dphi", "dg": ld} or {"dpg": (ld, dg's channel offset)}
      poison   the padding, the guard rows and the unused channels of every INPUT (of the backward's T and lse as well) hold the storage type's quiet NaN
      tape     (T as an (n * q, d) 16-bit image, lse (n, q) fp32) from the host for the backward, instead of the forward kernel's own"""
    from ted_spad_amd import _lib
    from ted_spad_amd.engine import _stream_ptr
    n, q, d = theta.shape
    k = phi.shape[1]
    tdt, code = (torch.float16, _lib.F16) if dtype == "f16" else (torch.bfloat16, _lib.BF16)
    scale = C.c_float(float(d) ** -0.5 if scale is None else scale)
    lib, sp = _lib.lib(), _stream_ptr()
    L = dict(theta=d, dt=d, t=d + 8, dtheta=d + 8)
    L.update(dict(pg=(2 * d, d), dpg=(2 * d + 8, d)) if sliced else dict(phi=d, g=d, dphi=d + 8, dg=d + 8))
    if ld is not None:
        for pair, one in (("pg", ("phi", "g")), ("dpg", ("dphi", "dg"))):
            if pair in ld or one[0] in ld:                # the caller chooses between one buffer and two
                for key in (pair,) + one:
                    L.pop(key, None)
        L.update(ld)
    fill = QUIET_NAN[dtype] if poison else 0
    G = GUARD_ROWS

    def source(rows, width, *parts):
        """A (G + rows + G, width) input image holding `parts` [(values (n, r, d), first channel)]; its first row's address."""
        host = torch.full((rows + 2 * G, width), fill, dtype=torch.int16)
        for x, c0 in parts:
            host[G:G + rows, c0:c0 + d] = x.to(tdt).view(torch.int16).reshape(rows, d)
        dev = host.cuda()
        return dev, dev.data_ptr() + G * width * 2

    def sink(rows, width):
        dev = torch.full((rows + 2 * G, width), SENTINEL, dtype=torch.int16, device="cuda")
        return dev, dev.data_ptr() + G * width * 2

    floats = lambda: torch.full((n * q + 2 * G,), LSE_GUARD, dtype=torch.float32, device="cuda")
    th, thp = source(n * q, L["theta"], (theta, 0))
    dtd, dtp = source(n * q, L["dt"], (dt, 0))
    if "pg" in L:
        ldp = ldg = L["pg"][0]
        pg, pp = source(n * k, ldp, (phi, 0), (g, L["pg"][1]))
        gp = pp + 2 * L["pg"][1]
    else:
        ldp, ldg = L["phi"], L["g"]
        (ph, pp), (gg, gp) = source(n * k, ldp, (phi, 0)), source(n * k, ldg, (g, 0))
    ldo = L["t"]
    (out0, o0p), (out1, o1p), (dth, dthp) = sink(n * q, ldo), sink(n * q, ldo), sink(n * q, L["dtheta"])
    lse = floats()
    lsep = lse.data_ptr() + 4 * G
    _lib.check(lib.tedspad_nl_attention_fwd(thp, L["theta"], pp, ldp, gp, ldg, o0p, ldo, n, q, k, d, scale, code, sp), "fwd")
    _lib.check(lib.tedspad_nl_attention_fwd_lse(thp, L["theta"], pp, ldp, gp, ldg, o1p, ldo, lsep, n, q, k, d, scale, code, sp), "fwd_lse")
    if "dpg" in L:
        lddp = lddg = L["dpg"][0]
        dpg, dpp = sink(n * k, lddp)
        dgp = dpp + 2 * L["dpg"][1]
    else:
        lddp, lddg = L["dphi"], L["dg"]
        (dph, dpp), (dgg, dgp) = sink(n * k, lddp), sink(n * k, lddg)
    nbytes = C.c_int64(0)
    _lib.check(lib.tedspad_nl_attention_bwd_workspace(n, q, C.byref(nbytes)), "workspace")
    assert nbytes.value == n * q * 4
    ws = floats()
    tp, lsein = o1p, lsep                                  # as the training path does: the forward's own T and lse
    if tape is not None or poison:
        if tape is not None:
            tin, tp = source(n * q, ldo, (tape[0].view(tdt).reshape(n, q, d), 0))
            lse_rows = tape[1].reshape(-1).float().cuda()
        else:                                              # the forward's results, with everything around them poisoned
            torch.cuda.synchronize()
            tin, tp = source(n * q, ldo)
            tin[G:G + n * q, :d] = out1[G:G + n * q, :d]
            lse_rows = lse[G:G + n * q]
        lin = torch.full((n * q + 2 * G,), float("nan") if poison else LSE_GUARD, dtype=torch.float32, device="cuda")
        lin[G:G + n * q] = lse_rows
        lsein = lin.data_ptr() + 4 * G
    _lib.check(lib.tedspad_nl_attention_bwd(thp, L["theta"], pp, ldp, gp, ldg, tp, ldo, dtp, L["dt"], lsein, dthp, L["dtheta"],
                                            dpp, lddp, dgp, lddg, ws.data_ptr() + 4 * G, n, q, k, d, scale, code, sp), "bwd")
    torch.cuda.synchronize()

    def image(t, rows, c0=0, others=()):
        host = t.cpu()
        assert bool((host[:G] == SENTINEL).all()) and bool((host[G + rows:] == SENTINEL).all()), "guard rows around an output were written"
        free = torch.ones(host.shape[1], dtype=torch.bool)
        for c in (c0,) + tuple(others):
            free[c:c + d] = False
        assert bool((host[G:G + rows, free] == SENTINEL).all()), "the padding of an output row was written"
        return host[G:G + rows, c0:c0 + d].contiguous()
    r = {"t0": image(out0, n * q), "t": image(out1, n * q), "dtheta": image(dth, n * q)}
    if "dpg" in L:
        off = L["dpg"][1]
        r["dphi"], r["dg"] = image(dpg, n * k, 0, (off,)), image(dpg, n * k, off, (0,))
    else:
        r["dphi"], r["dg"] = image(dph, n * k), image(dgg, n * k)
    for t in (lse, ws):
        host = t.cpu()
        assert bool((host[:G] == LSE_GUARD).all()) and bool((host[G + n * q:] == LSE_GUARD).all()), "guard floats around lse / the workspace were written"
    r["lse"] = lse[G:G + n * q].cpu().double().reshape(n, q)
    for key in ("t", "dtheta", "dphi", "dg"):
        r[key + "64"] = r[key].view(tdt).double().reshape(n, -1, d)
    return r


def lse_bound(ref_lse):
    """|lse - ref| <= 2^-15 + 2^-20 |ref| (the header)."""
    return 2.0 ** -15 + 2.0 ** -20 * ref_lse.abs()


def dg_bound(ref, dt, dtype):
    """|dg - ref| <= 2 u (P^T|dT| + |dg|), from the float64 reference alone (the header)."""
    return 2.0 * U[dtype] * (torch.einsum("nqk,nqd->nkd", ref["p"], dt.double().abs()) + ref["dg"].abs())


@functools.lru_cache(maxsize=None)
def result(name, variant, dtype):
    """(kernel results, float64 closed form at the kernel's inputs, upstream gradient) of a stored case; computed once and shared."""
    theta, phi, g, _ = case(name, variant, dtype)
    dt = upstream(name, variant, dtype)
    r = run(theta, phi, g, dt, dtype, SHAPES[name][5])
    return r, nl_grad_ref.attention_grads(theta, phi, g, dt, float(theta.shape[2]) ** -0.5), dt


@functools.lru_cache(maxsize=None)
def chain(name, variant, dtype):
    """rel-L2 against float64 of torch's own 16-bit bmm -> softmax -> bmm autograd on the GPU from the same tensors: (dtheta, dphi, dg)."""
    theta, phi, g, _ = case(name, variant, dtype)
    ref = result(name, variant, dtype)[1]
    tdt = tdt_of(dtype)
    th, ph, gg = (t.to(tdt).cuda().requires_grad_() for t in (theta, phi, g))
    p = torch.softmax(torch.bmm(th, ph.transpose(1, 2)) * float(theta.shape[2]) ** -0.5, dim=-1)
    torch.bmm(p, gg).backward(upstream(name, variant, dtype).to(tdt).cuda())
    return tuple(rel_l2(a.grad.double().cpu(), ref[k]) for a, k in ((th, "dtheta"), (ph, "dphi"), (gg, "dg")))


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("name", ["k1"] + GENERAL)
def test_fwd_lse_out_is_bit_equal_and_lse_within_its_bound(name, dtype):
    r, ref, _ = result(name, "plain", dtype)
    assert torch.equal(r["t"], r["t0"])
    err = (r["lse"] - ref["lse"]).abs()
    bound = lse_bound(ref["lse"])
    print("%s %s: max |lse err| / bound = %.3f" % (name, dtype, float((err / bound).max())))
    assert bool((err <= bound).all())


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_one_key_is_exact(dtype):
    """k = 1: P = 1, so dg[0] = sum_i dT[i] rounded once and dtheta = dphi = 0 bit for bit."""
    r, _, dt = result("k1", "plain", dtype)
    assert torch.equal(r["dg64"], dt.double().sum(dim=1, keepdim=True).float().to(tdt_of(dtype)).double())
    assert not r["dtheta"].view(tdt_of(dtype)).double().abs().max() and not r["dphi"].view(tdt_of(dtype)).double().abs().max()
    assert bool((r["dtheta"] == 0).all()) and bool((r["dphi"] == 0).all())


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_equal_logits_are_exact(dtype):
    """k = 32, d = 256 (scale = 2^-4), every phi row the same integer vector, theta integers: every row's logits are equal, P = 1/32 exactly. g in
    multiples of 32 keeps T an integer; dT has one channel of +-1 per query, so dP - D is an integer below 128 and dS = (dP - D) / 32 has eight
    significant bits: exact in both storage types. Every sum is then exact in fp32: dtheta = 0, dphi and dg are the float64 values rounded once."""
    n, t, h, w, d, _ = SHAPES["k32"]
    q, k = qk(SHAPES["k32"])
    assert (k, d) == (32, 256)
    ints = lambda tag, shape, lo, hi: torch.floor(synth_tensor(7, "eq/" + tag, shape) * (hi - lo + 1)) + lo
    theta = ints("theta", (n, q, d), -2, 2)
    phi = ints("phi", (n, 1, d), -2, 2).expand(n, k, d).contiguous()
    g = ints("g", (n, k, d), -2, 2) * 32.0
    dt = torch.zeros(n, q, d)
    ch = torch.floor(synth_tensor(7, "eq/ch", (n, q)) * d).long().clamp_(0, d - 1)
    dt.scatter_(2, ch.unsqueeze(2), torch.where(synth_tensor(7, "eq/sign", (n, q, 1)) < 0.5, -1.0, 1.0))
    r = run(theta, phi, g, dt, dtype, False)
    ref = nl_grad_ref.attention_grads(theta, phi, g, dt, 2.0 ** -4)
    tdt = tdt_of(dtype)
    assert float((ref["p"] - 1.0 / 32).abs().max()) < 1e-15
    # the same closed form with P = 1/32 put in: every product and sum below is exact in float64 (integers over powers of two), so `exact` IS the
    # float64 value up to the 1e-15 of its exp / log, and rounding it to the storage type (through fp32, which holds it exactly) is the one rounding
    g64, dt64, th64 = g.double(), dt.double(), theta.double()
    t = g64.sum(dim=1, keepdim=True).expand(n, q, d) / 32
    ds = (torch.einsum("nqd,nkd->nqk", dt64, g64) - (dt64 * t).sum(dim=2, keepdim=True)) / 32
    exact = dict(t=t, dg=dt64.sum(dim=1, keepdim=True).expand(n, k, d) / 32, dphi=torch.einsum("nqk,nqd->nkd", ds, th64) / 16, dtheta=torch.zeros(n, q, d).double())
    for key, v in exact.items():
        assert float((v - ref[key]).abs().max()) < 1e-12, key
        want = v.float().to(tdt).double()
        bad = int((r[key + "64"] != want).sum())
        print("equal logits %s %s: %d of %d elements differ, max |got - want| = %.3e (max |want| %.3e)" % (
            dtype, key, bad, want.numel(), float((r[key + "64"] - want).abs().max()), float(want.abs().max())))
    for key, v in exact.items():
        assert torch.equal(r[key + "64"], v.float().to(tdt).double()), key
    assert float(exact["dphi"].abs().max()) > 0 and float(ds.abs().max()) <= 4.0


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("name", GENERAL)
def test_dg_within_the_derived_bound(name, dtype):
    r, ref, dt = result(name, "plain", dtype)
    bound = dg_bound(ref, dt, dtype)
    err = (r["dg64"] - ref["dg"]).abs()
    print("%s %s: max |dg err| / bound = %.3f; bound / rms(dg) = %.4f" % (name, dtype, float((err / bound.clamp_min(1e-30)).max()),
                                                                        float(bound.mean() / ref["dg"].pow(2).mean().sqrt())))
    assert bool((err <= bound).all())


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("name", GENERAL)
def test_dtheta_dphi_against_torchs_16_bit_chain(name, dtype):
    r, ref, _ = result(name, "plain", dtype)
    c = chain(name, "plain", dtype)
    for key, cr in (("dtheta", c[0]), ("dphi", c[1])):
        e = rel_l2(r[key + "64"], ref[key])
        lim = 2.0 * max(cr, U[dtype])
        print("%s %s %s: fused rel-L2 %.3e, torch chain %.3e, ratio to the limit %.3f" % (name, dtype, key, e, cr, e / lim))
        assert e <= lim, (key, e, cr)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("variant", ["spike", "plus200", "minus200", "poison"])
@pytest.mark.parametrize("name", ["odd7", "layer3"])
def test_hard_inputs(name, variant, dtype):
    r, ref, dt = result(name, variant, dtype)
    for key in ("dtheta64", "dphi64", "dg64"):
        assert bool(torch.isfinite(r[key]).all()), key
    assert bool(torch.isfinite(r["lse"]).all())
    if variant == "poison":                      # the clean item alone gives the same bits as in the poisoned batch
        theta, phi, g, _ = case(name, variant, dtype)
        b = theta.shape[0] // 2
        q, k = theta.shape[1], phi.shape[1]
        alone = run(theta[b:b + 1], phi[b:b + 1], g[b:b + 1], dt[b:b + 1], dtype, SHAPES[name][5])
        for key, rows in (("dtheta", q), ("dphi", k), ("dg", k), ("t", q)):
            assert torch.equal(alone[key], r[key][b * rows:(b + 1) * rows]), key
        assert torch.equal(alone["lse"][0], r["lse"][b])
    else:
        bound = dg_bound(ref, dt, dtype)
        assert bool(((r["dg64"] - ref["dg"]).abs() <= bound).all())


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_two_runs_are_bit_identical(dtype):
    theta, phi, g, _ = case("layer3", "plain", dtype)
    a = result("layer3", "plain", dtype)[0]
    b = run(theta, phi, g, upstream("layer3", "plain", dtype), dtype, SHAPES["layer3"][5])
    for key in ("t", "dtheta", "dphi", "dg"):
        assert torch.equal(a[key], b[key]), key
    assert torch.equal(a["lse"], b["lse"])


def test_engine_wrappers_match_the_c_entries():
    from ted_spad_amd import engine as E
    theta, phi, g, _ = case("odd7", "plain", "f16")
    n, t, h, w, d, _ = SHAPES["odd7"]
    r = result("odd7", "plain", "f16")[0]
    act = lambda x, dims: E.Act(x.to(torch.float16).cuda().reshape(n, *dims, x.shape[2]).contiguous(), x.shape[2])
    pg = act(torch.cat([phi, g], dim=2), (t, h // 2, w // 2))
    th, dta = act(theta, (t, h, w)), act(upstream("odd7", "plain", "f16"), (t, h, w))
    ta, lse = E.nl_attention_lse(th, pg.slice(0, d), pg.slice(d, d), float(d) ** -0.5)
    dth, dph, dg = E.nl_attention_bwd(th, pg.slice(0, d), pg.slice(d, d), ta, lse, dta, float(d) ** -0.5)
    torch.cuda.synchronize()
    bits = lambda a: a.buf.cpu().view(torch.int16).reshape(-1, d)
    assert torch.equal(bits(ta), r["t"]) and torch.equal(lse.cpu().double(), r["lse"])
    assert torch.equal(bits(dth), r["dtheta"]) and torch.equal(bits(dph), r["dphi"]) and torch.equal(bits(dg), r["dg"])


def test_an_overflowing_dS_and_a_non_finite_dT_stay_visible():
    """The training path's convention (train_engine.GRAD_SCALE's note): no f16 store clamps, so an overflow reaches the gradients as inf / NaN where a loss
    scale's check finds it. dS = P (dP - D) is rounded to f16 INSIDE the kernel: with dT = 60000 sign(g[key 0]) the product dT . g[key 0] is 60000 sum|g|
    ~ 4e6 while dtheta, dphi of a clamped dS (65504 scale |phi|, summed over 15 keys with both signs) would stay far inside the range -- they must not come
    back finite. Likewise one NaN in dT: its query's dtheta row and dphi are non-finite, as dg is."""
    theta, phi, g, _ = case("rect", "plain", "f16")
    big = torch.where(g[:, :1] < 0, -60000.0, 60000.0).expand_as(theta).contiguous()
    r = run(theta, phi, g, big, "f16", False)
    assert not bool(torch.isfinite(r["dtheta64"]).all()) and not bool(torch.isfinite(r["dphi64"]).all())
    dt = upstream("rect", "plain", "f16").clone()
    dt[0, 7, 3] = float("nan")
    r = run(theta, phi, g, dt, "f16", False)
    assert not bool(torch.isfinite(r["dtheta64"][0, 7]).any()), "the poisoned query's dtheta row"
    assert bool(torch.isfinite(r["dtheta64"][0, :7]).all()) and bool(torch.isfinite(r["dtheta64"][0, 8:]).all()), "the other queries' rows"
    assert not bool(torch.isfinite(r["dphi64"]).any()) and not bool(torch.isfinite(r["dg64"][0, :, 3]).any())


# ---- the block as a module ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def train_golden():
    return dict(np.load(os.path.join(GOLDEN_DIR, "nl_train_golden.npz")))


@pytest.fixture(scope="module")
def train_meta():
    with open(os.path.join(GOLDEN_DIR, "nl_train_golden_meta.json")) as f:
        return json.load(f)


def make_block(name, meta, dims=None, shape=None):
    from ted_spad_amd.i3res50 import NonLocalBlock
    b = meta["cases"][name]
    p = name + ".nl."
    blk = NonLocalBlock(*(dims or b["dims"]))
    tmpl = OrderedDict((p + k, v) for k, v in blk.state_dict().items())
    sd = nl_ref.nl_state_dict(tmpl, meta["seed"], {p: b["gain"]})
    blk.load_state_dict(OrderedDict((k[len(p):], v) for k, v in sd.items()), strict=True)
    shape = tuple(shape or b["input"])
    return blk.cuda(), sd, p, synth_tensor(meta["seed"], name + "/in", shape, -1.0, 1.0), synth_tensor(meta["seed"], name + "/dy", shape, -1.0, 1.0)


def zero_grad_limit(golden, name, c):
    """The absolute limit an analytically zero bias gradient is held to: the issue's rule for out.bias (2e-2 sqrt(sum|dy|), tests/test_hip_train_ops.py:139)
    AND the gradient gate itself at the scale of the one bias gradient of the block that is not zero -- 5e-3 ||theta.bias.grad||: an error of that norm in
    theta.bias.grad, a sum of the same kind over the same pixels, is what its rel-L2 gate lets pass."""
    return min(2e-2 * c["dy_abs_sum"] ** 0.5, 5e-3 * float(golden[name + "/grad/theta.bias/norm"]))


def device_point(blk, x):
    """theta, phi, g, T and the batch statistics the device's own forward produced (float64 rows): where the float64 backward is evaluated when a
    gradient misses its gate against the fp32-input reference (the method of test_phase2_backward_at_the_devices_forward_point_vs_autograd)."""
    from ted_spad_amd import train_engine as TE
    from ted_spad_amd.autograd import _nl_act
    from ted_spad_amd.i3res50 import NonLocalBlock
    from ted_spad_amd.train_nets import NonLocalTrainer
    twin = NonLocalBlock(blk.dim_in, blk.dim_out, blk.dim_inner, dtype=blk.compute_dtype)      # the same parameters; the moved running statistics play no part
    twin.load_state_dict(blk.state_dict())
    twin = twin.cuda().train()
    TE.ARENA.reset(x.device)
    _, tape = NonLocalTrainer(twin).forward(_nl_act(x.cuda(), twin.compute_dtype, 1.0), "train")
    TE.flush_deferred()
    rows = lambda a: a.buf.double().flatten(1, 3).cpu()
    c = twin.dim_out
    mean, invstd = tape["bn"].mean[0, :c].double().cpu(), tape["bn"].invstd[0, :c].double().cpu()
    return dict(theta=rows(tape["theta"]), phi=rows(tape["phi"]), g=rows(tape["g"]), t=rows(tape["t"]), mean=mean, var=invstd ** -2 - twin.bn.eps)


@pytest.mark.parametrize("name", ["nl_block512", "nl_block1024"])
def test_block_train_mode_vs_reference(name, train_golden, train_meta):
    """NonLocalBlock(...).cuda().train()(x) and its backward in f16 (the bridge scales the upstream gradient by 256 and divides it out again) at the
    project's per-op gates: output 2e-3, running statistics 1e-3, each parameter gradient and the BRANCH's input gradient (dx - dy against the
    reference's dx - dy: the residual path alone would pass anything) 5e-3. A tensor that misses 5e-3 against the fp32-input reference must hold it at
    the device's own forward point."""
    blk, sd, p, x, dy = make_block(name, train_meta)
    c = train_meta["cases"][name]
    blk.train()
    xg = x.cuda().requires_grad_()
    y = blk(xg)
    assert y.dtype == torch.float32 and y.shape == x.shape
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    fix = lambda k: nl_grad_ref.vs_fixture(k[0], train_golden, name + "/" + k[1])[0]
    e = fix((y.detach().cpu(), "out"))
    print("%s out: rel-L2 %.3e" % (name, e))
    assert e < 2e-3
    for k in ("running_mean", "running_var"):
        e = fix((getattr(blk.bn, k).cpu(), k))
        print("%s %s: rel-L2 %.3e" % (name, k, e))
        assert e < 1e-3
    assert int(blk.bn.num_batches_tracked) == 1
    idx = nl_grad_ref.sample_index(x.numel())
    ref_branch = torch.as_tensor(train_golden[name + "/dx/sample"]).double() - dy.double().flatten()[idx]
    got = {"branch_dx": (xg.grad.cpu().double() - dy.double())}
    for k in nl_grad_ref.PARAMS:
        mod, leaf = k.split(".")
        got["grad/" + k] = getattr(getattr(blk, mod), leaf).grad.cpu().double()
    miss = {}
    for k, v in got.items():
        if k[5:] in nl_grad_ref.ZERO_GRADS["train"]:
            lim = zero_grad_limit(train_golden, name, c)
            print("%s %s (analytically 0): max |.| %.3e, limit %.3e" % (name, k, float(v.abs().max()), lim))
            assert float(v.abs().max()) < lim, k
            continue
        e = float((v.flatten()[idx] - ref_branch).norm() / ref_branch.norm()) if k == "branch_dx" else fix((v, k))
        print("%s %s: rel-L2 vs the fp32-input reference %.3e" % (name, k, e))
        if e >= 5e-3:
            miss[k] = e
    if miss or name == "nl_block512":          # the 512-channel case always goes through the second comparison, so that it is exercised; only a miss asserts
        at = nl_grad_ref.block_train(x, sd, p, dy, "train", eps=c["eps"], momentum=c["momentum"], given=device_point(blk, x))
        for k in got:
            if k[5:] in nl_grad_ref.ZERO_GRADS["train"]:
                continue
            e = rel_l2(got[k], at[k])
            print("%s %s: rel-L2 at the device's forward point %.3e%s" % (name, k, e, " (vs the reference %.3e)" % miss[k] if k in miss else ""))
            assert torch.isfinite(at[k]).all() and at[k].shape == got[k].shape
            if k in miss:
                assert e < 5e-3, k


def test_block_frozen_mode(train_meta):
    """eval() with gradients: bn buffers do not move, gamma / beta get no gradient, dx and the convolutions' gradients hold the train-mode gates against
    the float64 frozen-mode restatement."""
    name = "nl_block512"
    blk, sd, p, x, dy = make_block(name, train_meta)
    blk.eval()
    before = {k: v.clone() for k, v in blk.bn.state_dict().items()}
    xg = x.cuda().requires_grad_()
    y = blk(xg)
    y.backward(dy.cuda())
    ref = nl_grad_ref.block_train(x, sd, p, dy, "frozen")
    for k, v in blk.bn.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert blk.bn.weight.grad is None and blk.bn.bias.grad is None
    assert rel_l2(y.detach().cpu(), ref["out"]) < 2e-3
    e = rel_l2(xg.grad.cpu().double() - dy.double(), ref["branch_dx"])
    print("frozen branch dx: %.3e" % e)
    assert e < 5e-3
    for k in nl_grad_ref.PARAMS[:8]:
        mod, leaf = k.split(".")
        gr = getattr(getattr(blk, mod), leaf).grad.cpu().double()
        if k in nl_grad_ref.ZERO_GRADS["frozen"]:
            assert float(gr.abs().max()) < min(2e-2 * train_meta["cases"][name]["dy_abs_sum"] ** 0.5, 5e-3 * float(ref["grad/theta.bias"].norm())), k
            continue
        e = rel_l2(gr, ref["grad/" + k])
        print("frozen %s: %.3e" % (k, e))
        assert e < 5e-3, k


def test_block_eval_under_no_grad_is_the_packed_sequence(train_meta):
    from ted_spad_amd import engine as E
    from ted_spad_amd.i3res50 import nonlocal_forward, pack_nonlocal
    blk, _, _, x, _ = make_block("nl_block512", train_meta)
    blk.eval()
    with torch.no_grad():
        y = blk(x.cuda())
    P = {}
    pack_nonlocal(P, "", blk, blk.compute_dtype, torch.device("cuda"))
    a = E.Act(x.permute(0, 2, 3, 4, 1).contiguous().to(torch.float16).cuda(), x.shape[1])
    assert torch.equal(y, E.act_to_nchw(nonlocal_forward(P, "", blk, a)))
    with pytest.raises(Exception, match="no CPU path"):
        blk(x)


def test_pooled_away_row_and_column_get_nothing_through_phi_and_g(train_meta):
    """A 7 x 7 frame pools to 3 x 3: the last row / column reaches the output through the residual and theta only. With theta's parameters zeroed
    (dtheta's data gradient vanishes) the branch's input gradient is exactly zero there, and is not zero elsewhere. (The upstream gradient holds
    f16 values, so that the residual path returns it bit for bit.)"""
    blk, _, _, x, dy = make_block("nl_block512", train_meta)
    dy = dy.half().float()
    with torch.no_grad():
        blk.theta.weight.zero_()
    blk.train()
    xg = x.cuda().requires_grad_()
    blk(xg).backward(dy.cuda())
    branch = xg.grad.cpu() - dy
    assert float(branch[:, :, :, 6, :].abs().max()) == 0.0 and float(branch[:, :, :, :, 6].abs().max()) == 0.0
    assert float(branch[:, :, :, :6, :6].abs().max()) > 0.0


def test_bias_gradients_are_the_channel_sums_of_the_kernels_gradients(train_meta, monkeypatch):
    """phi.bias.grad is analytically zero in both modes, so no comparison with a reference can show that its PATH is wired: here theta's, phi's and g's
    bias gradients are held to the per-channel sums of the dtheta / dphi / dg the attention backward produced (spied), a cancelling sum of terms that are
    not small. Both sides sum the same stored 16-bit rows, so the tolerance is the fp32 summation's alone."""
    from ted_spad_amd import engine as E, train_engine as TE
    from ted_spad_amd.autograd import _nl_act
    from ted_spad_amd.train_nets import NonLocalTrainer
    blk, _, _, x, dy = make_block("nl_block512", train_meta)
    seen = {}
    bwd = E.nl_attention_bwd

    def spy(*a, **k):
        seen["grads"] = bwd(*a, **k)
        return seen["grads"]
    monkeypatch.setattr(E, "nl_attention_bwd", spy)
    TE.ARENA.reset(torch.device("cuda"))
    tr = NonLocalTrainer(blk.train())
    _, tape = tr.forward(_nl_act(x.cuda(), blk.compute_dtype, 1.0), "train")
    tr.backward(tape, _nl_act(dy.cuda(), blk.compute_dtype, TE.GRAD_SCALE))
    tr.flush_grads()
    TE.flush_deferred()
    for conv, grad in zip((blk.theta, blk.phi, blk.g), seen["grads"]):
        rows = grad.buf.double().flatten(0, 3).cpu()
        want, got = rows.sum(dim=0), conv.bias.grad.double().cpu()
        tol = rows.shape[0] * 2.0 ** -24 * float(rows.abs().sum(dim=0).max()) + 1e-6      # an fp32 sum of N stored values in any order: N u sum|x|
        print("bias path: max |grad - channel sum| %.3e, tolerance %.3e, sum over |terms| per channel %.3e" % (
            float((got - want).abs().max()), tol, float(rows.abs().sum(dim=0).mean())))
        assert float((got - want).abs().max()) < tol
        assert float(rows.abs().sum(dim=0).min()) > 100 * tol              # the sums cancel terms that are far above the tolerance


def test_train_mode_under_no_grad_moves_the_statistics_and_recycles_the_arena(train_meta):
    import gc
    from ted_spad_amd import train_engine as TE
    gc.collect()                                            # no tape of an earlier test is alive
    blk, sd, p, x, _ = make_block("nl_block512", train_meta)
    blk.train()
    ref = nl_grad_ref.block_train(x, sd, p, torch.zeros_like(x), "train")
    used = []
    with torch.no_grad():
        for i in range(3):
            y = blk(x.cuda())
            used.append(TE.ARENA.used)
            assert not y.requires_grad and int(blk.bn.num_batches_tracked) == i + 1
            if i == 0:
                assert rel_l2(y.cpu(), ref["out"]) < 2e-3
                assert rel_l2(blk.bn.running_mean.cpu(), ref["running_mean"]) < 1e-3 and rel_l2(blk.bn.running_var.cpu(), ref["running_var"]) < 1e-3
    assert used[0] == used[1] == used[2] > 0, used          # every call starts from a recycled arena: no growth, no per-request allocations
