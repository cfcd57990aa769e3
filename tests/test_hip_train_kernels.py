"""-m gpu: the memory-bound kernels of the training step (csrc/train_ops.hip, the idx / backward half of csrc/pool_layout.hip) one by one through the C ABI,
against the float64 references of tests/kernel_refs.py, in f16 and bf16, at the shapes where such kernels go wrong: C < Cz, channel groups that do not fill
a workgroup, pixel counts off the lane count, strides wider than the tensor, ties and non-finite values in the pooling windows. Inputs are pre-rounded to
their storage type; every output lives in a channel slice of a wider, sentinel-filled buffer whose other elements must come back untouched."""
import ctypes as Ct
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:         # (run as a script: the child process of the unrolled / rolled test)
    sys.path.insert(0, ROOT)

import kernel_refs as R  # noqa: E402

pytestmark = pytest.mark.gpu
D = torch.float64
DTS = ["f16", "bf16"]
EPS, MOM = 1e-5, 0.1
SENT = 1024.0            # exact in every type used here; no result below reaches it
F32 = R.F32_EPS


def L():
    from ted_spad_amd import _lib
    return _lib.lib()


def code(dt):
    from ted_spad_amd import _lib
    return {"f16": _lib.F16, "bf16": _lib.BF16, "f32": _lib.F32}[dt]


def S():
    return Ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def ok(rc):
    from ted_spad_amd import _lib
    assert rc == 0, _lib.last_error()


class In:
    """rows x c input values at channel offset `off` of a rows x ld device buffer; the other channels hold a value no result may depend on."""

    def __init__(self, t, ld, off, dtype):
        t = t.reshape(-1, t.shape[-1])
        assert ld >= off + t.shape[1]
        buf = torch.full((t.shape[0], ld), 1000.0, dtype=dtype)
        buf[:, off:off + t.shape[1]] = t.to(dtype)
        self.buf = buf.cuda()
        self.ptr = self.buf.data_ptr() + off * self.buf.element_size()
        self.ld = ld


class Out:
    """rows x c output slice at channel offset `off` of a (rows + 2) x ld buffer pre-filled with a sentinel (`init`: the slice's own initial value)."""

    def __init__(self, rows, c, ld, off, dtype, init=None, fill=SENT):
        assert ld >= off + c
        self.rows, self.c, self.off, self.ld, self.fill = rows, c, off, ld, fill
        buf = torch.full((rows + 2, ld), fill, dtype=dtype)
        if init is not None:
            buf[:rows, off:off + c] = init.reshape(rows, c).to(dtype)
        self.buf = buf.cuda()
        self.ptr = self.buf.data_ptr() + off * self.buf.element_size()

    def get(self):
        return self.buf[:self.rows, self.off:self.off + self.c].cpu().to(D)

    def raw(self):
        return self.buf[:self.rows, self.off:self.off + self.c].cpu()

    def intact(self):
        m = torch.ones(self.buf.shape, dtype=torch.bool)
        m[:self.rows, self.off:self.off + self.c] = False
        return bool((self.buf.cpu()[m] == self.fill).all())


def lds(c, wide):
    return (c + 16, 8) if wide else (c, 0)          # (pixel stride, channel offset)


def within(got, ref, bound, what):
    err = (got - ref).abs()
    bound = torch.as_tensor(bound, dtype=D).expand_as(err)
    bad = err > bound
    assert not bool(bad.any()), "%s: %d elements out of bound, worst error %.3e at bound %.3e" % (
        what, int(bad.sum()), float(err[bad].max()), float(bound[bad][err[bad].argmax()]))


def dev(t, dtype=torch.float32):
    return t.to(dtype).cuda()


def bn_case(seed, pixels, C, Cz, groups, dt, zf32):
    """z (groups, pixels, Cz) float64 holding values of the storage type, gamma / beta (C) fp32, and the fp32 batch sums (groups, 2, Cz)."""
    z, gamma, beta = R.bn_inputs(seed, pixels, C, Cz, groups, torch.float32 if zf32 else R.TDT[dt])
    stats = torch.stack([z.sum(1), (z * z).sum(1)], 1).float()
    return z, gamma, beta, stats


# ---- BatchNorm, group 1: tedspad_bn_train_apply ----------------------------------------------------------------------------------------------------------
def run_bn_train_apply(dt, z, zf32, stats, gamma, beta, res, relu, wide, rm=None, rv=None):
    G, P, Cz = z.shape
    C = gamma.shape[0]
    ld, off = lds(Cz, wide)
    zin = In(z, ld, off, torch.float32 if zf32 else R.TDT[dt])
    rin = In(res, ld, off, R.TDT[dt]) if res is not None else None
    y = Out(G * P, Cz, ld, off, R.TDT[dt])
    sld = Cz + 4
    st = torch.full((G, 2, sld), 1000.0)
    st[:, :, :Cz] = stats
    st, g_, b_ = st.cuda(), dev(gamma), dev(beta)
    mean, invstd = Out(G, Cz, Cz, 0, torch.float32), Out(G, Cz, Cz, 0, torch.float32)
    rmd, rvd = (dev(rm), dev(rv)) if rm is not None else (None, None)
    ok(L().tedspad_bn_train_apply(zin.ptr, code("f32" if zf32 else dt), st.data_ptr(), sld, P, g_.data_ptr(), b_.data_ptr(), EPS, MOM,
                                  rmd.data_ptr() if rm is not None else None, rvd.data_ptr() if rm is not None else None, mean.ptr, invstd.ptr, C,
                                  rin.ptr if rin else None, y.ptr, P, Cz, ld, ld, ld, int(relu), G, code(dt), S()))
    return y, mean, invstd, rmd, rvd


def check_bn_train_apply(dt, z, zf32, stats, gamma, beta, res, relu, wide, track):
    G, P, Cz = z.shape
    C = gamma.shape[0]
    rm, rv = (R.synth_tensor(2, "rm", (C,), -0.1, 0.1), R.synth_tensor(2, "rv", (C,), 0.5, 1.5)) if track else (None, None)
    y, mean, invstd, rmd, rvd = run_bn_train_apply(dt, z, zf32, stats, gamma, beta, res, relu, wide, rm, rv)
    got, gm, gi = y.get().view(G, P, Cz), mean.get(), invstd.get()
    assert y.intact() and mean.intact() and invstd.intact(), "wrote outside its slice"
    assert float(got[:, :, C:].abs().max() if Cz > C else 0.0) == 0.0, "channels in [C, Cz) must be 0"
    assert bool((gm[:, C:] == SENT).all()) and bool((gi[:, C:] == SENT).all())
    rmr, rvr = (rm.to(D), rv.to(D)) if track else (None, None)
    tol_rm = tol_rv = 0.0
    for g in range(G):
        f = R.bn_train_ref(z[g, :, :C], stats[g, 0, :C], stats[g, 1, :C], P, gamma, beta, EPS, res[g, :, :C] if res is not None else None, relu,
                           momentum=float(np.float32(MOM)), running_mean=rmr, running_var=rvr)
        within(got[g, :, :C], f["y"], R.ULP[dt] * f["y"].abs() + 16 * F32 * f["M"] + R.TINY[dt], "y group %d" % g)
        within(gm[g, :C], f["mean"], 8 * F32 * f["mean"].abs(), "mean")
        within(gi[g, :C], f["invstd"], 8 * F32 * f["invstd"], "invstd")
        if track:
            # the groups' momentum updates, in order: each adds 8 * 2^-24 of its absolute terms to what the earlier ones left
            tol_rm = (1 - MOM) * tol_rm + 8 * F32 * ((1 - MOM) * rmr.abs() + MOM * f["mean"].abs())
            tol_rv = (1 - MOM) * tol_rv + 8 * F32 * f["running_var"].abs()
            rmr, rvr = f["running_mean"], f["running_var"]
    if track:
        within(rmd.cpu().to(D), rmr, tol_rm, "running_mean")
        within(rvd.cpu().to(D), rvr, tol_rv, "running_var")


@pytest.mark.parametrize("C,Cz", R.BN_CHANNELS)
@pytest.mark.parametrize("dt", DTS)
def test_bn_train_apply(dt, C, Cz):
    """Cz >= 256 at these sizes runs the UF = 4 form, below that UF = 1; C < Cz the guarded per-element terms."""
    i = 0
    for pixels in R.BN_PIXELS:
        for groups in (1, 3):
            for zf32 in (False, True):
                z, gamma, beta, stats = bn_case(11, pixels, C, Cz, groups, dt, zf32)
                res = R.synth_tensor(11, "res", (groups, pixels, Cz), -2, 2).to(R.TDT[dt]).to(D)
                for with_res, relu in ((False, False), (False, True), (True, False), (True, True)):
                    i += 1
                    check_bn_train_apply(dt, z, zf32, stats, gamma, beta, res if with_res else None, relu, wide=bool(i & 1) ^ with_res, track=i % 3 != 0)


# ---- BatchNorm, group 2: tedspad_bn_finalize and tedspad_scale_shift_act on their own -----------------------------------------------------------------------
@pytest.mark.parametrize("C", [8, 72, 264])
@pytest.mark.parametrize("dt", DTS)
def test_bn_finalize_and_scale_shift_act(dt, C):
    for pixels in R.BN_PIXELS:
        z, gamma, beta, stats = bn_case(12, pixels, C, C, 1, dt, True)
        rm, rv = R.synth_tensor(2, "rm", (C,), -0.1, 0.1), R.synth_tensor(2, "rv", (C,), 0.5, 1.5)
        res = R.synth_tensor(12, "res", (pixels, C), -2, 2).to(R.TDT[dt]).to(D)
        st = torch.full((2, C + 4), 1000.0)
        st[:, :C] = stats[0]
        st, g_, b_, rmd, rvd = st.cuda(), dev(gamma), dev(beta), dev(rm), dev(rv)
        outs = [Out(1, C, C + 8, 4, torch.float32) for _ in range(4)]          # scale, shift, mean, invstd
        ok(L().tedspad_bn_finalize(st.data_ptr(), C + 4, pixels, g_.data_ptr(), b_.data_ptr(), EPS, MOM, rmd.data_ptr(), rvd.data_ptr(),
                                   outs[0].ptr, outs[1].ptr, outs[2].ptr, outs[3].ptr, C, S()))
        f = R.bn_train_ref(z[0], stats[0, 0], stats[0, 1], pixels, gamma, beta, EPS, None, False, momentum=float(np.float32(MOM)),
                           running_mean=rm, running_var=rv)
        assert all(o.intact() for o in outs)
        sc, sh = outs[0].get()[0], outs[1].get()[0]
        within(sc, f["scale"], 8 * F32 * f["scale"].abs(), "scale")
        within(sh, f["shift"], 8 * F32 * (beta.to(D).abs() + (f["mean"] * f["scale"]).abs()), "shift")
        within(outs[2].get()[0], f["mean"], 8 * F32 * f["mean"].abs(), "mean")
        within(outs[3].get()[0], f["invstd"], 8 * F32 * f["invstd"], "invstd")
        within(rmd.cpu().to(D), f["running_mean"], 8 * F32 * ((1 - MOM) * rm.to(D).abs() + MOM * f["mean"].abs()), "running_mean")
        within(rvd.cpu().to(D), f["running_var"], 8 * F32 * f["running_var"].abs(), "running_var")
        ok(L().tedspad_bn_finalize(st.data_ptr(), C + 4, pixels, g_.data_ptr(), b_.data_ptr(), EPS, MOM, None, None,
                                   outs[0].ptr, outs[1].ptr, outs[2].ptr, outs[3].ptr, C, S()))          # running statistics not tracked
        assert torch.equal(outs[0].get()[0], sc)
        for k, (with_res, relu) in enumerate(((False, False), (True, True), (False, True), (True, False))):
            ld, off = lds(C, k & 1)
            zin, rin, y = In(z[0], ld, off, torch.float32), In(res, ld, off, R.TDT[dt]), Out(pixels, C, ld, off, R.TDT[dt])
            ok(L().tedspad_scale_shift_act(zin.ptr, outs[0].buf.data_ptr() + 16, outs[1].buf.data_ptr() + 16, rin.ptr if with_res else None, y.ptr,
                                           pixels, C, ld, ld, ld, int(relu), code(dt), S()))
            v = z[0] * sc + sh + (res if with_res else 0)             # the kernel's own scale / shift: one multiply-add (+ add) in fp32
            M = (z[0] * sc).abs() + sh.abs() + (res.abs() if with_res else 0)
            ref = v.clamp_min(0) if relu else v
            assert y.intact()
            within(y.get(), ref, R.ULP[dt] * ref.abs() + 16 * F32 * M + R.TINY[dt], "scale_shift_act")


# ---- BatchNorm, groups 3 and 4: tedspad_bn_bwd_reduce, tedspad_bn_bwd_apply ---------------------------------------------------------------------------------
ZM = ["none", "z16", "z32"]
MM = ["nomask", "ymask", "zmask"]
COMBOS = [(zm, mm) for zm in ZM for mm in MM if not (zm == "none" and mm == "zmask")]


def bwd_case(dt, pixels, C, groups, zm, mm):
    """Forward quantities of one case as the backward kernels are handed them: mean / invstd fp32, y rounded to 16 bits; dy dyadic, zeroed in the band
    around 0 of a mask recomputed from z (there the fp32 and the float64 sign of z * s + b may differ). Returns the share of elements that zeroes too."""
    zf32 = zm != "z16"
    z, gamma, beta, stats = bn_case(13, pixels, C, C, groups, dt, zf32)
    mean = (stats[:, 0].to(D) / pixels).float()
    var = (stats[:, 1].to(D) / pixels - mean.to(D) ** 2).clamp_min(0)
    invstd = (1 / torch.sqrt(var + EPS)).float()
    ks = gamma.to(D) * invstd.to(D)                                    # (G, C)
    zs, b = z * ks[:, None], (beta.to(D) - mean.to(D) * ks)[:, None].expand_as(z)
    y = (zs + b).clamp_min(0).to(R.TDT[dt]).to(D)
    dy = R.dyadic(13, "dy", (groups, pixels, C))
    removed = 0.0
    if mm == "zmask":
        band = (zs + b).abs() < 4 * R.ULP[dt] * (zs.abs() + b.abs())
        removed = float(band.double().mean())
        dy = dy * ~band
    return z, gamma, beta, mean, invstd, y, dy, removed


def bwd_refs(z, gamma, beta, mean, invstd, y, dy, mm, sums=None):
    relu = mm != "nomask"
    return [R.bn_bwd_ref(dy[g], y[g] if mm == "ymask" else None, z[g], mean[g], invstd[g], gamma, beta, relu, sums=None if sums is None else sums[g])
            for g in range(z.shape[0])]


@pytest.mark.parametrize("C", R.BN_BWD_C)
@pytest.mark.parametrize("dt", DTS)
def test_bn_bwd_reduce(dt, C):
    removed, sizes, i = [], [], 0
    for pixels in R.BN_BWD_PIXELS:
        for groups in (1, 3):
            for zm, mm in COMBOS:
                i += 1
                z, gamma, beta, mean, invstd, y, dy, rem = bwd_case(dt, pixels, C, groups, zm, mm)
                if mm == "zmask":
                    removed.append(rem)
                    sizes.append(groups * pixels * C)
                refs = bwd_refs(z, gamma, beta, mean, invstd, y, dy, mm)
                wide = bool(i & 1)
                ld, off = lds(C, wide)
                dyi, yi = In(dy, ld, off, R.TDT[dt]), In(y, ld, off, R.TDT[dt])
                zi = In(z, ld, off, torch.float32 if zm == "z32" else R.TDT[dt])
                md, isd, g_, b_ = dev(mean), dev(invstd), dev(gamma), dev(beta)
                sld = C + 8
                sums = torch.zeros((groups, 2, sld), device="cuda")
                ok(L().tedspad_bn_bwd_reduce(dyi.ptr, yi.ptr if mm == "ymask" else None, zi.ptr if zm != "none" else None, code("f32" if zm == "z32" else dt),
                                             md.data_ptr(), isd.data_ptr(), g_.data_ptr(), b_.data_ptr(), sums.data_ptr(), sld, pixels, C, ld, ld, ld,
                                             int(mm != "nomask"), groups, code(dt), S()))
                got = sums.cpu().to(D)
                assert float(got[:, :, C:].abs().max()) == 0.0, "wrote between the rows of `sums`"
                for g, f in enumerate(refs):
                    what = "%s %s pixels %d group %d/%d" % (zm, mm, pixels, g, groups)
                    assert torch.equal(got[g, 0, :C], f["sum_g"]), "sum g is not exact: " + what            # dyadic: a dropped or doubled pixel cannot hide
                    if zm == "none":
                        assert float(got[g, 1].abs().max()) == 0.0, what
                    else:
                        within(got[g, 1, :C], f["sum_gx"], (pixels + 8) * F32 * f["abs_gx"], "sum g*xhat " + what)
    assert sum(removed) / len(removed) < 0.02, removed        # the band around 0 costs the mask-from-z cases < 2 % of their elements
    assert all(r < 0.02 for r, n in zip(removed, sizes) if n >= 255 * 8), list(zip(removed, sizes))      # and every case that has enough elements for a share


def apply_grid(pixels, C):          # the launcher's own grid (grid_for_iters(items, 8)): which dbias rows a launch can touch
    items = pixels * (C // 8)
    g, full = -(-items // 2048), -(-items // 256)
    if g < 512:
        g = min(full, 512)
    return max(1, min(g, 4096))


@pytest.mark.parametrize("C", R.BN_BWD_C)
@pytest.mark.parametrize("dt", DTS)
def test_bn_bwd_apply(dt, C):
    """C / 8 = 1, 3, 5, 9, 33 at these pixel counts: the LDS-tree, per-thread-atomic and per-element-atomic forms of the fused bias gradient."""
    i = 0
    for pixels in R.BN_BWD_PIXELS:
        for groups in (1, 3):
            for zm, mm in [c for c in COMBOS if c[0] != "none"]:
                i += 1
                z, gamma, beta, mean, invstd, y, dy, _ = bwd_case(dt, pixels, C, groups, zm, mm)
                exact = bwd_refs(z, gamma, beta, mean, invstd, y, dy, mm)
                sums = torch.stack([torch.stack([f["sum_g"], f["sum_gx"]]) for f in exact]).float()        # (G, 2, C): the reference's sums, in fp32
                refs = bwd_refs(z, gamma, beta, mean, invstd, y, dy, mm, sums=sums)
                wide, slots = bool(i & 1), (1, 4)[(i >> 1) & 1]
                ld, off = lds(C, wide)
                dyi, yi = In(dy, ld, off, R.TDT[dt]), In(y, ld, off, R.TDT[dt])
                zi = In(z, ld, off, torch.float32 if zm == "z32" else R.TDT[dt])
                md, isd, g_, b_ = dev(mean), dev(invstd), dev(gamma), dev(beta)
                sld = C + 8
                sd = torch.full((groups, 2, sld), 1000.0)
                sd[:, :, :C] = sums
                sd = sd.cuda()
                dz, dres = Out(groups * pixels, C, ld, off, R.TDT[dt]), Out(groups * pixels, C, ld, off, R.TDT[dt])
                dbias = torch.zeros((slots + 1, C), device="cuda")
                ok(L().tedspad_bn_bwd_apply(dyi.ptr, yi.ptr if mm == "ymask" else None, zi.ptr, code("f32" if zm == "z32" else dt), md.data_ptr(), isd.data_ptr(),
                                            g_.data_ptr(), b_.data_ptr(), sd.data_ptr(), sld, dz.ptr, dres.ptr, dbias.data_ptr(), slots, pixels, C,
                                            ld, ld, ld, ld, ld, int(mm != "nomask"), groups, code(dt), S()))
                assert dz.intact() and dres.intact(), "wrote outside its slice"
                gdz, gdres, gdb = dz.get().view(groups, pixels, C), dres.get().view(groups, pixels, C), dbias.cpu().to(D)
                want_db, abs_dz, max_dz = torch.zeros(C, dtype=D), torch.zeros(C, dtype=D), 0.0
                for g, f in enumerate(refs):
                    what = "%s %s pixels %d group %d/%d" % (zm, mm, pixels, g, groups)
                    terms = (f["ks"] * f["g"]).abs() + (f["A"] * z[g]).abs() + f["B"].abs()
                    within(gdz[g], f["dz"], R.ULP[dt] * f["dz"].abs() + 16 * F32 * terms + R.TINY[dt], "dz " + what)
                    assert torch.equal(gdres[g], f["dres"]), "dres is a 16-bit copy of the masked dy: " + what
                    want_db += gdz[g].sum(0)
                    abs_dz += gdz[g].abs().sum(0)
                    max_dz = max(max_dz, float(gdz[g].abs().max()))
                used = min(slots, apply_grid(pixels, C))
                assert float(gdb[used:].abs().max()) == 0.0, "dbias rows beyond the grid (and beyond dbias_slots) must stay 0"
                n = groups * pixels
                within(gdb.sum(0), want_db, (n + 8) * F32 * abs_dz + n * R.ULP[dt] / 2 * max_dz, "dbias %s %s pixels %d slots %d" % (zm, mm, pixels, slots))
                ok(L().tedspad_bn_bwd_apply(dyi.ptr, yi.ptr if mm == "ymask" else None, zi.ptr, code("f32" if zm == "z32" else dt), md.data_ptr(), isd.data_ptr(),
                                            g_.data_ptr(), b_.data_ptr(), sd.data_ptr(), sld, dz.ptr, None, None, 1, pixels, C,
                                            ld, ld, ld, ld, ld, int(mm != "nomask"), groups, code(dt), S()))
                # without dres / dbias (another instantiation of the kernel: its multiply-adds may be contracted differently): dz held to the same bound
                assert dz.intact()
                gdz2 = dz.get().view(groups, pixels, C)
                for g, f in enumerate(refs):
                    terms = (f["ks"] * f["g"]).abs() + (f["A"] * z[g]).abs() + f["B"].abs()
                    within(gdz2[g], f["dz"], R.ULP[dt] * f["dz"].abs() + 16 * F32 * terms + R.TINY[dt], "dz without dbias, group %d" % g)


def test_bn_bwd_apply_refuses_3528_channels():
    from ted_spad_amd import _lib
    C = 3528                    # [4][C] fp32 terms + the 9 KB reduction image exceed 64 KB from here on (the documented limit is 3520)
    t = torch.zeros(8, C, device="cuda")
    h = t.half()
    p = t.data_ptr()
    args = lambda c: (h.data_ptr(), None, p, _lib.F32, p, p, p, p, p, c, h.data_ptr(), None, None, 1, 8, c, c, c, c, c, 0, 0, 1, _lib.F16, S())
    assert L().tedspad_bn_bwd_apply(*args(C)) == -1           # TEDSPAD_EINVAL
    assert L().tedspad_bn_bwd_apply(*args(3520)) == 0, _lib.last_error()
    torch.cuda.synchronize()


# ---- BatchNorm, group 5: the launchers' rolled forms (their A/B knobs, read once per process: a child) against this process's -------------------------------
def unroll_cases():
    out = {}
    for dt in DTS:
        for C in (72, 512):
            for pixels in (37, 64):          # one workgroup per channel group in the reduce: no atomic-order freedom
                z16, gamma, beta, st16 = bn_case(14, pixels, C, C, 1, dt, False)
                z32, _, _, st32 = bn_case(14, pixels, C, C, 1, dt, True)
                res = R.synth_tensor(14, "res", (1, pixels, C), -2, 2).to(R.TDT[dt]).to(D)
                key = "%s_%d_%d_" % (dt, C, pixels)
                for zf32, z, st in ((False, z16, st16), (True, z32, st32)):
                    y, mean, invstd, _, _ = run_bn_train_apply(dt, z, zf32, st, gamma, beta, res, True, True)
                    out[key + "y%d" % zf32] = y.raw().view(torch.int16).numpy()
                    out[key + "mean%d" % zf32], out[key + "invstd%d" % zf32] = mean.raw().numpy(), invstd.raw().numpy()
                for zm, mm in COMBOS:
                    zz, gamma, beta, mean, invstd, y, dy, _ = bwd_case(dt, pixels, C, 1, zm, mm)
                    dyi, yi, zi = In(dy, C, 0, R.TDT[dt]), In(y, C, 0, R.TDT[dt]), In(zz, C, 0, torch.float32 if zm == "z32" else R.TDT[dt])
                    md, isd, g_, b_ = dev(mean), dev(invstd), dev(gamma), dev(beta)
                    sums = torch.zeros((2, C), device="cuda")
                    ok(L().tedspad_bn_bwd_reduce(dyi.ptr, yi.ptr if mm == "ymask" else None, zi.ptr if zm != "none" else None, code("f32" if zm == "z32" else dt),
                                                 md.data_ptr(), isd.data_ptr(), g_.data_ptr(), b_.data_ptr(), sums.data_ptr(), C, pixels, C, C, C, C,
                                                 int(mm != "nomask"), 1, code(dt), S()))
                    out[key + "sums_" + zm + mm] = sums.cpu().numpy()
    return out


def test_bn_unrolled_and_rolled_forms_bit_identical(tmp_path):
    """TEDSPAD_BNR_UNROLL=1 / TEDSPAD_BNA_UNROLL=1 keep the rolled loops everywhere; this process takes the launchers' own choice (UF = 4 at these sizes for
    the reduce and for the C = 512 apply). 'The sums keep their bits': every output must be bit-identical."""
    assert "TEDSPAD_BNR_UNROLL" not in os.environ and "TEDSPAD_BNA_UNROLL" not in os.environ
    path = str(tmp_path / "rolled.npz")
    env = dict(os.environ, TEDSPAD_BNR_UNROLL="1", TEDSPAD_BNA_UNROLL="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, timeout=120, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rolled, here = dict(np.load(path)), unroll_cases()
    assert sorted(rolled) == sorted(here) and len(here) > 100
    for k in here:
        assert here[k].tobytes() == rolled[k].tobytes(), k


# ---- max-pool forward with indices + backward ----------------------------------------------------------------------------------------------------------------
def pool_desc(n, thw, c, ldx, ldy, k, s, p, out, dt):
    from ted_spad_amd import _lib
    return _lib.PoolDesc(n, thw[0], thw[1], thw[2], c, ldx, ldy, k[0], k[1], k[2], s[0], s[1], s[2], p[0], p[1], p[2], out[0], out[1], out[2], 0, code(dt))


def run_maxpool(dt, x, k, s, p, dy=None, add=None, relu_mask=False):
    """x (n, t, h, w, c) float64 -> y, idx (and dx): every tensor a channel slice of a wider buffer."""
    n, thw, c = x.shape[0], tuple(x.shape[1:4]), x.shape[4]
    out = tuple(R.pool_out(a, b, d, e) for a, b, d, e in zip(thw, k, s, p))
    npx, nout = n * thw[0] * thw[1] * thw[2], n * out[0] * out[1] * out[2]
    xi, y = In(x, c + 16, 8, R.TDT[dt]), Out(nout, c, c + 24, 16, R.TDT[dt])
    idx = Out(nout, c, c, 0, torch.uint8, fill=200)
    d = pool_desc(n, thw, c, xi.ld, y.ld, k, s, p, out, dt)
    ok(L().tedspad_maxpool_fwd_idx(Ct.byref(d), xi.ptr, y.ptr, idx.ptr, S()))
    assert y.intact() and idx.intact()
    shape = (n,) + out + (c,)
    dx = None
    if dy is not None:
        dyi = In(dy, c + 8, 8, R.TDT[dt])
        addi = In(add, c + 16, 0, R.TDT[dt]) if add is not None else None
        dxo = Out(npx, c, c + 16, 8, R.TDT[dt])
        ok(L().tedspad_maxpool_bwd(Ct.byref(d), xi.ptr, idx.ptr, dyi.ptr, dyi.ld, addi.ptr if addi else None, addi.ld if addi else 0, dxo.ptr, dxo.ld,
                                   int(relu_mask), S()))
        assert dxo.intact()
        dx = dxo.get().view(x.shape)
    return y.get().view(shape), idx.raw().view(shape), dx


_pool_ref_cache = {}


def pool_ref(case, c):
    if (case[0], c) not in _pool_ref_cache:
        _, k, s, p, thw = case
        x = R.tie_values(7, "px", (2,) + thw + (c,))
        y, idx = R.maxpool_fwd_ref(x, k, s, p)
        dy, add = R.dyadic(7, "pdy", tuple(y.shape)), R.dyadic(7, "padd", tuple(x.shape))
        _pool_ref_cache[(case[0], c)] = (x, y, idx, dy, add, R.maxpool_bwd_ref(x, idx, dy, k, s, p), R.maxpool_bwd_ref(x, idx, dy, k, s, p, add=add, relu_mask=True))
    return _pool_ref_cache[(case[0], c)]


@pytest.mark.parametrize("case", R.POOL_CASES, ids=[c[0] for c in R.POOL_CASES])
@pytest.mark.parametrize("dt", DTS)
def test_maxpool_idx_and_backward_on_ties(dt, case):
    """ReLU-like inputs (half the values exactly 0): 'first maximum wins, as torch' decides most windows. y and dx bit for bit (dyadic gradients: every
    sum is exact), the index tensor everywhere. k2s2_fast runs maxpool_bwd_k2s2_kernel, k2s2_odd the generic kernel beside it (its last row and column
    lie in no window: dx = add there), the *_pad cases front padding."""
    _, k, s, p, thw = case
    for c in R.POOL_C:
        x, y, idx, dy, add, dx_plain, dx_full = pool_ref(case, c)
        gy, gidx, gdx = run_maxpool(dt, x, k, s, p, dy=dy)
        assert torch.equal(gy, y), "y c=%d" % c
        assert torch.equal(gidx, idx), "idx c=%d: %d of %d differ" % (c, int((gidx != idx).sum()), idx.numel())
        assert torch.equal(gdx, dx_plain), "dx c=%d" % c
        _, _, gdx = run_maxpool(dt, x, k, s, p, dy=dy, add=add, relu_mask=True)
        assert torch.equal(gdx, dx_full), "dx (+ add, ReLU mask) c=%d" % c


@pytest.mark.parametrize("dt", DTS)
def test_maxpool_idx_propagates_inf_and_nan(dt):
    """The training forward must hand an overflow on (DESIGN.md 'training precision'): +inf stays +inf (not the largest finite value), a NaN in a window
    makes the output NaN, with torch's index (the last NaN of the window) -- torch.nn.functional.max_pool3d's rule, in kernel_refs.maxpool_fwd_ref."""
    k, s, p, thw = (1, 3, 3), (1, 2, 2), (0, 1, 1), (1, 6, 6)
    x = R.tie_values(8, "nf", (1,) + thw + (8,))
    x[0, 0, 0, 0, :] = float("inf")
    x[0, 0, 2, 3, 0], x[0, 0, 3, 3, 0] = float("nan"), float("nan")
    x[0, 0, 5, 5, :] = float("-inf")
    y, idx = R.maxpool_fwd_ref(x, k, s, p)
    gy, gidx, _ = run_maxpool(dt, x, k, s, p)
    assert bool(torch.isinf(gy[0, 0, 0, 0]).all()) and bool((gy[0, 0, 0, 0] > 0).all()), gy[0, 0, 0, 0]
    assert torch.equal(torch.isnan(gy), torch.isnan(y)) and int(torch.isnan(y).sum()) >= 2
    assert torch.equal(torch.nan_to_num(gy, 7.0), torch.nan_to_num(y, 7.0))
    assert torch.equal(gidx, idx)


# ---- resize / copy / layout ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_upsample_nearest2x_fwd_bwd(dt):
    for h, w in ((1, 1), (3, 5), (8, 8)):
        for c in (8, 40):
            x = R.dyadic(21, "nx", (2, h, w, c))
            xi, y = In(x, c + 8, 0, R.TDT[dt]), Out(2 * 4 * h * w, c, c + 24, 8, R.TDT[dt])
            ok(L().tedspad_upsample_nearest2x_fwd(xi.ptr, y.ptr, 2, h, w, c, xi.ld, y.ld, S()))
            assert y.intact() and torch.equal(y.get().view(2, 2 * h, 2 * w, c), R.nearest2x_ref(x))
            dy = R.dyadic(21, "ndy", (2, 2 * h, 2 * w, c))
            old = R.dyadic(21, "nold", (2, h, w, c))
            for acc in (0, 1):
                dyi, dx = In(dy, c + 16, 8, R.TDT[dt]), Out(2 * h * w, c, c + 8, 8, R.TDT[dt], init=old)
                ok(L().tedspad_upsample_nearest2x_bwd(dyi.ptr, dx.ptr, 2, h, w, c, dyi.ld, dx.ld, acc, code(dt), S()))
                want = (R.nearest2x_bwd_ref(dy) + (old if acc else 0)).to(R.TDT[dt]).to(D)        # |sum| <= 10: exact up to the one 16-bit rounding
                assert dx.intact() and torch.equal(dx.get().view(2, h, w, c), want), (h, w, c, acc)


@pytest.mark.parametrize("dt", DTS)
def test_copy_and_add_channels(dt):
    for npix in (1, 257):
        for c in (8, 72):
            x, old = R.dyadic(22, "cx", (npix, c)), R.dyadic(22, "cold", (npix, c))
            xi, y = In(x, c + 8, 8, R.TDT[dt]), Out(npix, c, c + 32, 16, R.TDT[dt], init=old)
            ok(L().tedspad_add_channels(xi.ptr, y.ptr, npix, c, xi.ld, y.ld, code(dt), S()))
            assert y.intact() and torch.equal(y.get(), x + old)              # multiples of 1/16 up to 4: exact in both types
            ok(L().tedspad_copy_channels(xi.ptr, y.ptr, npix, c, xi.ld, y.ld, S()))
            assert y.intact() and torch.equal(y.get(), x)


@pytest.mark.parametrize("h,w,ho,wo", R.BILINEAR_CASES)
@pytest.mark.parametrize("dt", DTS)
def test_upsample_bilinear2x_fwd_and_bf16_bwd(dt, h, w, ho, wo):
    from conftest import rel_l2
    pt, pl = R.bilinear_pad(h, w, ho, wo)
    for c in (8, 24):
        x = R.synth_tensor(23, "bx", (2, h, w, c), -1, 1).to(R.TDT[dt]).to(D)
        ref, taps = R.bilinear2x_ref(x, ho, wo)
        xi, y = In(x, c + 8, 0, R.TDT[dt]), Out(2 * ho * wo, c, c + 16, 8, R.TDT[dt])
        ok(L().tedspad_upsample_bilinear2x_fwd(xi.ptr, y.ptr, 2, h, w, c, xi.ld, y.ld, ho, wo, pt, pl, code(dt), S()))
        got = y.get().view(2, ho, wo, c)
        assert y.intact()
        within(got, ref, R.ULP[dt] * ref.abs() + 2.0 ** -20 * taps, "bilinear %dx%d c=%d" % (h, w, c))
        border = torch.ones(ho, wo, dtype=torch.bool)
        border[pt:pt + 2 * h, pl:pl + 2 * w] = False
        assert float(got[:, border].abs().max() if border.any() else 0.0) == 0.0, "the zero border"
        # backward (bf16 here; f16 also in test_pool_and_upsample_backward): its 2e-3 rel-L2, x 8 for bf16's three fewer mantissa bits
        g = R.synth_tensor(23, "bg", (2, ho, wo, c), -1, 1).to(R.TDT[dt]).to(D)
        gi, dx = In(g, c + 16, 8, R.TDT[dt]), Out(2 * h * w, c, c + 8, 0, R.TDT[dt])
        ok(L().tedspad_upsample_bilinear2x_bwd(gi.ptr, dx.ptr, 2, h, w, c, gi.ld, dx.ld, ho, wo, pt, pl, code(dt), S()))
        assert dx.intact()
        assert rel_l2(dx.get().view(2, h, w, c).numpy(), R.bilinear2x_bwd_ref(g, h, w).numpy()) < 2e-3 * (8 if dt == "bf16" else 1)
        g2 = g.clone()
        g2[:, border] = 5.0                    # gradient arriving in the zero border reaches no input element
        gi2, dx2 = In(g2, c + 16, 8, R.TDT[dt]), Out(2 * h * w, c, c + 8, 0, R.TDT[dt])
        ok(L().tedspad_upsample_bilinear2x_bwd(gi2.ptr, dx2.ptr, 2, h, w, c, gi2.ld, dx2.ld, ho, wo, pt, pl, code(dt), S()))
        assert torch.equal(dx2.get(), dx.get())


@pytest.mark.parametrize("dt", DTS)
def test_global_avgpool_fwd_bwd(dt):
    for spatial in (1, 2, 3, 5, 98):
        for c in (8, 520):
            x = R.dyadic(24, "gx", (3, spatial, c))
            xi = In(x, c + 8, 0, R.TDT[dt])
            y = Out(3, c, c, 0, torch.float32)
            ok(L().tedspad_global_avgpool_fwd(xi.ptr, y.ptr, 3, spatial, c, xi.ld, code(dt), S()))
            ref = x.sum(1) / spatial                 # the fp32 sum is exact: one multiply by fl(1 / spatial) remains
            assert y.intact()
            within(y.get(), ref, 2.0 ** -23 * ref.abs(), "avgpool fwd spatial %d c %d" % (spatial, c))
            df = R.synth_tensor(24, "gdf", (3, c), -1, 1)
            mask = R.tie_values(24, "gm", (3, spatial, c))
            inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(spatial), dtype=torch.float32)
            full = (df * inv).view(3, 1, c).expand(3, spatial, c)              # the kernel's single fp32 product, then the one 16-bit rounding
            dfd = dev(df)
            for m in (None, mask):
                mi = In(m, c + 8, 8, R.TDT[dt]) if m is not None else None
                dx = Out(3 * spatial, c, c + 16, 8, R.TDT[dt])
                ok(L().tedspad_global_avgpool_bwd(dfd.data_ptr(), mi.ptr if mi else None, mi.ld if mi else 0, dx.ptr, 3, spatial, c, dx.ld, code(dt), S()))
                want = (full * (m > 0) if m is not None else full).to(R.TDT[dt]).to(D)
                assert dx.intact() and torch.equal(dx.get().view(3, spatial, c), want), (spatial, c, m is not None)


@pytest.mark.parametrize("dt", DTS)
def test_avgpool3d_s1_fwd(dt):
    kt, kh, kw, c = 2, 3, 3, 16
    for t, h, w in ((2, 3, 3), (3, 4, 4)):             # the map equal to the kernel, and one larger in each dimension
        x = R.dyadic(25, "ax", (2, t, h, w, c))
        xi = In(x, c + 8, 8, R.TDT[dt])
        to, ho, wo = t - kt + 1, h - kh + 1, w - kw + 1
        y = Out(2 * c, to * ho * wo, to * ho * wo, 0, torch.float32)
        ok(L().tedspad_avgpool3d_s1_fwd(xi.ptr, y.ptr, 2, t, h, w, c, xi.ld, kt, kh, kw, code(dt), S()))
        ref = torch.nn.functional.avg_pool3d(x.permute(0, 4, 1, 2, 3), (kt, kh, kw), 1)
        assert y.intact()
        within(y.get().view(2, c, to, ho, wo), ref, 2.0 ** -23 * ref.abs(), "avgpool3d")


@pytest.mark.parametrize("dt", DTS)
def test_layout_conversions(dt):
    for c in (1, 3, 8):
        for sig in (False, True):
            gy = R.dyadic(26, "lg", (2, c, 35))
            ys = torch.sigmoid(R.synth_tensor(26, "ls", (2, c, 35), -2, 2))
            out = Out(2 * 35, 8, 8, 0, R.TDT[dt])
            gyd, ysd = dev(gy), dev(ys)
            ok(L().tedspad_nchw_grad_to_channels_last(gyd.data_ptr(), ysd.data_ptr() if sig else None, out.ptr, 2, c, 35, code(dt), S()))
            got = out.get().view(2, 35, 8)
            assert out.intact() and float(got[..., c:].abs().max() if c < 8 else 0.0) == 0.0
            ref = (gy * (ys.to(D) * (1 - ys.to(D))) if sig else gy).permute(0, 2, 1)
            within(got[..., :c], ref, R.ULP[dt] * ref.abs() + 4 * F32 * ref.abs() + R.TINY[dt], "nchw_grad_to_channels_last")
    # 16-bit channels-last -> a non-contiguous view of a larger fp32 tensor
    n, c, t, h, w = 2, 3, 2, 3, 5
    x = R.dyadic(26, "sx", (n, t, h, w, c))
    xi = In(x, 8, 0, R.TDT[dt])
    big = torch.full((n, c + 1, t + 1, h + 2, w + 3), SENT, device="cuda")
    view = big[:, 1:, :t, 1:1 + h, 2:2 + w]
    sn, sc, st_, sh, sw = view.stride()
    ok(L().tedspad_channels_last_to_nchw_strided(xi.ptr, view.data_ptr(), n, c, t, h, w, 8, sn, sc, st_, sh, sw, code(dt), S()))
    assert torch.equal(view.cpu().to(D), x.permute(0, 4, 1, 2, 3))
    m = torch.ones(big.shape, dtype=torch.bool)
    m[:, 1:, :t, 1:1 + h, 2:2 + w] = False
    assert bool((big.cpu()[m] == SENT).all())


@pytest.mark.parametrize("dt", DTS)
def test_count_saturated(dt):
    rows, c, ld = 37, 16, 32
    bits = {"f16": dict(sat=0x7BFF, pinf=0x7C00, ninf=0xFC00, nan=0x7E00, one=0x3C00), "bf16": dict(sat=0x7F7F, pinf=0x7F80, ninf=0xFF80, nan=0x7FC0, one=0x3F80)}[dt]
    a = np.full((rows, ld), bits["one"], np.uint16)
    a[:, c:] = np.array([bits["sat"], bits["pinf"], bits["nan"], bits["ninf"]] * ((ld - c) // 4), np.uint16)       # the gap channels: never counted
    a[0, 0] = a[5, 15] = a[36, 7] = bits["sat"]
    a[1, 1] = a[36, 15] = bits["sat"] | 0x8000           # the negative limit
    a[2, 3] = a[20, 8] = bits["pinf"]
    a[3, 4] = bits["ninf"]
    a[4, 5] = a[36, 0] = a[17, 9] = bits["nan"]
    x = torch.from_numpy(a.view(np.int16)).cuda()
    out = torch.tensor([10, 20, 30], dtype=torch.int32).cuda()             # both counters are ADDED to
    ok(L().tedspad_count_saturated(x.data_ptr(), rows, c, ld, code(dt), out.data_ptr(), S()))
    assert out.cpu().tolist() == [10 + (5 if dt == "f16" else 0), 20 + 6, 30]          # bf16 stores are never clamped: nothing counts as saturated


if __name__ == "__main__":          # the child of test_bn_unrolled_and_rolled_forms_bit_identical
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    np.savez(sys.argv[1], **unroll_cases())
