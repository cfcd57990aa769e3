"""-m gpu: every entry point of csrc/mgfn.hip and csrc/mgfn_train.hip except tedspad_mgfn_msnsd, through the C ABI, element by element against the float64
references of tests/kernel_refs.py and their per-element bounds (derivations: the references' docstrings; the transcendental constants K_* = 11 are 10x the
ratios test_kernel_refs.py::test_mgfn_transcendental_constants measures: exp 1.04, erf 1.05, log 1.03, sqrt 1.07). A failure names the worst element.

Every case runs twice: with dense rows, and with every input and output in a buffer of ld = width + 4 (width + 1 where the kernel's access is scalar). Inputs
carry NaN in their gap columns and in two guard rows; outputs are prefilled with a sentinel, which gap columns and guard rows must still hold after the launch;
the two payloads must be equal bit for bit. Then: sequence isolation (the other sequences' rows set to NaN change no bit of the target's and leave it finite),
tile tails, hard values, and the refusals (a negative code, a message, the outputs untouched).

What a broken kernel trips, from reading the tests (each names the element): `src <= hi` for `src < hi` in gemm_kernel: test_gemm_tails (taps 3 and 5: the last row
of a sequence takes in the next one's first row; the last sequence the NaN guard row) and test_isolation_gemm_taps3; in relpos_kernel: test_relpos_tails,
test_isolation_relpos. attention_kernel without the `kval` mask: test_attention_tails (T = 31, 33, 65: the clamped last key counted again), test_attention_hard_values,
test_isolation_attention's lengths 5, 33, 7. `/ (C / heads)` for `% heads`: test_relpos_tails at heads 3 and 16. transpose_kernel without the zero fill up to ldo:
test_transpose_wgrad_tails at M % 16 != 0 (the sentinel stays in the padding; the image is compared exactly, and wgrad sums it). col_partial_kernel without the `min`:
test_col_reduce_tails and test_batchnorm_tails at every M that is no multiple of 128 (the NaN guard rows enter the sums)."""
import ctypes as Ct

import numpy as np
import pytest
import torch

import kernel_refs as R

pytestmark = pytest.mark.gpu
D = torch.float64
SENT = 1024.0
NAN = float("nan")
EPS, MOM = 1e-5, 0.1


def L():
    from ted_spad_amd import _lib
    return _lib.lib()


def S():
    return Ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def last_error():
    msg = L().tedspad_last_error()
    return msg.decode() if msg else ""


def ok(rc):
    assert rc == 0, last_error()


def syn(seed, name, shape, lo=-1.0, hi=1.0):
    return R.synth_tensor(seed, name, shape, lo, hi)


# ---- guarded buffers ------------------------------------------------------------------------------------------------------------------------------------
def inp(t, pad=0):
    """device copy of the (rows, width) fp32 matrix t in a (rows + 2, width + pad) buffer of NaN: gap columns and two guard rows; returns (buffer, ld)"""
    t = t.reshape(t.shape[0], -1).float()
    buf = torch.full((t.shape[0] + 2, t.shape[1] + pad), NAN, device="cuda")
    buf[:t.shape[0], :t.shape[1]] = t.cuda()
    return buf, t.shape[1] + pad


def out(rows, width, pad=0):
    """a (rows + 2, width + pad) device buffer of the sentinel; returns (buffer, ld)"""
    return torch.full((rows + 2, width + pad), SENT, device="cuda"), width + pad


def take(buf, rows, width, what):
    """the (rows, width) payload on the host, after checking that the gap columns and the guard rows still hold the sentinel"""
    b = buf.cpu()
    assert bool((b[rows:] == SENT).all()), "%s: a guard row was written" % what
    assert bool((b[:rows, width:] == SENT).all()), "%s: a gap column was written" % what
    return b[:rows, :width].clone()


def i32(t):
    return torch.as_tensor(t).to(torch.int32).cuda()


def within(got, ref_bound, what):
    ref, bound = ref_bound
    msg = R.worst(got.reshape(ref.shape), ref, bound)
    assert not msg, "%s: %s" % (what, msg)


def same_bits(a, b, what):
    a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    if not torch.equal(a, b):
        idx = tuple(int(i) for i in (a != b).nonzero()[0])
        raise AssertionError("%s: %d elements differ in bits, first at %s" % (what, int((a != b).sum()), idx))


def both(run, what):
    """run(strided) -> dict of host tensors: once dense, once strided; the payloads equal bit for bit. Returns the dense result."""
    dense, strided = run(False), run(True)
    for k in dense:
        same_bits(dense[k], strided[k], "%s %s: dense against strided rows" % (what, k))
    return dense


# ---- launchers: each returns a dict of host payloads, guards checked ------------------------------------------------------------------------------------------
def run_ln_stats(x, torch_ln, strided):
    M, C = x.shape
    X, ldx = inp(x, 4 * strided)
    st, _ = out(M, 2)
    ok(L().tedspad_mgfn_ln_stats(X.data_ptr(), ldx, M, C, EPS, torch_ln, st.data_ptr(), S()))
    return {"stats": take(st, M, 2, "ln_stats")}


def run_gemm(x, bounds, taps, w, bias, gelu, res, stats, N, strided):
    M, cin = x.shape
    X, ldx = inp(x, 4 * strided)
    Wd = w.reshape(N, taps * cin).float().cuda().contiguous()
    Bd = bias.float().cuda() if bias is not None else None
    Rb, ldr = inp(res, 1 * strided) if res is not None else (None, 0)
    St = inp(stats, 0)[0] if stats is not None else None
    Bn = i32(bounds) if bounds is not None else None
    Y, ldy = out(M, N, 1 * strided)
    ok(L().tedspad_mgfn_gemm(X.data_ptr(), ldx, Bn.data_ptr() if Bn is not None else None, taps, cin, St.data_ptr() if St is not None else None, Wd.data_ptr(),
                             Bd.data_ptr() if Bd is not None else None, int(gelu), Rb.data_ptr() if Rb is not None else None, ldr, Y.data_ptr(), ldy, M, N, S()))
    return {"y": take(Y, M, N, "gemm")}


def run_attention(qkv, off, heads, tmax, strided, do=None):
    """forward, and with do the backward on the forward's own output: o, dqkv, lse"""
    M, inner = qkv.shape[0], 64 * heads
    Q, ldq = inp(qkv, 4 * strided)
    Of = i32(off)
    O, ldo = out(M, inner, 1 * strided)
    ok(L().tedspad_mgfn_attention(Q.data_ptr(), ldq, Of.data_ptr(), len(off) - 1, tmax, heads, O.data_ptr(), ldo, S()))
    r = {"o": take(O, M, inner, "attention")}
    if do is not None:
        Oi, ldoi = inp(r["o"], 4 * strided)
        Dd, ldd = inp(do, 4 * strided)
        G, ldg = out(M, 3 * inner, 1 * strided)
        Ls, _ = out(M, 2 * heads)
        ok(L().tedspad_mgfn_attention_bwd(Q.data_ptr(), ldq, Oi.data_ptr(), ldoi, Dd.data_ptr(), ldd, Of.data_ptr(), len(off) - 1, tmax, heads, Ls.data_ptr(),
                                          G.data_ptr(), ldg, S()))
        r["dqkv"], r["lse"] = take(G, M, 3 * inner, "attention_bwd dqkv"), take(Ls, M, 2 * heads, "attention_bwd lse")
    return r


def run_relpos(v, bounds, heads, w, b, strided, dout=None):
    M, C = v.shape
    V, ldv = inp(v, 4 * strided)
    Bn, Wd, Bd = i32(bounds), w.float().cuda().contiguous(), b.float().cuda()
    O, ldo = out(M, C, 4 * strided)
    ok(L().tedspad_mgfn_relpos(V.data_ptr(), ldv, Bn.data_ptr(), M, C, heads, Wd.data_ptr(), Bd.data_ptr(), O.data_ptr(), ldo, S()))
    r = {"out": take(O, M, C, "relpos")}
    if dout is not None:
        Dd, ldd = inp(dout, 4 * strided)
        ws = torch.full((int(L().tedspad_mgfn_train_ws_floats(M, C)),), NAN, device="cuda")
        DV, lddv = out(M, C, 4 * strided)
        DW, _ = out(heads, 5)
        DB, _ = out(heads, 1)
        ok(L().tedspad_mgfn_relpos_bwd(Dd.data_ptr(), ldd, V.data_ptr(), ldv, Bn.data_ptr(), M, C, heads, Wd.data_ptr(), ws.data_ptr(), DV.data_ptr(), lddv,
                                       DW.data_ptr(), DB.data_ptr(), S()))
        r.update(dv=take(DV, M, C, "relpos_bwd dv"), dw=take(DW, heads, 5, "relpos_bwd dw"), db=take(DB, heads, 1, "relpos_bwd db"))
    return r


def run_head(x, lw, lb, fw, fb, strided, with_h=True):
    M, C = x.shape
    X, ldx = inp(x, 4 * strided)
    lwd, lbd, fwd = lw.float().cuda(), lb.float().cuda(), fw.float().cuda()
    H, _ = out(M, C)
    lg, sc, mg = out(M, 1)[0], out(M, 1)[0], out(M, 1)[0]
    ok(L().tedspad_mgfn_head(X.data_ptr(), ldx, M, C, lwd.data_ptr(), lbd.data_ptr(), fwd.data_ptr(), fb, EPS, H.data_ptr() if with_h else None, lg.data_ptr(),
                             sc.data_ptr(), mg.data_ptr(), S()))
    r = {"logit": take(lg, M, 1, "head logit"), "score": take(sc, M, 1, "head score"), "mag": take(mg, M, 1, "head mag")}
    if with_h:
        r["h"] = take(H, M, C, "head h")
    else:
        assert bool((H == SENT).all())
    return r


def run_head_bwd(score, dscore, fw, dh):
    M, C = dh.shape
    sd, dd, fwd = inp(score.reshape(M, 1))[0], inp(dscore.reshape(M, 1))[0], fw.float().cuda()
    DH, _ = out(M, C)
    DH[:M] = dh.cuda()
    DZ, _ = out(M, 1)
    ok(L().tedspad_mgfn_head_bwd(sd.data_ptr(), dd.data_ptr(), fwd.data_ptr(), M, C, DH.data_ptr(), DZ.data_ptr(), S()))
    return {"dh": take(DH, M, C, "head_bwd dh"), "dz": take(DZ, M, 1, "head_bwd dz")}


def run_ln_apply_bwd(x, stats, g, b, dy, add, torch_ln, strided):
    M, C = x.shape
    p = 4 * strided
    X, ldx = inp(x, p)
    St = inp(stats)[0]
    gd, bd = g.float().cuda(), b.float().cuda()
    Y, ldy = out(M, C, p)
    ok(L().tedspad_mgfn_ln_apply(X.data_ptr(), ldx, St.data_ptr(), gd.data_ptr(), bd.data_ptr(), M, C, Y.data_ptr(), ldy, S()))
    Dy, lddy = inp(dy, p)
    Ad, lda = inp(add, p) if add is not None else (None, 0)
    DX, lddx = out(M, C, p)
    ok(L().tedspad_mgfn_ln_bwd(Dy.data_ptr(), lddy, X.data_ptr(), ldx, St.data_ptr(), gd.data_ptr(), torch_ln, EPS, Ad.data_ptr() if add is not None else None, lda,
                               DX.data_ptr(), lddx, M, C, S()))
    return {"y": take(Y, M, C, "ln_apply"), "dx": take(DX, M, C, "ln_bwd")}


def run_col_reduce(a, mode, scale, x, st, strided):
    M, C = a.shape
    A, lda = inp(a, 1 * strided)
    X, ldx = inp(x, 1 * strided) if x is not None else (None, 0)
    Sd = inp(st.reshape(-1, 1))[0] if st is not None else None
    ws = torch.full((int(L().tedspad_mgfn_train_ws_floats(M, C)),), NAN, device="cuda")
    o0, o1 = out(1, C)[0], out(1, C)[0]
    ok(L().tedspad_mgfn_col_reduce(A.data_ptr(), lda, X.data_ptr() if x is not None else None, ldx, Sd.data_ptr() if st is not None else None, mode, M, C, scale,
                                   ws.data_ptr(), o0.data_ptr(), o1.data_ptr(), S()))
    return {"out0": take(o0, 1, C, "col_reduce out0")[0], "out1": take(o1, 1, C, "col_reduce out1")[0]}


def run_bn(x, g, b, rm, rv, dy, add, strided):
    M, C = x.shape
    p = 4 * strided
    X, ldx = inp(x, p)
    gd, bd = g.float().cuda(), b.float().cuda()
    ws = torch.full((int(L().tedspad_mgfn_train_ws_floats(M, C)),), NAN, device="cuda")
    stat, Y = out(1, 2 * C)[0], out(M, C, p)
    RM, RV = (out(1, C)[0], out(1, C)[0]) if rm is not None else (None, None)
    if rm is not None:
        RM[0], RV[0] = rm.cuda(), rv.cuda()
    ok(L().tedspad_mgfn_bn_train_fwd(X.data_ptr(), ldx, M, C, gd.data_ptr(), bd.data_ptr(), EPS, MOM, ws.data_ptr(), stat.data_ptr(),
                                     RM.data_ptr() if rm is not None else None, RV.data_ptr() if rm is not None else None, Y[0].data_ptr(), Y[1], S()))
    Dy, lddy = inp(dy, p)
    Ad, lda = inp(add, p) if add is not None else (None, 0)
    DX, lddx = out(M, C, p)
    dg, db = out(1, C)[0], out(1, C)[0]
    ok(L().tedspad_mgfn_bn_train_bwd(Dy.data_ptr(), lddy, X.data_ptr(), ldx, stat.data_ptr(), gd.data_ptr(), M, C, ws.data_ptr(), dg.data_ptr(), db.data_ptr(),
                                     Ad.data_ptr() if add is not None else None, lda, DX.data_ptr(), lddx, S()))
    r = {"y": take(Y[0], M, C, "bn y"), "stat": take(stat, 1, 2 * C, "bn stat")[0], "dx": take(DX, M, C, "bn dx"), "dgamma": take(dg, 1, C, "bn dgamma")[0],
         "dbeta": take(db, 1, C, "bn dbeta")[0]}
    if rm is not None:
        r.update(rm=take(RM, 1, C, "bn running_mean")[0], rv=take(RV, 1, C, "bn running_var")[0])
    return r


def run_crop_mean(a, b, seg, ncrops, tmax):
    nseg = seg[-1]
    Ad, Bd = inp(a.reshape(-1, 1))[0], (inp(b.reshape(-1, 1))[0] if b is not None else None)
    Ao, Bo, Sg = out(nseg, 1)[0], out(nseg, 1)[0], i32(seg)
    ok(L().tedspad_mgfn_crop_mean(Ad.data_ptr(), Ao.data_ptr(), Bd.data_ptr() if b is not None else None, Bo.data_ptr() if b is not None else None, Sg.data_ptr(),
                                  len(seg) - 1, tmax, ncrops, S()))
    r = {"a": take(Ao, nseg, 1, "crop_mean a")[:, 0]}
    if b is not None:
        r["b"] = take(Bo, nseg, 1, "crop_mean b")[:, 0]
    else:
        assert bool((Bo == SENT).all())
    return r


def run_gelu(x, dy):
    n = x.numel()
    X, Dy = inp(x.reshape(1, n))[0], inp(dy.reshape(1, n))[0]
    Y, DX = out(1, n)[0], out(1, n)[0]
    ok(L().tedspad_mgfn_gelu(X.data_ptr(), Y.data_ptr(), n, S()))
    ok(L().tedspad_mgfn_gelu_bwd(X.data_ptr(), Dy.data_ptr(), DX.data_ptr(), n, S()))
    return {"y": take(Y, 1, n, "gelu")[0], "dx": take(DX, 1, n, "gelu_bwd")[0]}


def r16(m):
    return (m + 15) // 16 * 16


def run_transpose(x, bounds, taps, ldo, strided):
    M, C = x.shape
    X, ldx = inp(x, 1 * strided)
    Bn = i32(bounds) if bounds is not None else None
    O, _ = out(taps * C, ldo)
    ok(L().tedspad_mgfn_transpose(X.data_ptr(), ldx, Bn.data_ptr() if Bn is not None else None, taps, M, C, O.data_ptr(), ldo, S()))
    return O, take(O, taps * C, ldo, "transpose")


def run_wgrad(AT, DYT, ldk, rows, N):
    """AT, DYT: device images (guarded buffers of run_transpose)"""
    nws = int(L().tedspad_mgfn_wgrad_ws_floats(ldk, rows, N))
    ws = torch.full((nws,), NAN, device="cuda") if nws else None
    DW, _ = out(rows, N)
    ok(L().tedspad_mgfn_wgrad(AT.data_ptr(), DYT.data_ptr(), ldk, rows, N, ws.data_ptr() if nws else None, DW.data_ptr(), S()))
    return take(DW, rows, N, "wgrad"), nws


# ---- tile tails, guards and strides -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("taps,cin", R.MGFN_GEMM_TAPS_CIN)
@pytest.mark.parametrize("M", R.MGFN_GEMM_M)
def test_gemm_tails(M, taps, cin):
    """Sequence ends on rows 32, 64 and 256 and one row either side, runs of length-1 sequences (R.gemm_lengths); every element against its bound."""
    off, bounds = R.mgfn_ragged(R.gemm_lengths(M))
    for N in R.MGFN_GEMM_N:
        tag = "%d_%d_%d_%d" % (M, taps, cin, N)
        x = syn(51, "x" + tag, (M, cin), -2, 2)
        w = syn(51, "w" + tag, (N, taps * cin)) / (taps * cin) ** 0.5
        bias, res = syn(51, "b" + tag, (N,), -0.5, 0.5), syn(51, "r" + tag, (M, N))
        combos = [(0, 0, 0, 0), (1, 1, 1, 0), (1, 0, 1, 0), (0, 1, 0, 0)] + ([(1, 1, 1, 1), (0, 0, 0, 1)] if taps == 1 else [])
        for wb, gelu, wr, ln in combos:
            stats = run_ln_stats(x, 0, False)["stats"] if ln else None
            args = (x, bounds if taps > 1 else None, taps, w, bias if wb else None, gelu, res if wr else None, stats)
            got = both(lambda s: run_gemm(*args, N, s), "gemm " + tag)["y"]
            within(got, R.mgfn_gemm_ref(*args), "gemm %s bias %d gelu %d res %d ln %d" % (tag, wb, gelu, wr, ln))


@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("tmax", [65, 100])
def test_attention_tails(heads, tmax):
    off, _ = R.mgfn_ragged(R.MGFN_ATT_LENGTHS)
    M, inner = off[-1], 64 * heads
    qkv, do = syn(52, "qkv%d" % heads, (M, 3 * inner), -2, 2), syn(52, "do%d" % heads, (M, inner))
    r = both(lambda s: run_attention(qkv, off, heads, tmax, s, do), "attention heads %d" % heads)
    within(r["o"], R.mgfn_attention_ref(qkv, off, heads), "attention")
    dq, lse = R.mgfn_attention_bwd_ref(qkv, r["o"], do, off, heads)
    within(r["dqkv"], dq, "attention_bwd dq | dk | dv")
    within(r["lse"], (lse[0].reshape(M, -1), lse[1].reshape(M, -1)), "attention_bwd lse")


@pytest.mark.parametrize("heads", [1, 3, 16])
def test_relpos_tails(heads):
    """Lengths 1 .. 6: every combination of masked taps; M = 142 crosses the 128-token chunk; C = 64 heads: a 4-channel vector straddles the head cycle of 3."""
    C = 64 * heads
    off, bounds = R.mgfn_ragged([1, 2, 3, 4, 5, 6, 110, 6, 5])
    M = off[-1]
    v, do = syn(53, "v%d" % heads, (M, C)), syn(53, "do%d" % heads, (M, C))
    w, b = syn(53, "w%d" % heads, (heads, 5)), syn(53, "b%d" % heads, (heads,), -0.5, 0.5)
    r = both(lambda s: run_relpos(v, bounds, heads, w, b, s, do), "relpos heads %d" % heads)
    within(r["out"], R.mgfn_relpos_ref(v, bounds, heads, w, b), "relpos")
    dv, dw, db = R.mgfn_relpos_bwd_ref(do, v, bounds, heads, w)
    within(r["dv"], dv, "relpos_bwd dv")
    within(r["dw"], dw, "relpos_bwd dw")
    within(r["db"][:, 0], db, "relpos_bwd db")


def _check_stats(got, x, torch_ln, what):
    mu, rs, dmu, drs = R.mgfn_ln_stats_ref(x, EPS, torch_ln)
    within(got[:, 0], (mu, dmu + R.FLOOR32), what + " mean")
    within(got[:, 1], (rs, drs + R.FLOOR32), what + " rs")


@pytest.mark.parametrize("C", R.MGFN_ROW_C)
@pytest.mark.parametrize("M", R.MGFN_ROW_M)
def test_row_kernels_tails(M, C):
    """ln_stats, ln_apply, ln_bwd (both flavours, with and without `add`), head (with and without h), head_bwd: four waves per block, 256 channels per pass."""
    tag = "%d_%d" % (M, C)
    x = syn(54, "x" + tag, (M, C), -3, 5)
    g, b = syn(54, "g" + tag, (C,), 0.5, 1.5), syn(54, "b" + tag, (C,), -0.5, 0.5)
    dy, add = syn(54, "dy" + tag, (M, C)), syn(54, "add" + tag, (M, C))
    for torch_ln in (0, 1):
        st = both(lambda s: run_ln_stats(x, torch_ln, s), "ln_stats")["stats"]
        _check_stats(st, x, torch_ln, "ln_stats torch_ln %d" % torch_ln)
        for a in (add, None):
            r = both(lambda s: run_ln_apply_bwd(x, st, g, b, dy, a, torch_ln, s), "ln_apply / ln_bwd")
            within(r["y"], R.mgfn_ln_apply_ref(x, st, g, b), "ln_apply torch_ln %d" % torch_ln)
            within(r["dx"], R.mgfn_ln_bwd_ref(dy, x, st, g, torch_ln, EPS, a), "ln_bwd torch_ln %d add %d" % (torch_ln, a is not None))
    fw, dsc, dh = syn(54, "fw" + tag, (C,), -0.5, 0.5), syn(54, "ds" + tag, (M,)), syn(54, "dh" + tag, (M, C))
    r = both(lambda s: run_head(x, g, b, fw, 0.05, s), "head")
    ref = R.mgfn_head_ref(x, g, b, fw, 0.05, EPS)
    for key in ("h", "logit", "score", "mag"):
        within(r[key], ref[key], "head " + key)
    nh = run_head(x, g, b, fw, 0.05, True, with_h=False)
    for key in ("logit", "score", "mag"):
        same_bits(nh[key], r[key], "head with h == NULL: " + key)
    hb = run_head_bwd(r["score"][:, 0], dsc, fw, dh)
    rdh, rdz = R.mgfn_head_bwd_ref(r["score"][:, 0], dsc, fw, dh)
    within(hb["dh"], rdh, "head_bwd dh")
    within(hb["dz"], rdz, "head_bwd dz")


@pytest.mark.parametrize("C", R.MGFN_COL_C)
@pytest.mark.parametrize("M", R.MGFN_COL_M)
def test_col_reduce_tails(M, C):
    tag = "%d_%d" % (M, C)
    a, x = syn(55, "a" + tag, (M, C)), syn(55, "x" + tag, (M, C), -3, 5)
    st_row = torch.stack([x.mean(1), 1 / (x.var(1, unbiased=False) + 1e-5).sqrt()], 1)
    st_col = torch.cat([x.mean(0), 1 / (x.var(0, unbiased=False) + 1e-5).sqrt()])
    rowf = syn(55, "rf" + tag, (M,))
    for mode, xx, st in ((0, None, None), (1, x, st_row), (2, x, st_col), (3, None, st_col), (3, None, None), (4, None, rowf)):
        r = both(lambda s: run_col_reduce(a, mode, 0.5, xx, st, s), "col_reduce mode %d" % mode)
        r0, r1 = R.mgfn_col_reduce_ref(a, mode, 0.5, xx, st)
        within(r["out0"], r0, "col_reduce mode %d%s out0" % (mode, "" if st is not None or mode != 3 else " (st == NULL)"))
        within(r["out1"], r1, "col_reduce mode %d out1" % mode)
    same_bits(run_col_reduce(a, 3, 0.5, None, None, False)["out0"], run_col_reduce(a, 0, 0.5, None, None, False)["out0"], "mode 3 with st == NULL is mode 0")


@pytest.mark.parametrize("running", [1, 0])
@pytest.mark.parametrize("C", [4, 260])
@pytest.mark.parametrize("M", [1, 2, 129])
def test_batchnorm_tails(M, C, running):
    tag = "%d_%d" % (M, C)
    x = syn(56, "x" + tag, (M, C), -3, 5)
    x[:, 1] = 2.5                                                       # one constant channel
    g, b = syn(56, "g" + tag, (C,), 0.5, 1.5), syn(56, "b" + tag, (C,), -0.2, 0.2)
    rm, rv = (syn(56, "rm" + tag, (C,), -0.1, 0.1), syn(56, "rv" + tag, (C,), 0.5, 1.5)) if running else (None, None)
    dy, add = syn(56, "dy" + tag, (M, C)), syn(56, "add" + tag, (M, C))
    r = both(lambda s: run_bn(x, g, b, rm, rv, dy, add, s), "bn")
    f = R.mgfn_bn_fwd_ref(x, g, b, EPS, MOM, rm, rv)
    within(r["y"], f["y"], "bn y")
    within(r["stat"][:C], f["mean"], "bn mean")
    within(r["stat"][C:], f["invstd"], "bn invstd")
    if running:
        within(r["rm"], f["running_mean"], "bn running_mean")
        within(r["rv"], f["running_var"], "bn running_var (M = 1: the biased variance)")
    bw = R.mgfn_bn_bwd_ref(dy, x, r["stat"], g, add)
    for key in ("dx", "dgamma", "dbeta"):
        within(r[key], bw[key], "bn " + key)
    r2 = run_bn(x, g, b, rm, rv, dy, None, False)
    within(r2["dx"], R.mgfn_bn_bwd_ref(dy, x, r2["stat"], g, None)["dx"], "bn dx without add")


@pytest.mark.parametrize("with_b", [1, 0])
@pytest.mark.parametrize("ncrops", [1, 10])
def test_crop_mean_tails(ncrops, with_b):
    seg = [0, 1, 257, 514]                                             # T = 1, 256, 257
    a, b = syn(57, "a%d" % ncrops, (ncrops * seg[-1],), 0, 1), (syn(57, "b%d" % ncrops, (ncrops * seg[-1],), 0, 30) if with_b else None)
    for tmax in (257, 300):
        r = run_crop_mean(a, b, seg, ncrops, tmax)
        within(r["a"], R.mgfn_crop_mean_ref(a, seg, ncrops), "crop_mean a")
        if with_b:
            within(r["b"], R.mgfn_crop_mean_ref(b, seg, ncrops), "crop_mean b")


GELU_HARD = [0.0, -0.0, 2.0 ** -140, -2.0 ** -140, 1e-3, -1e-3, 0.7, -0.7, 3.0, -3.0, 6.0, -6.0, 10.0, -10.0, 40.0, -40.0]


@pytest.mark.parametrize("n", [4, 1020, 1028])
def test_gelu_tails(n):
    x, dy = syn(58, "x%d" % n, (n,), -6, 6), syn(58, "dy%d" % n, (n,))
    r = run_gelu(x, dy)
    within(r["y"], R.mgfn_gelu_ref(x), "gelu")
    within(r["dx"], R.mgfn_gelu_bwd_ref(x, dy), "gelu_bwd")


@pytest.mark.parametrize("C", [16, 80])
@pytest.mark.parametrize("M", R.MGFN_WGRAD_M)
def test_transpose_wgrad_tails(M, C):
    """rows = 3 C = 48 / 240 (rows % 64 != 0), N = 64; M <= 128: one K slice, ws == NULL; 129, 300: several; M % 16 != 0: the zero padding up to ldk feeds the sum."""
    taps, N = 3, 64
    off, bounds = R.mgfn_ragged(R.gemm_lengths(M))
    ldk, rows = r16(M), taps * C
    tag = "%d_%d" % (M, C)
    x, dy = syn(59, "x" + tag, (M, C), -2, 2), syn(59, "dy" + tag, (M, N))
    AT, at = run_transpose(x, bounds, taps, ldk, False)
    DYT, dyt = run_transpose(dy, None, 1, ldk, False)
    for got, src, bn, tp, what in ((at, x, bounds, taps, "transpose of the 3-tap window"), (dyt, dy, None, 1, "transpose of dy")):
        R.same(got.to(D), R.mgfn_transpose_ref(src, bn, tp, ldk), what)
        wide = run_transpose(src, bn, tp, ldk + 16, True)[1]                       # strided input rows, a wider image: the same payload, zeros up to ldo
        R.same(wide.to(D), R.mgfn_transpose_ref(src, bn, tp, ldk + 16), what + " (ldx = C + 1, ldo + 16)")
    dw, nws = run_wgrad(AT, DYT, ldk, rows, N)
    assert (nws == 0) == (M <= 128) and R.mgfn_wgrad_slices(ldk, rows, N)[1] == (1 if M <= 128 else 2 if M == 129 else 3)
    within(dw, R.mgfn_wgrad_ref(at, dyt), "wgrad")
    same_bits(dw, run_wgrad(AT, DYT, ldk, rows, N)[0], "wgrad twice")


# ---- sequence isolation -----------------------------------------------------------------------------------------------------------------------------------------
ISO_LENGTHS = [5, 33, 1, 64, 7]


def _isolated(run, tensors, off, what):
    """run(tensors) -> (M, .) per-token output. For the first, a middle and the last sequence: with every other sequence's rows of every tensor set to NaN, the
    target's rows are finite and bit-identical to those of the plain run."""
    plain = run(tensors)
    for tgt in (0, len(off) // 2 - 1, len(off) - 2):
        b0, b1 = off[tgt], off[tgt + 1]
        poisoned = []
        for t in tensors:
            p = torch.full_like(t, NAN)
            p[b0:b1] = t[b0:b1]
            poisoned.append(p)
        got = run(poisoned)
        assert bool(torch.isfinite(got[b0:b1]).all()), "%s: sequence %d is not finite beside NaN neighbours" % (what, tgt)
        same_bits(got[b0:b1], plain[b0:b1], "%s: sequence %d alone against in the batch" % (what, tgt))


def test_isolation_gemm_taps3():
    off, bounds = R.mgfn_ragged(ISO_LENGTHS)
    M, cin, N = off[-1], 48, 64
    x, w, bias = syn(60, "x", (M, cin), -2, 2), syn(60, "w", (N, 3 * cin)) / 12, syn(60, "b", (N,))
    _isolated(lambda t: run_gemm(t[0], bounds, 3, w, bias, 1, None, None, N, True)["y"], [x], off, "gemm taps 3")


@pytest.mark.parametrize("heads", [1, 3])
def test_isolation_attention(heads):
    off, _ = R.mgfn_ragged(ISO_LENGTHS)
    M, inner = off[-1], 64 * heads
    qkv, do = syn(61, "qkv%d" % heads, (M, 3 * inner), -2, 2), syn(61, "do%d" % heads, (M, inner))
    _isolated(lambda t: run_attention(t[0], off, heads, 64, True)["o"], [qkv], off, "attention")
    _isolated(lambda t: run_attention(t[0], off, heads, 64, True, t[1])["dqkv"], [qkv, do], off, "attention_bwd dq | dk | dv")


def test_isolation_relpos():
    off, bounds = R.mgfn_ragged(ISO_LENGTHS)
    M, heads, C = off[-1], 3, 192
    v, do, w, b = syn(62, "v", (M, C)), syn(62, "do", (M, C)), syn(62, "w", (heads, 5)), syn(62, "b", (heads,))
    _isolated(lambda t: run_relpos(t[0], bounds, heads, w, b, True)["out"], [v], off, "relpos")
    _isolated(lambda t: run_relpos(t[0], bounds, heads, w, b, True, t[1])["dv"], [v, do], off, "relpos_bwd dv")


def test_isolation_crop_mean():
    seg, nc = [0, 3, 260, 261, 300], 10
    a, b = syn(63, "a", (nc * seg[-1],), 0, 1), syn(63, "b", (nc * seg[-1],), 0, 30)
    tok = [nc * s for s in seg]                                       # a video's crops are contiguous: tokens nc * seg[v] .. nc * seg[v + 1]
    plain = run_crop_mean(a, b, seg, nc, 257)
    for v in (0, 1, 3):
        pa, pb = torch.full_like(a, NAN), torch.full_like(b, NAN)
        pa[tok[v]:tok[v + 1]], pb[tok[v]:tok[v + 1]] = a[tok[v]:tok[v + 1]], b[tok[v]:tok[v + 1]]
        got = run_crop_mean(pa, pb, seg, nc, 257)
        for k in ("a", "b"):
            assert bool(torch.isfinite(got[k][seg[v]:seg[v + 1]]).all())
            same_bits(got[k][seg[v]:seg[v + 1]], plain[k][seg[v]:seg[v + 1]], "crop_mean %s: video %d alone against in the batch" % (k, v))


# ---- hard values ------------------------------------------------------------------------------------------------------------------------------------------------
def test_attention_hard_values():
    """One batch: logits of about +-200 with a pair of equal and a pair of opposite rows; all keys equal (the softmax is uniform: the output is the mean of v); one
    dominant key. Forward and backward finite and within bound."""
    heads, lengths = 1, [40, 33, 33]
    off, _ = R.mgfn_ragged(lengths)
    M = off[-1]
    qkv, do = syn(64, "qkv", (M, 192)), syn(64, "do", (M, 64))
    qkv[:40, :128] *= 9.0
    qkv[0, 64:128] = qkv[0, :64]                                       # k_0 = q_0: a logit of |q_0|^2 / 8, about +200
    qkv[1] = qkv[0]                                                    # a pair of equal rows
    qkv[2, 64:128] = qkv[2, :64]
    qkv[3, :128] = -qkv[2, :128]                                       # a pair of opposite rows: logits of about +200 and -200 side by side
    qkv[40:73, 64:128] = qkv[40, 64:128]                               # all keys equal
    qkv[73:, :64] = qkv[73:, :64].abs()
    qkv[73:, 64:128] *= 0.01
    qkv[73 + 5, 64:128] = 4.0                                          # one dominant key: its logit is 4 sum |q| / 8, about 16, the others' about 0
    r = both(lambda s: run_attention(qkv, off, heads, 40, s, do), "attention hard")
    assert bool(torch.isfinite(r["o"]).all()) and bool(torch.isfinite(r["dqkv"]).all()) and bool(torch.isfinite(r["lse"]).all())
    fwd = R.mgfn_attention_ref(qkv, off, heads)
    S = (qkv[:40, :64].double() * 0.125) @ qkv[:40, 64:128].double().t()
    assert float(S.max()) > 150 and float(S.min()) < -150, (float(S.max()), float(S.min()))
    within(r["o"], fwd, "attention, hard values")
    same_bits(r["o"][1], r["o"][0], "two equal rows")
    uni = qkv[40:73, 128:].double().mean(0)
    assert float((r["o"][40:73].double() - uni).abs().max()) <= float(fwd[1][40:73].max()), "all keys equal: the output is not the mean of v"
    dq, lse = R.mgfn_attention_bwd_ref(qkv, r["o"], do, off, heads)
    within(r["dqkv"], dq, "attention_bwd, hard values")
    within(r["lse"], (lse[0].reshape(M, -1), lse[1].reshape(M, -1)), "attention_bwd lse, hard values")


@pytest.mark.parametrize("C", [4, 260])
@pytest.mark.parametrize("torch_ln", [0, 1])
def test_layernorm_hard_rows(torch_ln, C):
    """Row 1: 1000 + noise of 1e-2 (the two-pass variance holds its bound; E[x^2] - mean^2 would not: test_kernel_refs.py). Row 2: constant 3: rs is exactly 1 / eps
    or 1 / sqrt(eps), y == b exactly; ln_bwd: the torch flavour finite and within bound. The MGFN flavour's own formula divides by std = 0 there, float64 included
    (0 * inf, or 0 times the reciprocal of the rounding residue of 1 / rs - eps): the float64 restatement gives no value and no bound for that row of dx, so nothing
    is asserted on it -- the other rows of the same launch are checked as everywhere."""
    M = 5
    x = syn(65, "x%d" % C, (M, C), -3, 5)
    x[1] = 1000.0 + 0.01 * x[1]
    x[2] = 3.0
    g, b, dy = syn(65, "g%d" % C, (C,), 0.5, 1.5), syn(65, "b%d" % C, (C,), -0.5, 0.5), syn(65, "dy%d" % C, (M, C))
    st = both(lambda s: run_ln_stats(x, torch_ln, s), "ln_stats")["stats"]
    _check_stats(st[[0, 1, 3, 4]], x[[0, 1, 3, 4]], torch_ln, "ln_stats, hard rows")
    e32 = np.float32(EPS)
    want = np.float32(1) / np.sqrt(e32) if torch_ln else np.float32(1) / e32
    assert float(st[2, 0]) == 3.0 and float(st[2, 1]) == float(want), (st[2].tolist(), float(want))
    r = both(lambda s: run_ln_apply_bwd(x, st, g, b, dy, None, torch_ln, s), "ln_apply / ln_bwd")
    within(r["y"], R.mgfn_ln_apply_ref(x, st, g, b), "ln_apply, hard rows")
    same_bits(r["y"][2], b, "constant row: y == b")
    ref = R.mgfn_ln_bwd_ref(dy, x, st, g, torch_ln, EPS)
    rows = [0, 1, 2, 3, 4] if torch_ln else [0, 1, 3, 4]
    assert bool(torch.isfinite(ref[0][rows]).all())
    within(r["dx"][rows], (ref[0][rows], ref[1][rows]), "ln_bwd, hard rows")
    if torch_ln:                                                        # the head: the same LayerNorm inside
        fw = syn(65, "fw%d" % C, (C,), -0.5, 0.5)
        h = run_head(x, g, b, fw, 0.05, True)
        ref = R.mgfn_head_ref(x, g, b, fw, 0.05, EPS)
        for key in ("h", "logit", "score", "mag"):
            within(h[key][[0, 1, 3, 4]], tuple(t[[0, 1, 3, 4]] for t in ref[key]), "head %s, hard rows" % key)
        same_bits(h["h"][2], b, "head, constant row: h == ln_b")


def test_gelu_hard_values():
    x = torch.tensor(GELU_HARD, dtype=torch.float32)
    dy = torch.tensor([1.0, -1.0, 0.5, -0.5] * 4)
    r = run_gelu(x, dy)
    y, dx = R.mgfn_gelu_ref(x), R.mgfn_gelu_bwd_ref(x, dy)
    assert bool(torch.isfinite(r["y"]).all()) and bool(torch.isfinite(r["dx"]).all())
    within(r["y"], y, "gelu, hard values")
    within(r["dx"], dx, "gelu_bwd, hard values")
    t = torch.nn.functional.gelu(x)
    zero = (t == 0) & (r["y"] == 0)
    assert int(zero.sum()) >= 3 and torch.equal(torch.signbit(r["y"][zero]), torch.signbit(t[zero])), "sign of zero"
    exact = 0
    for i in range(len(GELU_HARD)):                                     # the tails: exact where float64 itself rounds to 0 / x (gelu), 0 / dy (backward)
        if float(y[0][i]) in (0.0, float(x[i])):
            assert float(r["y"][i]) == float(y[0][i]), (GELU_HARD[i], float(r["y"][i]))
            exact += 1
        if float(dx[0][i]) in (0.0, float(dy[i])):
            assert float(r["dx"][i]) == float(dx[0][i]), (GELU_HARD[i], float(r["dx"][i]))
            exact += 1
    assert exact >= 8                                                   # +-0, 10, +-40 forward; 10, +-40 backward


@pytest.mark.parametrize("fb", [100.0, -100.0])
def test_head_saturated(fb):
    """fc_b = +-100: the scores are exactly 1 / 0, dz is exactly 0 and dh is unchanged bit for bit, for dscore of mixed sign."""
    M, C = 5, 260
    x, lw, lb = syn(66, "x", (M, C), -3, 5), syn(66, "lw", (C,), 0.5, 1.5), syn(66, "lb", (C,), -0.1, 0.1)
    fw, dsc, dh = syn(66, "fw", (C,), -0.05, 0.05), syn(66, "ds", (M,)), syn(66, "dh", (M, C))
    assert bool((dsc > 0).any()) and bool((dsc < 0).any())
    r = run_head(x, lw, lb, fw, fb, True)
    ref = R.mgfn_head_ref(x, lw, lb, fw, fb, EPS)
    for key in ("h", "logit", "score", "mag"):
        within(r[key], ref[key], "head %s, saturated" % key)
    assert bool((r["score"] == (1.0 if fb > 0 else 0.0)).all())
    hb = run_head_bwd(r["score"][:, 0], dsc, fw, dh)
    assert bool((hb["dz"] == 0).all())
    same_bits(hb["dh"], dh, "head_bwd with a saturated sigmoid: dh")


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    """Arguments each entry point's own message names: a negative code, a non-empty tedspad_last_error(), and the sentinel-filled outputs untouched."""
    lib, st = L(), S()
    M, C, N = 8, 64, 64
    f = lambda *shape: torch.zeros(shape, device="cuda")                 # noqa: E731
    x, w, bias, res, stats = f(M + 1, C + 4), f(N, 3 * C), f(N), f(M, N), f(M, 2)
    bounds = i32(R.mgfn_ragged([M])[1])
    off = i32([0, M])
    outs = [torch.full((M + 2, 3 * C + 8), SENT, device="cuda") for _ in range(4)]
    o0, o1, o2, o3 = (o.data_ptr() for o in outs)
    X, Wp, Bp, Rp, Sp, Bn, Of = (t.data_ptr() for t in (x, w, bias, res, stats, bounds, off))
    g, ws = f(4 * C), f(4096)
    G, WS = g.data_ptr(), ws.data_ptr()
    big = 65535 * 32 + 1
    cases = {
        "ln_stats: misaligned x": lambda: lib.tedspad_mgfn_ln_stats(X + 4, C, M, C, EPS, 0, o0, st),
        "ln_stats: ldx < C": lambda: lib.tedspad_mgfn_ln_stats(X, C - 4, M, C, EPS, 0, o0, st),
        "ln_stats: C % 4": lambda: lib.tedspad_mgfn_ln_stats(X, C, M, C - 1, EPS, 0, o0, st),
        "gemm: N % 64": lambda: lib.tedspad_mgfn_gemm(X, C, None, 1, C, None, Wp, Bp, 0, None, 0, o0, N, M, N - 16, st),
        "gemm: cin % 16": lambda: lib.tedspad_mgfn_gemm(X, C, None, 1, C - 8, None, Wp, Bp, 0, None, 0, o0, N, M, N, st),
        "gemm: even taps": lambda: lib.tedspad_mgfn_gemm(X, C, Bn, 2, C, None, Wp, Bp, 0, None, 0, o0, N, M, N, st),
        "gemm: taps > 1 without bounds": lambda: lib.tedspad_mgfn_gemm(X, C, None, 3, C, None, Wp, Bp, 0, None, 0, o0, N, M, N, st),
        "gemm: stats with taps 3": lambda: lib.tedspad_mgfn_gemm(X, C, Bn, 3, C, Sp, Wp, Bp, 0, None, 0, o0, N, M, N, st),
        "gemm: ldx < cin": lambda: lib.tedspad_mgfn_gemm(X, C - 4, None, 1, C, None, Wp, Bp, 0, None, 0, o0, N, M, N, st),
        "gemm: ldy < N": lambda: lib.tedspad_mgfn_gemm(X, C, None, 1, C, None, Wp, Bp, 0, None, 0, o0, N - 1, M, N, st),
        "gemm: ldres < N": lambda: lib.tedspad_mgfn_gemm(X, C, None, 1, C, None, Wp, Bp, 0, Rp, N - 1, o0, N, M, N, st),
        "gemm: misaligned x": lambda: lib.tedspad_mgfn_gemm(X + 4, C, None, 1, C, None, Wp, Bp, 0, None, 0, o0, N, M, N, st),
        "gemm: y == x": lambda: lib.tedspad_mgfn_gemm(o0, C, None, 1, C, None, Wp, Bp, 0, None, 0, o0, N, M, N, st),
        "attention: ldqkv < 3 heads 64": lambda: lib.tedspad_mgfn_attention(X, 3 * 64 - 4, Of, 1, M, 1, o0, 64, st),
        "attention: ldo < heads 64": lambda: lib.tedspad_mgfn_attention(X, 192, Of, 1, M, 1, o0, 63, st),
        "attention: misaligned qkv": lambda: lib.tedspad_mgfn_attention(X + 4, 192, Of, 1, M, 1, o0, 64, st),
        "attention: tmax / 32 > 65535": lambda: lib.tedspad_mgfn_attention(X, 192, Of, 1, big, 1, o0, 64, st),
        "attention: heads > 65535": lambda: lib.tedspad_mgfn_attention(X, 3 * 64 * 65536, Of, 1, M, 65536, o0, 64 * 65536, st),
        "attention_bwd: tmax / 32 > 65535": lambda: lib.tedspad_mgfn_attention_bwd(X, 192, G, 64, G, 64, Of, 1, big, 1, o1, o0, 192, st),
        "attention_bwd: lddqkv < 3 heads 64": lambda: lib.tedspad_mgfn_attention_bwd(X, 192, G, 64, G, 64, Of, 1, M, 1, o1, o0, 191, st),
        "attention_bwd: lddo % 4": lambda: lib.tedspad_mgfn_attention_bwd(X, 192, G, 64, G, 65, Of, 1, M, 1, o1, o0, 192, st),
        "relpos: in place": lambda: lib.tedspad_mgfn_relpos(o0, C, Bn, M, C, 1, Wp, Bp, o0, C, st),
        "relpos: ldv < C": lambda: lib.tedspad_mgfn_relpos(X, C - 4, Bn, M, C, 1, Wp, Bp, o0, C, st),
        "relpos: ldo < C": lambda: lib.tedspad_mgfn_relpos(X, C, Bn, M, C, 1, Wp, Bp, o0, C - 4, st),
        "relpos: misaligned out": lambda: lib.tedspad_mgfn_relpos(X, C, Bn, M, C, 1, Wp, Bp, o0 + 4, C, st),
        "relpos_bwd: in place": lambda: lib.tedspad_mgfn_relpos_bwd(o0, C, X, C, Bn, M, C, 1, Wp, WS, o0, C, o1, o2, st),
        "relpos_bwd: C % heads": lambda: lib.tedspad_mgfn_relpos_bwd(G, C, X, C, Bn, M, C, 3, Wp, WS, o0, C, o1, o2, st),
        "head: ldx < C": lambda: lib.tedspad_mgfn_head(X, C - 4, M, C, G, G, G, 0.0, EPS, o0, o1, o2, o3, st),
        "head: misaligned fc_w": lambda: lib.tedspad_mgfn_head(X, C, M, C, G, G, G + 4, 0.0, EPS, o0, o1, o2, o3, st),
        "head_bwd: C % 4": lambda: lib.tedspad_mgfn_head_bwd(G, G, G, M, C - 2, o0, o1, st),
        "crop_mean: b without b_out": lambda: lib.tedspad_mgfn_crop_mean(G, o0, G, None, Of, 1, M, 1, st),
        "crop_mean: ncrops 0": lambda: lib.tedspad_mgfn_crop_mean(G, o0, None, None, Of, 1, M, 0, st),
        "col_reduce: mode 1 without x": lambda: lib.tedspad_mgfn_col_reduce(G, C, None, 0, Sp, 1, M, C, 1.0, WS, o0, o1, st),
        "col_reduce: mode 2 without out1": lambda: lib.tedspad_mgfn_col_reduce(G, C, X, C, Sp, 2, M, C, 1.0, WS, o0, None, st),
        "col_reduce: mode 4 without st": lambda: lib.tedspad_mgfn_col_reduce(G, C, None, 0, None, 4, M, C, 1.0, WS, o0, o1, st),
        "col_reduce: lda < C": lambda: lib.tedspad_mgfn_col_reduce(G, C - 1, None, 0, None, 0, M, C, 1.0, WS, o0, o1, st),
        "col_reduce: mode 5": lambda: lib.tedspad_mgfn_col_reduce(G, C, None, 0, None, 5, M, C, 1.0, WS, o0, o1, st),
        "ln_apply: ldy < C": lambda: lib.tedspad_mgfn_ln_apply(X, C, Sp, G, G, M, C, o0, C - 4, st),
        "ln_apply: misaligned y": lambda: lib.tedspad_mgfn_ln_apply(X, C, Sp, G, G, M, C, o0 + 4, C, st),
        "ln_bwd: lddx % 4": lambda: lib.tedspad_mgfn_ln_bwd(G, C, X, C, Sp, G, 1, EPS, None, 0, o0, C + 1, M, C, st),
        "ln_bwd: ldadd < C": lambda: lib.tedspad_mgfn_ln_bwd(G, C, X, C, Sp, G, 1, EPS, G, C - 4, o0, C, M, C, st),
        "bn_train_fwd: running_mean without running_var": lambda: lib.tedspad_mgfn_bn_train_fwd(X, C, M, C, G, G, EPS, MOM, WS, o1, o2, None, o0, C, st),
        "bn_train_fwd: ldy < C": lambda: lib.tedspad_mgfn_bn_train_fwd(X, C, M, C, G, G, EPS, MOM, WS, o1, None, None, o0, C - 4, st),
        "bn_train_bwd: misaligned dx": lambda: lib.tedspad_mgfn_bn_train_bwd(G, C, X, C, G, G, M, C, WS, o1, o2, None, 0, o0 + 4, C, st),
        "gelu: n % 4": lambda: lib.tedspad_mgfn_gelu(G, o0, 6, st),
        "gelu_bwd: misaligned dx": lambda: lib.tedspad_mgfn_gelu_bwd(G, G, o0 + 4, 8, st),
        "transpose: ldo < M": lambda: lib.tedspad_mgfn_transpose(X, C, None, 1, M, C, o0, M - 1, st),
        "transpose: even taps": lambda: lib.tedspad_mgfn_transpose(X, C, Bn, 2, M, C, o0, 16, st),
        "transpose: taps > 1 without bounds": lambda: lib.tedspad_mgfn_transpose(X, C, None, 3, M, C, o0, 16, st),
        "wgrad: ldk % 16": lambda: lib.tedspad_mgfn_wgrad(G, G, 8, 4, 64, None, o0, st),
        "wgrad: N % 64": lambda: lib.tedspad_mgfn_wgrad(G, G, 16, 4, 32, None, o0, st),
        "wgrad: slices without ws": lambda: lib.tedspad_mgfn_wgrad(G, G, 304, 4, 64, None, o0, st),
    }
    assert R.mgfn_wgrad_slices(304, 4, 64)[1] > 1
    for name, call in cases.items():
        rc = call()
        msg = last_error()
        assert rc < 0 and msg, "%s: code %d, message %r" % (name, rc, msg)
        torch.cuda.synchronize()
        for o in outs:
            assert bool((o == SENT).all()), "%s: an output was written" % name
