"""-m gpu: the small fp32 kernels that close every training and evaluation step, through the C ABI, element by element: tedspad_linear_fwd (csrc/head.hip: five
kernels behind one dispatch), tedspad_bce_head_fwd_bwd (csrc/bce_head.hip) and tedspad_vote_accumulate / tedspad_vote_finalize / tedspad_softmax_ce_eval
(csrc/action_eval.hip), against the references and case tables of tests/kernel_refs.py (their conditions and their sensitivity: tests/test_kernel_refs.py).

Two kinds of comparison. EXACT: inputs on which every partial sum is exact in fp32 in any order (integers below 2^24; dyadic gradients; the vote sums, whose
order the kernel fixes): the kernel must be torch.equal to the reference. BOUNDED: realistic magnitudes against float64 with a per-element bound derived from
the chain lengths and the K_* constants (the references' docstrings); each such test prints its worst error / bound ratio per quantity. Every output lives in
front of a sentinel region that must come back untouched, every input in front of NaN."""
import ctypes as Ct

import numpy as np
import pytest
import torch

import kernel_refs as R

pytestmark = pytest.mark.gpu
D = torch.float64
SENT = 1024.0
GUARD = 512                                     # sentinel elements behind every output
ISENT = {torch.int32: -7, torch.uint8: 0x7E}


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


def inp(t):
    """device copy of the fp32 tensor t, NaN behind it; returns (buffer, pointer)"""
    t = torch.as_tensor(t).to(torch.float32).reshape(-1)
    buf = torch.full((t.numel() + GUARD,), float("nan"), device="cuda")
    buf[:t.numel()] = t.cuda()
    return buf, buf.data_ptr()


def out(n, dtype=torch.float32, fill=None):
    """n elements on the device followed by GUARD more, all holding the sentinel (`fill`: the payload's initial values)"""
    buf = torch.full((n + GUARD,), SENT if dtype == torch.float32 else ISENT[dtype], dtype=dtype, device="cuda")
    if fill is not None:
        buf[:n] = torch.as_tensor(fill).reshape(-1).to(dtype).cuda()
    return buf


def take(buf, n, what, shape=None):
    """the payload on the host, after checking the sentinel region"""
    b = buf.cpu()
    sent = SENT if buf.dtype == torch.float32 else ISENT[buf.dtype]
    assert bool((b[n:] == sent).all()), "%s: written behind its end" % what
    return b[:n].clone().reshape(shape if shape is not None else (n,))


def untouched(buf, what):
    assert bool((buf == (SENT if buf.dtype == torch.float32 else ISENT[buf.dtype])).all()), "%s was written" % what


def ptr(buf):
    return buf.data_ptr() if buf is not None else None


def bounded(got, ref_bound, what, ratios):
    ref, bound = ref_bound
    ratios[what.split()[-1]] = max(ratios.get(what.split()[-1], 0.0), R.worst_ratio(got, ref, bound))
    msg = R.worst(got.reshape(ref.shape), ref, bound)
    assert not msg, "%s: %s" % (what, msg)


# ---- tedspad_linear_fwd ----------------------------------------------------------------------------------------------------------------------------------------
def run_linear(xb, wb, sb, bb, B, K, N, relu, what):
    y = out(B * N)
    ok(L().tedspad_linear_fwd(xb[1], wb[1], sb[1] if sb else None, bb[1] if bb else None, y.data_ptr(), B, K, N, relu, S()))
    return take(y, B * N, what, (B, N))


@pytest.mark.parametrize("form,B,K,N", R.LINEAR_CASES)
def test_linear_every_form_bit_for_bit(form, B, K, N):
    """Integer x and w, power-of-two scales, even shifts: every partial sum is an integer below 2^24 and the epilogue is exact, so each kernel -- the row names
    the one it reaches, R.linear_form -- must equal the integer product under all four (scale, shift) combinations, with and without the ReLU."""
    assert R.linear_form(B, K, N)[0] == form
    x, w, scale, shift = R.linear_exact_inputs(B, K, N)
    xb, wb, sb, bb = inp(x), inp(w), inp(scale), inp(shift)
    fails = []
    for sc, sh, relu in R.LINEAR_EPILOGUES:
        what = "linear %s (%d, %d, %d) scale %d shift %d relu %d" % (form, B, K, N, sc, sh, relu)
        got = run_linear(xb, wb, sb if sc else None, bb if sh else None, B, K, N, relu, what)
        want = R.linear_ref(x, w, scale if sc else None, shift if sh else None, relu)["y"]
        R.same(got.to(D), want, what, fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("form,B,K,N", R.LINEAR_CASES)
def test_linear_every_form_realistic(form, B, K, N):
    """Head-like magnitudes against the float64 product; per element (chain + 8) 2^-24 sum |x||w| through the epilogue, chain = R.linear_chain."""
    x, w, scale, shift = R.linear_real_inputs(B, K, N)
    xb, wb, sb, bb = inp(x), inp(w), inp(scale), inp(shift)
    chain, ratios = R.linear_chain(B, K, N), {}
    for sc, sh, relu in ((1, 1, 1), (0, 1, 0), (1, 0, 0), (0, 0, 1)):
        what = "linear %s (%d, %d, %d) scale %d shift %d relu %d y" % (form, B, K, N, sc, sh, relu)
        got = run_linear(xb, wb, sb if sc else None, bb if sh else None, B, K, N, relu, what)
        r = R.linear_ref(x, w, scale if sc else None, shift if sh else None, relu, chain=chain)
        bounded(got, (r["y"], r["bound"]), what, ratios)
    print("linear %s (%d, %d, %d): worst error / bound %.3f" % (form, B, K, N, ratios["y"]))


@pytest.mark.parametrize("B,K,N", [(8, 256, 5), (64, 16, 9), (24, 260, 3)])
def test_linear_refuses_misaligned_x_and_w(B, K, N):
    """An x or a w that is 4 bytes off 16-byte alignment (the float4 loads need it): a non-zero code, a message, y untouched."""
    xb = torch.zeros(B * K + 4, device="cuda")
    wb = torch.zeros(N * K + 4, device="cuda")
    y = out(B * N)
    assert xb.data_ptr() % 16 == 0 and wb.data_ptr() % 16 == 0
    for dx, dw in ((4, 0), (0, 4), (4, 4)):
        rc = L().tedspad_linear_fwd(xb.data_ptr() + dx, wb.data_ptr() + dw, None, None, y.data_ptr(), B, K, N, 0, S())
        assert rc != 0 and "aligned" in last_error(), (rc, last_error())
    torch.cuda.synchronize()
    untouched(y, "y of a refused call")
    ok(L().tedspad_linear_fwd(xb.data_ptr(), wb.data_ptr(), None, None, y.data_ptr(), B, K, N, 0, S()))
    assert bool((take(y, B * N, "y") == 0).all())


# ---- tedspad_bce_head_fwd_bwd ------------------------------------------------------------------------------------------------------------------------------
def run_bce(f, W, bias, y, gs, logits=True, grads=True, what="bce"):
    """One call on fresh guarded buffers; returns a dict of host payloads (and the device buffers under '_bufs')."""
    B, N = y.shape
    K = f.shape[1]
    fb, yb = inp(f), inp(y)
    Wb, bb = (inp(W) if W is not None else None), (inp(bias) if bias is not None else None)
    zl, ls = (out(B * N) if logits else None), out(1)
    df = out(B * K) if grads else None
    dW, db = (out(N * K), out(N)) if (grads and W is not None) else (None, None)
    ok(L().tedspad_bce_head_fwd_bwd(fb[1], Wb[1] if Wb else None, bb[1] if bb else None, yb[1], ptr(zl), ls.data_ptr(), ptr(df), ptr(dW), ptr(db), B, K, N,
                                    Ct.c_float(gs), S()))
    r = {"loss": take(ls, 1, what + " loss"), "_bufs": (zl, ls, df, dW, db)}
    if logits:
        r["logits"] = take(zl, B * N, what + " logits", (B, N))
    if grads:
        r["df"] = take(df, B * K, what + " df", (B, K))
        if W is not None:
            r["dW"], r["db"] = take(dW, N * K, what + " dW", (N, K)), take(db, N, what + " db")
    return r


def bce_bounded(r, ref, what, ratios, keys=("loss", "df", "dW", "db")):
    for k in keys:
        bounded(r[k], ref[k], "%s %s" % (what, k), ratios)


@pytest.mark.parametrize("B,K,N", R.BCE_CASES)
def test_bce_head_exact_gradients(B, K, N):
    """Logits restricted to 0 and |z| >= 40: sigmoid - y is 0.5 - y, 1 - y or -y exactly, whatever the device's expf returns, so g is a known dyadic number and
    the logits, df, dW and db must EQUAL the float64 reference (grad_scale 256). Every workgroup derives its columns of df / dW from logits it recomputes
    itself: a wrong logit in any of them shows in its own 256 columns. The loss (not exact: log1p) is held by its bound."""
    f, W, bias, y = R.bce_exact_inputs(B, K, N)
    what = "bce exact (%d, %d, %d)" % (B, K, N)
    r = run_bce(f, W, bias, y, R.BCE_EXACT_SCALE, what=what)
    ref = R.bce_head_ref(f, W, bias, y, R.BCE_EXACT_SCALE)
    fails = []
    R.same(r["logits"].to(D), ref["logits"][0], what + " logits", fails)
    for k in ("df", "dW", "db"):
        R.same(r[k].to(D), ref[k][0].float().to(D), "%s %s" % (what, k), fails,
               detail=(lambda g, w_: "; workgroup (256 columns) of the first: %d" % (int((g != w_).nonzero()[0][-1]) // 256)) if k != "db" else None)
    assert not fails, "\n".join(fails)
    ratios = {}
    bce_bounded(r, ref, what, ratios, keys=("loss",))
    print("%s: loss error / bound %.3f" % (what, ratios["loss"]))


@pytest.mark.parametrize("B,K,N", R.BCE_CASES)
def test_bce_head_dense_integers(B, K, N):
    """Dense integer f and W over all of K: the logits equal the integer product plus bias (the forward's K reduction, in every lane and sweep); loss, df, dW and
    db per element, from the kernel's own logits, so that the bounds cover its roundings after the reduction only. grad_scale 3: a scale that rounds."""
    f, W, bias, y = R.bce_dense_inputs(B, K, N)
    what = "bce dense (%d, %d, %d)" % (B, K, N)
    r = run_bce(f, W, bias, y, R.BCE_DENSE_SCALE, what=what)
    R.same(r["logits"].to(D), R.bce_head_ref(f, W, bias, y)["logits"][0], what + " logits")
    ratios = {}
    bce_bounded(r, R.bce_head_ref(f, W, bias, y, R.BCE_DENSE_SCALE, logits=r["logits"]), what, ratios)
    print("%s: worst error / bound %s" % (what, " ".join("%s %.3f" % kv for kv in sorted(ratios.items()))))


@pytest.mark.parametrize("B,K,N", [(128, 260, 64), (1, 4, 1)])
def test_bce_head_forms_of_the_call(B, K, N):
    """No bias; no logits buffer; loss only (the buffers of an earlier call stay as they were); grad_scale 256 against 1 bit for bit; a second run bit-identical."""
    f, W, bias, y = R.bce_dense_inputs(B, K, N)
    what = "bce forms (%d, %d, %d)" % (B, K, N)
    base = run_bce(f, W, bias, y, 1.0, what=what)
    again = run_bce(f, W, bias, y, 1.0, what=what + " again")
    for k in ("logits", "loss", "df", "dW", "db"):
        assert torch.equal(again[k], base[k]), "%s: %s differs between two runs" % (what, k)
    big = run_bce(f, W, bias, y, 256.0, what=what + " x256")
    assert torch.equal(big["loss"], base["loss"]) and torch.equal(big["logits"], base["logits"])
    for k in ("df", "dW", "db"):
        assert torch.equal(big[k], base[k] * 256.0), "%s: %s at grad_scale 256 is not 256 x" % (what, k)
    ratios = {}
    nb = run_bce(f, W, None, y, 1.0, what=what + " no bias")
    R.same(nb["logits"].to(D), R.bce_head_ref(f, W, None, y)["logits"][0], what + " logits without a bias")
    bce_bounded(nb, R.bce_head_ref(f, W, None, y, 1.0, logits=nb["logits"]), what + " no bias", ratios)
    nl = run_bce(f, W, bias, y, 1.0, logits=False, what=what + " no logits")
    for k in ("loss", "df", "dW", "db"):
        assert torch.equal(nl[k], base[k]), "%s: %s differs without a logits buffer" % (what, k)
    before = [b.clone() for b in base["_bufs"]]
    lo = run_bce(f, W, bias, y, 1.0, grads=False, what=what + " loss only")
    assert torch.equal(lo["loss"], base["loss"]) and torch.equal(lo["logits"], base["logits"])
    l2 = run_bce(f, W, bias, y, 1.0, logits=False, grads=False, what=what + " loss alone")
    assert torch.equal(l2["loss"], base["loss"])
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, base["_bufs"])), "a loss-only call wrote to an earlier call's buffers"
    print("%s: worst error / bound %s" % (what, " ".join("%s %.3f" % kv for kv in sorted(ratios.items()))))


@pytest.mark.parametrize("B,N", [(128, 64), (1, 1)])
def test_bce_logits_mode_at_its_limits(B, N):
    """W == NULL: f holds the logits, here from {0, +-40, +-80}: df = g * grad_scale with g exact; then realistic logits up to |z| = 80 against the bounds."""
    z = 40.0 * (R._draw(79, "bcel%d" % N, (B, N), 5) - 2)
    y = torch.tensor([0.25, 0.5, 1.0], dtype=D)[R._draw(79, "bcely%d" % N, (B, N), 3).long()]
    what = "bce logits mode (%d, %d)" % (B, N)
    r = run_bce(z, None, None, y, R.BCE_EXACT_SCALE, what=what)
    ref = R.bce_head_ref(z, None, None, y, R.BCE_EXACT_SCALE)
    R.same(r["logits"].to(D), z, what + " logits")
    R.same(r["df"].to(D), ref["df"][0].float().to(D), what + " df")
    ratios = {}
    bce_bounded(r, ref, what, ratios, keys=("loss",))
    z2 = R.synth_tensor(79, "bcelz%d" % N, (B, N), -80, 80)
    y2 = R.synth_tensor(79, "bcely2%d" % N, (B, N))
    r2 = run_bce(z2, None, None, y2, R.BCE_DENSE_SCALE, logits=False, what=what + " realistic")
    bce_bounded(r2, R.bce_head_ref(z2, None, None, y2, R.BCE_DENSE_SCALE), what + " realistic", ratios, keys=("loss", "df"))
    lo = run_bce(z2, None, None, y2, 1.0, logits=False, grads=False, what=what + " loss only")
    assert torch.equal(lo["loss"], r2["loss"])
    print("%s: worst error / bound %s" % (what, " ".join("%s %.3f" % kv for kv in sorted(ratios.items()))))


def test_bce_head_refusals():
    """Logits mode with K != N or with a bias; only some of df / dW / db; a misaligned df: a non-zero code and a message, nothing written."""
    B, K, N = 4, 8, 8
    f, W, bias, y = (torch.zeros(n + 4, device="cuda") for n in (B * K, N * K, N, B * N))
    zl, ls, df, dW, db = out(B * N), out(1), out(B * K + 4), out(N * K), out(N)
    a = dict(f=f.data_ptr(), W=W.data_ptr(), bias=bias.data_ptr(), y=y.data_ptr(), logits=zl.data_ptr(), loss=ls.data_ptr(), df=df.data_ptr(), dW=dW.data_ptr(),
             db=db.data_ptr(), B=B, K=K, N=N)
    assert df.data_ptr() % 16 == 0

    def call(**kw):
        v = dict(a, **kw)
        return L().tedspad_bce_head_fwd_bwd(v["f"], v["W"], v["bias"], v["y"], v["logits"], v["loss"], v["df"], v["dW"], v["db"], v["B"], v["K"], v["N"],
                                            Ct.c_float(1.0), S())
    bad = [("logits mode with K != N", dict(W=None, bias=None, dW=None, db=None, K=4), "logits mode"),
           ("logits mode with a bias", dict(W=None, dW=None, db=None), "logits mode"),
           ("logits mode with dW", dict(W=None, bias=None, db=None), "logits mode"),
           ("df alone", dict(dW=None, db=None), "df, dW and db"), ("dW and db without df", dict(df=None), "df, dW and db"), ("no db", dict(db=None), "df, dW and db"),
           ("a misaligned df", dict(df=df.data_ptr() + 4), "aligned"), ("a misaligned dW", dict(dW=dW.data_ptr() + 4), "aligned"),
           ("a misaligned f", dict(f=f.data_ptr() + 4), "aligned"), ("K % 4", dict(K=6), "K % 4"), ("B above the limit", dict(B=129), "B <= 128"),
           ("N above the limit", dict(N=65), "N <= 64")]
    for name, kw, word in bad:
        rc = call(**kw)
        assert rc != 0 and word in last_error(), (name, rc, last_error())
    torch.cuda.synchronize()
    for b, name in ((zl, "logits"), (ls, "loss"), (df, "df"), (dW, "dW"), (db, "db")):
        untouched(b, name + " of a refused call")
    ok(call())


# ---- the vote kernels and tedspad_softmax_ce_eval --------------------------------------------------------------------------------------------------------------
def run_accumulate(probs, vid, sums, counts, V, parts=None):
    """sums / counts after the launch(es) over the row ranges `parts` (default: one launch), as numpy"""
    B, C = probs.shape
    pb = inp(torch.from_numpy(probs))
    sb, cb = out(V * C, fill=torch.from_numpy(sums)), out(V, torch.int32, fill=torch.from_numpy(counts))
    for a, b in (parts or [(0, B)]):
        host = np.ascontiguousarray(np.asarray(vid[a:b], np.int32))
        dev = torch.from_numpy(host).cuda()
        ok(L().tedspad_vote_accumulate(pb[1] + 4 * a * C, dev.data_ptr(), host.ctypes.data, sb.data_ptr(), cb.data_ptr(), b - a, C, V, S()))
        torch.cuda.synchronize()
    return take(sb, V * C, "vote sums", (V, C)).numpy(), take(cb, V, "vote counts").numpy()


@pytest.mark.parametrize("B", R.VOTE_B)
@pytest.mark.parametrize("C", R.VOTE_C)
def test_vote_accumulate_bit_for_bit(B, C):
    """One fp32 add per row and class, in row order, from what `sums` held: equal in every bit to the host walk (R.vote_accumulate_ref), over one to four
    workgroups, long runs, strict alternation and single rows; the video no row names keeps its sums and its count; two launches over a split batch equal one."""
    probs, vid, sums, counts, V = R.vote_inputs(B, C)
    ws, wc = R.vote_accumulate_ref(probs, vid, sums, counts)
    s, c = run_accumulate(probs, vid, sums, counts, V)
    fails = []
    R.same(torch.from_numpy(s.view(np.int32).copy()), torch.from_numpy(ws.view(np.int32).copy()), "vote sums (%d, %d), as bits" % (B, C), fails)
    R.same(torch.from_numpy(c), torch.from_numpy(wc), "vote counts (%d, %d)" % (B, C), fails)
    if B > 1:
        h = B // 2 + 1
        s2, c2 = run_accumulate(probs, vid, sums, counts, V, parts=[(0, h), (h, B)])
        R.same(torch.from_numpy(s2.view(np.int32).copy()), torch.from_numpy(ws.view(np.int32).copy()), "vote sums (%d, %d) in two launches, as bits" % (B, C), fails)
        R.same(torch.from_numpy(c2), torch.from_numpy(wc), "vote counts (%d, %d) in two launches" % (B, C), fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("V", R.VOTE_FINAL_V)
@pytest.mark.parametrize("C", R.VOTE_C)
def test_vote_finalize_division_and_ties(V, C):
    """mean = numpy's fp32 division; among exactly equal maxima -- in two neighbouring lanes, in one lane 64 classes apart, in the first and the last class --
    the highest index wins; a video without rows: zeros, -1, not correct."""
    sums, counts, labels, want = R.vote_finalize_inputs(V, C)
    sb, cb, lb = inp(torch.from_numpy(sums)), torch.from_numpy(counts).cuda(), torch.from_numpy(labels).cuda()
    mean, pred, cor = out(V * C), out(V, torch.int32), out(V, torch.uint8)
    ok(L().tedspad_vote_finalize(sb[1], cb.data_ptr(), lb.data_ptr(), mean.data_ptr(), pred.data_ptr(), cor.data_ptr(), V, C, S()))
    wm, wp, wc = R.vote_finalize_ref(sums, counts, labels)
    fails = []
    R.same(take(mean, V * C, "vote mean", (V, C)), torch.from_numpy(wm), "vote mean (%d, %d)" % (V, C), fails)
    R.same(take(pred, V, "vote pred"), torch.from_numpy(wp), "vote top-1 (%d, %d)" % (V, C), fails)
    R.same(take(cor, V, "vote correct"), torch.from_numpy(wc), "vote correct (%d, %d)" % (V, C), fails)
    assert not fails, "\n".join(fails)
    assert [int(p) for p, w in zip(wp, want) if w != -2] == [w for w in want if w != -2]


@pytest.mark.parametrize("C", [2, 65])
def test_softmax_ce_eval_at_the_batch_limit(C):
    """B = 1024, the most the kernel takes (64 rows per wave; the whole row-loss array in LDS): the top-1 class equal to the float64 argmax on every row,
    probabilities and row losses per element, the mean within its chain's bound."""
    B = 1024
    z, lab = R.sce_logits(B, C)
    zb, lb = inp(z), lab.cuda()
    probs, rows, loss, pred = out(B * C), out(B), out(1), out(B, torch.int32)
    lab_h = np.ascontiguousarray(lab.numpy())
    ok(L().tedspad_softmax_ce_eval(zb[1], lb.data_ptr(), lab_h.ctypes.data, probs.data_ptr(), rows.data_ptr(), loss.data_ptr(), pred.data_ptr(), B, C, S()))
    ref = R.softmax_ce_ref(z, lab)
    got_pred = take(pred, B, "pred")
    R.same(got_pred.long(), ref["pred"], "softmax_ce_eval top-1 (%d, %d)" % (B, C))
    ratios = {}
    bounded(take(probs, B * C, "probs", (B, C)), ref["probs"], "softmax_ce_eval (%d, %d) probs" % (B, C), ratios)
    bounded(take(rows, B, "row loss"), ref["row_loss"], "softmax_ce_eval (%d, %d) row_loss" % (B, C), ratios)
    bounded(take(loss, 1, "loss"), ref["loss"], "softmax_ce_eval (%d, %d) loss" % (B, C), ratios)
    print("softmax_ce_eval (%d, %d): worst error / bound %s" % (B, C, " ".join("%s %.3f" % kv for kv in sorted(ratios.items()))))
