"""-m gpu: every kernel of csrc/mgfn_train.hip against fp64 torch autograd on the same inputs, over ragged batches. Bound: the 1e-5 rel-L2
of tests/test_hip_mgfn.py; for the long token reductions (weight / bias gradients), where fp32 itself may not reach it, 10x the error of
torch's own fp32 CPU result against fp64 on the same inputs, measured in the test (both are printed). Reductions are run twice and
compared bit for bit."""
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2
from kernel_refs import mgfn_attention_torch, mgfn_conv_autograd as _conv_ref, mgfn_relpos_torch
from ted_spad_amd import _lib
from ted_spad_amd import mgfn as K
from ted_spad_amd.engine import _stream_ptr
from ted_spad_amd.synth import synth_tensor

import mgfn_train_restate as R

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 3, 5, 32, 33, 70]
BOUND = 1e-5


def _ragged(lengths):
    L = torch.tensor(lengths, dtype=torch.int64)
    off = torch.zeros(len(L) + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(L, 0)
    st = off[:-1].repeat_interleave(L)
    bounds = torch.stack([st, st + L.repeat_interleave(L)], 1).to(torch.int32).cuda()
    return off.tolist(), bounds, off.to(torch.int32).cuda()


def _check(name, got, ref, ref32=None):
    """rel-L2 of got against the fp64 ref within BOUND, or (ref32 given: torch's fp32 CPU result) within 10x ref32's own error."""
    ref = ref.detach().cpu().double().numpy()
    e = rel_l2(got.detach().cpu().double().numpy(), ref)
    bound = BOUND
    if ref32 is not None:
        e32 = rel_l2(ref32.detach().cpu().double().numpy(), ref)
        bound = max(BOUND, 10 * e32)
        print("%-36s rel-L2 %.2e   torch fp32 CPU %.2e   bound %.2e" % (name, e, e32, bound))
    else:
        print("%-36s rel-L2 %.2e" % (name, e))
    assert e <= bound, (name, e, bound)


WG = {"k3_80x64": (3, 80, 64), "k3_128x128": (3, 128, 128), "k1_1024x4096": (1, 1024, 4096), "k1_4096x1024": (1, 4096, 1024)}


@pytest.mark.parametrize("lengths", [LENGTHS, [1500, 7]], ids=["ragged", "chunks"])
@pytest.mark.parametrize("mode", list(WG))
def test_wgrad_and_bias_grad_vs_fp64(mode, lengths):
    taps, cin, N = WG[mode]
    off, bounds, _ = _ragged(lengths)
    M = off[-1]
    tag = "%s/%d" % (mode, M)
    x = synth_tensor(11, "wg_x" + tag, (M, cin), -2, 2)
    if cin == 80:
        x[:, 65:] = 0                                              # F + 1 = 65 channels padded to 80, the pad is zero
    dy = synth_tensor(11, "wg_dy" + tag, (M, N), -1, 1)
    xc, dc = x.cuda(), dy.cuda()
    runs = []
    for _ in range(2):
        dw = K.token_wgrad(xc, dc, bounds if taps > 1 else None, taps, cin)
        db = K.col_reduce(dc)[0]
        runs.append((dw.clone(), db.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    w0, b0 = torch.zeros(N, taps, cin), torch.zeros(N)
    _, dw64, db64 = _conv_ref(x.double(), w0.double(), b0.double(), taps, off, dy.double())
    _, dw32, db32 = _conv_ref(x, w0, b0, taps, off, dy)
    _check("wgrad " + tag, runs[0][0], dw64, dw32)
    _check("bias grad " + tag, runs[0][1], db64, db32)
    if cin == 80:
        assert float(runs[0][0][:, :, 65:].abs().max()) == 0.0


@pytest.mark.parametrize("mode", ["k3_128x128", "k1_1024x4096", "k1_4096x1024"])
def test_dgrad_vs_fp64(mode):
    taps, cin, N = WG[mode]
    off, bounds, _ = _ragged(LENGTHS)
    M = off[-1]
    w = synth_tensor(12, "dg_w" + mode, (N, taps, cin), -1, 1) / (taps * cin) ** 0.5
    dy = synth_tensor(12, "dg_dy" + mode, (M, N), -1, 1)
    res = synth_tensor(12, "dg_r" + mode, (M, cin), -1, 1)
    wt = w.flip(1).permute(2, 1, 0).contiguous().cuda()             # (cin, tap, N), taps reversed
    dx = K.token_gemm(dy.cuda(), wt, None, cin, bounds if taps > 1 else None, taps, N, res.cuda())
    dx64, _, _ = _conv_ref(torch.zeros(M, cin, dtype=torch.float64), w.double(), torch.zeros(N, dtype=torch.float64), taps, off, dy.double())
    _check("dgrad " + mode, dx, dx64 + res.double())


@pytest.mark.parametrize("C", [64, 1024])
@pytest.mark.parametrize("torch_ln", [0, 1])
def test_layernorm_fwd_bwd_vs_fp64(torch_ln, C):
    M = sum(LENGTHS)
    tag = "%d/%d" % (torch_ln, C)
    x = synth_tensor(13, "ln_x" + tag, (M, C), -3, 5)
    g, b = synth_tensor(13, "ln_g" + tag, (C,), 0.5, 1.5), synth_tensor(13, "ln_b" + tag, (C,), -0.1, 0.1)
    dy, add = synth_tensor(13, "ln_dy" + tag, (M, C), -1, 1), synth_tensor(13, "ln_add" + tag, (M, C), -1, 1)
    xc, gc, bc, dc, ac = x.cuda(), g.cuda(), b.cuda(), dy.cuda(), add.cuda()
    L, st = _lib.lib(), _stream_ptr()
    s = torch.empty((M, 2), device="cuda")
    _lib.check(L.tedspad_mgfn_ln_stats(xc.data_ptr(), C, M, C, 1e-5, torch_ln, s.data_ptr(), st))
    y, dx = torch.empty_like(xc), torch.empty_like(xc)
    _lib.check(L.tedspad_mgfn_ln_apply(xc.data_ptr(), C, s.data_ptr(), gc.data_ptr(), bc.data_ptr(), M, C, y.data_ptr(), C, st))
    _lib.check(L.tedspad_mgfn_ln_bwd(dc.data_ptr(), C, xc.data_ptr(), C, s.data_ptr(), gc.data_ptr(), torch_ln, 1e-5, ac.data_ptr(), C,
                                     dx.data_ptr(), C, M, C, st))
    db, dg = K.col_reduce(dc, xc, s, 1)
    db2, dg2 = K.col_reduce(dc, xc, s, 1)
    assert torch.equal(db, db2) and torch.equal(dg, dg2)
    xd, gd, bd = (t.double().requires_grad_(True) for t in (x, g, b))
    if torch_ln:
        yd = F.layer_norm(xd, (C,), gd, bd, 1e-5)
    else:                                                           # utils.py:108-111
        mu = xd.mean(1, keepdim=True)
        yd = (xd - mu) / (((xd - mu) ** 2).mean(1, keepdim=True).sqrt() + 1e-5) * gd + bd
    (yd * dy.double()).sum().backward()
    _check("ln y " + tag, y, yd)
    _check("ln dx " + tag, dx, xd.grad + add.double())
    _check("ln dg " + tag, dg, gd.grad)
    _check("ln db " + tag, db, bd.grad)


@pytest.mark.parametrize("M", [sum(LENGTHS), 1507])
def test_batchnorm_train_fwd_bwd_vs_fp64(M):
    C = 128
    tag = "%d" % M
    x = synth_tensor(14, "bn_x" + tag, (M, C), -3, 5)
    g, b = synth_tensor(14, "bn_g", (C,), 0.5, 1.5), synth_tensor(14, "bn_b", (C,), -0.2, 0.2)
    rm, rv = synth_tensor(14, "bn_rm", (C,), -0.1, 0.1), synth_tensor(14, "bn_rv", (C,), 0.5, 1.5)
    dy, add = synth_tensor(14, "bn_dy" + tag, (M, C), -1, 1), synth_tensor(14, "bn_add" + tag, (M, C), -1, 1)
    L, st = _lib.lib(), _stream_ptr()
    xc, gc, bc, dc, ac = x.cuda(), g.cuda(), b.cuda(), dy.cuda(), add.cuda()
    ws = torch.empty(int(L.tedspad_mgfn_train_ws_floats(M, C)), device="cuda")
    outs = []
    for _ in range(2):
        rmc, rvc = rm.cuda(), rv.cuda()
        stat, y, dx = torch.empty(2 * C, device="cuda"), torch.empty_like(xc), torch.empty_like(xc)
        dgam, dbet = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
        _lib.check(L.tedspad_mgfn_bn_train_fwd(xc.data_ptr(), C, M, C, gc.data_ptr(), bc.data_ptr(), 1e-5, 0.1, ws.data_ptr(), stat.data_ptr(),
                                               rmc.data_ptr(), rvc.data_ptr(), y.data_ptr(), C, st))
        _lib.check(L.tedspad_mgfn_bn_train_bwd(dc.data_ptr(), C, xc.data_ptr(), C, stat.data_ptr(), gc.data_ptr(), M, C, ws.data_ptr(),
                                               dgam.data_ptr(), dbet.data_ptr(), ac.data_ptr(), C, dx.data_ptr(), C, st))
        outs.append([t.clone() for t in (y, stat, rmc, rvc, dx, dgam, dbet)])
    assert all(torch.equal(p, q) for p, q in zip(*outs))
    y, stat, rmc, rvc, dx, dgam, dbet = outs[0]
    bn = torch.nn.BatchNorm1d(C).double().train()
    with torch.no_grad():
        bn.weight.copy_(g), bn.bias.copy_(b), bn.running_mean.copy_(rm), bn.running_var.copy_(rv)
    xd = x.double().requires_grad_(True)
    yd = bn(xd)
    (yd * dy.double()).sum().backward()
    _check("bn y " + tag, y, yd)
    _check("bn mean " + tag, stat[:C], x.double().mean(0))
    _check("bn invstd " + tag, stat[C:], 1 / (x.double().var(0, unbiased=False) + 1e-5).sqrt())
    _check("bn running_mean " + tag, rmc, bn.running_mean)
    _check("bn running_var " + tag, rvc, bn.running_var)
    _check("bn dx " + tag, dx, xd.grad + add.double())
    _check("bn dgamma " + tag, dgam, bn.weight.grad)
    _check("bn dbeta " + tag, dbet, bn.bias.grad)


def test_gelu_fwd_bwd_vs_fp64():
    n = 146 * 256
    x = synth_tensor(15, "gelu_x", (n,), -6, 6)
    dy = synth_tensor(15, "gelu_dy", (n,), -1, 1)
    xc, dc = x.cuda(), dy.cuda()
    y, dx = torch.empty_like(xc), torch.empty_like(xc)
    _lib.check(_lib.lib().tedspad_mgfn_gelu(xc.data_ptr(), y.data_ptr(), n, _stream_ptr()))
    _lib.check(_lib.lib().tedspad_mgfn_gelu_bwd(xc.data_ptr(), dc.data_ptr(), dx.data_ptr(), n, _stream_ptr()))
    xd = x.double().requires_grad_(True)
    yd = F.gelu(xd)
    (yd * dy.double()).sum().backward()
    _check("gelu", y, yd)
    _check("gelu bwd", dx, xd.grad)


@pytest.mark.parametrize("heads", [1, 2, 16])
def test_attention_bwd_vs_fp64(heads):
    off, _, off_d = _ragged(LENGTHS)
    M, inner = off[-1], 64 * heads
    qkv = synth_tensor(16, "attb%d" % heads, (M, 3 * inner), -2, 2)
    do = synth_tensor(16, "attb_do%d" % heads, (M, inner), -1, 1)
    qc, dc = qkv.cuda(), do.cuda()
    L, st = _lib.lib(), _stream_ptr()
    o, dqkv, lse = torch.empty((M, inner), device="cuda"), torch.full((M, 3 * inner), float("nan"), device="cuda"), torch.empty((M, heads, 2), device="cuda")
    _lib.check(L.tedspad_mgfn_attention(qc.data_ptr(), 3 * inner, off_d.data_ptr(), len(LENGTHS), max(LENGTHS), heads, o.data_ptr(), inner, st))
    _lib.check(L.tedspad_mgfn_attention_bwd(qc.data_ptr(), 3 * inner, o.data_ptr(), inner, dc.data_ptr(), inner, off_d.data_ptr(), len(LENGTHS),
                                            max(LENGTHS), heads, lse.data_ptr(), dqkv.data_ptr(), 3 * inner, st))
    first = dqkv.clone()
    _lib.check(L.tedspad_mgfn_attention_bwd(qc.data_ptr(), 3 * inner, o.data_ptr(), inner, dc.data_ptr(), inner, off_d.data_ptr(), len(LENGTHS),
                                            max(LENGTHS), heads, lse.data_ptr(), dqkv.data_ptr(), 3 * inner, st))
    assert torch.equal(first, dqkv)
    _, grad = mgfn_attention_torch(qkv, off, heads, torch.float64, do)
    for name, sl in (("dq", slice(0, inner)), ("dk", slice(inner, 2 * inner)), ("dv", slice(2 * inner, 3 * inner))):
        _check("attention bwd %s heads=%d" % (name, heads), dqkv[:, sl], grad[:, sl])


@pytest.mark.parametrize("heads", [2, 16])
def test_relpos_bwd_vs_fp64(heads):
    off, bounds, _ = _ragged(LENGTHS)
    M, C = off[-1], 64 * heads
    v = synth_tensor(17, "rpb_v%d" % heads, (M, C), -1, 1)
    w = synth_tensor(17, "rpb_w%d" % heads, (heads, 5), -1, 1)
    do = synth_tensor(17, "rpb_do%d" % heads, (M, C), -1, 1)
    L, st = _lib.lib(), _stream_ptr()
    vc, wc, dc = v.cuda(), w.cuda(), do.cuda()
    ws = torch.empty(int(L.tedspad_mgfn_train_ws_floats(M, C)), device="cuda")
    outs = []
    for _ in range(2):
        dv, dw, db = torch.empty_like(vc), torch.empty((heads, 5), device="cuda"), torch.empty(heads, device="cuda")
        _lib.check(L.tedspad_mgfn_relpos_bwd(dc.data_ptr(), C, vc.data_ptr(), C, bounds.data_ptr(), M, C, heads, wc.data_ptr(), ws.data_ptr(),
                                             dv.data_ptr(), C, dw.data_ptr(), db.data_ptr(), st))
        outs.append((dv.clone(), dw.clone(), db.clone()))
    assert all(torch.equal(p, q) for p, q in zip(*outs))
    _, dv64, dw64, db64 = mgfn_relpos_torch(v, w, torch.zeros(heads), off, heads, torch.float64, do)
    _check("relpos bwd dv heads=%d" % heads, outs[0][0], dv64)
    _check("relpos bwd dw heads=%d" % heads, outs[0][1], dw64)
    _check("relpos bwd db heads=%d" % heads, outs[0][2], db64)


def test_head_bwd_vs_fp64():
    M, C = sum(LENGTHS), 1024
    x = synth_tensor(18, "hb_x", (M, C), -3, 5)
    lw, lb = synth_tensor(18, "hb_lw", (C,), 0.5, 1.5), synth_tensor(18, "hb_lb", (C,), -0.1, 0.1)
    fw = synth_tensor(18, "hb_fw", (C,), -0.05, 0.05)
    dscore = synth_tensor(18, "hb_ds", (M,), 0.2, 1)          # one sign: d fc.bias = sum_m dz_m is a single number, and with mixed signs it
                                                               # cancels to ~1e-3 of sum |dz|, which no fp32 sum resolves to 1e-5
    dh_sel = synth_tensor(18, "hb_dh", (M, C), -1, 1)
    dh_sel[torch.arange(M) % 3 != 0] = 0                              # most rows receive no feature gradient
    L, st = _lib.lib(), _stream_ptr()
    xc, lwc, lbc, fwc, dsc = x.cuda(), lw.cuda(), lb.cuda(), fw.cuda(), dscore.cuda()
    h, lg, sc, mg = torch.empty((M, C), device="cuda"), *(torch.empty(M, device="cuda") for _ in range(3))
    _lib.check(L.tedspad_mgfn_head(xc.data_ptr(), C, M, C, lwc.data_ptr(), lbc.data_ptr(), fwc.data_ptr(), 0.05, 1e-5, h.data_ptr(), lg.data_ptr(),
                                   sc.data_ptr(), mg.data_ptr(), st))
    dh, dz = dh_sel.cuda(), torch.empty(M, device="cuda")
    _lib.check(L.tedspad_mgfn_head_bwd(sc.data_ptr(), dsc.data_ptr(), fwc.data_ptr(), M, C, dh.data_ptr(), dz.data_ptr(), st))
    dfw, dfb = K.col_reduce(h, None, dz, 4)
    s = torch.empty((M, 2), device="cuda")
    _lib.check(L.tedspad_mgfn_ln_stats(xc.data_ptr(), C, M, C, 1e-5, 1, s.data_ptr(), st))
    dlb, dlw = K.col_reduce(dh, xc, s, 1)
    dx = torch.empty_like(xc)
    _lib.check(L.tedspad_mgfn_ln_bwd(dh.data_ptr(), C, xc.data_ptr(), C, s.data_ptr(), lwc.data_ptr(), 1, 1e-5, None, 0, dx.data_ptr(), C, M, C, st))
    xd, lwd, lbd, fwd = (t.double().requires_grad_(True) for t in (x, lw, lb, fw))
    fbd = torch.tensor(0.05, dtype=torch.float64, requires_grad=True)
    hd = F.layer_norm(xd, (C,), lwd, lbd, 1e-5)
    sd = torch.sigmoid(hd @ fwd + fbd)
    ((sd * dscore.double()).sum() + (hd * dh_sel.double()).sum()).backward()
    _check("head bwd dx", dx, xd.grad)
    _check("head bwd dln_w", dlw, lwd.grad)
    _check("head bwd dln_b", dlb, lbd.grad)
    _check("head bwd dfc_w", dfw, fwd.grad)
    _check("head bwd dfc_b", dfb[:1], fbd.grad.view(1))


# ---- MSNSD + cost -----------------------------------------------------------------------------------------------------------------------
def _msnsd(h, scores, n, nc, T, k, masks, labels):
    """Runs crop_mean + tedspad_mgfn_msnsd on h (2n nc T, C), scores (2n nc T) (device). Returns a dict of device tensors."""
    C, M = h.shape[1], h.shape[0]
    L, st = _lib.lib(), _stream_ptr()
    mags = h.norm(dim=1).contiguous()
    cs, cm = torch.empty(2 * n * T, device="cuda"), torch.empty(2 * n * T, device="cuda")
    seg = (torch.arange(2 * n + 1) * T).to(torch.int32).cuda()
    _lib.check(L.tedspad_mgfn_crop_mean(scores.data_ptr(), cs.data_ptr(), mags.data_ptr(), cm.data_ptr(), seg.data_ptr(), 2 * n, T, nc, st))
    f = dict(device="cuda", dtype=torch.float32)
    o = dict(idx=torch.empty((2 * n, k), dtype=torch.int32, device="cuda"), vid=torch.empty(2 * n, **f), l1=torch.empty((2, n * nc, k), **f),
             losses=torch.empty(8, **f), dl1=torch.empty((2, n * nc, k), **f), dcs=torch.empty(2 * n * T, **f), dvid=torch.empty(2 * n, **f),
             dscore=torch.empty(M, **f), dh=torch.full((M, C), float("nan"), **f))
    mk = torch.stack(masks).float().cuda().contiguous()
    lab = labels.float().cuda()
    _lib.check(L.tedspad_mgfn_msnsd(h.data_ptr(), cs.data_ptr(), cm.data_ptr(), mk.data_ptr(), lab.data_ptr(), n, nc, T, C, k, o["idx"].data_ptr(),
                                    o["vid"].data_ptr(), o["l1"].data_ptr(), o["losses"].data_ptr(), o["dl1"].data_ptr(), o["dcs"].data_ptr(),
                                    o["dvid"].data_ptr(), o["dscore"].data_ptr(), o["dh"].data_ptr(), st))
    return o


def _msnsd_ref(h, scores, n, nc, T, k, masks, labels):
    hd = h.double().view(2 * n * nc, T, -1).requires_grad_(True)
    sd = scores.double().view(2 * n * nc, T).requires_grad_(True)
    r = R.msnsd_cost(hd, sd, n, nc, tuple(m.double() for m in masks), labels[:n].double(), labels[n:].double(), k)
    r["cost"].backward()
    return r, hd.grad.view(h.shape), sd.grad.view(-1)


def _compare_msnsd(name, o, r, dh, ds, n):
    names = ("cost", "loss_smooth", "loss_sparse", "loss_cls", "loss_con", "loss_con_n", "loss_con_a", "loss_total")
    for i, nm in enumerate(names):
        got, want = float(o["losses"][i]), float(r[nm])
        print("%s %-12s %.9g (fp64 %.9g)" % (name, nm, got, want))
        assert abs(got - want) <= 1e-5 * max(abs(want), 1e-30), (name, nm, got, want)
    assert torch.equal(o["idx"][:n].cpu().long(), r["idx_normal"]) and torch.equal(o["idx"][n:].cpu().long(), r["idx_abnormal"])
    _check(name + " video scores", o["vid"], torch.cat((r["score_normal"], r["score_abnormal"])).view(-1))
    _check(name + " d score", o["dscore"], ds)
    _check(name + " d h", o["dh"], dh)


def _row_scale(n, nc):
    """(2n, nc, 1, 1): crops and videos 15-50 % apart in magnitude, so that the L1 norms the contrastive terms subtract (second half of the
    crop-major rows against the first) differ by far more than their fp32 rounding and the loss terms are well conditioned."""
    v = torch.arange(2 * n, dtype=torch.float32).remainder(n).view(2 * n, 1, 1, 1)
    c = torch.arange(nc, dtype=torch.float32).view(1, nc, 1, 1)
    return 1 + 0.3 * c / nc + 0.2 * v


@pytest.mark.parametrize("shape", [(2, 10, 32, 1024), (3, 2, 5, 64), (2, 1, 3, 64)], ids=["n2c10T32", "n3c2T5", "n2c1T3"])
def test_msnsd_cost_vs_restatement(shape):
    n, nc, T, C = shape
    k, M = 3, 2 * n * nc * T
    tag = "%d_%d_%d" % (n, nc, T)
    h = synth_tensor(19, "ms_h" + tag, (M, C), -1, 1)
    # a per-segment scale 1 + 0.05 rank: the crop-mean magnitudes of a video are ~5 % apart, far above fp32 rounding (safe top-k gaps)
    perm = torch.stack([torch.randperm(T, generator=torch.Generator().manual_seed(v)) for v in range(2 * n)])
    h = (h.view(2 * n, nc, T, C) * (1 + 0.05 * perm.float()).view(2 * n, 1, T, 1) * _row_scale(n, nc)).reshape(M, C).contiguous()
    scores = synth_tensor(19, "ms_s" + tag, (M,), 0.05, 0.95)
    masks = [(synth_tensor(19, "ms_m%d" % i + tag, (n, T)) >= (0.0 if T <= 5 else 0.5)).float() / 0.3 for i in range(2)]
    labels = torch.cat((torch.zeros(n), torch.ones(n)))
    o = _msnsd(h.cuda(), scores.cuda(), n, nc, T, k, masks, labels)
    r, dh, ds = _msnsd_ref(h, scores, n, nc, T, k, masks, labels)
    _compare_msnsd("msnsd " + tag, o, r, dh, ds, n)


@pytest.mark.parametrize("case", ["hinge_open", "hinge_closed", "log_clamp", "few_survivors"])
def test_msnsd_cost_hand_made(case):
    """Both branches of clamp(margin - d, 0): rows of L1 norm ~C |h|, so |h| ~ 0.01 keeps the distance under the margin of 200 and |h| ~ 1
    puts it far above; the -100 log clamp: a video score of exactly 0 under label 1 and exactly 1 under label 0; fewer than k survivors."""
    n, nc, T, C, k = 2, 2, 6, 64, 3
    M = 2 * n * nc * T
    h = synth_tensor(20, "hm_h" + case, (M, C), -1, 1)
    perm = torch.stack([torch.randperm(T, generator=torch.Generator().manual_seed(7 + v)) for v in range(2 * n)])
    h = (h.view(2 * n, nc, T, C) * (1 + 0.05 * perm.float()).view(2 * n, 1, T, 1) * _row_scale(n, nc)).reshape(M, C)
    scale = 0.01 if case == "hinge_open" else 1.0
    h = h * scale
    h.view(2 * n, nc * T, C)[n:] *= 40.0                               # abnormal rows 40x the normal ones
    h = h.contiguous()
    scores = synth_tensor(20, "hm_s" + case, (M,), 0.05, 0.95)
    masks = [torch.ones(n, T) / 0.3 for _ in range(2)]
    labels = torch.cat((torch.zeros(n), torch.ones(n)))
    if case == "log_clamp":
        sv = scores.view(2 * n, nc, T)
        sv[0] = 1.0                                                    # normal video 0 (label 0): log(1 - s) = -inf -> -100
        sv[n] = 0.0                                                    # abnormal video 0 (label 1): log(s) = -inf -> -100
    if case == "few_survivors":
        masks[0][1] = 0
        masks[0][1, 4] = 1 / 0.3                                       # abnormal video 1: one survivor -> picks 4, then 0, 1 (lowest index)
    o = _msnsd(h.cuda(), scores.cuda(), n, nc, T, k, masks, labels)
    r, dh, ds = _msnsd_ref(h, scores, n, nc, T, k, masks, labels)
    d = F.pairwise_distance(r["abn_feamagnitude"].norm(p=1, dim=2), r["nor_feamagnitude"].norm(p=1, dim=2))
    if case == "hinge_open":
        assert (d < 200).all() and float(r["loss_con"]) > 0
    else:
        assert (d > 200).all() and float(r["loss_con"]) == 0
    if case == "log_clamp":
        assert abs(float(r["loss_cls"]) - (200.0 + float(-torch.log(1 - r["score_normal"][1]) - torch.log(r["score_abnormal"][1]))) / 4) < 1e-9
    if case == "few_survivors":
        assert o["idx"][n + 1].tolist() == [4, 0, 1]
    _compare_msnsd("msnsd " + case, o, r, dh, ds, n)
