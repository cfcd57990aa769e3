"""-m gpu: fused loss kernels (value + gradients) against the golden vectors captured from
the reference's own NTXentLoss / TripletMarginLoss / CrossEntropyLoss and the float64 oracle."""
import numpy as np
import pytest
import torch

from conftest import rel_l2
from ted_spad_amd.synth import synth_tensor

pytestmark = pytest.mark.gpu


def _unit(name, shape):
    return torch.nn.functional.normalize(synth_tensor(0, name, shape, -1, 1), dim=1)


def test_ntxent_golden(golden):
    from ted_spad_amd.losses import NTXentLoss
    zi = _unit("ntx_zi", (12, 128)).cuda().requires_grad_()
    zj = _unit("ntx_zj", (12, 128)).cuda().requires_grad_()
    l = NTXentLoss("cuda", 12, 0.1, False)(zi, zj)
    l.backward()
    assert abs(l.item() - golden["ntxent_value"][0]) < 2e-5 * abs(golden["ntxent_value"][0])
    assert rel_l2(zi.grad.cpu(), golden["ntxent_grad_zi"]) < 1e-4
    assert rel_l2(zj.grad.cpu(), golden["ntxent_grad_zj"]) < 1e-4


@pytest.mark.parametrize("n,c,cos", [(1, 2, False), (4, 128, False), (12, 128, True), (32, 256, False), (17, 64, True)])
def test_ntxent_vs_oracle(n, c, cos):
    from oracle import losses_ref
    from ted_spad_amd.losses import NTXentLoss
    zi0 = synth_tensor(1, "zi%d" % n, (n, c), -1, 1) * 0.3
    zj0 = synth_tensor(1, "zj%d" % n, (n, c), -1, 1) * 0.3
    zi, zj = zi0.cuda().requires_grad_(), zj0.cuda().requires_grad_()
    l = NTXentLoss("cuda", n, 0.1, cos)(zi, zj)
    (l * 2.0).backward()  # also checks scaling by the incoming gradient
    ref = losses_ref.nt_xent_np(zi0.numpy(), zj0.numpy(), 0.1, use_cosine=cos)
    assert abs(l.item() - ref) < 1e-4 * max(1.0, abs(ref))
    a, b = zi0.double().requires_grad_(), zj0.double().requires_grad_()
    if cos:
        lr = losses_ref.nt_xent_torch(torch.nn.functional.normalize(a, dim=1, eps=1e-8), torch.nn.functional.normalize(b, dim=1, eps=1e-8), 0.1)
    else:
        lr = losses_ref.nt_xent_torch(a, b, 0.1)
    (lr * 2.0).backward()
    if n > 1 or not cos:
        assert rel_l2(zi.grad.cpu(), a.grad) < 2e-4
        assert rel_l2(zj.grad.cpu(), b.grad) < 2e-4


def test_triplet_and_ce_golden(golden):
    from ted_spad_amd.losses import CrossEntropyLoss, TripletMarginLoss
    a, p, n = (_unit("trip_" + s, (8, 128)).cuda().requires_grad_() for s in "apn")
    l = TripletMarginLoss(margin=1)(a, p, n)
    l.backward()
    assert abs(l.item() - golden["triplet_value"][0]) < 1e-5
    for t, k in ((a, "a"), (p, "p"), (n, "n")):
        assert rel_l2(t.grad.cpu(), golden["triplet_grad_" + k]) < 1e-5
    lg = synth_tensor(0, "ce_logits", (8, 102), -3, 3).cuda().requires_grad_()
    lab = torch.from_numpy(golden["ce_labels"]).cuda()
    lc = CrossEntropyLoss()(lg, lab)
    lc.backward()
    assert abs(lc.item() - golden["ce_value"][0]) < 1e-5
    assert rel_l2(lg.grad.cpu(), golden["ce_grad"]) < 1e-5


def test_triplet_inactive_rows_and_margin():
    from oracle import losses_ref
    from ted_spad_amd.losses import TripletMarginLoss
    a = synth_tensor(2, "ta", (6, 128), -1, 1)
    p = a + synth_tensor(2, "tp", (6, 128), -1, 1) * 0.05
    n = a + synth_tensor(2, "tn", (6, 128), -1, 1) * 5.0   # far negatives: hinge inactive
    n[3:] = a[3:] + synth_tensor(2, "tn2", (3, 128), -1, 1) * 0.05   # near negatives: active
    A, P, Nn = (t.cuda().requires_grad_() for t in (a, p, n))
    l = TripletMarginLoss(margin=1)(A, P, Nn)
    l.backward()
    ad, pd, nd = (t.double().requires_grad_() for t in (a, p, n))
    lr = losses_ref.triplet_torch(ad, pd, nd)
    lr.backward()
    assert abs(l.item() - lr.item()) < 1e-5
    assert float(A.grad[:3].abs().max()) == 0.0
    assert rel_l2(A.grad.cpu(), ad.grad) < 1e-4 and rel_l2(Nn.grad.cpu(), nd.grad) < 1e-4 and rel_l2(P.grad.cpu(), pd.grad) < 1e-4


# ---- the kernels' edges, through the C ABI (value-only mode included), against float64 torch (tests/kernel_refs.py) --------------------------------------------
def _S():
    import ctypes as Ct
    return Ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ok(rc):
    from ted_spad_amd import _lib
    assert rc == 0, _lib.last_error()


def _ce(logits, labels, grads=True):
    from ted_spad_amd import _lib
    b, c = logits.shape
    lg, lab = logits.cuda(), labels.cuda()
    loss, ws = torch.full((2,), 1024.0, device="cuda"), torch.empty(b, device="cuda")
    dl = torch.full((b + 1, c), 1024.0, device="cuda")
    _ok(_lib.lib().tedspad_cross_entropy_fwd_bwd(lg.data_ptr(), lab.data_ptr(), loss.data_ptr(), ws.data_ptr(), dl.data_ptr() if grads else None, b, c, _S()))
    assert float(loss[1]) == 1024.0 and bool((dl[b] == 1024.0).all()) and (grads or bool((dl == 1024.0).all()))
    return float(loss[0]), dl[:b].cpu()


CE_CASES = {"plain": 3.0, "pm80": 80.0, "one_1e4_above": None}


@pytest.mark.parametrize("kind", list(CE_CASES))
@pytest.mark.parametrize("B,C", [(1, 1), (3, 63), (5, 65), (8, 1000)])
def test_cross_entropy_edges(B, C, kind):
    import kernel_refs as R
    a = CE_CASES[kind] or 3.0
    lg = synth_tensor(5, "ce%d" % C, (B, C), -a, a)
    lab = (synth_tensor(5, "cel%d" % C, (B,)) * C).long().clamp_(0, C - 1)
    if kind == "one_1e4_above":
        lg[torch.arange(B), lab] += 1e4             # the loss of these rows is 0, and finite: the max subtraction at work
    ref, dref = R.cross_entropy_ref(lg, lab)
    val, dl = _ce(lg, lab)
    assert np.isfinite(val) and abs(val - float(ref)) < 1e-5 + 1e-4 * abs(float(ref))
    assert bool(torch.isfinite(dl).all())
    if kind == "one_1e4_above" or C == 1:
        assert val == 0.0 and float(dl.abs().max()) < 1e-30 and float(dref.abs().max()) < 1e-30
    else:
        assert rel_l2(dl, dref) < 1e-4
    assert _ce(lg, lab, grads=False)[0] == val      # value-only mode: dlogits == NULL


def _triplet(a, p, n, grads=True):
    import ctypes as Ct
    from ted_spad_amd import _lib
    b, c = a.shape
    A, P, N = a.cuda(), p.cuda(), n.cuda()
    loss, ws = torch.full((2,), 1024.0, device="cuda"), torch.empty(b, device="cuda")
    g = [torch.full((b + 1, c), 1024.0, device="cuda") for _ in range(3)]
    ptrs = [t.data_ptr() if grads else None for t in g]
    _ok(_lib.lib().tedspad_triplet_fwd_bwd(A.data_ptr(), P.data_ptr(), N.data_ptr(), loss.data_ptr(), ws.data_ptr(), ptrs[0], ptrs[1], ptrs[2], b, c,
                                           Ct.c_float(1.0), Ct.c_float(1e-6), _S()))
    assert float(loss[1]) == 1024.0 and all(bool((t[b] == 1024.0).all()) for t in g) and (grads or all(bool((t == 1024.0).all()) for t in g))
    return float(loss[0]), [t[:b].cpu() for t in g]


@pytest.mark.parametrize("C", [1, 65, 130])
def test_triplet_edges(C):
    import kernel_refs as R
    a = synth_tensor(6, "ta%d" % C, (5, C), -1, 1)
    p = a + synth_tensor(6, "tp%d" % C, (5, C), -1, 1) * 0.3
    n = a + synth_tensor(6, "tn%d" % C, (5, C), -1, 1) * 0.05      # near negatives: the hinge of every row is active
    p[2] = a[2]                                       # a == p exactly: distance sqrt(C) * eps, the gradient is that of float64 torch, not 0 / NaN
    ref = R.triplet_ref(a, p, n)
    val, grads = _triplet(a, p, n)
    assert abs(val - float(ref[0])) < 1e-5
    for got, want in zip(grads, ref[1:]):
        assert bool(torch.isfinite(got).all()) and rel_l2(got, want) < 1e-4
        assert rel_l2(got[2], want[2]) < 1e-4 and float(want[2].abs().max()) > 0
    assert _triplet(a, p, n, grads=False)[0] == val   # value-only mode


def _ntxent(zi, zj, t, cos, grads=True):
    import ctypes as Ct
    from ted_spad_amd import _lib
    n, c = zi.shape
    a, b = zi.cuda(), zj.cuda()
    loss = torch.full((2,), 1024.0, device="cuda")
    g = [torch.full((n + 1, c), 1024.0, device="cuda") for _ in range(2)]
    rc = _lib.lib().tedspad_ntxent_fwd_bwd(a.data_ptr(), b.data_ptr(), loss.data_ptr(), g[0].data_ptr() if grads else None, g[1].data_ptr() if grads else None,
                                           n, c, Ct.c_float(t), int(cos), _S())
    if rc != 0:
        return rc, None
    assert float(loss[1]) == 1024.0 and all(bool((x[n] == 1024.0).all()) for x in g) and (grads or all(bool((x == 1024.0).all()) for x in g))
    return float(loss[0]), [x[:n].cpu() for x in g]


@pytest.mark.parametrize("cos", [False, True])
@pytest.mark.parametrize("N,C,scale", [(32, 256, 0.15), (32, 2, 0.3), (12, 128, None)])
def test_ntxent_limits_and_large_logits(N, C, scale, cos):
    import kernel_refs as R
    zi, zj = synth_tensor(7, "nzi%d" % C, (N, C), -1, 1), synth_tensor(7, "nzj%d" % C, (N, C), -1, 1)
    if scale is None:       # logits reach +-200: |z|^2 / T = 200 on the diagonal blocks' largest entries (cosine: the same through a temperature of 1 / 200)
        t = 0.005 if cos else 0.1
        if not cos:
            nrm = torch.cat([zi, zj]).norm(dim=1).max()
            zi, zj = zi * (20.0 ** 0.5 / nrm), zj * (20.0 ** 0.5 / nrm)
        zj[0] = -zi[1]       # a pair of opposite rows and a pair of equal ones: logits near -200 and +200 off the diagonal
        zj[2] = zi[3]
    else:
        t = 0.1
        zi, zj = zi * scale, zj * scale
    ref = R.ntxent_ref(zi, zj, t, cos)
    if scale is None:
        r = torch.cat([zj, zi]).double()
        r = torch.nn.functional.normalize(r, dim=1) if cos else r
        s = r @ r.t() / t
        s.fill_diagonal_(0)
        assert float(s.max()) > 100 and float(s.min()) < -100
    val, grads = _ntxent(zi, zj, t, cos)
    assert np.isfinite(val) and abs(val - float(ref[0])) < 1e-4 * max(1.0, abs(float(ref[0])))
    assert rel_l2(grads[0], ref[1]) < 2e-4 and rel_l2(grads[1], ref[2]) < 2e-4
    assert _ntxent(zi, zj, t, cos, grads=False)[0] == val       # value-only mode


def test_ntxent_refuses_what_it_cannot_hold():
    z = synth_tensor(7, "r", (33, 64), -1, 1)
    assert _ntxent(z, z, 0.1, False)[0] == -1                    # 2N > 64
    z = synth_tensor(7, "r", (4, 63), -1, 1)
    assert _ntxent(z, z, 0.1, False)[0] == -1                    # odd C
