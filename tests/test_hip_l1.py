"""-m gpu: the fused L1 loss / gradient kernels (csrc/l1_loss.hip) through the C ABI against a float64 host reference computed from the same 16-bit
output and fp32 target: gradient records and the fp32 copy bit for bit, the loss inside the bound its fixed summation order gives.

The loss bound. Every term |float(y) - x| is >= 0. A lane adds L terms in sequence (3 per pixel record in the train form, 1 per element in the flat form,
`iters` items per lane), then everything is a binary tree over P = threads * max_blocks slots (missing ones are exact zeros): the relative error of the
sum, and the bound held here, is (L + log2(P)) * 2^-24, with L and P from the kernel's own constants (tedspad_l1_block_threads / tedspad_l1_max_blocks).
To first order that also covers the rounding of each term's fp32 subtraction (a lane's first addition, to 0, is exact) and the final division (a tree
level that adds zeros is exact) -- except for the division when all max_blocks workgroups run, one 2^-24. Measured: 5e-10 ... 8e-8, bounds 1.2e-6 ... 2.3e-6."""
import ctypes as Ct
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DTS = {"f16": torch.float16, "bf16": torch.bfloat16}
MIN_NORMAL = {"f16": 2.0 ** -14, "bf16": 2.0 ** -126}
SENT = 1000.0


def L():
    from ted_spad_amd import _lib
    return _lib.lib()


def code(dt):
    from ted_spad_amd import _lib
    return {"f16": _lib.F16, "bf16": _lib.BF16}[dt]


def S():
    return Ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def ok(rc):
    assert rc == 0, L().tedspad_last_error()


def constants():
    return L().tedspad_l1_block_threads(), L().tedspad_l1_max_blocks()


def loss_bound(items, terms_per_item):
    """(relative bound of the module docstring, iters) for `items` work items of `terms_per_item` terms each."""
    threads, max_blocks = constants()
    blocks = min(-(-items // threads), max_blocks)
    iters = -(-items // (blocks * threads))
    return (terms_per_item * iters + math.log2(threads * max_blocks)) * 2.0 ** -24, iters


def g32_of(scale, numel):
    return np.float32(scale) / np.float32(numel)          # the launcher's one fp32 division


def bits(t):
    return t.contiguous().view(torch.int16)


def make_case(n, h, w, ld, dt, seed=0, device="cuda"):
    """y: (n,1,h,w,ld) buffer, the 8-channel records at channel offset ld - 8; channels 3-7 of a record hold NaN (never valid), everything outside the
    records a sentinel. x: fp32 (n,3,h,w), every 11th element an exact tie. Returns (buf, off, yv (n,3,h,w) storage-type values, x)."""
    gen = torch.Generator(device=device).manual_seed(1000 * seed + n * 131 + h * 17 + w)
    tdt = DTS[dt]
    yv = (torch.rand((n, 3, h, w), generator=gen, device=device) * 2.0 - 0.5).to(tdt)
    x = torch.rand((n, 3, h, w), generator=gen, device=device)
    tie = (torch.arange(n * 3 * h * w, device=device) % 11 == 0).view(n, 3, h, w)      # 9 %: every 11th element, the first included
    x = torch.where(tie, yv.float(), x).contiguous()
    off = ld - 8
    buf = torch.full((n, 1, h, w, ld), SENT, dtype=tdt, device=device)
    buf[..., off + 3:off + 8] = float("nan")
    buf[:, 0, :, :, off:off + 3] = yv.permute(0, 2, 3, 1)
    return buf, off, yv, x


def run_train(buf, off, x, scale, dt, want_y32=True):
    """The train form through the C ABI with guard records behind every output. Returns (loss 0-d, dl (n,h,w,8), y32 or None)."""
    n, _, h, w, ld = buf.shape
    npix = n * h * w
    tdt = DTS[dt]
    dl = torch.full((npix + 2, 8), SENT, dtype=tdt, device="cuda")
    y32 = torch.full((npix * 3 + 5,), SENT, dtype=torch.float32, device="cuda") if want_y32 else None
    ws = torch.zeros(L().tedspad_l1_ws_floats() + 1, dtype=torch.float32, device="cuda")
    ws[-1] = SENT
    loss = torch.full((2,), SENT, dtype=torch.float32, device="cuda")
    ok(L().tedspad_l1_loss_grad_cl(buf.data_ptr() + 2 * off, ld, x.data_ptr(), dl.data_ptr(), y32.data_ptr() if want_y32 else None, ws.data_ptr(),
                                   loss.data_ptr(), n, h * w, Ct.c_float(scale), code(dt), S()))
    assert torch.all(dl[npix:] == SENT) and float(ws[-1]) == SENT and float(loss[1]) == SENT, "a write behind an output"
    if want_y32:
        assert torch.all(y32[npix * 3:] == SENT)
        y32 = y32[:npix * 3].view(n, 3, h, w)
    return loss[0], dl[:npix].view(n, h, w, 8), y32


SHAPES = [(1, 1, 1), (1, 1, 63), (1, 5, 13), (2, 16, 16), (3, 17, 65)]


def _shapes():
    threads, max_blocks = 256, 1024            # checked against the library in the test (no library at collection time)
    return SHAPES + [(5, 1, (threads * max_blocks + 1) // 5)]


@pytest.mark.parametrize("dt", sorted(DTS))
@pytest.mark.parametrize("ld", [8, 16])
@pytest.mark.parametrize("shape", _shapes())
def test_train_form_vs_float64(shape, ld, dt):
    n, h, w = shape
    threads, max_blocks = constants()
    if shape not in SHAPES:
        assert n * h * w == threads * max_blocks + 1, "the last shape is one pixel more than a full grid-stride pass of the kernel"
    buf, off, yv, x = make_case(n, h, w, ld, dt)
    before = buf.clone()
    numel, scale = n * 3 * h * w, 256.0
    loss, dl, y32 = run_train(buf, off, x, scale, dt)
    assert torch.equal(bits(buf), bits(before)), "the input buffer (sentinels included) must survive"
    d = yv.double() - x.double()
    assert int((d == 0).sum()) >= max(1, int(0.05 * numel)) and (numel < 8 or (bool((d > 0).any()) and bool((d < 0).any())))
    g16 = torch.tensor(float(g32_of(scale, numel))).to(DTS[dt])                      # rounded ONCE, round to nearest even
    want = (torch.sign(d).float() * g16.float()).to(DTS[dt]).permute(0, 2, 3, 1)     # exact: 0 or +-g16
    assert torch.equal(bits(dl[..., :3]), bits(want.cuda())), "gradient channels 0-2"
    assert torch.all(bits(dl[..., 3:]) == 0), "gradient channels 3-7 are (+)0"
    assert torch.equal(y32.view(torch.int32), yv.float().view(torch.int32)), "the fp32 copy is float(y)"
    ref = float(d.abs().mean())
    rel, iters = loss_bound(n * h * w, 3)
    print("train %s ld %d %s: loss %.9g ref %.9g |err|/ref %.3e bound %.3e (iters %d)" % (shape, ld, dt, float(loss), ref, abs(float(loss) - ref) / ref, rel, iters))
    assert abs(float(loss) - ref) <= rel * ref
    loss2, dl2, none = run_train(buf, off, x, scale, dt, want_y32=False)             # y32 = NULL changes nothing else
    assert none is None and torch.equal(loss2, loss) and torch.equal(bits(dl2), bits(dl))


@pytest.mark.parametrize("numel", [1, 63, 64, 65, 4099])
@pytest.mark.parametrize("with_dy", [True, False])
def test_flat_form_vs_float64(numel, with_dy):
    gen = torch.Generator(device="cuda").manual_seed(numel)
    y = torch.rand(numel, generator=gen, device="cuda") * 2.0 - 0.5
    x = torch.rand(numel, generator=gen, device="cuda")
    x = torch.where(torch.arange(numel, device="cuda") % 11 == 0, y, x)              # ties: every 11th element, the first included
    if numel == 4099:
        y, x = y.view(1, 4099), x.view(1, 4099)                                      # any layout: only numel counts
    scale = 256.0
    dy = torch.full((numel + 3,), SENT, device="cuda") if with_dy else None
    ws = torch.zeros(L().tedspad_l1_ws_floats(), device="cuda")
    loss = torch.full((2,), SENT, device="cuda")
    ok(L().tedspad_l1_loss_flat(y.data_ptr(), x.data_ptr(), dy.data_ptr() if with_dy else None, ws.data_ptr(), loss.data_ptr(), numel, 1, numel, Ct.c_float(scale), S()))
    assert float(loss[1]) == SENT
    d = y.double() - x.double()
    ref = float(d.abs().mean())
    rel, iters = loss_bound(numel, 1)
    print("flat %d: loss %.9g ref %.9g |err|/ref %.3e bound %.3e" % (numel, float(loss[0]), ref, abs(float(loss[0]) - ref) / max(ref, 1e-300), rel))
    assert abs(float(loss[0]) - ref) <= rel * ref
    if with_dy:
        want = torch.sign(y - x) * torch.tensor(g32_of(scale, numel), device="cuda")                 # fp32
        assert torch.equal(dy[:numel].view(torch.int32), want.reshape(-1).view(torch.int32)) and torch.all(dy[numel:] == SENT)
        assert int((want == 0).sum()) >= 1


def test_module_wrappers_and_autograd():
    """losses.l1_flat / losses.L1Loss: the value is the kernel's, the gradient sign(y - x) / numel scaled by the incoming gradient."""
    from ted_spad_amd.losses import L1Loss, l1_flat
    gen = torch.Generator(device="cuda").manual_seed(3)
    y = (torch.rand((2, 3, 5, 7), generator=gen, device="cuda") - 0.3).requires_grad_()
    x = torch.rand((2, 3, 5, 7), generator=gen, device="cuda")
    loss = L1Loss()(y, x)
    assert loss.dim() == 0 and torch.equal(loss.detach(), l1_flat(y.detach(), x))
    (loss * 3.0).backward()
    want = torch.sign(y.detach() - x) * torch.tensor(g32_of(1.0, y.numel()), device="cuda") * 3.0
    assert torch.equal(y.grad, want)
    assert abs(loss.item() - float(torch.nn.functional.l1_loss(y.detach().double(), x.double()))) <= loss_bound(y.numel(), 1)[0] * loss.item()
    with pytest.raises(ValueError):
        L1Loss()(y, x[:1])
    with pytest.raises(NotImplementedError):
        L1Loss(reduction="sum")


@pytest.mark.parametrize("dt", sorted(DTS))
def test_gradient_is_bit_equal_to_the_existing_conversion(dt):
    """The train form's records == nchw_grad_to_act(sign(float(y) - x) * g32): the rounding of the path that existed before."""
    from ted_spad_amd import train_engine as TE
    from ted_spad_amd.engine import Act
    from ted_spad_amd.losses import l1_train
    n, h, w = 3, 17, 65
    buf, off, yv, x = make_case(n, h, w, 8, dt, seed=1)
    numel = n * 3 * h * w
    for scale in (256.0, 1.0, 2.0 ** 15):
        loss, dl, y32 = l1_train(Act(buf, 8, 0), x, scale, want_y32=True)
        g32 = torch.tensor(g32_of(scale, numel), device="cuda")
        old = TE.nchw_grad_to_act(torch.sign(yv.float() - x) * g32, None, (1, h, w), dtype=dt)
        assert dl.dims == old.dims and dl.ld == old.ld == 8 and torch.equal(bits(dl.buf), bits(old.buf)), scale
        assert torch.equal(y32, yv.float())


@pytest.mark.parametrize("shape", [(2, 16, 16), (3, 17, 65), (5, 1, 52429)])
def test_both_forms_give_the_same_loss_bits_on_the_same_values(shape):
    """An (n,3,h,w) fp32 pair goes through the flat form pixel by pixel -- the train form's partition and order: `evaluate` and `step` (and losses.L1Loss
    behind the autograd bridge) report the same number for the same output."""
    from ted_spad_amd.losses import l1_flat
    n, h, w = shape
    buf, off, yv, x = make_case(n, h, w, 8, "f16", seed=5)
    loss, dl, y32 = run_train(buf, off, x, 256.0, "f16")
    lf, dy = l1_flat(y32.clone(), x, grad_scale=256.0)
    assert torch.equal(lf.view(torch.int32), loss.view(torch.int32))
    want = torch.sign(y32 - x) * torch.tensor(g32_of(256.0, x.numel()), device="cuda")
    assert torch.equal(dy, want)
    plain = l1_flat(y32.reshape(-1), x.reshape(-1))                                   # index order: the same mean to rounding
    assert abs(float(plain) - float(lf)) <= 2 * loss_bound(x.numel(), 1)[0] * float(lf)


@pytest.mark.parametrize("dt", sorted(DTS))
def test_full_batch_gradient_is_a_normal_number(dt):
    """numel = 32 * 3 * 224 * 224 (plain buffers, no network) with the automatic loss scale: every non-tie gradient element is a NORMAL number of the
    storage type (with the constant scale 256 it would be an f16 subnormal, which the matrix cores flush), and the loss still meets its bound."""
    from ted_spad_amd.pretrain import auto_loss_scale
    n, h, w = 32, 224, 224
    numel = n * 3 * h * w
    assert numel == 4816896
    buf, off, yv, x = make_case(n, h, w, 8, dt, seed=2)
    scale = auto_loss_scale(numel, dt)
    loss, dl, _ = run_train(buf, off, x, scale, dt, want_y32=False)
    d = yv.double() - x.double()
    g = dl[..., :3].permute(0, 3, 1, 2).float().abs()
    nontie = d != 0
    assert torch.all(g[~nontie] == 0) and torch.all(torch.isfinite(g))
    assert float(g[nontie].min()) >= MIN_NORMAL[dt] and float(g[nontie].min()) == float(g[nontie].max())
    if dt == "f16":
        assert float(torch.tensor(float(g32_of(256.0, numel))).half()) < MIN_NORMAL["f16"]          # the trap this guards
    ref = float(d.abs().mean())
    rel, iters = loss_bound(n * h * w, 3)
    print("full batch %s: scale %g g %.4e loss %.9g ref %.9g |err|/ref %.3e bound %.3e (iters %d)" % (dt, scale, float(g[nontie].min()), float(loss), ref, abs(float(loss) - ref) / ref, rel, iters))
    assert iters > 1 and abs(float(loss) - ref) <= rel * ref


@pytest.mark.parametrize("dt", sorted(DTS))
def test_one_nan_poisons_the_loss_and_its_own_gradient_element_only(dt):
    n, h, w = 2, 16, 16
    buf, off, yv, x = make_case(n, h, w, 8, dt, seed=3)
    buf[1, 0, 7, 5, 1] = float("nan")
    loss, dl, y32 = run_train(buf, off, x, 256.0, dt)
    assert math.isnan(float(loss))
    bad = torch.isnan(dl.float())
    assert int(bad.sum()) == 1 and bool(bad[1, 7, 5, 1]) and torch.all(torch.isfinite(dl.float()[~bad]))
    assert int(torch.isnan(y32).sum()) == 1 and bool(torch.isnan(y32[1, 1, 7, 5]))
    # the flat form likewise
    y = yv.float()
    y[1, 1, 7, 5] = float("nan")
    from ted_spad_amd.losses import l1_flat
    lf, dy = l1_flat(y, x, grad_scale=1.0)
    assert math.isnan(float(lf)) and int(torch.isnan(dy).sum()) == 1 and bool(torch.isnan(dy[1, 1, 7, 5]))


def test_two_runs_are_bit_identical():
    n, h, w = 5, 1, 52429
    buf, off, yv, x = make_case(n, h, w, 8, "f16", seed=4)
    a = run_train(buf, off, x, 256.0, "f16")
    b = run_train(buf, off, x, 256.0, "f16")
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(bits(a[1]), bits(b[1])) and torch.equal(a[2], b[2])
    from ted_spad_amd.losses import l1_flat
    y = yv.float()
    la, da = l1_flat(y, x, grad_scale=8.0)
    lb, db = l1_flat(y, x, grad_scale=8.0)
    assert torch.equal(la.view(torch.int32), lb.view(torch.int32)) and torch.equal(da, db)


def test_bad_arguments_are_refused_with_a_message():
    buf, off, yv, x = make_case(1, 4, 4, 8, "f16")
    dl = torch.zeros((16, 8), dtype=torch.float16, device="cuda")
    ws = torch.zeros(L().tedspad_l1_ws_floats(), device="cuda")
    loss = torch.zeros(1, device="cuda")
    good = dict(y=buf.data_ptr(), ld=8, x=x.data_ptr(), dl=dl.data_ptr(), y32=None, ws=ws.data_ptr(), loss=loss.data_ptr(), n=1, hw=16, dtype=0)

    def train(**kw):
        a = dict(good, **kw)
        return L().tedspad_l1_loss_grad_cl(a["y"], a["ld"], a["x"], a["dl"], a["y32"], a["ws"], a["loss"], a["n"], a["hw"], Ct.c_float(256.0), a["dtype"], S())
    ok(train())
    for kw in (dict(y=None), dict(x=None), dict(dl=None), dict(ws=None), dict(loss=None), dict(n=0), dict(n=-1), dict(hw=0), dict(ld=7), dict(ld=0),
               dict(dtype=2), dict(dtype=-1), dict(dtype=7)):
        assert train(**kw) == -1, kw
        assert b"tedspad_l1_loss_grad_cl" in L().tedspad_last_error(), kw
    y = yv.float()

    def flat(yp=y.data_ptr(), xp=x.data_ptr(), wsp=ws.data_ptr(), lp=loss.data_ptr(), numel=48, c=3, hw=16):
        return L().tedspad_l1_loss_flat(yp, xp, None, wsp, lp, numel, c, hw, Ct.c_float(1.0), S())
    ok(flat())
    ok(flat(c=1, hw=48))
    for kw in (dict(yp=None), dict(xp=None), dict(wsp=None), dict(lp=None), dict(numel=0), dict(numel=-5), dict(c=0), dict(hw=0), dict(c=3, hw=5), dict(c=5, hw=16)):
        assert flat(**kw) == -1, kw
        assert b"tedspad_l1_loss_flat" in L().tedspad_last_error(), kw
    torch.cuda.synchronize()
