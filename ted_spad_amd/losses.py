"""The three losses of the anonymizer training step on MI355X, behind the reference's own
class interfaces. Each forward is ONE fused HIP launch that also produces the input
gradients, which `backward` scales by the incoming gradient.

    NTXentLoss(device, batch_size, temperature, use_cosine_similarity)(zis, zjs)   aux_code/nt_xent_original.py:7-70
    TripletMarginLoss(margin=1.0)(anchor, positive, negative)                       train_anonymizer.py:349-350,115
    CrossEntropyLoss()(logits, labels)                                              train_anonymizer.py:347,107
    BCEWithLogitsLoss()(logits, targets)                                            privacy_training/train_privacy.py:157,52
    L1Loss()(output, inputs)                                                        fa_pretraining/train_reconstruction.py:111,46

The reference re-instantiates NTXentLoss (and rebuilds its numpy mask) every iteration
(train_anonymizer.py:82,155); here the mask is in-kernel.
"""
import ctypes as C

import torch
import torch.nn as nn

from . import _lib, head
from .engine import _stream_ptr, require_cuda


def _f32(t):
    return t.contiguous().float()


class _NTXentFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, zis, zjs, temperature, cosine):
        require_cuda(zis, "NTXentLoss")
        zi, zj = _f32(zis), _f32(zjs)
        n, c = zi.shape
        loss = torch.empty(1, dtype=torch.float32, device=zi.device)
        dzi, dzj = torch.empty_like(zi), torch.empty_like(zj)
        _lib.check(_lib.lib().tedspad_ntxent_fwd_bwd(zi.data_ptr(), zj.data_ptr(), loss.data_ptr(), dzi.data_ptr(), dzj.data_ptr(),
                                                     n, c, C.c_float(temperature), int(cosine), _stream_ptr()), "tedspad_ntxent_fwd_bwd")
        ctx.save_for_backward(dzi, dzj)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        dzi, dzj = ctx.saved_tensors
        return dzi * g, dzj * g, None, None


class NTXentLoss(nn.Module):
    def __init__(self, device, batch_size, temperature, use_cosine_similarity):
        super().__init__()
        self.batch_size, self.temperature, self.device = batch_size, temperature, device
        self.use_cosine_similarity = bool(use_cosine_similarity)

    def forward(self, zis, zjs):
        if zis.shape[0] != self.batch_size or zjs.shape != zis.shape:
            raise ValueError("NTXentLoss built for batch_size=%d got %s / %s" % (self.batch_size, tuple(zis.shape), tuple(zjs.shape)))
        return _NTXentFn.apply(zis, zjs, float(self.temperature), self.use_cosine_similarity)


class _TripletFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, p, n, margin, eps):
        require_cuda(a, "TripletMarginLoss")
        a, p, n = _f32(a), _f32(p), _f32(n)
        b, c = a.shape
        loss = torch.empty(1, dtype=torch.float32, device=a.device)
        ws = torch.empty(b, dtype=torch.float32, device=a.device)
        da, dp, dn = torch.empty_like(a), torch.empty_like(a), torch.empty_like(a)
        _lib.check(_lib.lib().tedspad_triplet_fwd_bwd(a.data_ptr(), p.data_ptr(), n.data_ptr(), loss.data_ptr(), ws.data_ptr(),
                                                      da.data_ptr(), dp.data_ptr(), dn.data_ptr(), b, c, C.c_float(margin),
                                                      C.c_float(eps), _stream_ptr()), "tedspad_triplet_fwd_bwd")
        ctx.save_for_backward(da, dp, dn)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        da, dp, dn = ctx.saved_tensors
        return da * g, dp * g, dn * g, None, None


class TripletMarginLoss(nn.Module):
    def __init__(self, margin=1.0, p=2.0, eps=1e-6):
        super().__init__()
        if p != 2.0:
            raise NotImplementedError("only p=2 (the reference's default)")
        self.margin, self.eps = margin, eps

    def forward(self, anchor, positive, negative):
        return _TripletFn.apply(anchor, positive, negative, float(self.margin), float(self.eps))


class _CEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels):
        require_cuda(logits, "CrossEntropyLoss")
        lg = _f32(logits)
        lab = labels.contiguous().long()
        b, c = lg.shape
        loss = torch.empty(1, dtype=torch.float32, device=lg.device)
        ws = torch.empty(b, dtype=torch.float32, device=lg.device)
        dl = torch.empty_like(lg)
        _lib.check(_lib.lib().tedspad_cross_entropy_fwd_bwd(lg.data_ptr(), lab.data_ptr(), loss.data_ptr(), ws.data_ptr(),
                                                            dl.data_ptr(), b, c, _stream_ptr()), "tedspad_cross_entropy_fwd_bwd")
        ctx.save_for_backward(dl)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (dl,) = ctx.saved_tensors
        return dl * g, None


class CrossEntropyLoss(nn.Module):
    def forward(self, logits, labels):
        return _CEFn.apply(logits, labels)


class _BCEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target):
        lg = _f32(logits)
        _, loss, dl, _, _ = head.bce_head(lg.reshape(-1, lg.shape[-1]), target.reshape(-1, lg.shape[-1]))
        ctx.save_for_backward(dl)
        ctx.shape = logits.shape
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (dl,) = ctx.saved_tensors
        return (dl * g).view(ctx.shape), None


def _l1_ws(device):
    return torch.empty(_lib.lib().tedspad_l1_ws_floats(), dtype=torch.float32, device=device)


def l1_flat(y, x, grad_scale=None):
    """mean |y - x| of two fp32 tensors of one shape (any layout, made contiguous) as a 0-d fp32 device tensor, in a fixed summation order
    (tedspad_l1_loss_flat). With grad_scale also dy = sign(y - x) * fp32(grad_scale / numel), shaped like y: returns (loss, dy).
    An (n,3,h,w) pair -- images -- is added pixel by pixel, the order of `l1_train`: on the same values the two give the same bits."""
    require_cuda(y, "L1Loss")
    if y.shape != x.shape or y.numel() == 0:
        raise ValueError("L1Loss: input %s and target %s must have the same non-empty shape" % (tuple(y.shape), tuple(x.shape)))
    yc, xc = _f32(y), _f32(x)
    c, hw = (3, yc.shape[2] * yc.shape[3]) if yc.dim() == 4 and yc.shape[1] == 3 else (1, yc.numel())
    loss = torch.empty(1, dtype=torch.float32, device=yc.device)
    dy = torch.empty_like(yc) if grad_scale is not None else None
    _lib.check(_lib.lib().tedspad_l1_loss_flat(yc.data_ptr(), xc.data_ptr(), dy.data_ptr() if dy is not None else None, _l1_ws(yc.device).data_ptr(),
                                               loss.data_ptr(), yc.numel(), c, hw, C.c_float(grad_scale or 0.0), _stream_ptr()), "tedspad_l1_loss_flat")
    return loss[0] if dy is None else (loss[0], dy)


def l1_train(y, x, grad_scale, want_y32=False):
    """The train form (tedspad_l1_loss_grad_cl): y = the 16-bit channels-last Act of a 3-channel output (8-channel records, t == 1), x = the fp32
    (n,3,h,w) target. Returns (loss 0-d fp32, dl: the (n,1,h,w,8) gradient Act with sign(float(y) - x) * grad_scale / numel in channels 0-2,
    y32: the fp32 NCHW copy of y or None)."""
    from .engine import Act, dtype_code
    n, t, h, w = y.dims
    if t != 1 or tuple(x.shape) != (n, 3, h, w) or x.dtype != torch.float32 or not x.is_cuda:
        raise ValueError("l1_train: y is (%d,%d,%d,%d,8) channels-last, the target must be fp32 cuda (%d,3,%d,%d), got %s %s"
                         % (n, t, h, w, n, h, w, tuple(x.shape), x.dtype))
    xc = x.contiguous()
    dl = Act.empty(n, 1, h, w, 8, y.buf.dtype, y.buf.device)
    loss = torch.empty(1, dtype=torch.float32, device=y.buf.device)
    y32 = torch.empty_like(xc) if want_y32 else None
    code = dtype_code(y.buf)
    _lib.check(_lib.lib().tedspad_l1_loss_grad_cl(y.ptr, y.ld, xc.data_ptr(), dl.ptr, y32.data_ptr() if want_y32 else None, _l1_ws(xc.device).data_ptr(),
                                                  loss.data_ptr(), n, h * w, C.c_float(grad_scale), code, _stream_ptr()), "tedspad_l1_loss_grad_cl")
    return loss[0], dl, y32


class _L1Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, target):
        loss, dy = l1_flat(y, target, grad_scale=1.0)
        ctx.save_for_backward(dy)
        ctx.shape = y.shape
        return loss

    @staticmethod
    def backward(ctx, g):
        (dy,) = ctx.saved_tensors
        return (dy * g).view(ctx.shape), None


class L1Loss(nn.Module):
    """nn.L1Loss() with its default mean reduction (fa_pretraining/train_reconstruction.py:111,46): value and d(loss)/d(input) = sign(input - target) / numel
    from the flat form of the L1 kernel. No gradient w.r.t. the target (the script's target is its data)."""

    def __init__(self, size_average=None, reduce=None, reduction="mean"):
        super().__init__()
        if size_average is not None or reduce is not None or reduction != "mean":
            raise NotImplementedError("L1Loss: only the default mean reduction is built; train_reconstruction.py:111 uses nothing else")

    def forward(self, input, target):
        return _L1Fn.apply(input, target)


class BCEWithLogitsLoss(nn.Module):
    """nn.BCEWithLogitsLoss() with its defaults (mean reduction, no weight / pos_weight): the value and d(loss)/d(logits) in one launch
    (the logits mode of tedspad_bce_head_fwd_bwd). Rows of at most 64 logits, at most 128 rows; no gradient w.r.t. the target."""

    def __init__(self, weight=None, size_average=None, reduce=None, reduction="mean", pos_weight=None):
        super().__init__()
        if weight is not None or pos_weight is not None or size_average is not None or reduce is not None or reduction != "mean":
            raise NotImplementedError("BCEWithLogitsLoss: only the default form (mean reduction, no weight / pos_weight) is built; "
                                      "train_privacy.py:157 uses nothing else")

    def forward(self, logits, target):
        if logits.shape != target.shape or logits.dim() == 0:
            raise ValueError("BCEWithLogitsLoss: logits %s and target %s must have the same (non-scalar) shape" % (tuple(logits.shape), tuple(target.shape)))
        return _BCEFn.apply(logits, target)
