"""ResNet-50 I3D ("largei3d", 2048-d clip feature) on MI355X.

Mirrors the reference module `I3Res50` (aux_code/models/large_i3d.py:130-263): same
constructor arguments, same `state_dict` key names, `forward(x) -> (logits, feat)` and
`extract_features(x) -> (B, 2048, 1, 1, 1)`. The arithmetic is the HIP implicit-GEMM conv
kernel with the BatchNorm / residual / ReLU epilogue fused (include/tedspad_hip.h); the
network is just the launch sequence below.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn

from . import _lib, engine as E
from .params import BNParams, ConvParams, LinearParams, params_signature

# (planes, blocks, spatial stride, temp_conv) -- large_i3d.py:142-145
LAYER_PLAN = ((64, 3, 1, (1, 1, 1)), (128, 4, 2, (1, 0, 1, 0)), (256, 6, 2, (1, 0, 1, 0, 1, 0)), (512, 3, 2, (0, 1, 0)))


class NonLocalBlock(nn.Module):
    """Parameter layout of large_i3d.py:86-100: theta / phi / g (dim_in -> dim_inner) and out (dim_inner -> dim_out) are 1x1x1 convolutions WITH bias,
    bn a BatchNorm3d(dim_out); the max-pool in front of phi and g has no parameters. Inside I3Res50 the block is inference only (`nonlocal_forward` is its
    launch sequence there); on its own it is a differentiable module: `forward` is the reference's (large_i3d.py:102-125) on fp32 (n, c, t, h, w), in
    train() and eval(), through `autograd.nonlocal_block_forward`."""

    def __init__(self, dim_in, dim_out, dim_inner, dtype=E.DEFAULT_DTYPE):
        super().__init__()
        self.dim_in, self.dim_inner, self.dim_out = dim_in, dim_inner, dim_out
        self.compute_dtype = dtype
        self.theta = ConvParams(dim_in, dim_inner, (1, 1, 1), bias=True, init="kaiming_fan_out")
        self.phi = ConvParams(dim_in, dim_inner, (1, 1, 1), bias=True, init="kaiming_fan_out")
        self.g = ConvParams(dim_in, dim_inner, (1, 1, 1), bias=True, init="kaiming_fan_out")
        self.out = ConvParams(dim_inner, dim_out, (1, 1, 1), bias=True, init="kaiming_fan_out")
        self.bn = BNParams(dim_out)

    def forward(self, x):
        from .autograd import nonlocal_block_forward
        return nonlocal_block_forward(self, x)


def has_nonlocal(model) -> bool:
    """True if `model` (an I3Res50, or a wrapper that holds one as `.i3d`) was built with use_nl=True."""
    return any(isinstance(m, NonLocalBlock) for m in model.modules())


def refuse_nonlocal_training(model, who: str) -> None:
    """The non-local blocks run in eval() only: every training entry point calls this where it is constructed."""
    if model is not None and has_nonlocal(model):
        raise NotImplementedError("%s: this network has non-local blocks (use_nl=True) and their backward is not built -- inference only "
                                  "(extract_features / forward in eval()); train a use_nl=False network" % who)


def pack_nonlocal(P: dict, p: str, nl: NonLocalBlock, dtype, device) -> None:
    """The three weight images of a non-local block into the packed dict `P` under prefix `p`: everything but the attention core runs on the conv kernel."""
    P[p + "theta"] = E.PackedConv(nl.theta.weight, None, nl.theta.bias, dtype=dtype, device=device)             # scale 1, shift = bias
    # phi and g read the same pooled tensor: ONE GEMM with cout = 2 * dim_inner; the attention kernel takes the two halves as slices of its output
    P[p + "phi_g"] = E.PackedConv(torch.cat([nl.phi.weight.detach(), nl.g.weight.detach()]), None, torch.cat([nl.phi.bias.detach(), nl.g.bias.detach()]),
                                  dtype=dtype, device=device)
    s, b = E.fold_bn(nl.bn.weight, nl.bn.bias, nl.bn.running_mean, nl.bn.running_var, nl.bn.eps, conv_bias=nl.out.bias)
    P[p + "out"] = E.PackedConv(nl.out.weight, s, b, dtype=dtype, device=device)                                # out + bn as one scale / shift


def nonlocal_forward(P: dict, p: str, nl: NonLocalBlock, a: E.Act) -> E.Act:
    """NonLocalBlock.forward (large_i3d.py:102-125) in eval mode on the channels-last tensor `a`: five launches, the q x k score matrix is never written."""
    if a.dims[2] < 2 or a.dims[3] < 2:
        raise ValueError("%s the block's (1,2,2) max-pool needs frames of at least 2 x 2, got %s" % (p, a.dims[2:],))
    theta = P[p + "theta"](a, relu=False)                                                # :107
    mp = E.maxpool(a, (1, 2, 2), (1, 2, 2))                                              # :95,106: floor semantics, an odd last row / column is dropped
    pg = P[p + "phi_g"](mp, relu=False)                                                  # :108-109
    d = nl.dim_inner
    t = E.nl_attention(theta, pg.slice(0, d), pg.slice(d, d), float(d) ** -0.5)          # :112-119 (csrc/nonlocal.hip)
    return P[p + "out"](t, residual=a, relu=False)                                       # :121-124: out + bn + residual, no ReLU


class Bottleneck(nn.Module):
    """Parameter layout of large_i3d.py:42-84 (conv1 3x1x1|1x1x1, conv2 1x3x3, conv3 1x1x1)."""
    expansion = 4

    def __init__(self, inplanes, planes, stride, has_down, temp_conv, use_nl=False):
        super().__init__()
        self.conv1 = ConvParams(inplanes, planes, (1 + 2 * temp_conv, 1, 1), init="kaiming_fan_out")
        self.bn1 = BNParams(planes)
        self.conv2 = ConvParams(planes, planes, (1, 3, 3), init="kaiming_fan_out")
        self.bn2 = BNParams(planes)
        self.conv3 = ConvParams(planes, planes * 4, (1, 1, 1), init="kaiming_fan_out")
        self.bn3 = BNParams(planes * 4)
        self.downsample = None
        if has_down:
            self.downsample = nn.Sequential(ConvParams(inplanes, planes * 4, (1, 1, 1), init="kaiming_fan_out"),
                                            BNParams(planes * 4))
        self.stride, self.temp_conv = stride, temp_conv
        self.nl = NonLocalBlock(planes * 4, planes * 4, planes * 4 // 2) if use_nl else None      # large_i3d.py:57-58


class I3Res50(nn.Module):
    feature_dim = 2048       # width of the clip feature (large_i3d.py:262)

    def __init__(self, num_classes=400, use_nl=False, dtype=E.DEFAULT_DTYPE):
        super().__init__()
        self.use_nl = bool(use_nl)
        self.conv1 = ConvParams(3, 64, (5, 7, 7), init="kaiming_fan_out")
        self.bn1 = BNParams(64)
        inplanes = 64
        for li, (planes, blocks, stride, tc) in enumerate(LAYER_PLAN, 1):
            blks = []
            for i in range(blocks):
                # nonlocal_mod = 2 on layer2 and layer3 only, never on a layer's block 0 (large_i3d.py:141-145,166-169)
                nl = self.use_nl and li in (2, 3) and i >= 1 and i % 2 == 1
                blks.append(Bottleneck(inplanes, planes, stride if i == 0 else 1, i == 0, tc[i], use_nl=nl))
                inplanes = planes * 4
            setattr(self, "layer%d" % li, nn.Sequential(*blks))
        self.fc = LinearParams(2048, num_classes)
        self.drop_p = 0.5
        self.compute_dtype = dtype
        self._packed = None
        self._packed_sig = None

    # ---- weight packing (BN folded to fp32 scale/shift; 16-bit K-major weights) --------
    def _bn_fold(self, bn: BNParams):
        return E.fold_bn(bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)

    def packed(self):
        sig = (params_signature(self), self.compute_dtype)
        if self._packed is None or self._packed_sig != sig:
            dev = self.conv1.weight.device
            E.require_cuda(self.conv1.weight, "I3Res50")
            P = {}
            s, b = self._bn_fold(self.bn1)
            P["stem"] = E.PackedConv(self.conv1.weight, s, b, stride=(2, 2, 2), dtype=self.compute_dtype, device=dev, pair_w=3)
            P["stem_pt"] = E.StemPT(self.conv1.weight, s, b, stride=(2, 2, 2), pads=(2, 3, 3), dtype=self.compute_dtype, device=dev)
            for li in range(1, 5):
                for i, blk in enumerate(getattr(self, "layer%d" % li)):
                    self._pack_block(P, "layer%d.%d." % (li, i), li, blk, dev)
            for i in range(len(self.layer1) - 1):               # a plain layer1 tail that also emits the next block's conv1 (four-frame clips)
                p, q = "layer1.%d." % i, "layer1.%d." % (i + 1)
                w1 = self.layer1[i + 1].conv1.weight
                if (p + "tail") in P and E.BneckTailFold.supported(P[p + "tail"], w1):
                    P[p + "fold"] = E.BneckTailFold(P[p + "tail"], P[q + "conv1"], w1)
                elif (p + "tail") in P and E.BneckTailFoldDual.supported(P[p + "tail"], w1):      # layer1.0: the downsample tail does the same
                    P[p + "fold2"] = E.BneckTailFoldDual(P[p + "tail"], P[q + "conv1"], w1)
            self._packed, self._packed_sig = P, sig
        return self._packed

    def _pack_block(self, P: dict, p: str, li: int, blk: Bottleneck, dev) -> None:
        """The images of one bottleneck of layer `li` into `P` under prefix `p`. Every BatchNorm of the block is folded ONCE; the objects that need it
        share that (scale, shift) read-only (PackedConv views the vectors, BneckFrame clones them)."""
        dt = self.compute_dtype
        w1, w2, w3 = blk.conv1.weight, blk.conv2.weight, blk.conv3.weight
        wd = blk.downsample[0].weight if blk.downsample is not None else None
        s1, b1 = self._bn_fold(blk.bn1)
        s2, b2 = self._bn_fold(blk.bn2)
        s3, b3 = self._bn_fold(blk.bn3)
        P[p + "conv1"] = E.PackedConv(w1, s1, b1, dtype=dt, device=dev)
        if li >= 2 and blk.temp_conv and E.TPairConv.supported(w1):      # layers behind maxpool2: T = 2 at 16-frame clips
            P[p + "conv1_tp"] = E.TPairConv(w1, s1, b1, dtype=dt, device=dev)
        P[p + "conv2"] = E.PackedConv(w2, s2, b2, stride=(1, blk.stride, blk.stride), dtype=dt, device=dev)
        P[p + "conv3"] = E.PackedConv(w3, s3, b3, dtype=dt, device=dev)
        if wd is not None:
            sd, bd = self._bn_fold(blk.downsample[1])
            P[p + "down"] = E.PackedConv(wd, sd, bd, stride=(1, blk.stride, blk.stride), dtype=dt, device=dev)
        elif E.BneckFrame.supported(w1, w2, w3):
            # layer3's plain blocks: the whole bottleneck in one launch, a workgroup per 14 x 14 frame
            P[p + "frame"] = E.BneckFrame(w1, s1, b1, w2, s2, b2, w3, s3, b3, dtype=dt, device=dev)
        if li in (1, 2) and E.BneckTail.supported(P[p + "conv2"], w3, wd):
            if wd is None:
                P[p + "tail"] = E.BneckTail(P[p + "conv2"], w3, s3, b3)
            elif blk.stride == 1:
                P[p + "tail"] = E.BneckTail(P[p + "conv2"], w3, s3, b3, wd, sd, bd)
        if wd is not None and blk.stride == 2:      # conv3 + bn3 and the strided downsample branch as one K-concatenated GEMM
            P[p + "dual"] = E.PackedConv.fused_pair(w3, s3, b3, wd, sd, bd, dtype=dt, device=dev)
        if blk.nl is not None:
            pack_nonlocal(P, p + "nl.", blk.nl, dt, dev)

    # ---- the launch sequence ---------------------------------------------------------------
    def _check_geometry(self, frames: int, h: int, w: int, shape) -> None:
        """Refuses, before anything is launched, the clips the reference itself cannot process: its pooling layers raise on an input smaller than their
        window (large_i3d.py:138 maxpool1, :139 maxpool2, :95 the non-local blocks' pool), where the launches below would compute an empty tensor.
        frames: what maxpool1 leaves of the clip's T; (h, w): the clip's frame size."""
        h, w = E.conv_out(h, 7, 2, 3, 3), E.conv_out(w, 7, 2, 3, 3)
        if h < 3 or w < 3:
            raise ValueError("I3Res50: maxpool1's 3 x 3 window needs a conv1 output of at least 3 x 3, that is frames of at least 5 x 5 pixels; "
                             "got %s" % (shape,))
        if frames < 2:
            raise ValueError("I3Res50: maxpool2 pools over frame pairs behind maxpool1, which takes clips of at least 7 frames (two frame pairs of stem "
                             "records); got %s" % (shape,))
        h, w = E.conv_out(h, 3, 2, 0, 0), E.conv_out(w, 3, 2, 0, 0)
        for li in range(1, 5):
            layer = getattr(self, "layer%d" % li)
            if len(layer):
                s = layer[0].stride
                h, w = E.conv_out(h, 3, s, 1, 1), E.conv_out(w, 3, s, 1, 1)
            if any(blk.nl is not None for blk in layer) and (h < 2 or w < 2):
                raise ValueError("I3Res50: the non-local blocks' (1,2,2) max-pool needs frames of at least 2 x 2, layer%d's are %d x %d; got %s" % (
                    li, h, w, shape))

    def _trunk(self, x: torch.Tensor, taps=None, records: torch.Tensor = None) -> E.Act:
        """conv1 .. layer4 (large_i3d.py:229-238 == :251-260) on a (B,3,T,H,W) fp32 clip batch -- or, with `records`, on the persistent stem's own 16-bit input
        layout X[n][tp][h][2][w/2][24] (engine.StemPT.layout; preprocess.crop_resize_records writes it straight from uint8 frames). `taps`: a dict that
        receives the stage outputs; the network then runs its generic sequence, every convolution a launch of its own."""
        if self.training:
            raise NotImplementedError("a bare I3Res50 in train() mode has no caller in the reference: training goes through wrapper_i3d "
                                      "(load_ft_model('largei3d'); ted_spad_amd/autograd.py) or train_step.AnonymizerTrainStep")
        P = self.packed()
        a = self._stem(P, x, taps, records)
        if taps is not None:
            taps["maxpool1"] = a
        if self.check_saturation:
            self._sat = E.count_saturated(a, self._sat)
        pooled, h_next = False, None
        for li in range(1, 5):
            if li == 2 and not pooled:
                a = E.maxpool(a, (2, 1, 1), (2, 1, 1))                   # large_i3d.py:139
            layer = getattr(self, "layer%d" % li)
            for i, blk in enumerate(layer):
                p = "layer%d.%d." % (li, i)
                # the last layer1 block may fuse maxpool2 into its tail or its conv3
                a, h_next, fused_pool = self._bottleneck(P, p, blk, a, h_next, taps is None, li == 1 and i == len(layer) - 1)
                pooled = pooled or fused_pool
                if blk.nl is not None:
                    a = nonlocal_forward(P, p + "nl.", blk.nl, a)
                    if taps is not None:
                        taps[p + "nl"] = a
            if taps is not None:
                taps["layer%d" % li] = a
            if self.check_saturation:
                self._sat = E.count_saturated(a, self._sat)
        return a

    def _stem(self, P: dict, x: torch.Tensor, taps, records: torch.Tensor) -> E.Act:
        """conv1 + bn1 + ReLU + maxpool1 (large_i3d.py:229-232) in the form the input takes, behind the input checks: nothing is launched on an input
        that is refused."""
        if records is not None:
            E.require_cuda(records, "I3Res50")
            if not (E.STEM_PT and E.STEM_POOL) or "stem_pt" not in P:
                raise _lib.TedSpadHipError("I3Res50: the stem-record input needs the persistent stem with the fused pool (TEDSPAD_STEM_PT / TEDSPAD_STEM_POOL are off, "
                                           "or this weight shape has no persistent stem): feed the (B,3,T,H,W) clip instead")
            st = P["stem_pt"]
            if records.dim() != 6 or tuple(records.shape[3:]) != (2, records.shape[4], 24) or records.dtype != st.torch_dtype or not records.is_contiguous():
                raise ValueError("expected contiguous stem records (n, frame pairs, h, 2, w/2, 24) of %s, got %s %s" % (st.torch_dtype, tuple(records.shape), records.dtype))
            if records.shape[1] < 1 or (records.shape[2] + 1) // 2 < 3 or records.shape[4] < 3:
                raise ValueError("stem records need at least one frame pair and frames of 5 x 6 pixels for conv1 + maxpool1, got %s" % (tuple(records.shape),))
            self._check_geometry(int(records.shape[1]), int(records.shape[2]), 2 * int(records.shape[4]), tuple(records.shape))
            return st.conv_pool(records)                                 # from the records (the LDS-DMA loader of csrc/conv_stem_pt.hip)
        E.require_cuda(x, "I3Res50")
        if x.dim() != 5 or x.shape[1] != 3:
            raise ValueError("expected (B,3,T,H,W), got %s" % (tuple(x.shape),))
        if x.shape[4] % 2:
            raise ValueError("W must be even")
        self._check_geometry(E.conv_out(int(x.shape[2]), 5, 2, 2, 2) // 2, int(x.shape[3]), int(x.shape[4]), tuple(x.shape))
        st = P["stem_pt"]
        if E.STEM_PT and taps is None and st.applies(x):
            # the persistent stem kernel: the 112 x 112 x 8-frame stem tensor is never written
            if not (E.STEM_POOL and x.shape[3] >= 5 and x.shape[4] >= 6):
                return E.maxpool(st(x), (1, 3, 3), (1, 2, 2))            # the spatial half of MaxPool3d((2,3,3), 2)
            if E.STEM_CLIP and (st.VARIANT & 4) and st.direct_applies(x):
                return st.conv_pool_clip(x)                              # ... straight from the fp32 NCTHW clip: no layout pass either
            return st.conv_pool(st.layout(x))                            # ... and the spatial half: only the pooled tensor is written
        a = E.clip_to_act(x, cpad=4, dtype=self.compute_dtype)           # (B,T,H,W/2, 2px x 4ch)
        a = P["stem"](a, pads=(2, 3, P["stem"].pair_pw), pads_back=(2, 3, 1))   # the same conv in pixel-pair form, K = 5*7*4*8
        if taps is not None:
            taps["stem"] = a
        return E.maxpool(a, (2, 3, 3), (2, 2, 2))                        # large_i3d.py:138

    def _bottleneck(self, P: dict, p: str, blk: Bottleneck, a: E.Act, h_next, fused: bool, last_l1: bool):
        """One bottleneck (large_i3d.py:61-84) on the block input `a`, in the first form that applies. h_next: conv1 + bn1 + ReLU of this block where the
        previous block's fold already made it, else None. fused: the fused forms may be used (no taps). last_l1: layer1's last block, which may pool over
        frame pairs as well (maxpool2, large_i3d.py:139). Returns (block output, the next block's h_next or None, whether maxpool2 is in the output)."""
        bf = P.get(p + "frame") if fused else None
        if bf is not None and bf.applies(a):
            return bf(a), None, False                                     # conv1 -> conv2 -> conv3 + residual: only the block input and output touch HBM
        tp = P.get(p + "conv1_tp") if fused else None
        if h_next is not None:
            h = h_next                                                    # conv1 + bn1 + ReLU came out of the previous block's tail (BneckTailFold)
        elif tp is not None and tp.applies(a, (blk.temp_conv, 0, 0)):
            h = tp(a)                                                     # two frames: both outputs from ONE K = 2*cin GEMM, no products on zero padding
        else:
            h = P[p + "conv1"](a, pads=(blk.temp_conv, 0, 0))
        tail = P.get(p + "tail") if (E.BNECK_TAIL and fused) else None
        if tail is not None and tail.cmid == 128 and not E.BNECK_TAIL128:
            tail = None
        if tail is not None and tail.applies(h, (0, 1, 1)) and (not last_l1 or (E.BNECK_TAIL_POOL and not tail.dual and h.dims[1] % 2 == 0)):
            # conv2 + bn2 + ReLU + conv3 + bn3 + (residual | downsample branch) + ReLU in one launch: the 64-channel tensor between
            # the two convolutions is never written (large_i3d.py:69-84)
            fold = P.get(p + "fold") if not last_l1 else None
            fold2 = P.get(p + "fold2") if not last_l1 else None
            if tail.dual and fold2 is not None and fold2.applies(h, (0, 1, 1), a):
                return (*fold2(h, x2=a), False)                           # the downsample tail and the next block's conv1 + bn1 + ReLU (BneckTailFoldDual)
            if tail.dual:
                return tail(h, pads=(0, 1, 1), x2=a), None, False
            if fold is not None and fold.applies(h, (0, 1, 1), a):
                return (*fold(h, residual=a), False)                      # ... and the next block's conv1 (3x1x1) + bn1 + ReLU: the block output is not read for it again
            return tail(h, pads=(0, 1, 1), residual=a, pool_t2=last_l1), None, last_l1
        h = P[p + "conv2"](h, pads=(0, 1, 1))
        if blk.downsample is not None and fused and P[p + "conv3"].dual_supported(P[p + "down"], h, a):
            # layer1.0: conv3 + bn3 and the downsample branch in one launch (the 256-channel downsample tensor
            # is never written; both branches stay fp32 until the sum)
            return P[p + "conv3"].call_dual(h, P[p + "down"], a, relu=True), None, False
        if (p + "dual") in P and fused and P[p + "dual"].dual_p8_supported(h, a, (blk.stride, blk.stride)):
            # layer2.0 / 3.0 / 4.0: the same pair as ONE GEMM over [W3*s3 | Wd*sd] on the ping-pong kernel
            return P[p + "dual"].call_dual_p8(h, a, (blk.stride, blk.stride), relu=True), None, False
        res = P[p + "down"](a, relu=False) if blk.downsample is not None else a
        if last_l1 and fused and P[p + "conv3"].pool_t2_supported(h):
            # the block's tail and maxpool2 in one launch: the 256-channel tensor is only written after the temporal
            # pooling (half the bytes, no separate pool pass)
            return P[p + "conv3"].call_pool_t2(h, residual=res, relu=True), None, True
        return P[p + "conv3"](h, residual=res, relu=True), None, False    # bn3 + (+= residual) + ReLU fused

    # ---- f16 head-room, observable -----------------------------------------------------------------------------------
    check_saturation = os.environ.get("TEDSPAD_CHECK_SATURATION", "0") == "1"
    _sat = None

    def saturation_counts(self, reset: bool = True):
        """(elements at +-65504, non-finite elements) seen in the stage outputs (maxpool1, layer1..4) of every forward since the last reset, with
        `check_saturation = True` (or TEDSPAD_CHECK_SATURATION=1): the inference stores saturate instead of overflowing (csrc/common.h), silently -- a released
        checkpoint whose activations outgrow f16 shows up here (one read pass per stage output: off by default). Reads the device counter (a sync)."""
        if self._sat is None:
            return 0, 0
        v = self._sat.cpu().numpy().astype("uint32")
        if reset:
            self._sat.zero_()
        return int(v[0]), int(v[1])

    def extract_features(self, x: torch.Tensor) -> torch.Tensor:
        """large_i3d.py:249-263 -> (B, 2048, 1, 1, 1) fp32."""
        a = self._trunk(x)
        return E.global_avgpool(a).view(x.shape[0], -1, 1, 1, 1)

    def extract_features_records(self, records: torch.Tensor) -> torch.Tensor:
        """`extract_features` of clips handed over as the stem's input records (preprocess.crop_resize_records: uint8 frames -> records in one launch;
        StemPT.layout: an fp32 clip batch -> records) -> (B, 2048, 1, 1, 1) fp32. Bit-identical to extract_features of the fp32 clips the records encode."""
        a = self._trunk(None, records=records)
        return E.global_avgpool(a).view(records.shape[0], -1, 1, 1, 1)

    def forward(self, x: torch.Tensor):
        """large_i3d.py:228-246 -> (logits (B,nc), feat). `feat = x.squeeze()` drops the batch
        dim at B=1 exactly like the reference. Dropout is identity in eval."""
        from . import head
        f = E.global_avgpool(self._trunk(x))
        feat = f.view(x.shape[0], -1, 1, 1, 1).squeeze()
        logits = head.linear(f, self.fc.weight, self.fc.bias)
        return logits, feat
