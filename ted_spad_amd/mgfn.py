"""MGFN (anomaly_detection_mgfn/models/mgfn.py) inference on the HIP path.

`MGFN` holds the reference's parameters under the reference's key names (a checkpoint of `mgfn()` loads with `load_state_dict`) in the
parameter holders of params.py, whose forward raises: all arithmetic runs in csrc/mgfn.hip, in fp32. `forward(video)` returns test.py's
5-tuple for one `(1, ncrops, T, F+1)` video; `score(videos)` scores a list of `(T_i, ncrops, F+1)` feature tensors (what
`mgfn_feed.getitem(test_mode=True)` returns) as one ragged batch. The module's own entry points are inference only (train mode raises);
training runs through `MGFNTrainStep` below: the train-mode forward with a tape, MSNSD's training branch, the cost of train.py:96-100 and
the whole backward, on the kernels of csrc/mgfn_train.hip.

Token order of a batch: video, crop, segment. Every crop sequence is its own temporal conv / attention sequence, as in the reference,
where the crops are the batch dimension of `(bs * ncrops, C, T)`."""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib
from ._lib import check
from .engine import _stream_ptr, require_cuda
from .params import BNParams, ConvParams, LinearParams, _NoForward, params_signature
from .train_step import StepDriver

DIMS = (64, 128, 1024)


def _r16(n):
    return (n + 15) // 16 * 16


class MGFNLayerNormParams(_NoForward):
    """`g`, `b` (1, dim, 1) of MGFN's LayerNorm (utils/utils.py:101-111; applied by the kernels as (x - mean) / (std + eps), Q-M1)."""

    def __init__(self, dim, eps=1e-5):
        super().__init__()
        self.eps = eps
        self.g = nn.Parameter(torch.ones(1, dim, 1))
        self.b = nn.Parameter(torch.zeros(1, dim, 1))


class LayerNormParams(_NoForward):
    """`weight`, `bias` (dim) of to_logits' nn.LayerNorm (applied by tedspad_mgfn_head as (x - mean) / sqrt(var + eps))."""

    def __init__(self, dim, eps=1e-5):
        super().__init__()
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(dim))
        self.bias = nn.Parameter(torch.zeros(dim))


def _conv(cin, cout, k, bias=True):
    return ConvParams(cin, cout, (k,), bias=bias)


def _feed_forward(dim, repe):
    # keys `0.g/b`, `1.weight/bias`, `4.weight/bias` as in utils/utils.py:114-121; slots 2 and 3 (GELU, Dropout) hold no parameters
    return nn.ModuleList([MGFNLayerNormParams(dim), _conv(dim, dim * repe, 1), _NoForward(), _NoForward(), _conv(dim * repe, dim, 1)])


class FOCUS(_NoForward):
    """utils/utils.py:124-137: eval BatchNorm -> to_v -> depthwise 5-tap rel_pos (head-interleaved, Q-M2) -> to_out."""

    def __init__(self, dim, heads):
        super().__init__()
        self.heads = heads
        self.norm = BNParams(dim)
        self.to_v = _conv(dim, 64 * heads, 1, bias=False)
        self.rel_pos = ConvParams(1, heads, (5,), bias=True)            # groups = heads: weight (heads, 1, 5)
        self.to_out = _conv(64 * heads, dim, 1)


class GLANCE(_NoForward):
    """utils/utils.py:150-165: MGFN LayerNorm -> to_qkv -> softmax attention per 64-channel head -> to_out."""

    def __init__(self, dim, heads):
        super().__init__()
        self.heads = heads
        self.norm = MGFNLayerNormParams(dim)
        self.to_qkv = _conv(dim, 3 * 64 * heads, 1, bias=False)
        self.to_out = _conv(64 * heads, dim, 1)


class Backbone(_NoForward):
    """models/mgfn.py:88-118: `layers.i` = (scc k = 3 conv, GLANCE or FOCUS, feed-forward)."""

    def __init__(self, dim, depth, heads, mgfn_type, ff_repe):
        super().__init__()
        block = {"gb": GLANCE, "fb": FOCUS}
        if mgfn_type not in block:
            raise ValueError("MGFN: block type must be 'gb' (GLANCE) or 'fb' (FOCUS), got %r" % mgfn_type)
        self.layers = nn.ModuleList(
            [nn.ModuleList([_conv(dim, dim, 3), block[mgfn_type](dim, heads), _feed_forward(dim, ff_repe)]) for _ in range(depth)])


class MGFN(nn.Module):
    """models/mgfn.py:130-182 with option.py's defaults. `state_dict()` has the reference's keys and shapes (145 tensors at the defaults)."""

    def __init__(self, feature_size=2048, depths=(3, 3, 2), mgfn_types=("gb", "fb", "fb"), mag_ratio=0.1, lokernel=5, dim_head=64, ff_repe=4,
                 dims=DIMS):
        super().__init__()
        if dim_head != 64:
            raise NotImplementedError("MGFN: the GLANCE / FOCUS blocks of the reference always use 64-channel heads (dim_head=64)")
        del lokernel                       # accepted as the reference does, which never passes it on: rel_pos always has 5 taps
        if len(depths) != len(dims) or len(mgfn_types) != len(dims):
            raise ValueError("MGFN: one depth and one block type per stage")
        self.feature_size, self.mag_ratio, self.dims = int(feature_size), float(mag_ratio), tuple(dims)
        self.depths = tuple(int(d) for d in depths)
        self.mgfn_types = tuple(t.lower() for t in mgfn_types)
        self.to_tokens = _conv(feature_size, dims[0], 3)
        self.stages = nn.ModuleList([
            nn.ModuleList([Backbone(dims[i], depth, dims[i] // 64, t, ff_repe),
                           nn.ModuleList([MGFNLayerNormParams(dims[i]), _conv(dims[i], dims[i + 1], 1)]) if i + 1 < len(dims) else None])
            for i, (depth, t) in enumerate(zip(self.depths, self.mgfn_types))])
        self.to_logits = nn.ModuleList([LayerNormParams(dims[-1])])
        self.fc = LinearParams(dims[-1], 1)
        self.to_mag = _conv(1, dims[0], 3)
        self._packed, self._packed_sig = None, None

    # ---- packed device weights (rebuilt when any parameter / buffer changes) ----------------------------------------------------------
    def packed(self):
        sig = params_signature(self)
        if self._packed is None or self._packed_sig != sig:
            require_cuda(self.to_tokens.weight, "MGFN")
            dev = self.to_tokens.weight.device

            def d(t):
                return t.detach().to(torch.float64)

            def out(t):
                return t.to(device=dev, dtype=torch.float32).contiguous()

            def ln_fold(ln, conv_w, conv_b=None):
                # conv(LN(x)) = sum_c ((x_c - mean) rs) g_c W[n, c] + (sum_c b_c W[n, c] + bias_n)
                w = d(conv_w)[:, :, 0]
                b = w @ d(ln.b).view(-1)
                if conv_b is not None:
                    b = b + d(conv_b)
                return out(w * d(ln.g).view(1, -1)), out(b)

            F = self.feature_size
            cin0 = _r16(F + 1)
            w0 = torch.zeros(self.dims[0], 3, cin0, dtype=torch.float64, device=dev)
            w0[:, :, :F] = d(self.to_tokens.weight).permute(0, 2, 1)
            w0[:, :, F] = self.mag_ratio * d(self.to_mag.weight)[:, 0, :]            # x_f + mag_ratio * to_mag(x_m), one K = 3 (F+1) GEMM
            P = {"cin0": cin0, "w0": out(w0), "b0": out(d(self.to_tokens.bias) + self.mag_ratio * d(self.to_mag.bias)), "stages": []}
            for si, (backbone, down) in enumerate(self.stages):
                dim = self.dims[si]
                blocks = []
                for scc, attn, ff in backbone.layers:
                    blk = {"scc_w": out(d(scc.weight).permute(0, 2, 1)), "scc_b": out(d(scc.bias))}
                    if isinstance(attn, GLANCE):
                        blk["type"] = "gb"
                        blk["qkv_w"], blk["qkv_b"] = ln_fold(attn.norm, attn.to_qkv.weight)
                    else:
                        blk["type"] = "fb"
                        bn = attn.norm
                        s = d(bn.weight) / torch.sqrt(d(bn.running_var) + bn.eps)
                        t = d(bn.bias) - d(bn.running_mean) * s
                        wv = d(attn.to_v.weight)[:, :, 0]
                        blk["v_w"], blk["v_b"] = out(wv * s.view(1, -1)), out(wv @ t)   # eval BatchNorm folded into to_v
                        blk["rel_w"], blk["rel_b"] = out(d(attn.rel_pos.weight)[:, 0, :]), out(d(attn.rel_pos.bias))
                    blk["heads"] = attn.heads
                    blk["out_w"], blk["out_b"] = out(d(attn.to_out.weight)[:, :, 0]), out(d(attn.to_out.bias))
                    blk["ff1_w"], blk["ff1_b"] = ln_fold(ff[0], ff[1].weight, ff[1].bias)
                    blk["ff2_w"], blk["ff2_b"] = out(d(ff[4].weight)[:, :, 0]), out(d(ff[4].bias))
                    blocks.append(blk)
                st = {"dim": dim, "blocks": blocks}
                if down is not None:
                    st["down_w"], st["down_b"] = ln_fold(down[0], down[1].weight, down[1].bias)
                P["stages"].append(st)
            ln = self.to_logits[0]
            P["ln_w"], P["ln_b"], P["ln_eps"] = out(d(ln.weight)), out(d(ln.bias)), float(ln.eps)
            P["fc_w"], P["fc_b"] = out(d(self.fc.weight).view(-1)), float(self.fc.bias.detach().float().cpu()[0])
            self._packed, self._packed_sig = P, sig
        return self._packed

    def _check_eval(self):
        if self.training:
            raise NotImplementedError("MGFN: forward / infer / score are inference entry points, call .eval() first; one training iteration "
                                      "(train-mode forward, MSNSD, the MGFN loss, backward, Adam) is MGFNTrainStep(model, batch_size).step(...)")

    # ---- one ragged batch -------------------------------------------------------------------------------------------------------------
    def infer(self, videos, keep_h=False):
        """Runs the list of `(T_i, ncrops, F+1)` videos as ONE ragged batch. Returns a dict of device tensors: `logits`, `scores`, `mags`
        per token (video, crop, segment order), `crop_scores` / `crop_mags` (the crop means, per segment, videos concatenated), `lengths`
        and, with keep_h, `h` (tokens, 1024): the to_logits LayerNorm output."""
        self._check_eval()
        P = self.packed()
        F, nc = self.feature_size, None
        dev = self.to_tokens.weight.device
        lengths = []
        for v in videos:
            require_cuda(v, "MGFN")
            if v.dim() != 3 or v.shape[2] != F + 1:
                raise ValueError("MGFN: each video must be (T, ncrops, %d), got %s" % (F + 1, tuple(v.shape)))
            if nc is None:
                nc = v.shape[1]
            if v.shape[1] != nc or v.shape[0] < 1:
                raise ValueError("MGFN: every video needs T >= 1 and the same number of crops")
            lengths.append(int(v.shape[0]))
        if not lengths:
            raise ValueError("MGFN: no videos")
        seq_len = torch.tensor(lengths, dtype=torch.int64).repeat_interleave(nc)
        seq_off = torch.zeros(len(seq_len) + 1, dtype=torch.int64)
        seq_off[1:] = torch.cumsum(seq_len, 0)
        M = int(seq_off[-1])
        starts = seq_off[:-1].repeat_interleave(seq_len)
        bounds = torch.stack([starts, starts + seq_len.repeat_interleave(seq_len)], 1).to(torch.int32).to(dev, non_blocking=True)
        seq_off_d = seq_off.to(torch.int32).to(dev, non_blocking=True)
        seg_off = torch.zeros(len(lengths) + 1, dtype=torch.int64)
        seg_off[1:] = torch.cumsum(torch.tensor(lengths, dtype=torch.int64), 0)
        seg_off_d = seg_off.to(torch.int32).to(dev, non_blocking=True)
        tmax = max(lengths)

        cin0 = P["cin0"]
        x0 = torch.empty((M, cin0), dtype=torch.float32, device=dev)
        x0[:, F + 1:].zero_()
        o = 0
        for v, T in zip(videos, lengths):
            x0[o:o + nc * T, :F + 1].view(nc, T, F + 1).copy_(v.permute(1, 0, 2))
            o += nc * T

        L, st = _lib.lib(), _stream_ptr()
        bptr = bounds.data_ptr()

        def gemm(x, w, b, N, taps=1, cin=None, stats=None, gelu=False, res=None):
            y = torch.empty((M, N), dtype=torch.float32, device=dev)
            check(L.tedspad_mgfn_gemm(x.data_ptr(), x.stride(0), bptr if taps > 1 else None, taps, cin or x.shape[1],
                                      stats.data_ptr() if stats is not None else None, w.data_ptr(), b.data_ptr(), int(gelu),
                                      res.data_ptr() if res is not None else None, res.stride(0) if res is not None else 0, y.data_ptr(), N, M, N,
                                      st), "tedspad_mgfn_gemm")
            return y

        def stats_of(x, eps=1e-5):
            s = torch.empty((M, 2), dtype=torch.float32, device=dev)
            check(L.tedspad_mgfn_ln_stats(x.data_ptr(), x.stride(0), M, x.shape[1], eps, 0, s.data_ptr(), st), "tedspad_mgfn_ln_stats")
            return s

        x = gemm(x0, P["w0"], P["b0"], self.dims[0], taps=3, cin=cin0)
        del x0
        for S in P["stages"]:
            dim = S["dim"]
            for blk in S["blocks"]:
                x = gemm(x, blk["scc_w"], blk["scc_b"], dim, taps=3, res=x)                      # x = scc(x) + x
                heads = blk["heads"]
                if blk["type"] == "gb":
                    qkv = gemm(x, blk["qkv_w"], blk["qkv_b"], 3 * 64 * heads, stats=stats_of(x))
                    a = torch.empty((M, 64 * heads), dtype=torch.float32, device=dev)
                    check(L.tedspad_mgfn_attention(qkv.data_ptr(), qkv.stride(0), seq_off_d.data_ptr(), len(seq_len), tmax, heads, a.data_ptr(),
                                                   a.stride(0), st), "tedspad_mgfn_attention")
                    del qkv
                else:
                    v = gemm(x, blk["v_w"], blk["v_b"], 64 * heads)
                    a = torch.empty_like(v)
                    check(L.tedspad_mgfn_relpos(v.data_ptr(), v.stride(0), bptr, M, v.shape[1], heads, blk["rel_w"].data_ptr(),
                                                blk["rel_b"].data_ptr(), a.data_ptr(), a.stride(0), st), "tedspad_mgfn_relpos")
                    del v
                x = gemm(a, blk["out_w"], blk["out_b"], dim, res=x)                              # x = attn(x) + x
                del a
                hid = gemm(x, blk["ff1_w"], blk["ff1_b"], blk["ff1_w"].shape[0], stats=stats_of(x), gelu=True)
                x = gemm(hid, blk["ff2_w"], blk["ff2_b"], dim, res=x)                            # x = ff(x) + x
                del hid
            if "down_w" in S:
                x = gemm(x, S["down_w"], S["down_b"], S["down_w"].shape[0], stats=stats_of(x))
        C = x.shape[1]
        logits, scores, mags = (torch.empty(M, dtype=torch.float32, device=dev) for _ in range(3))
        h = torch.empty((M, C), dtype=torch.float32, device=dev) if keep_h else None
        check(L.tedspad_mgfn_head(x.data_ptr(), x.stride(0), M, C, P["ln_w"].data_ptr(), P["ln_b"].data_ptr(), P["fc_w"].data_ptr(), P["fc_b"],
                                  P["ln_eps"], h.data_ptr() if keep_h else None, logits.data_ptr(), scores.data_ptr(), mags.data_ptr(), st),
              "tedspad_mgfn_head")
        nseg = int(seg_off[-1])
        crop_scores, crop_mags = torch.empty(nseg, dtype=torch.float32, device=dev), torch.empty(nseg, dtype=torch.float32, device=dev)
        check(L.tedspad_mgfn_crop_mean(scores.data_ptr(), crop_scores.data_ptr(), mags.data_ptr(), crop_mags.data_ptr(), seg_off_d.data_ptr(),
                                       len(lengths), tmax, nc, st), "tedspad_mgfn_crop_mean")
        return {"logits": logits, "scores": scores, "mags": mags, "crop_scores": crop_scores, "crop_mags": crop_mags, "h": h,
                "lengths": lengths, "ncrops": nc}

    def score(self, videos, max_tokens=None):
        """Per-video `(T_i,)` crop-mean scores for a list of `(T_i, ncrops, F+1)` device tensors, run as ONE ragged batch. Any T_i >= 1
        works; the reference needs T >= 3 (Q-M3). `max_tokens` (optional) bounds the device memory instead: consecutive videos then run
        in batches of at most that many tokens (a longer video alone). A video's scores are bit-identical whichever batch it runs in."""
        self._check_eval()
        videos = list(videos)
        if max_tokens is None:
            r = self.infer(videos)
            return list(torch.split(r["crop_scores"], r["lengths"]))
        out, group, ntok = [], [], 0
        for v in videos + [None]:
            n = 0 if v is None else int(v.shape[0]) * int(v.shape[1])
            if group and (v is None or ntok + n > max_tokens):
                r = self.infer(group)
                out.extend(torch.split(r["crop_scores"], r["lengths"]))
                group, ntok = [], 0
            if v is not None:
                group.append(v)
                ntok += n
        return out

    def forward(self, video):
        """test.py's call `model(input)` in eval mode: video (1, ncrops, T, F+1) -> (score_abnormal, score_normal, abn_feamagnitude,
        nor_feamagnitude, scores) as MSNSD returns them with bs = 1 (models/mgfn.py:18-86): scores (1, T, 1) crop means; the top-3
        segments by crop-mean magnitude of the to_logits output; their mean score (1, 1); their features (ncrops, 3, 1024). With bs = 1 the
        abnormal outputs are the normal ones. T < 3 raises in the top-3 selection, as in the reference (Q-M3)."""
        self._check_eval()
        if video.dim() != 4 or video.shape[0] != 1:
            raise ValueError("MGFN.forward: video must be (1, ncrops, T, F+1) as test.py feeds it (bs = 1)")
        nc, T = video.shape[1], video.shape[2]
        r = self.infer([video[0].permute(1, 0, 2)], keep_h=True)
        scores = r["crop_scores"].view(1, T, 1)
        idx = torch.topk(r["crop_mags"].view(1, T), 3, dim=1)[1]                           # MSNSD: dropout is the identity in eval
        score_abnormal = torch.mean(torch.gather(scores, 1, idx.unsqueeze(2)), dim=1)
        feat = r["h"].view(nc, T, -1)[:, idx[0], :]
        return score_abnormal, score_abnormal, feat, feat, scores


# ---- training ---------------------------------------------------------------------------------------------------------------------------
def token_gemm(x, w, b, N, bounds=None, taps=1, cin=None, res=None):
    """tedspad_mgfn_gemm on all rows of x: y = A w^T + b [+ res], A = x or its k-tap window (bounds (rows, 2) int32)."""
    R = x.shape[0]
    y = torch.empty((R, N), dtype=torch.float32, device=x.device)
    check(_lib.lib().tedspad_mgfn_gemm(x.data_ptr(), x.stride(0), bounds.data_ptr() if taps > 1 else None, taps, cin or x.shape[1], None,
                                       w.data_ptr(), b.data_ptr() if b is not None else None, 0, res.data_ptr() if res is not None else None,
                                       res.stride(0) if res is not None else 0, y.data_ptr(), N, R, N, _stream_ptr()), "tedspad_mgfn_gemm")
    return y


def transposed_window(x, bounds=None, taps=1, cin=None):
    """(taps * cin, r16(M)) image of x's k-tap window matrix, token axis last and zero padded (tedspad_mgfn_transpose)."""
    M, C = x.shape[0], cin or x.shape[1]
    out = torch.empty((taps * C, _r16(M)), dtype=torch.float32, device=x.device)
    check(_lib.lib().tedspad_mgfn_transpose(x.data_ptr(), x.stride(0), bounds.data_ptr() if taps > 1 else None, taps, M, C, out.data_ptr(),
                                            out.stride(0), _stream_ptr()), "tedspad_mgfn_transpose")
    return out


def token_wgrad(a, dy, bounds=None, taps=1, cin=None):
    """dW (N, taps, cin) = sum_m dy[m, n] A[m, t, c], A the k-tap window of a (zero outside the sequence): tedspad_mgfn_wgrad on the
    transposed images, the token axis as K. Fixed token slices added in order: no atomics, the same bits every run."""
    at, dyt = transposed_window(a, bounds, taps, cin), transposed_window(dy)
    rows, N, L = at.shape[0], dy.shape[1], _lib.lib()
    nws = int(L.tedspad_mgfn_wgrad_ws_floats(at.shape[1], rows, N))
    ws = torch.empty(nws, dtype=torch.float32, device=a.device) if nws else None
    dwt = torch.empty((rows, N), dtype=torch.float32, device=a.device)
    check(L.tedspad_mgfn_wgrad(at.data_ptr(), dyt.data_ptr(), at.shape[1], rows, N, ws.data_ptr() if nws else None, dwt.data_ptr(),
                               _stream_ptr()), "tedspad_mgfn_wgrad")
    return dwt.t().reshape(N, taps, cin or a.shape[1])


def col_reduce(a, x=None, st=None, mode=0, scale=1.0, ws=None):
    """tedspad_mgfn_col_reduce over all rows of a (M, C): (out0, out1), each (C). Modes: include/tedspad_hip.h."""
    M, C = a.shape
    L = _lib.lib()
    if ws is None:
        ws = torch.empty(int(L.tedspad_mgfn_train_ws_floats(M, C)), dtype=torch.float32, device=a.device)
    o0, o1 = torch.empty(C, dtype=torch.float32, device=a.device), torch.empty(C, dtype=torch.float32, device=a.device)
    check(L.tedspad_mgfn_col_reduce(a.data_ptr(), a.stride(0), x.data_ptr() if x is not None else None, x.stride(0) if x is not None else 0,
                                    st.data_ptr() if st is not None else None, mode, M, C, scale, ws.data_ptr(), o0.data_ptr(), o1.data_ptr(),
                                    _stream_ptr()), "tedspad_mgfn_col_reduce")
    return o0, o1


LOSS_NAMES = ("cost", "loss_smooth", "loss_sparse", "loss_cls", "loss_con", "loss_con_n", "loss_con_a", "loss_total")


class MGFNTrainStep(StepDriver):
    """One iteration of anomaly_detection_mgfn/train.py:79-106 on the HIP path, for `model` (an MGFN on the device).

    forward_backward(ninput, ainput, nlabel, alabel, masks=None): the train-mode forward (models/mgfn.py:183-203; FOCUS's BatchNorm1d on the
    batch statistics of all tokens, running statistics and num_batches_tracked updated), MSNSD's training branch (:18-86), the cost
    (train.py:96-100) and the backward; every parameter's gradient is left in `.grad`. step(...) adds the Adam update of main.py:72-73
    (weight decay added to the gradient). `masks` = (select_idx, select_idx_normal), the two MSNSD dropout outputs, each (batch_size, T) of
    0 / 1/(1-p); None draws them on the device (torch's dropout; with a `generator`, Bernoulli(1-p) / (1-p) from it).

    Top-k ties (fewer than k segments survive a mask) go to the lowest index; torch leaves them unspecified. Refused (ValueError):
    batch_size == 1, ncrops * batch_size odd, T < k."""

    def __init__(self, model, batch_size, lr=1e-3, weight_decay=5e-4, dropout_rate=0.7, k=3, generator=None):
        if not isinstance(model, MGFN):
            raise TypeError("MGFNTrainStep: model must be a ted_spad_amd.mgfn.MGFN")
        if int(batch_size) == 1:
            raise ValueError("MGFNTrainStep: batch_size == 1 makes MSNSD take its inference branch, which replaces the abnormal half by the "
                             "normal one (models/mgfn.py:38-41); train with batch_size >= 2")
        if int(batch_size) < 1 or not 1 <= int(k) <= 8 or not 0.0 <= float(dropout_rate) < 1.0:
            raise ValueError("MGFNTrainStep: needs batch_size >= 2, 1 <= k <= 8 and 0 <= dropout_rate < 1")
        require_cuda(model.to_tokens.weight, "MGFNTrainStep")
        super().__init__(loss_scale=1.0, env=False)                   # fp32 throughout: no scale, the floats are always read back
        self.model, self.n, self.k, self.p, self.generator = model, int(batch_size), int(k), float(dropout_rate), generator
        self.opt = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=weight_decay)             # main.py:72-73; `set_lr` is :91-93
        self._geo = {}

    # ---- shapes ----
    def _geometry(self, nc, T, dev):
        key = (nc, T, str(dev))
        if key not in self._geo:
            nseq = 2 * self.n * nc
            seq_off = torch.arange(nseq + 1, dtype=torch.int64) * T
            starts = seq_off[:-1].repeat_interleave(T)
            bounds = torch.stack([starts, starts + T], 1).to(torch.int32).to(dev)
            seg_off = (torch.arange(2 * self.n + 1, dtype=torch.int64) * T).to(torch.int32).to(dev)
            self._geo[key] = (bounds, seq_off.to(torch.int32).to(dev), seg_off, nseq)
        return self._geo[key]

    def _check(self, ninput, ainput, nlabel, alabel, masks):
        m, n, k = self.model, self.n, self.k
        for name, x in (("ninput", ninput), ("ainput", ainput)):
            require_cuda(x, "MGFNTrainStep")
            if x.dim() != 4 or x.shape[0] != n or x.shape[3] != m.feature_size + 1 or x.dtype != torch.float32:
                raise ValueError("MGFNTrainStep: %s must be fp32 (batch_size = %d, ncrops, T, %d), got %s %s" % (
                    name, n, m.feature_size + 1, x.dtype, tuple(x.shape)))
        if ninput.shape != ainput.shape:
            raise ValueError("MGFNTrainStep: ninput and ainput must have the same shape")
        nc, T = int(ninput.shape[1]), int(ninput.shape[2])
        if (nc * n) % 2:
            raise ValueError("MGFNTrainStep: ncrops * batch_size = %d is odd: train.py:64 splits the selected features at len / 2 into halves "
                             "of unequal length, and the reference itself fails in pairwise_distance" % (nc * n))
        if T < k:
            raise ValueError("MGFNTrainStep: T = %d segments < k = %d: MSNSD's top-k needs at least k segments" % (T, k))
        if nlabel.numel() < n or alabel.numel() < n:
            raise ValueError("MGFNTrainStep: nlabel and alabel need batch_size entries each")
        if masks is not None:
            if len(masks) != 2 or any(tuple(t.shape) != (n, T) for t in masks):
                raise ValueError("MGFNTrainStep: masks must be (select_idx, select_idx_normal), each (batch_size, T) = (%d, %d)" % (n, T))
        return nc, T

    def _masks(self, masks, T, dev):
        if masks is None:
            ones = torch.ones((2, self.n, T), dtype=torch.float32, device=dev)
            if self.generator is None:
                return torch.nn.functional.dropout(ones, self.p, True)                     # models/mgfn.py:43-44, 65-66
            return torch.bernoulli(ones * (1.0 - self.p), generator=self.generator) / (1.0 - self.p)
        return torch.stack([t.to(device=dev, dtype=torch.float32) for t in masks]).contiguous()

    # ---- one iteration ----
    def forward_backward(self, ninput, ainput, nlabel, alabel, masks=None):
        """Inputs (batch_size, ncrops, T, F+1) fp32 on the device, labels (batch_size) each. Returns a dict: the Python floats `cost`,
        `loss_smooth`, `loss_sparse`, `loss_cls`, `loss_con`, `loss_con_n`, `loss_con_a`, `loss_total`, and the device tensors
        `score_normal`, `score_abnormal` (batch_size, 1), `scores` (2 batch_size, T, 1), `idx_normal`, `idx_abnormal` (batch_size, k)."""
        model, n, k = self.model, self.n, self.k
        nc, T = self._check(ninput, ainput, nlabel, alabel, masks)
        self._begin()                                                                   # (no arena; the gradients are assigned, not accumulated)
        model.train()                                                                   # train.py:81
        dev = model.to_tokens.weight.device
        bounds, seq_off_d, seg_off_d, nseq = self._geometry(nc, T, dev)
        F, M = model.feature_size, 2 * n * nc * T
        L, st = _lib.lib(), _stream_ptr()
        bptr = bounds.data_ptr()
        f32 = dict(dtype=torch.float32, device=dev)
        ws = torch.empty(int(L.tedspad_mgfn_train_ws_floats(M, 4 * max(model.dims))), **f32)
        grads = {}

        def gemm(x, w, b, N, taps=1, cin=None, res=None):
            return token_gemm(x, w, b, N, bounds if taps > 1 else None, taps, cin, res)

        def wgrad(a, dy, taps=1, cin=None):
            return token_wgrad(a, dy, bounds if taps > 1 else None, taps, cin)

        def colsum(a, x=None, stt=None, mode=0):
            return col_reduce(a, x, stt, mode, ws=ws)

        def stats_of(x, torch_ln=0, eps=1e-5):
            s = torch.empty((M, 2), **f32)
            check(L.tedspad_mgfn_ln_stats(x.data_ptr(), x.stride(0), M, x.shape[1], eps, torch_ln, s.data_ptr(), st), "tedspad_mgfn_ln_stats")
            return s

        def ln_fwd(x, ln):
            s = stats_of(x, 0, ln.eps)
            y = torch.empty_like(x)
            check(L.tedspad_mgfn_ln_apply(x.data_ptr(), x.stride(0), s.data_ptr(), ln.g.data_ptr(), ln.b.data_ptr(), M, x.shape[1], y.data_ptr(),
                                          y.stride(0), st), "tedspad_mgfn_ln_apply")
            return y, s

        def ln_bwd(dy, x, s, g, torch_ln, eps, add=None):
            dx = torch.empty_like(x)
            check(L.tedspad_mgfn_ln_bwd(dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), s.data_ptr(), g.data_ptr(), torch_ln, eps,
                                        add.data_ptr() if add is not None else None, add.stride(0) if add is not None else 0, dx.data_ptr(),
                                        dx.stride(0), M, x.shape[1], st), "tedspad_mgfn_ln_bwd")
            return dx

        def mgfn_ln_bwd(dy, x, s, ln, add=None):
            db, dg = colsum(dy, x, s, 1)
            grads[ln.g], grads[ln.b] = dg.view_as(ln.g), db.view_as(ln.b)
            return ln_bwd(dy, x, s, ln.g, 0, ln.eps, add)

        def w1x1(conv):
            return conv.weight.detach().view(conv.weight.shape[0], conv.weight.shape[1])

        def conv1x1_bwd(conv, a, dy, res=None):
            """Gradients of a 1x1 conv y = a W^T + b: sets dW, db; returns dy W (+ res)."""
            grads[conv.weight] = wgrad(a, dy).permute(0, 2, 1).reshape(conv.weight.shape)
            if conv.bias is not None:
                grads[conv.bias] = colsum(dy)[0]
            wt = w1x1(conv).t().contiguous()
            return gemm(dy, wt, None, wt.shape[0], res=res)

        # ---- forward with a tape (models/mgfn.py:185-200) ----
        cin0 = _r16(F + 1)
        x0 = torch.zeros((M, cin0), **f32)
        x0[:, :F + 1].view(2, n * nc * T, F + 1)[0].copy_(ninput.reshape(-1, F + 1))     # train.py:85: normal videos first
        x0[:, :F + 1].view(2, n * nc * T, F + 1)[1].copy_(ainput.reshape(-1, F + 1))
        w0 = torch.zeros((model.dims[0], 3, cin0), **f32)
        w0[:, :, :F] = model.to_tokens.weight.detach().permute(0, 2, 1)
        w0[:, :, F] = model.mag_ratio * model.to_mag.weight.detach()[:, 0, :]            # x_f + mag_ratio * to_mag(x_m): one K = 3 (F+1) GEMM
        b0 = model.to_tokens.bias.detach() + model.mag_ratio * model.to_mag.bias.detach()
        x = gemm(x0, w0, b0, model.dims[0], taps=3, cin=cin0)
        tape = []
        for si, (backbone, down) in enumerate(model.stages):
            dim = model.dims[si]
            for scc, attn, ff in backbone.layers:
                t = {"x_in": x, "scc": scc, "attn": attn, "ff": ff}
                x1 = gemm(x, scc.weight.detach().permute(0, 2, 1).contiguous(), scc.bias.detach(), dim, taps=3, res=x)     # x = scc(x) + x
                heads = attn.heads
                if isinstance(attn, GLANCE):
                    xn, s1 = ln_fwd(x1, attn.norm)
                    qkv = gemm(xn, w1x1(attn.to_qkv), None, 3 * 64 * heads)
                    a = torch.empty((M, 64 * heads), **f32)
                    check(L.tedspad_mgfn_attention(qkv.data_ptr(), qkv.stride(0), seq_off_d.data_ptr(), nseq, T, heads, a.data_ptr(), a.stride(0),
                                                   st), "tedspad_mgfn_attention")
                    t.update(qkv=qkv)
                else:
                    bn = attn.norm
                    xn, s1 = torch.empty_like(x1), torch.empty(2 * dim, **f32)
                    check(L.tedspad_mgfn_bn_train_fwd(x1.data_ptr(), x1.stride(0), M, dim, bn.weight.data_ptr(), bn.bias.data_ptr(), bn.eps,
                                                      bn.momentum, ws.data_ptr(), s1.data_ptr(), bn.running_mean.data_ptr(),
                                                      bn.running_var.data_ptr(), xn.data_ptr(), xn.stride(0), st), "tedspad_mgfn_bn_train_fwd")
                    bn.num_batches_tracked.add_(1)          # also tells packed() that the running statistics changed (params_signature)
                    v = gemm(xn, w1x1(attn.to_v), None, 64 * heads)
                    a = torch.empty_like(v)
                    rw = attn.rel_pos.weight.detach().view(heads, 5)
                    check(L.tedspad_mgfn_relpos(v.data_ptr(), v.stride(0), bptr, M, v.shape[1], heads, rw.data_ptr(), attn.rel_pos.bias.data_ptr(),
                                                a.data_ptr(), a.stride(0), st), "tedspad_mgfn_relpos")
                    t.update(v=v)
                x2 = gemm(a, w1x1(attn.to_out), attn.to_out.bias.detach(), dim, res=x1)                                     # x = attn(x) + x
                xn2, s2 = ln_fwd(x2, ff[0])
                pre = gemm(xn2, w1x1(ff[1]), ff[1].bias.detach(), ff[1].weight.shape[0])
                hid = torch.empty_like(pre)
                check(L.tedspad_mgfn_gelu(pre.data_ptr(), hid.data_ptr(), pre.numel(), st), "tedspad_mgfn_gelu")
                x = gemm(hid, w1x1(ff[4]), ff[4].bias.detach(), dim, res=x2)                                                # x = ff(x) + x
                t.update(x1=x1, xn=xn, s1=s1, a=a, x2=x2, xn2=xn2, s2=s2, pre=pre, hid=hid)
                tape.append(t)
            if down is not None:
                xn, s = ln_fwd(x, down[0])
                tape.append({"down": down, "x_in": x, "xn": xn, "s": s})
                x = gemm(xn, w1x1(down[1]), down[1].bias.detach(), down[1].weight.shape[0])
        C = x.shape[1]
        ln = model.to_logits[0]
        logits, scores, mags = (torch.empty(M, **f32) for _ in range(3))
        h = torch.empty((M, C), **f32)
        fcw = model.fc.weight.detach().view(-1)
        check(L.tedspad_mgfn_head(x.data_ptr(), x.stride(0), M, C, ln.weight.data_ptr(), ln.bias.data_ptr(), fcw.data_ptr(),
                                  float(model.fc.bias.detach()[0]), ln.eps, h.data_ptr(), logits.data_ptr(), scores.data_ptr(), mags.data_ptr(),
                                  st), "tedspad_mgfn_head")
        crop_scores, crop_mags = torch.empty(2 * n * T, **f32), torch.empty(2 * n * T, **f32)
        check(L.tedspad_mgfn_crop_mean(scores.data_ptr(), crop_scores.data_ptr(), mags.data_ptr(), crop_mags.data_ptr(), seg_off_d.data_ptr(),
                                       2 * n, T, nc, st), "tedspad_mgfn_crop_mean")

        # ---- MSNSD + cost, forward and gradient (models/mgfn.py:18-86, train.py:88-100) ----
        mk = self._masks(masks, T, dev)
        labels = torch.cat((nlabel.reshape(-1)[:n], alabel.reshape(-1)[:n])).to(**f32).contiguous()        # train.py:93-94, 58
        idx = torch.empty((2 * n, k), dtype=torch.int32, device=dev)
        vid_score, dvid, losses = torch.empty(2 * n, **f32), torch.empty(2 * n, **f32), torch.empty(8, **f32)
        l1, dl1 = torch.empty((2, n * nc, k), **f32), torch.empty((2, n * nc, k), **f32)
        dcs, dscore, dh = torch.empty(2 * n * T, **f32), torch.empty(M, **f32), torch.empty((M, C), **f32)
        check(L.tedspad_mgfn_msnsd(h.data_ptr(), crop_scores.data_ptr(), crop_mags.data_ptr(), mk.data_ptr(), labels.data_ptr(), n, nc, T, C, k,
                                   idx.data_ptr(), vid_score.data_ptr(), l1.data_ptr(), losses.data_ptr(), dl1.data_ptr(), dcs.data_ptr(),
                                   dvid.data_ptr(), dscore.data_ptr(), dh.data_ptr(), st), "tedspad_mgfn_msnsd")
        self._post({name: losses[i] for i, name in enumerate(LOSS_NAMES)})

        # ---- backward ----
        dz = torch.empty(M, **f32)
        check(L.tedspad_mgfn_head_bwd(scores.data_ptr(), dscore.data_ptr(), fcw.data_ptr(), M, C, dh.data_ptr(), dz.data_ptr(), st),
              "tedspad_mgfn_head_bwd")
        dfw, dfb = colsum(h, None, dz, 4)
        grads[model.fc.weight], grads[model.fc.bias] = dfw.view_as(model.fc.weight), dfb[:1].clone()
        s_last = stats_of(x, 1, ln.eps)
        grads[ln.bias], grads[ln.weight] = colsum(dh, x, s_last, 1)
        dx = ln_bwd(dh, x, s_last, ln.weight, 1, ln.eps)
        del h, dh
        for t in reversed(tape):
            if "down" in t:
                down = t["down"]
                dxn = conv1x1_bwd(down[1], t["xn"], dx)
                dx = mgfn_ln_bwd(dxn, t["x_in"], t["s"], down[0])
                continue
            scc, attn, ff = t["scc"], t["attn"], t["ff"]
            heads = attn.heads
            # feed-forward: x = ff(x2) + x2
            dhid = conv1x1_bwd(ff[4], t["hid"], dx)
            dpre = torch.empty_like(dhid)
            check(L.tedspad_mgfn_gelu_bwd(t["pre"].data_ptr(), dhid.data_ptr(), dpre.data_ptr(), dpre.numel(), st), "tedspad_mgfn_gelu_bwd")
            del dhid
            dxn2 = conv1x1_bwd(ff[1], t["xn2"], dpre)
            del dpre
            dx2 = mgfn_ln_bwd(dxn2, t["x2"], t["s2"], ff[0], add=dx)
            # attention: x2 = attn(x1) + x1
            da = conv1x1_bwd(attn.to_out, t["a"], dx2)
            if isinstance(attn, GLANCE):
                qkv = t["qkv"]
                dqkv, lse = torch.empty_like(qkv), torch.empty((M, heads, 2), **f32)
                check(L.tedspad_mgfn_attention_bwd(qkv.data_ptr(), qkv.stride(0), t["a"].data_ptr(), t["a"].stride(0), da.data_ptr(), da.stride(0),
                                                   seq_off_d.data_ptr(), nseq, T, heads, lse.data_ptr(), dqkv.data_ptr(), dqkv.stride(0), st),
                      "tedspad_mgfn_attention_bwd")
                dxn = conv1x1_bwd(attn.to_qkv, t["xn"], dqkv)
                dx1 = mgfn_ln_bwd(dxn, t["x1"], t["s1"], attn.norm, add=dx2)
            else:
                bn, v = attn.norm, t["v"]
                dv, dw, db = torch.empty_like(v), torch.empty((heads, 5), **f32), torch.empty(heads, **f32)
                rw = attn.rel_pos.weight.detach().view(heads, 5)
                check(L.tedspad_mgfn_relpos_bwd(da.data_ptr(), da.stride(0), v.data_ptr(), v.stride(0), bptr, M, v.shape[1], heads, rw.data_ptr(),
                                                ws.data_ptr(), dv.data_ptr(), dv.stride(0), dw.data_ptr(), db.data_ptr(), st),
                      "tedspad_mgfn_relpos_bwd")
                grads[attn.rel_pos.weight], grads[attn.rel_pos.bias] = dw.view_as(attn.rel_pos.weight), db
                dxn = conv1x1_bwd(attn.to_v, t["xn"], dv)
                x1 = t["x1"]
                dx1, dgam, dbet = torch.empty_like(x1), torch.empty(x1.shape[1], **f32), torch.empty(x1.shape[1], **f32)
                check(L.tedspad_mgfn_bn_train_bwd(dxn.data_ptr(), dxn.stride(0), x1.data_ptr(), x1.stride(0), t["s1"].data_ptr(),
                                                  bn.weight.data_ptr(), M, x1.shape[1], ws.data_ptr(), dgam.data_ptr(), dbet.data_ptr(),
                                                  dx2.data_ptr(), dx2.stride(0), dx1.data_ptr(), dx1.stride(0), st), "tedspad_mgfn_bn_train_bwd")
                grads[bn.weight], grads[bn.bias] = dgam, dbet
            # scc: x1 = scc(x_in) + x_in; the data gradient is the same conv with the taps reversed
            grads[scc.weight] = wgrad(t["x_in"], dx1, taps=3).permute(0, 2, 1).contiguous()
            grads[scc.bias] = colsum(dx1)[0]
            wflip = scc.weight.detach().flip(2).permute(1, 2, 0).contiguous()            # (cin, tap, cout)
            dx = gemm(dx1, wflip, None, wflip.shape[0], taps=3, cin=dx1.shape[1], res=dx1)
            t.clear()
        dw0 = wgrad(x0, dx, taps=3, cin=cin0)
        db0 = colsum(dx)[0]
        grads[model.to_tokens.weight] = dw0[:, :, :F].permute(0, 2, 1).contiguous()
        grads[model.to_mag.weight] = (model.mag_ratio * dw0[:, :, F]).unsqueeze(1).contiguous()
        grads[model.to_tokens.bias], grads[model.to_mag.bias] = db0, model.mag_ratio * db0
        for prm in model.parameters():
            prm.grad = grads[prm].reshape(prm.shape)
        out = self._collect()
        out.update(score_normal=vid_score[:n].view(n, 1), score_abnormal=vid_score[n:].view(n, 1), scores=crop_scores.view(2 * n, T, 1),
                   idx_normal=idx[:n].long(), idx_abnormal=idx[n:].long())
        return out

    def step(self, ninput, ainput, nlabel, alabel, masks=None):
        """forward_backward, then optimizer.step() (train.py:103-106). Returns forward_backward's dict."""
        from . import train_engine as TE
        out = self.forward_backward(ninput, ainput, nlabel, alabel, masks)
        self.opt.step()
        TE.mark_updated(self.model.parameters())
        self.iteration += 1
        return out
