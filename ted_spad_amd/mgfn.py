"""MGFN (anomaly_detection_mgfn/models/mgfn.py) inference on the HIP path.

`MGFN` holds the reference's parameters under the reference's key names (a checkpoint of `mgfn()` loads with `load_state_dict`) in the
parameter holders of params.py, whose forward raises: all arithmetic runs in csrc/mgfn.hip, in fp32. `forward(video)` returns test.py's
5-tuple for one `(1, ncrops, T, F+1)` video; `score(videos)` scores a list of `(T_i, ncrops, F+1)` feature tensors (what
`mgfn_feed.getitem(test_mode=True)` returns) as one ragged batch. Training (MSNSD in train mode, the MGFN loss, every backward) is not
built: train mode raises.

Token order of a batch: video, crop, segment. Every crop sequence is its own temporal conv / attention sequence, as in the reference,
where the crops are the batch dimension of `(bs * ncrops, C, T)`."""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib
from ._lib import check
from .engine import _stream_ptr, require_cuda
from .params import BNParams, ConvParams, LinearParams, _NoForward, params_signature

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
            raise NotImplementedError("MGFN: training (MSNSD in train mode, the MGFN loss, the backward of every block) is not built on the "
                                      "HIP path; call .eval() for inference")

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
