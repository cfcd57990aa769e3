"""A torch restatement of MGFN's eval-mode forward (anomaly_detection_mgfn/models/mgfn.py:183-203 and the blocks of utils/utils.py:101-180),
written from the equations, for the tests (fp64) and the benchmark's eager baseline (fp32, batch 1). It reads a state_dict with the
reference's key names; `cfg` = (feature_size, depths, types, mag_ratio)."""
import torch
import torch.nn.functional as F

DIMS = (64, 128, 1024)


def _mgfn_ln(x, sd, p, eps=1e-5):
    # utils.py:108-111: divide by (biased std + eps) over the channel axis of (B, C, T)
    mean = x.mean(1, keepdim=True)
    std = ((x - mean) ** 2).mean(1, keepdim=True).sqrt()
    return (x - mean) / (std + eps) * sd[p + "g"] + sd[p + "b"]


def _conv(x, sd, p, padding=0, groups=1):
    return F.conv1d(x, sd[p + "weight"], sd.get(p + "bias"), padding=padding, groups=groups)


def _glance(x, sd, p, heads):
    # utils.py:167-180: LN -> to_qkv -> per-head softmax((q / 8) k^T) v over time, heads blocked ('b (h d) n') -> to_out
    B, C, T = x.shape
    qkv = _conv(_mgfn_ln(x, sd, p + "norm."), sd, p + "to_qkv.")
    q, k, v = (t.reshape(B, heads, 64, T).transpose(2, 3) for t in qkv.chunk(3, dim=1))
    a = torch.softmax((q * 0.125) @ k.transpose(2, 3), dim=-1) @ v
    return _conv(a.transpose(2, 3).reshape(B, heads * 64, T), sd, p + "to_out.")


def _focus(x, sd, p, heads):
    # utils.py:140-147: eval BatchNorm -> to_v -> depthwise 5-tap conv where channel ch uses filter ch % heads ('b (c h)') -> to_out
    n = p + "norm."
    x = (x - sd[n + "running_mean"].view(1, -1, 1)) / torch.sqrt(sd[n + "running_var"].view(1, -1, 1) + 1e-5) * sd[n + "weight"].view(1, -1, 1) \
        + sd[n + "bias"].view(1, -1, 1)
    v = _conv(x, sd, p + "to_v.")
    C = v.shape[1]
    w = sd[p + "rel_pos.weight"].repeat(C // heads, 1, 1)          # row ch = filter ch % heads
    b = sd[p + "rel_pos.bias"].repeat(C // heads)
    out = F.conv1d(v, w, b, padding=2, groups=C)
    return _conv(out, sd, p + "to_out.")


def forward(sd, video, cfg):
    """video (1, ncrops, T, F+1) -> dict(logits (ncrops, T), scores (ncrops, T), h (ncrops, T, 1024), mags (ncrops, T),
    crop_scores (T,), crop_mags (T,)) in the dtype of `sd` / `video`."""
    feature_size, depths, types, mag_ratio = cfg
    _, nc, T, _ = video.shape
    x = video[0].permute(0, 2, 1)                                      # (ncrops, F+1, T)
    x = _conv(x[:, :feature_size], sd, "to_tokens.", padding=1) + mag_ratio * _conv(x[:, feature_size:], sd, "to_mag.", padding=1)
    for si, (depth, t) in enumerate(zip(depths, types)):
        dim, heads = DIMS[si], DIMS[si] // 64
        for li in range(depth):
            p = "stages.%d.0.layers.%d." % (si, li)
            x = _conv(x, sd, p + "0.", padding=1) + x
            x = (_glance if t == "gb" else _focus)(x, sd, p + "1.", heads) + x
            hdn = F.gelu(_conv(_mgfn_ln(x, sd, p + "2.0."), sd, p + "2.1."))
            x = _conv(hdn, sd, p + "2.4.") + x
        if si < len(depths) - 1:
            x = _conv(_mgfn_ln(x, sd, "stages.%d.1.0." % si), sd, "stages.%d.1.1." % si)
    h = F.layer_norm(x.permute(0, 2, 1), (x.shape[1],), sd["to_logits.0.weight"], sd["to_logits.0.bias"], 1e-5)
    logits = (h @ sd["fc.weight"].t())[..., 0] + sd["fc.bias"]
    scores = torch.sigmoid(logits)
    mags = h.norm(dim=2)
    return dict(logits=logits, scores=scores, h=h, mags=mags, crop_scores=scores.mean(0), crop_mags=mags.mean(0))
