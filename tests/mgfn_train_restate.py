"""A differentiable torch restatement of one MGFN training iteration (anomaly_detection_mgfn/train.py:79-100 with models/mgfn.py:18-86 and
183-203 under model.train()), written from the equations, for the tests (fp64) and the training benchmark's torch baseline (fp32). It is
functional over a state_dict with the reference's key names; `cfg` = (feature_size, depths, types, mag_ratio). MSNSD's two dropout outputs
are supplied (`masks` = (select_idx, select_idx_normal), each (n, T) of 0 / 1/(1-p)), so nothing here is random.

Differences from tests/mgfn_restate.py (eval): FOCUS's BatchNorm1d uses the batch statistics of all tokens and the new running statistics
are returned; MSNSD runs its training branch; top-k ties go to the lowest index (torch leaves them unspecified)."""
import torch
import torch.nn.functional as F

from mgfn_restate import DIMS, _conv, _glance, _mgfn_ln


def topk_lowest_index(x, k):
    """Indices of the k largest per row, descending, ties to the lowest index."""
    return torch.sort(x, dim=1, descending=True, stable=True)[1][:, :k]


def _focus_train(x, sd, p, heads, bn_out):
    # utils.py:140-147 in train mode: nn.BatchNorm1d over (batch, time) of (B, C, T), biased variance for the output, unbiased for running_var
    n = p + "norm."
    mean = x.mean((0, 2))
    var = ((x - mean.view(1, -1, 1)) ** 2).mean((0, 2))
    cnt = x.shape[0] * x.shape[2]
    if bn_out is not None:
        with torch.no_grad():
            bn_out[n + "running_mean"] = 0.9 * sd[n + "running_mean"] + 0.1 * mean
            bn_out[n + "running_var"] = 0.9 * sd[n + "running_var"] + 0.1 * var * cnt / max(cnt - 1, 1)
            bn_out[n + "num_batches_tracked"] = sd[n + "num_batches_tracked"] + 1
    x = (x - mean.view(1, -1, 1)) / torch.sqrt(var.view(1, -1, 1) + 1e-5) * sd[n + "weight"].view(1, -1, 1) + sd[n + "bias"].view(1, -1, 1)
    v = _conv(x, sd, p + "to_v.")
    C = v.shape[1]
    w = sd[p + "rel_pos.weight"].repeat(C // heads, 1, 1)          # row ch = filter ch % heads
    b = sd[p + "rel_pos.bias"].repeat(C // heads)
    return _conv(F.conv1d(v, w, b, padding=2, groups=C), sd, p + "to_out.")


def backbone_train(sd, video, cfg, bn_out=None):
    """video (bs, ncrops, T, F+1) -> h (bs * ncrops, T, 1024) the to_logits output, scores (bs * ncrops, T) (models/mgfn.py:185-200)."""
    feature_size, depths, types, mag_ratio = cfg
    bs, nc, T, c = video.shape
    x = video.reshape(bs * nc, T, c).permute(0, 2, 1)
    x = _conv(x[:, :feature_size], sd, "to_tokens.", padding=1) + mag_ratio * _conv(x[:, feature_size:], sd, "to_mag.", padding=1)
    for si, (depth, t) in enumerate(zip(depths, types)):
        heads = DIMS[si] // 64
        for li in range(depth):
            p = "stages.%d.0.layers.%d." % (si, li)
            x = _conv(x, sd, p + "0.", padding=1) + x
            x = (_glance(x, sd, p + "1.", heads) if t == "gb" else _focus_train(x, sd, p + "1.", heads, bn_out)) + x
            hdn = F.gelu(_conv(_mgfn_ln(x, sd, p + "2.0."), sd, p + "2.1."))
            x = _conv(hdn, sd, p + "2.4.") + x
        if si < len(depths) - 1:
            x = _conv(_mgfn_ln(x, sd, "stages.%d.1.0." % si), sd, "stages.%d.1.1." % si)
    h = F.layer_norm(x.permute(0, 2, 1), (x.shape[1],), sd["to_logits.0.weight"], sd["to_logits.0.bias"], 1e-5)
    scores = torch.sigmoid((h @ sd["fc.weight"].t())[..., 0] + sd["fc.bias"])
    return h, scores


def check_shapes(n, ncrops, T, k):
    """The cases MGFNTrainStep refuses."""
    if n == 1:
        raise ValueError("MGFN training: batch_size == 1 makes MSNSD take its inference branch (models/mgfn.py:38-41)")
    if (ncrops * n) % 2:
        raise ValueError("MGFN training: ncrops * batch_size must be even (train.py:64 halves the selected features)")
    if T < k:
        raise ValueError("MGFN training: T = %d segments < k = %d" % (T, k))


def msnsd_cost(h, scores, n, ncrops, masks, nlabel, alabel, k=3):
    """MSNSD's training branch (models/mgfn.py:18-86) and the cost of train.py:88-100 on h (2n * ncrops, T, C), scores (2n * ncrops, T)."""
    T, C = h.shape[1], h.shape[2]
    check_shapes(n, ncrops, T, k)
    crop_scores = scores.view(2 * n, ncrops, T).mean(1)                                     # :23
    mags = h.norm(p=2, dim=2).view(2 * n, ncrops, T).mean(1)                                # :32-33
    idx_abn = topk_lowest_index(mags[n:].detach() * masks[0], k)                            # :47-48
    idx_nor = topk_lowest_index(mags[:n].detach() * masks[1], k)                            # :67-68

    def select(feat, idx):                                                                  # :51-58: crop-major rows, crop * n + video
        feat = feat.view(n, ncrops, T, C).permute(1, 0, 2, 3)
        return torch.gather(feat, 2, idx.view(1, n, k, 1).expand(ncrops, n, k, C)).reshape(ncrops * n, k, C)

    abn_feat, nor_feat = select(h[n * ncrops:], idx_abn), select(h[:n * ncrops], idx_nor)
    score_abnormal = torch.gather(crop_scores[n:], 1, idx_abn).mean(1, keepdim=True)        # :60-62
    score_normal = torch.gather(crop_scores[:n], 1, idx_nor).mean(1, keepdim=True)          # :80-81

    def contrastive(o1, o2, label, margin=200.0):                                           # train.py:28-32
        d = F.pairwise_distance(o1, o2, keepdim=True)
        return torch.mean((1 - label) * d ** 2 + label * torch.clamp(margin - d, min=0.0) ** 2)

    score = torch.cat((score_normal, score_abnormal), 0).squeeze(1)
    label = torch.cat((nlabel, alabel), 0).to(score.dtype)
    sep = (ncrops * n) // 2
    la, ln_ = abn_feat.norm(p=1, dim=2), nor_feat.norm(p=1, dim=2)
    loss_cls = F.binary_cross_entropy(score, label)                                         # :66
    loss_con = contrastive(la, ln_, 1)                                                      # :67
    loss_con_n = contrastive(ln_[sep:], ln_[:sep], 0)                                       # :69
    loss_con_a = contrastive(la[sep:], la[:sep], 0)                                         # :72
    loss_total = loss_cls + (0.001 * loss_con + loss_con_a + loss_con_n) * 0.001            # :74
    abn = crop_scores[n:].reshape(-1)                                                       # :88-91 (the flattened abnormal half)
    loss_sparse = 8e-3 * torch.norm(abn, dim=0)                                             # :8-10, :97
    nxt = torch.cat((abn[1:], abn[-1:]))
    loss_smooth = 8e-4 * torch.sum((nxt - abn) ** 2)                                        # :13-20, :98
    cost = loss_total + loss_smooth + loss_sparse                                           # :100
    return dict(cost=cost, loss_smooth=loss_smooth, loss_sparse=loss_sparse, loss_cls=loss_cls, loss_con=loss_con, loss_con_n=loss_con_n,
                loss_con_a=loss_con_a, loss_total=loss_total, score_normal=score_normal, score_abnormal=score_abnormal,
                scores=crop_scores.unsqueeze(2), idx_normal=idx_nor, idx_abnormal=idx_abn, nor_feamagnitude=nor_feat,
                abn_feamagnitude=abn_feat, crop_mags=mags)


def train_cost(sd, ninput, ainput, nlabel, alabel, masks, cfg, k=3, bn_out=None):
    """One iteration's forward: inputs (n, ncrops, T, F+1) each; returns msnsd_cost's dict. `bn_out` (a dict) receives the BatchNorm
    buffers as the train-mode forward leaves them."""
    video = torch.cat((ninput, ainput), 0)                                                  # train.py:85
    n, ncrops = ninput.shape[0], ninput.shape[1]
    check_shapes(n, ncrops, video.shape[2], k)
    h, scores = backbone_train(sd, video, cfg, bn_out)
    return msnsd_cost(h, scores, n, ncrops, masks, nlabel, alabel, k)


def grads(sd, ninput, ainput, nlabel, alabel, masks, cfg, k=3):
    """(result dict, {parameter key: gradient}, bn_out) of one iteration in the dtype of `sd`."""
    buffers = ("running_mean", "running_var", "num_batches_tracked")
    leaf = {key: (v.clone().requires_grad_(True) if not key.endswith(buffers) else v) for key, v in sd.items()}
    bn_out = {}
    r = train_cost(leaf, ninput, ainput, nlabel, alabel, masks, cfg, k, bn_out)
    r["cost"].backward()
    g = {key: v.grad for key, v in leaf.items() if v.requires_grad}
    return {key: (v.detach() if torch.is_tensor(v) else v) for key, v in r.items()}, g, bn_out
