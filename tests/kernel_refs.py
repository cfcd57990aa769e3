"""float64 references of the memory-bound training kernels (csrc/train_ops.hip, the idx / backward half of csrc/pool_layout.hip, csrc/head.hip, csrc/loss.hip)
and the two value generators their tests use. A plain helper module: tests/test_kernel_refs.py checks every reference here against float64 torch (autograd) on
the CPU, the -m gpu op tests (test_hip_train_kernels.py, test_hip_head_ops.py, test_hip_losses.py) compare the kernels with them.

Activations are channels-last: (pixels, C) for the BatchNorm kernels, (n, t, h, w, c) for the pools, (n, h, w, c) for the resizes. Everything returned is a
float64 torch tensor (indices: uint8 / int64)."""
import numpy as np
import torch
import torch.nn.functional as F

from ted_spad_amd.synth import synth_tensor

D = torch.float64
ULP = {"f16": 2.0 ** -10, "bf16": 2.0 ** -7}          # the suite's per-element relative step of a stored 16-bit value
TINY = {"f16": 2.0 ** -24, "bf16": 2.0 ** -133}       # smallest subnormal of the type
TDT = {"f16": torch.float16, "bf16": torch.bfloat16}
F32_EPS = 2.0 ** -24


# ---- value generators ------------------------------------------------------------------------------------------------------------------------------
def tie_values(seed, name, shape):
    """ReLU-like data: u in [0, 1) -> {0, 0, 0.5, 1}[floor(4 u)]: half the values exactly 0, ties everywhere, exact in f16 and bf16."""
    u = synth_tensor(seed, name, shape).to(D)
    return torch.tensor([0.0, 0.0, 0.5, 1.0], dtype=D)[torch.floor(4.0 * u).long().clamp_(0, 3)]


def dyadic(seed, name, shape, bits=4):
    """Multiples of 2^-bits in [-2, 2]: sums of a few thousand of them are exact in fp32, and in f16 / bf16 after one rounding."""
    u = synth_tensor(seed, name, shape).to(D)
    steps = 4 * (1 << bits) + 1
    return torch.floor(u * steps).clamp_(0, steps - 1) / (1 << bits) - 2.0


# ---- train-mode BatchNorm: the kernels' own definition ------------------------------------------------------------------------------------------------
def bn_train_ref(z, sum, sumsq, count, gamma, beta, eps, res, relu, momentum=0.1, running_mean=None, running_var=None):
    """y = act((z - mean) * gamma * invstd + beta (+ res)) from the batch sums the kernel is handed: mean = sum / count, biased var = max(sumsq / count -
    mean^2, 0). z (pixels, C); res (pixels, C) or None. Returns a dict: y, mean, invstd, scale, shift, running_mean / running_var (the momentum update
    with the unbiased variance, None without running statistics) and M = |z * scale| + |shift| + |res|, the magnitude a per-element bound scales with."""
    z, sum, sumsq, gamma, beta = (torch.as_tensor(t).to(D) for t in (z, sum, sumsq, gamma, beta))
    mean = sum / count
    var = (sumsq / count - mean * mean).clamp_min(0.0)
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma * invstd
    shift = beta - mean * scale
    v = z * scale + shift
    M = (z * scale).abs() + shift.abs()
    if res is not None:
        v = v + res.to(D)
        M = M + res.to(D).abs()
    out = {"y": v.clamp_min(0.0) if relu else v, "mean": mean, "invstd": invstd, "scale": scale, "shift": shift, "M": M,
           "running_mean": None, "running_var": None}
    if running_mean is not None:
        unb = var * count / (count - 1.0) if count > 1 else var
        out["running_mean"] = (1.0 - momentum) * running_mean.to(D) + momentum * mean
        out["running_var"] = (1.0 - momentum) * running_var.to(D) + momentum * unb
    return out


def bn_bwd_ref(dy, y_or_None, z, mean, invstd, gamma, beta, relu, sums=None):
    """Backward of the above for one statistics group. g = dy * mask, mask = y > 0 (from the stored output), or, with y None, the forward's own
    z * s + b > 0 (s = gamma * invstd, b = beta - mean * s); no mask without relu. Returns a dict: g (= dres), sum_g, sum_gx (the two channel sums),
    dz = ks * g + A * z + B with ks = gamma * invstd, A = -ks * invstd * sum_gx / M, B = -ks * sum_g / M - A * mean (M = pixels; `sums` = (sum_g, sum_gx)
    replaces the exact sums: what tedspad_bn_bwd_apply is handed), sum_dz, abs_gx = sum |g * xhat|, and ks / A / B for the bounds."""
    dy, z, mean, invstd, gamma, beta = (torch.as_tensor(t).to(D) for t in (dy, z, mean, invstd, gamma, beta))
    ks = gamma * invstd
    if not relu:
        mask = torch.ones_like(dy)
    elif y_or_None is not None:
        mask = (y_or_None.to(D) > 0).to(D)
    else:
        mask = ((z * ks + (beta - mean * ks)) > 0).to(D)
    g = dy * mask
    xhat = (z - mean) * invstd
    sum_g, sum_gx = g.sum(0), (g * xhat).sum(0)
    s0, s1 = (sum_g, sum_gx) if sums is None else (sums[0].to(D), sums[1].to(D))
    npx = z.shape[0]
    A = -ks * invstd * s1 / npx
    B = -ks * s0 / npx - A * mean
    dz = ks * g + A * z + B
    return {"g": g, "dres": g, "sum_g": sum_g, "sum_gx": sum_gx, "dz": dz, "sum_dz": dz.sum(0), "abs_gx": (g * xhat).abs().sum(0), "ks": ks, "A": A, "B": B}


# ---- max-pool with window-local first-maximum indices, explicit loops ---------------------------------------------------------------------------------
def pool_out(size, k, s, p):
    return (size + 2 * p - k) // s + 1


def maxpool_fwd_ref(x, k, s, p):
    """x (n, t, h, w, c); kernel k, stride s, FRONT padding p (taps outside the input are skipped: nn.MaxPool3d). torch's scan: start at the first tap
    inside the input, then a strictly larger value -- or any NaN -- takes over. Returns y (n, to, ho, wo, c) and the window-local index
    (dt * kh + dh) * kw + dw of the element taken, uint8."""
    x = x.to(D).numpy()
    n, T, H, W, c = x.shape
    To, Ho, Wo = (pool_out(a, b, d, e) for a, b, d, e in zip((T, H, W), k, s, p))
    y = np.zeros((n, To, Ho, Wo, c))
    idx = np.zeros((n, To, Ho, Wo, c), np.uint8)
    for to in range(To):
        for ho in range(Ho):
            for wo in range(Wo):
                m, am, first = np.full((n, c), -np.inf), np.zeros((n, c), np.uint8), True
                for dt in range(k[0]):
                    for dh in range(k[1]):
                        for dw in range(k[2]):
                            it, ih, iw = to * s[0] - p[0] + dt, ho * s[1] - p[1] + dh, wo * s[2] - p[2] + dw
                            if not (0 <= it < T and 0 <= ih < H and 0 <= iw < W):
                                continue
                            v = x[:, it, ih, iw, :]
                            take = np.ones((n, c), bool) if first else ((v > m) | np.isnan(v))
                            m = np.where(take, v, m)
                            am = np.where(take, np.uint8((dt * k[1] + dh) * k[2] + dw), am)
                            first = False
                y[:, to, ho, wo, :], idx[:, to, ho, wo, :] = m, am
    return torch.from_numpy(y), torch.from_numpy(idx)


def maxpool_bwd_ref(x, idx, dy, k, s, p, add=None, relu_mask=False):
    """dx[i] = (add[i]) + sum over the windows o containing i of dy[o] * [idx[o] == i's window-local index]; relu_mask: zero where x <= 0."""
    x, dy, idx = x.to(D).numpy(), dy.to(D).numpy(), idx.numpy()
    n, T, H, W, c = x.shape
    _, To, Ho, Wo, _ = dy.shape
    dx = np.zeros_like(x) if add is None else add.to(D).numpy().copy()
    for to in range(To):
        for ho in range(Ho):
            for wo in range(Wo):
                for dt in range(k[0]):
                    for dh in range(k[1]):
                        for dw in range(k[2]):
                            it, ih, iw = to * s[0] - p[0] + dt, ho * s[1] - p[1] + dh, wo * s[2] - p[2] + dw
                            if 0 <= it < T and 0 <= ih < H and 0 <= iw < W:
                                dx[:, it, ih, iw, :] += dy[:, to, ho, wo, :] * (idx[:, to, ho, wo, :] == (dt * k[1] + dh) * k[2] + dw)
    if relu_mask:
        dx = dx * (x > 0)
    return torch.from_numpy(dx)


def maxpool_tie_share(x, k, s, p):
    """Share of (window, channel) pairs whose maximum is attained more than once."""
    x = x.to(D).numpy()
    n, T, H, W, c = x.shape
    To, Ho, Wo = (pool_out(a, b, d, e) for a, b, d, e in zip((T, H, W), k, s, p))
    tied = total = 0
    for to in range(To):
        for ho in range(Ho):
            for wo in range(Wo):
                taps = [x[:, it, ih, iw, :] for it in range(to * s[0] - p[0], to * s[0] - p[0] + k[0]) if 0 <= it < T
                        for ih in range(ho * s[1] - p[1], ho * s[1] - p[1] + k[1]) if 0 <= ih < H
                        for iw in range(wo * s[2] - p[2], wo * s[2] - p[2] + k[2]) if 0 <= iw < W]
                v = np.stack(taps)
                tied += int(((v == v.max(0)).sum(0) > 1).sum())
                total += n * c
    return tied / total


def local_to_flat_index(idx, shape_thw, k, s, p):
    """window-local uint8 index (n, to, ho, wo, c) -> the flat input index t * H * W + h * W + w that F.max_pool3d(return_indices=True) reports."""
    T, H, W = shape_thw
    li = idx.long()
    _, To, Ho, Wo, _ = idx.shape
    dt, dh, dw = li // (k[1] * k[2]), (li // k[2]) % k[1], li % k[2]
    to = torch.arange(To).view(1, To, 1, 1, 1)
    ho = torch.arange(Ho).view(1, 1, Ho, 1, 1)
    wo = torch.arange(Wo).view(1, 1, 1, Wo, 1)
    return ((to * s[0] - p[0] + dt) * H + (ho * s[1] - p[1] + dh)) * W + (wo * s[2] - p[2] + dw)


# ---- thin wrappers over float64 torch -----------------------------------------------------------------------------------------------------------------
def _nchw(x):
    return x.to(D).permute(0, 3, 1, 2)


def nearest2x_ref(x):
    """(n, h, w, c) -> (n, 2h, 2w, c): F.interpolate(scale_factor=2, mode='nearest')."""
    return F.interpolate(_nchw(x), scale_factor=2, mode="nearest").permute(0, 2, 3, 1).contiguous()


def nearest2x_bwd_ref(dy):
    """(n, 2h, 2w, c) -> (n, h, w, c): the sums of the 2 x 2 blocks."""
    n, h2, w2, c = dy.shape
    return dy.to(D).view(n, h2 // 2, 2, w2 // 2, 2, c).sum((2, 4))


def bilinear_pad(h, w, ho, wo):
    dyy, dxx = ho - 2 * h, wo - 2 * w
    return dyy // 2, dxx // 2


def bilinear2x_ref(x, ho, wo):
    """(n, h, w, c) -> (n, ho, wo, c): nn.Upsample(scale_factor=2, mode='bilinear', align_corners=True) + F.pad to the skip size (unet_parts.py:50-62).
    Also returns the sum of the four |taps| behind every output element (0 in the border), for the bound on the fp32 source-index arithmetic."""
    n, h, w, c = x.shape
    pt, pl = bilinear_pad(h, w, ho, wo)
    up = F.interpolate(_nchw(x), scale_factor=2, mode="bilinear", align_corners=True)
    up = F.pad(up, [pl, wo - 2 * w - pl, pt, ho - 2 * h - pt]).permute(0, 2, 3, 1).contiguous()
    a = x.to(D).abs()
    h0 = (torch.arange(2 * h) * (h - 1)) // max(2 * h - 1, 1)
    w0 = (torch.arange(2 * w) * (w - 1)) // max(2 * w - 1, 1)
    h1, w1 = (h0 + 1).clamp_max(h - 1), (w0 + 1).clamp_max(w - 1)
    taps = torch.zeros((n, ho, wo, c), dtype=D)
    taps[:, pt:pt + 2 * h, pl:pl + 2 * w] = a[:, h0][:, :, w0] + a[:, h0][:, :, w1] + a[:, h1][:, :, w0] + a[:, h1][:, :, w1]
    return up, taps


def bilinear2x_bwd_ref(dy, h, w):
    """gradient of bilinear2x_ref w.r.t. x, by float64 autograd: dy (n, ho, wo, c) -> (n, h, w, c)."""
    n, ho, wo, c = dy.shape
    x = torch.zeros((n, h, w, c), dtype=D, requires_grad=True)
    pt, pl = bilinear_pad(h, w, ho, wo)
    up = F.interpolate(_nchw(x), scale_factor=2, mode="bilinear", align_corners=True)
    up = F.pad(up, [pl, wo - 2 * w - pl, pt, ho - 2 * h - pt]).permute(0, 2, 3, 1)
    up.backward(dy.to(D))
    return x.grad


def bn1d_train_ref(x, gamma, beta, eps, relu, dy=None):
    """nn.BatchNorm1d in train mode (+ ReLU) on (B, C), float64 torch with autograd. B = 1 (torch refuses it): the kernel's documented rule -- the biased
    variance, 0, also feeds the running statistics. Returns y, mean, invstd, unbiased (B > 1) variance, and with dy: dx, dgamma, dbeta."""
    x = x.to(D).clone().requires_grad_()
    gamma, beta = gamma.to(D).clone().requires_grad_(), beta.to(D).clone().requires_grad_()
    B = x.shape[0]
    mean = x.detach().mean(0)
    var = x.detach().var(0, unbiased=False)
    if B > 1:
        u = F.batch_norm(x, None, None, gamma, beta, training=True, eps=eps)
    else:
        u = (x - x.mean(0)) / torch.sqrt(x.var(0, unbiased=False) + eps) * gamma + beta
    y = F.relu(u) if relu else u
    out = {"y": y.detach(), "mean": mean, "invstd": 1.0 / torch.sqrt(var + eps), "var_run": var * B / (B - 1) if B > 1 else var}
    if dy is not None:
        y.backward(dy.to(D))
        out.update(dx=x.grad, dgamma=gamma.grad, dbeta=beta.grad)
    return out


def l2_normalize_ref(x, eps, dy=None):
    """F.normalize(p=2, dim=1) (+ its gradient by autograd)."""
    x = x.to(D).clone().requires_grad_()
    y = F.normalize(x, p=2.0, dim=1, eps=eps)
    if dy is None:
        return y.detach(), None
    y.backward(dy.to(D))
    return y.detach(), x.grad


def _with_grads(fn, *ts):
    ts = [t.to(D).clone().requires_grad_() for t in ts]
    l = fn(*ts)
    l.backward()
    return (l.detach(),) + tuple(t.grad for t in ts)


def cross_entropy_ref(logits, labels):
    """nn.CrossEntropyLoss() (mean): value, dlogits."""
    return _with_grads(lambda lg: F.cross_entropy(lg, labels), logits)


def triplet_ref(a, p, n, margin=1.0, eps=1e-6):
    """nn.TripletMarginLoss(margin, p=2, eps): value, da, dp, dn."""
    return _with_grads(lambda a_, p_, n_: F.triplet_margin_loss(a_, p_, n_, margin=margin, p=2.0, eps=eps), a, p, n)


def ntxent_ref(zis, zjs, temperature, use_cosine):
    """NTXentLoss (aux_code/nt_xent_original.py:49-70) in its closed form: CE over S / T without the main diagonal, target the +-N diagonal, mean over
    the 2N rows; cosine: rows normalised as nn.CosineSimilarity does (eps 1e-8). value, dzis, dzjs."""
    def f(zi, zj):
        if use_cosine:
            zi, zj = F.normalize(zi, dim=1, eps=1e-8), F.normalize(zj, dim=1, eps=1e-8)
        r = torch.cat([zj, zi])
        n2 = r.shape[0]
        s = (r @ r.t()) / temperature
        s = s.masked_fill(torch.eye(n2, dtype=torch.bool), float("-inf"))
        return F.cross_entropy(s, (torch.arange(n2) + n2 // 2) % n2)
    return _with_grads(f, zis, zjs)


# ---- the shapes the op tests run (tests/test_kernel_refs.py checks the references at the same ones) ---------------------------------------------------
BN_CHANNELS = [(8, 8), (3, 8), (20, 24), (40, 40), (72, 72), (264, 264), (512, 512)]       # (C, Cz) of bn_train_apply
BN_PIXELS = [1, 7, 255, 257, 1000]
BN_BWD_C = [8, 24, 40, 72, 264]            # C / 8 = 1, 3, 5, 9, 33
BN_BWD_PIXELS = [1, 7, 255, 257, 1999]
POOL_CASES = [   # id, kernel, stride, front pad, (t, h, w)
    ("k233s2", (2, 3, 3), (2, 2, 2), (0, 0, 0), (4, 13, 13)),
    ("k2s2_fast", (1, 2, 2), (1, 2, 2), (0, 0, 0), (2, 12, 10)),
    ("k2s2_odd", (1, 2, 2), (1, 2, 2), (0, 0, 0), (2, 13, 11)),
    ("k211_t", (2, 1, 1), (2, 1, 1), (0, 0, 0), (5, 3, 3)),
    ("k3s2_pad", (1, 3, 3), (1, 2, 2), (0, 1, 1), (1, 14, 14)),
    ("k333s1_pad", (3, 3, 3), (1, 1, 1), (1, 1, 1), (3, 5, 6)),
]
POOL_C = [8, 24, 72]
BILINEAR_CASES = [(1, 3, 2, 6), (6, 5, 13, 11), (7, 7, 14, 14)]       # h, w -> ho, wo


def bn_inputs(seed, pixels, C, Cz, groups, dt):
    """z (groups, pixels, Cz) pre-rounded to the storage type `dt` (a torch dtype; torch.float32: not rounded): per group and channel centred, then moved
    by at most half its standard deviation (|batch mean| <= batch std: E[x^2] - mean^2 cancels nothing), groups at different scales; plus gamma, beta."""
    raw = synth_tensor(seed, "bnz", (groups, pixels, Cz), -1, 1).to(D)
    gain = torch.tensor([1.0, 0.25, 3.0], dtype=D)[:groups].view(groups, 1, 1)
    off = synth_tensor(seed, "bnoff", (groups, 1, Cz), -0.5, 0.5).to(D)
    cen = raw - raw.mean(1, keepdim=True)
    z = (cen + off * cen.std(1, unbiased=False, keepdim=True)) * gain
    if pixels == 1:      # one value per channel: mean = z, std = 0. |z| <= 1.5 * 2^-10 keeps the cancellation in E[x^2] - mean^2 (~3 z^2 2^-24) below 2^-24 of eps = 1e-5
        z = off * gain * 2.0 ** -10
    z = z.to(dt).to(D)
    gamma = synth_tensor(seed, "bng", (C,), 0.5, 1.5)
    gamma = torch.where(synth_tensor(seed, "bngs", (C,)) < 0.25, -gamma, gamma)       # some negative scales
    beta = synth_tensor(seed, "bnb", (C,), -0.5, 0.5)
    return z, gamma, beta
