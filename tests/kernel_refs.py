"""float64 references of the memory-bound training kernels (csrc/train_ops.hip, the idx / backward half of csrc/pool_layout.hip, csrc/head.hip, csrc/loss.hip)
and the two value generators their tests use; then the exact-arithmetic conv references and case tables of tests/test_hip_conv_exact.py and, at the end, the chain
references, input conditions and case tables of the fused forward kernels (tests/test_hip_fused_exact.py), then the case table of the plain forward conv and the launcher's
acceptance rule per tile configuration (fwd_accepts; tests/test_hip_conv_fwd_exact.py), then the inference max-pool reference, its launcher's selection restated
(maxpool_form) and the pool / clip-layout case tables of tests/test_hip_infer_pool.py, and last the weight-image, BatchNorm-fold and gradient-unpack references (numpy) and
case table of tests/test_hip_pack_exact.py; at the very end the MGFN kernels' references with their per-element bounds (tests/test_hip_mgfn_edges.py) and the torch
restatements the older MGFN kernel tests share; last of all the references and case tables of the fp32 head, BCE and vote kernels
(tests/test_hip_head_exact.py). A plain helper module: tests/test_kernel_refs.py checks every reference here against float64 torch (autograd) on
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


# ---- exact-arithmetic conv references (tests/test_hip_conv_exact.py) ------------------------------------------------------------------------------------
# Small-integer operands make every product and every partial sum of the conv kernels an integer below 2^24: exact in fp32 whatever the order of the float
# atomics, the K order of a tile, the pixel splits or the MFMA shape. The kernels must then equal these float64 references BIT FOR BIT (rounded once where
# the output is 16-bit). Tensors are (n, c, t, h, w) float64; weights (co, ci, kt, kh, kw); pads are (t, h, w) FRONT / BACK zero padding.
def small_ints(seed, name, shape, lo=-2, hi=2, density=0.5):
    """Integers in [lo, hi], a share 1 - density of them forced to 0: exact in f16 and bf16."""
    u = synth_tensor(seed, name, shape).to(D)
    keep = synth_tensor(seed, name + "/keep", shape).to(D) < density
    return (torch.floor(u * (hi - lo + 1)).clamp_(0, hi - lo) + lo) * keep


def _pad5(x, pf, pb):
    return F.pad(x, [pf[2], pb[2], pf[1], pb[1], pf[0], pb[0]])


def _chan(v):
    return torch.as_tensor(v).to(D).view(1, -1, 1, 1, 1)


def _epilogue(v, residual, mask, relu):
    if residual is not None:
        v = v + residual.to(D)
    if relu:
        v = v.clamp_min(0.0)
    if mask is not None:
        v = torch.where(mask.to(D) > 0, v, torch.zeros_like(v))
    return v


def conv_fwd_ref64(x, w, stride, pf, pb, scale=None, shift=None, residual=None, mask=None, relu=False):
    """(y, z): z = scale[co] * conv3d(x, w) + shift[co] (what `stats` and a plain `y32` see), y = mask > 0 ? act(z + residual) : 0."""
    z = F.conv3d(_pad5(x.to(D), pf, pb), w.to(D), stride=tuple(stride))
    if scale is not None:
        z = z * _chan(scale)
    if shift is not None:
        z = z + _chan(shift)
    return _epilogue(z, residual, mask, relu), z


def conv_dgrad_ref64(dy, w, x_shape, stride, pf, pb, scale=None, residual=None, mask=None, relu=False):
    """d(x) of y = conv3d(pad(x), w * scale[co]) for the output gradient dy, by float64 autograd; then (+ residual), ReLU, mask as above."""
    x = torch.zeros(tuple(x_shape), dtype=D, requires_grad=True)
    y = F.conv3d(_pad5(x, pf, pb), w.to(D), stride=tuple(stride))
    g = dy.to(D)
    y.backward(g * _chan(scale) if scale is not None else g)
    return _epilogue(x.grad, residual, mask, relu)


def conv_wgrad_ref64(x, dy, w_shape, stride, pf, pb):
    """d(w) of y = conv3d(pad(x), w) for the output gradient dy, by float64 autograd."""
    w = torch.zeros(tuple(w_shape), dtype=D, requires_grad=True)
    F.conv3d(_pad5(x.to(D), pf, pb), w, stride=tuple(stride)).backward(dy.to(D))
    return w.grad


def conv_stats_ref64(z, groups=1):
    """z (n, c, ...) -> (groups, 2, c): the sum and the sum of squares per channel over the pixels of each group of n / groups consecutive samples."""
    n, c = z.shape[:2]
    assert n % groups == 0
    zz = z.to(D).reshape(groups, n // groups, c, -1)
    return torch.stack([zz.sum((1, 3)), (zz * zz).sum((1, 3))], dim=1)


def exact_in_fp32(*abs_sums, stats_z=None):
    """The exactness gate: every argument is a compared quantity recomputed on ABSOLUTE values in float64 (sum |x||w|, sum |dy||x|, sum |z|, sum z^2).
    All of them below 2^24 means that every partial sum the kernel can form, in any order, is an integer fp32 holds exactly. Where batch statistics are
    compared, |z| < 4096 as well (z^2 < 2^24). A condition on the test's inputs, not a tolerance: a shape that breaks it needs sparser or smaller inputs."""
    for a in abs_sums:
        a = torch.as_tensor(a).to(D)
        assert bool((a == a.round()).all()), "not integer-valued"
        assert float(a.abs().max()) < 2.0 ** 24, float(a.abs().max())
    if stats_z is not None:
        assert float(torch.as_tensor(stats_z).abs().max()) < 4096.0
    return True


def round_once(t64, dtype):
    """float64 -> fp32 (exact: checked) -> the 16-bit storage type, round-to-nearest-even; returned as float64."""
    f = t64.to(torch.float32)
    assert torch.equal(f.to(D), t64.to(D)), "not exact in fp32"
    return f.to(TDT[dtype]).to(D)


def first_mismatch(got, want):
    """'' if equal, else the count of differing elements and the first differing index with both values (NaN == NaN, +0 == -0 do not count)."""
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = (got != want) & ~(torch.isnan(got) & torch.isnan(want))
    if not bool(bad.any()):
        return ""
    idx = tuple(int(i) for i in bad.nonzero()[0])
    return "%d of %d differ; first at %s: got %r, want %r" % (int(bad.sum()), bad.numel(), idx, float(got[idx]), float(want[idx]))


def wgrad_form(cin_k, cout8, k, stride, pf, in_thw, out_thw, n):
    """The launch form tedspad_conv_wgrad picks (csrc/conv_wgrad.hip, the launcher's own formulas) and its number of pixel splits:
    ('narrow' <1,4> | 'wide' <2,4> | '2x2' <2,2> | 'three' | 'patch', splits)."""
    K = k[0] * k[1] * k[2] * cin_k
    kpad = (K + 63) // 64 * 64
    nkc = kpad // 64
    M = n * out_thw[0] * out_thw[1] * out_thw[2]
    narrow = (cout8 + 127) // 128 * 128 - cout8 >= 64
    wide = (not narrow) and (nkc + 3) // 4 * 4 * 100 <= nkc * 115
    if tuple(k) == (1, 3, 3) and tuple(stride) == (1, 1, 1) and tuple(pf) == (0, 1, 1) and tuple(out_thw) == tuple(in_thw) and cin_k % 64 == 0 and 9 * cin_k <= kpad:
        tiles = (cin_k // 64) * ((cout8 + 63) // 64)
        w, h = in_thw[2], in_thw[1]
        tw, th = (w + 15) // 16, (h + 3) // 4
        if tw * 16 * 100 <= w * 115 and w >= 14:
            npatch = n * in_thw[0] * th * tw
            sp = max(1, min((256 + tiles - 1) // tiles, (npatch + 7) // 8))
            pps = (npatch + sp - 1) // sp
            return "patch", (npatch + pps - 1) // pps
        sp = max(1, min((256 + tiles - 1) // tiles, (M + 511) // 512))
        rows = ((M + sp - 1) // sp + 63) // 64 * 64
        return "three", (M + rows - 1) // rows
    k_tiles = (nkc + 3) // 4 if (narrow or wide) else (nkc + 1) // 2
    tiles = k_tiles * ((cout8 + 63) // 64 if narrow else (cout8 + 127) // 128)
    sp = max(1, min((1024 + tiles - 1) // tiles, (M + 511) // 512))
    rows = ((M + sp - 1) // sp + 63) // 64 * 64
    return ("narrow" if narrow else "wide" if wide else "2x2"), (M + rows - 1) // rows


def conv_out_dims(thw, k, stride, pf, pb):
    return tuple((a + f + b - kk) // s + 1 for a, kk, s, f, b in zip(thw, k, stride, pf, pb))


class ConvCase:
    """One row of the case tables below: input dims (n, t, h, w), channels, kernel, stride, front / back pads (default: k // 2 both), the launch form of the
    weight gradient the row is there for. `pair_w`: the stem in pixel-pair form (engine.stem_pair_form: 8 kernel channels = 2 pixels x 4, stride 1 along w)."""

    def __init__(self, name, dims, cin, cout, k, stride=(1, 1, 1), pf=None, pb=None, form=None, multi_split=False, pair_w=None):
        self.name, self.dims, self.cin, self.cout, self.k, self.stride = name, tuple(dims), cin, cout, tuple(k), tuple(stride)
        self.pf = tuple(kk // 2 for kk in k) if pf is None else tuple(pf)
        self.pb = self.pf if pb is None else tuple(pb)
        self.form, self.multi_split, self.pair_w = form, multi_split, pair_w
        self.out = conv_out_dims(self.dims[1:], self.k, self.stride, self.pf, self.pb)

    def kernel_geometry(self):
        """(cin_k, k, stride, pf, in_thw) as the kernels see the conv: the pixel-pair stem reads 8-channel pixel pairs with stride 1 along w."""
        n, t, h, w = self.dims
        if self.pair_w is None:
            return (self.cin + 7) // 8 * 8, self.k, self.stride, self.pf, (t, h, w)
        pw2 = (self.pair_w + 1) // 2
        kw2 = (self.k[2] + 2 * pw2 - self.pair_w + 1) // 2
        return 8, (self.k[0], self.k[1], kw2), (self.stride[0], self.stride[1], 1), (self.pf[0], self.pf[1], pw2), (t, h, w // 2)

    def launch_form(self):
        cin_k, k, stride, pf, thw = self.kernel_geometry()
        return wgrad_form(cin_k, (self.cout + 7) // 8 * 8, k, stride, pf, thw, self.out, self.dims[0])

    def tensors(self, seed=11, density=0.75):
        """x, w, dy: small integers."""
        n, t, h, w = self.dims
        x = small_ints(seed, self.name + "x", (n, self.cin, t, h, w), density=density)
        wt = small_ints(seed, self.name + "w", (self.cout, self.cin) + self.k, density=density)
        dy = small_ints(seed, self.name + "dy", (n, self.cout) + self.out, density=density)
        return x, wt, dy


S2 = (1, 2, 2)
WGRAD_POINTWISE = [
    ConvCase("narrow_64_64", (2, 2, 9, 9), 64, 64, (1, 1, 1), form="narrow"),
    ConvCase("narrow_64_40", (2, 2, 9, 9), 64, 40, (1, 1, 1), form="narrow"),
    ConvCase("narrow_40_64", (2, 2, 9, 9), 40, 64, (1, 1, 1), form="narrow"),       # K = 40 < kpad = 64: padding columns
    ConvCase("wide_256_128", (2, 2, 7, 9), 256, 128, (1, 1, 1), form="wide"),
    ConvCase("2x2_192_128", (2, 2, 7, 9), 192, 128, (1, 1, 1), form="2x2"),
    ConvCase("2x2_64_256", (2, 2, 7, 9), 64, 256, (1, 1, 1), form="2x2"),
]
WGRAD_THREE = [ConvCase("three_c%d_w%d_h%d" % (c, w, h), (n, t, h, w), c, 72, (1, 3, 3), form="three", multi_split=ms)
               for c in (64, 128) for n, t, h, w, ms in ((2, 1, 9, 7, False), (2, 1, 9, 20, False), (1, 2, 3, 65, False), (2, 1, 30, 20, True))]
WGRAD_PATCH = [ConvCase("patch_w%d_h%d" % (w, h), (1, 3, h, w), 128, 96, (1, 3, 3), form="patch") for w in (14, 16, 30, 63) for h in (5, 9)]
GATHER_CASES = [       # the generic gather kernel (and the data gradient's strided cases)
    ConvCase("t3_T2", (2, 2, 7, 9), 64, 128, (3, 1, 1), form="2x2"),
    ConvCase("t3_T3", (2, 3, 7, 9), 128, 64, (3, 1, 1), form="narrow"),
    ConvCase("s2_15", (2, 2, 15, 15), 64, 128, (1, 3, 3), S2, form="2x2"),
    ConvCase("s2_14", (2, 1, 14, 14), 128, 128, (1, 3, 3), S2, form="wide"),
    ConvCase("pw_s2", (2, 2, 15, 14), 64, 128, (1, 1, 1), S2, form="2x2"),
    ConvCase("k333_s2_tfsame", (2, 4, 9, 9), 64, 64, (3, 3, 3), (2, 2, 2), pf=(0, 1, 1), pb=(1, 1, 1), form="narrow"),
    ConvCase("stem_pair", (2, 8, 32, 32), 3, 64, (5, 7, 7), (2, 2, 2), pf=(2, 3, 3), form="narrow", pair_w=3),
]
WGRAD_CASES = WGRAD_POINTWISE + WGRAD_THREE + WGRAD_PATCH + GATHER_CASES
DGRAD_CASES = GATHER_CASES + [
    ConvCase("d_3x3", (2, 2, 12, 11), 64, 64, (1, 3, 3)),
    ConvCase("d_1x1", (2, 2, 9, 9), 64, 256, (1, 1, 1)),
]
EPILOGUE_CASES = [     # PackedConv.__call__ under every tile configuration: dims, cin, cout, kernel, the configurations that must have run
    (ConvCase("e_3x3_64_64", (6, 1, 20, 37), 64, 64, (1, 3, 3)), (5, 32, 33, 38, 40)),
    (ConvCase("e_3x3_128_136", (3, 1, 33, 16), 128, 136, (1, 3, 3)), (5, 32, 33, 38)),
    (ConvCase("e_1x1_64_128", (6, 2, 12, 12), 64, 128, (1, 1, 1)), (1, 5)),
]
EPILOGUE_GROUPS = 3


def case_by_name(table, name):
    return next(c for c in table if c.name == name)


def epilogue_tensors(case, seed=17):
    """x, w, bias, residual, mask for an EPILOGUE_CASES row: integers sparse enough that the sums of z and z^2 over all rows pass the gate."""
    n, t, h, w = case.dims
    x = small_ints(seed, case.name + "x", (n, case.cin, t, h, w), density=0.5)
    wt = small_ints(seed, case.name + "w", (case.cout, case.cin) + case.k, density=0.5)
    bias = small_ints(seed, case.name + "b", (case.cout,), density=1.0)
    res = small_ints(seed, case.name + "r", (n, case.cout) + case.out, lo=-8, hi=8, density=1.0)
    mask = signed_zero_mask(seed, case.name + "m", (n, case.cout) + case.out)
    return x, wt, bias, res, mask


def signed_zero_mask(seed, name, shape):
    """Mask values drawn from {-1, -0.0, +0.0, 1}: only the last keeps the element (mask > 0)."""
    u = synth_tensor(seed, name, shape).to(D)
    return torch.tensor([-1.0, -0.0, 0.0, 1.0, 1.0, 1.0], dtype=D)[torch.floor(6.0 * u).long().clamp_(0, 5)]


# ---- exact-arithmetic references of the fused forward kernels (tests/test_hip_fused_exact.py) -------------------------------------------------------------
# The same method carried through the fused stages: integer inputs, integer weights, power-of-two BatchNorm scales and integer shifts keep every value of
# a stage on a dyadic grid (its `step`: the input's step times the smallest scale) and every fp32 partial sum exact; the ONE rounding of a 16-bit
# intermediate is round-to-nearest-even of an exactly known number (round_once), and a rounded grid value is still on the grid, so the next stage is exact
# again. A fused kernel must equal these references bit for bit. A stage is (w, stride, (pads_front, pads_back), scale, shift, residual, relu).
def same(got, want, what, fails=None, detail=None):
    """torch.equal, with the count and the first differing index on a mismatch (+ detail(got, want), a test's own words about where). With `fails`, a list, the
    message is appended to it instead of raised."""
    msg = first_mismatch(got, want)
    if msg and detail is not None:
        msg += detail(got, want)
    if not msg and not torch.equal(got, want):           # a NaN on both sides: first_mismatch lets it pass, torch.equal does not
        msg = "not torch.equal"
    if msg:
        print("%s: %s" % (what, msg))
    if fails is not None:
        if msg:
            fails.append("%s: %s" % (what, msg))
        return not msg
    assert not msg, "%s: %s" % (what, msg)
    return True


def pow2_scales(c, exps=(-1, -2)):
    """Per-channel scales 2^exps[c % len(exps)]: neighbouring channels differ."""
    return torch.tensor([2.0 ** e for e in exps], dtype=D)[torch.arange(c) % len(exps)]


def nonzero_ints(seed, name, shape, lo=-8, hi=8):
    """Integers in [lo, hi] without 0 (a 0 becomes 3)."""
    v = small_ints(seed, name, shape, lo=lo, hi=hi, density=1.0)
    return torch.where(v == 0, torch.full_like(v, 3.0), v)


def exact_in_fp32_steps(abs_sum, step):
    """The exactness gate on a dyadic grid: `abs_sum` (a compared quantity recomputed on absolute values) in units of the power-of-two `step` is an integer
    below 2^24, so every partial sum the kernel can form, in any order, is a multiple of `step` that fp32 holds exactly."""
    assert step > 0 and float(np.log2(step)) == round(float(np.log2(step))), step
    return exact_in_fp32(torch.as_tensor(abs_sum).to(D) / step)


def chain_ref64(x, stages, dtype, step=1.0, fp32_out=False):
    """x (n, c, t, h, w) on a grid of `step` through the stages; every stage's output is rounded once to `dtype` (the last one not with fp32_out: a kernel
    that stores fp32). Returns one dict per stage: y (rounded, float64), raw (before the rounding, after the ReLU), abs (sum |x||w| scale + |shift| +
    |residual| on the rounded input), step (the grid of raw)."""
    out, cur = [], x.to(D)
    for i, (w, stride, (pf, pb), scale, shift, residual, relu) in enumerate(stages):
        raw, _ = conv_fwd_ref64(cur, w, stride, pf, pb, scale=scale, shift=shift, residual=residual, relu=relu)
        _, a = conv_fwd_ref64(cur.abs(), w.abs(), stride, pf, pb, scale=scale, shift=None if shift is None else torch.as_tensor(shift).abs())
        if residual is not None:
            a = a + residual.to(D).abs()
        if scale is not None:
            step = step * float(torch.as_tensor(scale).abs().min())
        last = i == len(stages) - 1
        y = raw.clone() if (last and fp32_out) else round_once(raw, dtype)
        out.append({"y": y, "raw": raw, "abs": a, "step": step, "stored16": not (last and fp32_out), "relu": relu})
        cur = y
    return out


def rounding_stats(raw, dtype):
    """(share of elements the 16-bit store changes, number of exact ties among them that round-to-nearest-even resolves TOWARDS zero: rounding half away from
    zero gets those wrong). v is a tie iff its mirror image 2 v - r about the rounded value r is representable too."""
    r = round_once(raw, dtype)
    moved = r != raw
    mirror = 2.0 * raw - r
    tie = moved & (mirror.to(torch.float32).to(TDT[dtype]).to(D) == mirror)
    return float(moved.double().mean()), int((tie & (r.abs() < raw.abs())).sum())


def fused_conditions(stages, dtype, what="", mix=None):
    """Conditions 1-3 on a chain_ref64 result (or any list of such dicts), asserted; returns per 16-bit stage (rounded share, ties towards zero) and prints
    the largest absolute-value sum in steps. 1: every absolute-value sum in units of the stage's step is an integer below 2^24. 2: every stored 16-bit value is
    below 65504 in magnitude (the inference store saturates, the reference does not). 3: every stage with a ReLU is alive: >= 25 % positive, >= 25 % zero.
    4, with a `mix` that promises it for this type (Mix.rounds): the store of every 16-bit stage before the last changes >= 1 % of it, exact ties among them."""
    stats = []
    for i, s in enumerate(stages):
        assert exact_in_fp32_steps(s["abs"], s["step"])
        if s["stored16"]:
            assert float(s["y"].abs().max()) < 65504.0, (what, i, float(s["y"].abs().max()))
        pos, zero = float((s["y"] > 0).double().mean()), float((s["y"] == 0).double().mean())
        if s["relu"]:
            assert pos >= 0.25 and zero >= 0.25, (what, i, pos, zero)
        st = rounding_stats(s["raw"], dtype) if s["stored16"] else (0.0, 0)
        stats.append(st)
        print("%s %s stage %d: largest |sum| %.0f steps of 2^%d, largest value %.1f, positive %.2f, zero %.2f, rounded %.3f, ties to even towards zero %d" % (
            what, dtype, i, float(s["abs"].max()) / s["step"], round(float(np.log2(s["step"]))), float(s["y"].abs().max()), pos, zero, st[0], st[1]))
        if mix is not None and dtype in mix.rounds and i < len(stages) - 1:
            assert rounding_happens(stats, i), (what, dtype, i, st)
    return stats


def rounding_happens(stats, stage):
    """Condition 4 for one (case, dtype): at least 1 % of the intermediate `stage` is changed by its store, exact ties among them."""
    return stats[stage][0] >= 0.01 and stats[stage][1] >= 1


def bn_is_telling(scale, shift):
    """Condition 5: the scales are powers of two that differ between neighbouring channels, the shifts non-zero integers (a swapped or shifted channel index
    changes the result). `scale` None: a plain bias."""
    shift = torch.as_tensor(shift).to(D)
    assert bool((shift != 0).all()) and bool((shift == shift.round()).all())
    if scale is not None:
        e = torch.log2(torch.as_tensor(scale).to(D))
        assert bool((e == e.round()).all()) and bool((e[1:] != e[:-1]).all())
    return True


def dual_ref64(x, w1, s1, b1, x2, w2, s2, b2, stride2=1, relu=True):
    """relu(s1 * conv(x, w1) + b1 + s2 * conv_strided(x2, w2) + b2) for two 1x1x1 convs, the second sampling x2 with the spatial stride `stride2` on the first
    one's pixels. Returns (raw, abs): abs on absolute values."""
    z, st = (0, 0, 0), (1, stride2, stride2)
    h, w = x.shape[3], x.shape[4]
    def two(xa, wa, xb, wb, ba, bb):
        _, a = conv_fwd_ref64(xa, wa, (1, 1, 1), z, z, scale=s1, shift=ba)
        _, b = conv_fwd_ref64(xb, wb, st, z, z, scale=s2, shift=bb)
        return a + b[:, :, :, :h, :w]
    raw = two(x, w1, x2, w2, b1, b2)
    return (raw.clamp_min(0.0) if relu else raw), two(x.abs(), w1.abs(), x2.abs(), w2.abs(), b1.abs(), b2.abs())


def pair_max_t(y):
    """max over frame pairs (2 k, 2 k + 1) of (n, c, t, h, w); an unpaired last frame is dropped as nn.MaxPool3d((2, 1, 1), (2, 1, 1)) does."""
    tp = y.shape[2] // 2
    return torch.maximum(y[:, :, 0:2 * tp:2], y[:, :, 1:2 * tp:2])


def max_pool_ref64(y, k, s):
    return F.max_pool3d(y.to(D), tuple(k), tuple(s))


def upsample2x_nchw(x):
    """nearest x2 along h and w of (n, c, t, h, w)."""
    return x.repeat_interleave(2, dim=3).repeat_interleave(2, dim=4)


P0, P011 = ((0, 0, 0), (0, 0, 0)), ((0, 1, 1), (0, 1, 1))
ONE = (1, 1, 1)


class Mix:
    """How a fused case draws its integers: activations in [-x_hi, x_hi] at x_density, per conv the weights in [-hi, hi] at a density, the scale exponents."""

    def __init__(self, x_hi, x_density, weights, exps=(-1, -2), rounds=()):
        """rounds: the types whose 16-bit intermediates the mix promises to round, ties included (condition 4; fused_conditions asserts it)."""
        self.x_hi, self.x_density, self.weights, self.exps, self.rounds = x_hi, x_density, weights, exps, tuple(rounds)

    def x(self, seed, name, shape):
        return small_ints(seed, name, shape, lo=-self.x_hi, hi=self.x_hi, density=self.x_density)

    def w(self, i, seed, name, shape):
        hi, density = self.weights[i]
        return small_ints(seed, name, shape, lo=-hi, hi=hi, density=density)

    def bn(self, seed, name, c):
        return pow2_scales(c, self.exps), nonzero_ints(seed, name + "b", (c,))


BOTH = ("f16", "bf16")
SMALL = Mix(2, 0.5, [(2, 0.1), (2, 0.1), (2, 0.25)])              # bf16 rounds the second intermediate only, f16 neither
BIG = Mix(8, 1.0, [(16, 1.0), (2, 0.03), (2, 0.03)], rounds=BOTH)              # stage sums above 2048 steps: f16 rounds too


class BneckFrameCase:
    """engine.BneckFrame: conv1 (1x1x1 | 3x1x1, 1024 -> 256) -> conv2 (1x3x3) -> conv3 (256 -> 1024) + the input as residual, 14 x 14 frames."""

    def __init__(self, name, temporal, n, t, mix):
        self.name, self.temporal, self.n, self.t, self.mix = name, temporal, n, t, mix

    def tensors(self, seed=23):
        m, nm, kt = self.mix, self.name, 3 if self.temporal else 1
        x = m.x(seed, nm + "x", (self.n, 1024, self.t, 14, 14))
        ws = [m.w(0, seed, nm + "w1", (256, 1024, kt, 1, 1)), m.w(1, seed, nm + "w2", (256, 256, 1, 3, 3)), m.w(2, seed, nm + "w3", (1024, 256, 1, 1, 1))]
        bn = [m.bn(seed, nm + "bn%d" % i, c) for i, c in enumerate((256, 256, 1024))]
        return x, ws, bn

    def stages(self, x, ws, bn):
        pt = ((1, 0, 0), (1, 0, 0)) if self.temporal else P0
        return [(ws[0], ONE, pt, bn[0][0], bn[0][1], None, True), (ws[1], ONE, P011, bn[1][0], bn[1][1], None, True), (ws[2], ONE, P0, bn[2][0], bn[2][1], x, True)]


BNECK_FRAME_CASES = [BneckFrameCase("plain_1x3", False, 1, 3, SMALL), BneckFrameCase("plain_3x2_big", False, 3, 2, BIG),
                     BneckFrameCase("temporal_2x2", True, 2, 2, SMALL), BneckFrameCase("temporal_1x2_big", True, 1, 2, BIG)]


TAIL_SMALL = Mix(8, 1.0, [(4, 1.0), (2, 0.25), (2, 0.25)], rounds=("bf16",))       # the 64 / 128-channel intermediate above 256 steps: bf16 rounds it
TAIL_BIG = Mix(8, 1.0, [(32, 1.0), (2, 0.25), (2, 0.25)], rounds=BOTH)        # ... above 2048 steps: f16 rounds it too


class BneckTailCase:
    """engine.BneckTail: conv2 (1x3x3, cmid -> cmid) -> conv3 (cmid -> 4 cmid) + residual | + the downsample branch on x2 (64 -> 256) | + residual and the
    temporal pair max. `forms`: which of 'residual', 'dual', 'pool' the case runs (the 128-channel kernel is the plain block only; the pool needs an even t)."""

    def __init__(self, dims, cmid, mix):
        self.dims, self.cmid, self.cout3, self.mix = tuple(dims), cmid, 4 * cmid, mix
        self.name = "c%d_%dx%dx%dx%d" % ((cmid,) + self.dims)
        self.forms = ("residual",) if cmid == 128 else ("residual", "dual") + (("pool",) if dims[1] % 2 == 0 else ())

    def tensors(self, seed=29):
        m, nm, c, (n, t, h, w) = self.mix, self.name, self.cmid, self.dims
        d = {"x": m.x(seed, nm + "x", (n, c, t, h, w)), "w2": m.w(0, seed, nm + "w2", (c, c, 1, 3, 3)), "w3": m.w(1, seed, nm + "w3", (self.cout3, c, 1, 1, 1)),
             "res": nonzero_ints(seed, nm + "r", (n, self.cout3, t, h, w))}
        d["s2"], d["b2"] = m.bn(seed, nm + "bn2", c)
        d["s3"], d["b3"] = m.bn(seed, nm + "bn3", self.cout3)
        if c == 64:
            d["x2"], d["wd"] = m.x(seed, nm + "x2", (n, 64, t, h, w)), m.w(2, seed, nm + "wd", (self.cout3, 64, 1, 1, 1))
            d["sd"], d["bd"] = pow2_scales(self.cout3, tuple(reversed(m.exps))), nonzero_ints(seed, nm + "bnd", (self.cout3,))
        return d

    def reference(self, d, dtype):
        """{form: [mid stage, output stage]} as chain_ref64 gives them; 'dual' adds the second conv to the output stage, 'pool' takes the pair max of 'residual'."""
        mid = chain_ref64(d["x"], [(d["w2"], ONE, P011, d["s2"], d["b2"], None, True)], dtype)[0]
        out = {}
        for form in self.forms:
            if form == "dual":
                raw, a = dual_ref64(mid["y"], d["w3"], d["s3"], d["b3"], d["x2"], d["wd"], d["sd"], d["bd"])
                step = mid["step"] * 0.25
                out[form] = [mid, {"y": round_once(raw, dtype), "raw": raw, "abs": a, "step": step, "stored16": True, "relu": True}]
            else:
                last = chain_ref64(mid["y"], [(d["w3"], ONE, P0, d["s3"], d["b3"], d["res"], True)], dtype, step=mid["step"])[0]
                if form == "pool":
                    last = dict(last, y=pair_max_t(last["y"]), raw=pair_max_t(last["raw"]))
                out[form] = [mid, last]
        return out


BNECK_TAIL64_CASES = [BneckTailCase((2, 3, 7, 9), 64, TAIL_BIG), BneckTailCase((1, 1, 16, 16), 64, TAIL_SMALL), BneckTailCase((3, 6, 9, 11), 64, TAIL_SMALL),
                      BneckTailCase((1, 2, 20, 55), 64, TAIL_BIG)]
BNECK_TAIL128_CASES = [BneckTailCase((2, 3, 7, 9), 128, TAIL_BIG), BneckTailCase((1, 1, 16, 16), 128, TAIL_SMALL), BneckTailCase((4, 2, 14, 30), 128, TAIL_SMALL)]

UPP_SMALL = Mix(8, 1.0, [(4, 1.0), (2, 0.1), (2, 0.1)], rounds=("bf16",))
UPP_BIG = Mix(8, 1.0, [(32, 1.0), (2, 0.1), (2, 0.1)], rounds=BOTH)


class UppTailCase:
    """tedspad_unetpp_tail_fwd: nearest x2 of the (n, h / 2, w / 2, 64) input -> conv-bn-relu 64 -> 32 -> conv-bn-relu 32 -> 32 -> the 3x3 head 32 -> 3 + bias, fp32
    (n, 3, h, w). `walk`: more than twice as many 16 x 16 patches as the device has compute units (256; the grid is min(patches, units)), so workgroups walk two and three
    patches: the head of a patch runs inside the loop, and the third patch is fetched into an X buffer that the first one used."""

    def __init__(self, n, h, w, mix, walk=False):
        self.n, self.h, self.w, self.mix, self.walk = n, h, w, mix, walk
        self.name = "%dx%dx%d" % (n, h, w)
        self.npatch = n * ((h + 15) // 16) * ((w + 15) // 16)

    def tensors(self, seed=31):
        m, nm = self.mix, self.name
        d = {"x": m.x(seed, nm + "x", (self.n, 64, 1, self.h // 2, self.w // 2)), "w1": m.w(0, seed, nm + "w1", (32, 64, 1, 3, 3)),
             "w2": m.w(1, seed, nm + "w2", (32, 32, 1, 3, 3)), "w3": m.w(2, seed, nm + "w3", (3, 32, 1, 3, 3)), "bias": nonzero_ints(seed, nm + "b3", (3,))}
        d["s1"], d["b1"] = m.bn(seed, nm + "bn1", 32)
        d["s2"], d["b2"] = m.bn(seed, nm + "bn2", 32)
        return d

    def reference(self, d, dtype):
        return chain_ref64(upsample2x_nchw(d["x"]), [(d["w1"], ONE, P011, d["s1"], d["b1"], None, True), (d["w2"], ONE, P011, d["s2"], d["b2"], None, True),
                                                     (d["w3"], ONE, P011, None, d["bias"], None, False)], dtype, fp32_out=True)


UPP_TAIL_CASES = [UppTailCase(1, 16, 16, UPP_BIG), UppTailCase(2, 18, 34, UPP_SMALL), UppTailCase(3, 48, 80, UPP_BIG), UppTailCase(2, 2, 2, UPP_SMALL),
                  UppTailCase(6, 138, 170, UPP_SMALL, walk=True)]


# ---- the single-stage fused kernels: no 16-bit intermediate, one store --------------------------------------------------------------------------------------
POINT = Mix(8, 1.0, [(4, 1.0), (4, 1.0)])
STEM = Mix(4, 1.0, [(2, 1.0)])
TPAIR_CASES = [(1, 5, 3, 128, 256), (3, 9, 11, 512, 384)]                                     # n, h, w, cin, cout
DUAL_CASES = [((3, 4, 11, 13), 256, 64), ((1, 2, 30, 31), 256, 128), ((2, 1, 5, 5), 64, 64)]        # dims, cout, ld2
DUAL_P8_CASES = [((3, 2, 14, 14), 128, 256, 512, 2), ((2, 2, 7, 9), 256, 512, 1024, 2), ((1, 3, 5, 5), 64, 64, 256, 1), ((2, 1, 28, 27), 128, 64, 256, 2)]
POOL_T2_CASES = [((2, 5, 7, 9), 128, 72, False), ((2, 2, 16, 16), 64, 64, True)]                # dims, cin, cout, residual
STEM_CASES = [(2, 3, 16, 32, 32), (3, 3, 5, 18, 72), (1, 2, 8, 66, 24)]                         # n, c, t, h, w


def _stage(raw, a, step, dtype, relu=True):
    return {"y": round_once(raw, dtype), "raw": raw, "abs": a, "step": step, "stored16": True, "relu": relu}


def negative_ints(seed, name, shape, lo=-8):
    """Integers in [lo, -1]: a stage whose output is a max over several ReLU outputs keeps a quarter of zeros only if most of them are zero."""
    return -nonzero_ints(seed, name, shape, lo=lo, hi=-lo).abs()


def tpair_reference(case, dtype, seed=37):
    """engine.TPairConv: a 3x1x1 'same' conv + BN + ReLU on a two-frame tensor."""
    n, h, w, cin, cout = case
    nm = "tp%d_%d" % (h, cin)
    d = {"x": POINT.x(seed, nm + "x", (n, cin, 2, h, w)), "w": POINT.w(0, seed, nm + "w", (cout, cin, 3, 1, 1))}
    d["s"], d["b"] = POINT.bn(seed, nm + "bn", cout)
    return d, chain_ref64(d["x"], [(d["w"], ONE, ((1, 0, 0), (1, 0, 0)), d["s"], d["b"], None, True)], dtype)


def dual_tensors(dims, c1, c2, cout, stride, seed, nm):
    n, t, h, w = dims
    h2, w2 = (h - 1) * stride + 1 + (stride - 1), (w - 1) * stride + 1                  # odd / even source grids
    d = {"x": POINT.x(seed, nm + "x", (n, c1, t, h, w)), "x2": POINT.x(seed, nm + "x2", (n, c2, t, h2, w2)),
         "w1": POINT.w(0, seed, nm + "w1", (cout, c1, 1, 1, 1)), "w2": POINT.w(1, seed, nm + "w2", (cout, c2, 1, 1, 1))}
    d["s1"], d["b1"] = POINT.bn(seed, nm + "bn1", cout)
    d["s2"], d["b2"] = pow2_scales(cout, (-2, -1)), nonzero_ints(seed, nm + "bn2b", (cout,))
    return d


def dual_reference(case, dtype, seed=41):
    """PackedConv.call_dual: two 1x1x1 convs on 64 channels summed before the one store."""
    dims, cout, ld2 = case
    d = dual_tensors(dims, 64, 64, cout, 1, seed, "du%d_%d" % (dims[2], ld2))
    raw, a = dual_ref64(d["x"], d["w1"], d["s1"], d["b1"], d["x2"], d["w2"], d["s2"], d["b2"])
    return d, [_stage(raw, a, 0.25, dtype)]


def dual_p8_reference(case, dtype, seed=43):
    """PackedConv.call_dual_p8: [W1 s1 | W2 s2] as one GEMM over [x ; x2 sampled with the spatial stride]; the scales are folded into the 16-bit weights (a
    power of two times a small integer: exact)."""
    dims, c1, c2, cout, stride = case
    d = dual_tensors(dims, c1, c2, cout, stride, seed, "p8%d_%d" % (dims[2], c1))
    for k in ("w1", "w2"):
        ws = d[k] * _chan(d["s" + k[1]]).view(-1, 1, 1, 1, 1)
        assert all(torch.equal(ws.to(TDT[t]).to(D), ws) for t in TDT)
    raw, a = dual_ref64(d["x"], d["w1"], d["s1"], d["b1"], d["x2"], d["w2"], d["s2"], d["b2"], stride2=stride)
    return d, [_stage(raw, a, 0.25, dtype)]


def pool_t2_reference(case, dtype, seed=47):
    """PackedConv.call_pool_t2: 1x1x1 conv + BN (+ residual) + ReLU + the max over frame pairs. Returns the stage before the max and the one after it."""
    dims, cin, cout, use_res = case
    n, t, h, w = dims
    nm = "pt%d_%d" % (h, cin)
    d = {"x": POINT.x(seed, nm + "x", (n, cin, t, h, w)), "w": POINT.w(0, seed, nm + "w", (cout, cin, 1, 1, 1)), "s": pow2_scales(cout),
         "b": negative_ints(seed, nm + "b", (cout,), lo=-32), "res": nonzero_ints(seed, nm + "r", (n, cout, t, h, w)) if use_res else None}
    st = chain_ref64(d["x"], [(d["w"], ONE, P0, d["s"], d["b"], d["res"], True)], dtype)[0]
    return d, [st, dict(st, y=pair_max_t(st["y"]), raw=pair_max_t(st["raw"]))]


def stem_reference(case, dtype, seed=53, lit=0.55, lo=-2):
    """engine.StemPT: conv 5x7x7 / 2 / pad (2, 3, 3) + BN + ReLU on an integer clip, the max over output-frame pairs, the (1, 3, 3) / (1, 2, 2) max pool.
    Returns the tensors and three stages: the conv, the pair max (StemPT.conv), the pooled tensor (conv_pool, conv_pool_clip); a max of exact values is exact,
    and rounding is monotonic: max then round = round then max. The clip is zero beyond the first `lit` of its longer spatial axis and every shift is negative,
    so there the ReLU yields whole zero pool windows: the pooled output too keeps a quarter of zeros (a max over 18 independent values would keep none), and an
    epilogue that lost its ReLU shows in all three."""
    n, c, t, h, w = case
    nm = "st%d_%d" % (h, w)
    clip = STEM.x(seed, nm + "x", case)
    if h >= w:
        clip[:, :, :, int(lit * h):] = 0.0
    else:
        clip[..., int(lit * w):] = 0.0
    d = {"clip": clip, "w": STEM.w(0, seed, nm + "w", (64, c, 5, 7, 7)), "s": pow2_scales(64), "b": negative_ints(seed, nm + "b", (64,), lo=lo)}
    st = chain_ref64(d["clip"], [(d["w"], (2, 2, 2), ((2, 3, 3), (2, 3, 3)), d["s"], d["b"], None, True)], dtype)[0]
    pair = dict(st, y=pair_max_t(st["y"]), raw=pair_max_t(st["raw"]))
    pool = dict(pair, y=max_pool_ref64(pair["y"], (1, 3, 3), (1, 2, 2)), raw=max_pool_ref64(pair["raw"], (1, 3, 3), (1, 2, 2)))
    return d, [st, pair, pool]


# ---- the plain forward conv under every tile configuration (tests/test_hip_conv_fwd_exact.py) ------------------------------------------------------------------
# One single-stage chain per row: integer x and w, power-of-two scales, non-zero integer shifts, ReLU; every live tile configuration that takes the row must equal
# chain_ref64 bit for bit, and must take it exactly where fwd_accepts -- the launcher's acceptance rule restated from the code -- says so.
def cl(t, dtype, ld=None, coff=0, seed=0):
    """(n, c, t, h, w) float64 cpu -> channels-last Act on the GPU; with `ld`: a slice [coff, coff + c) of a wider buffer whose other channels hold
    non-zero integers (a kernel that reads past its slice picks them up)."""
    from ted_spad_amd import engine as E
    v = t.permute(0, 2, 3, 4, 1).contiguous()
    c = v.shape[-1]
    if ld is None:
        return E.Act(v.to(TDT[dtype]).cuda(), c)
    buf = small_ints(seed, "slicefill", tuple(v.shape[:4]) + (ld,), lo=1, hi=3, density=1.0)
    buf[..., coff:coff + c] = v
    return E.Act(buf.to(TDT[dtype]).cuda(), c, coff)


def nc(a):
    """Act -> (n, c, t, h, w) float64 cpu."""
    return a.buf.double().cpu()[..., a.coff:a.coff + a.c].permute(0, 4, 1, 2, 3)


NUM_TILE_CFGS = 40                         # conv_igemm.hip NUM_CFGS; the GPU file checks it against tedspad_conv_num_tile_cfgs()
RETIRED_CFGS = (15, 16, 37, 39)
LIVE_CFGS = tuple(c for c in range(1, NUM_TILE_CFGS + 1) if c not in RETIRED_CFGS)
KTAB_MAX_BYTES, KTAB_SMALL_BYTES, LDS_LIMIT = 10240, 1024, 160 * 1024       # conv_common.h; launch.h raise_lds
# conv_igemm.hip launch_cfg: the K-table bytes KT of every generic tile (0: table-free), the (FR, KS, TW) of the stem halo tiles, narrow_sibling
GENERIC_KT = {1: KTAB_MAX_BYTES, 2: KTAB_MAX_BYTES, 3: KTAB_MAX_BYTES, 4: KTAB_MAX_BYTES, 5: KTAB_MAX_BYTES, 6: KTAB_SMALL_BYTES, 7: KTAB_SMALL_BYTES,
              8: KTAB_SMALL_BYTES, 10: KTAB_SMALL_BYTES, 11: KTAB_MAX_BYTES, 12: KTAB_MAX_BYTES, 13: KTAB_MAX_BYTES, 14: KTAB_MAX_BYTES, 17: 0, 18: 0,
              22: KTAB_MAX_BYTES, 23: 0, 24: KTAB_MAX_BYTES, 35: 0, 36: 0}
STEM_TILES = {9: (1, 1, 32), 20: (2, 1, 32), 21: (1, 2, 32), 29: (1, 1, 16), 30: (1, 2, 16), 31: (2, 1, 16)}
NARROW_SIBLING = {1: 2, 24: 2, 3: 4, 6: 7, 11: 12, 13: 14, 22: 14, 18: 17, 23: 17, 35: 17, 36: 17}
SPLIT_K_TILES = (22, 23, 24, 35, 36)
FWD_EXTRAS = ("mask", "y32", "stats", "ostrided", "gathered")       # + ("stats_rows", rows) for grouped statistics


class FwdGeo:
    """A ConvCase as tedspad_conv_fwd_ex sees it (conv_fwd_impl's ConvKP): kernel-form channels, kernel, strides and front pads, the padded K, the output rows."""

    def __init__(self, case, n=None):
        self.cin, self.k, self.stride, self.pf, self.thw = case.kernel_geometry()
        self.n, self.out, self.cout = case.dims[0] if n is None else n, tuple(case.out), (case.cout + 7) // 8 * 8
        self.kpad = (self.k[0] * self.k[1] * self.k[2] * self.cin + 63) // 64 * 64
        self.nk, self.utap = self.kpad // 64, self.cin % 64 == 0
        self.M = self.n * self.out[0] * self.out[1] * self.out[2]
        self.pointwise = self.k == (1, 1, 1) and self.stride == (1, 1, 1) and self.pf == (0, 0, 0) and self.out == tuple(self.thw)
        self.same, self.stride1 = self.out == tuple(self.thw), self.stride == (1, 1, 1)

    def with_cout(self, cout):
        g = FwdGeo.__new__(FwdGeo)
        g.__dict__.update(self.__dict__)
        g.cout = cout
        return g


def _extras(extras):
    names = set(e if isinstance(e, str) else e[0] for e in extras)
    assert names <= set(FWD_EXTRAS) | {"stats_rows"}, names
    rows = next((e[1] for e in extras if not isinstance(e, str)), 0)
    if rows:
        names.add("stats")
    return names, rows


def fwd_refusals_one(cfg, g, extras=()):
    """Every clause of ONE launch's acceptance rule that the geometry `g` (a FwdGeo) fails under the forced tile `cfg`, by name ([]: the tile takes it)."""
    ex, rows = _extras(extras)
    kt, kh, kw = g.k
    T, H, W = g.thw
    plain = not (ex & {"mask", "y32", "stats", "ostrided"})
    bad = []
    # conv_fwd_impl, before any tile is looked at: statistics groups of >= 256 rows; gathered sources on the chunk-major halo tiles only
    if rows and rows < 256:
        bad.append("stats_rows<256")
    if "gathered" in ex:
        if cfg not in (32, 33, 38, 39, 40):
            bad.append("gathered:tile")
        if kt != 1 or g.cin % 64 or g.cin // 64 > 8:
            bad.append("gathered:geometry")
    if cfg in RETIRED_CFGS or not 1 <= cfg <= NUM_TILE_CFGS:       # launch_cfg: case 15 / 16 / 37 / 39
        return bad + ["retired"]
    if cfg in GENERIC_KT:      # launch<>: `if (KT == 0 ? !p.utap : p.Kpad > KT)`; the generic kernel has every epilogue and, with one K tile, a split-K tile's second wave set multiplies its half of it
        KT = GENERIC_KT[cfg]
        if KT == 0 and not g.utap:
            bad.append("generic:cin%64")
        if KT and g.kpad > KT:
            bad.append("generic:kpad>%d" % KT)
    elif cfg in STEM_TILES:      # conv_fwd_impl `if (cfg == 9 || ...)` and launch_stem_halo
        FR, KS, TW = STEM_TILES[cfg]
        if g.cin != 8:
            bad.append("stem:cin!=8")
        if ex & {"mask", "y32", "ostrided"}:
            bad.append("stem:extras")
        if rows and rows % (g.out[0] * g.out[1] * g.out[2]):
            bad.append("stem:stats_rows")
        if g.cout > 64:
            bad.append("stem:cout>64")
        if g.stride[2] != 1:
            bad.append("stem:sw!=1")
        if g.kpad > 8 * 256 * 8:
            bad.append("stem:kpad")
        TH = 256 // TW
        HH, WH, HT = (TH - 1) * g.stride[1] + kh, (TW - 1) * g.stride[2] + kw, kt + (FR - 1) * g.stride[0]
        P = HT * HH * WH
        main = (P + 63) // 64 * 64 * 16 + (2 if FR == 1 else 4) * 8192 + g.nk * 32
        if max(main, 256 * FR * 68 * 4) > LDS_LIMIT:
            bad.append("stem:lds")
    elif cfg == 19:            # conv_pw.hip launch_conv_pw
        if not g.pointwise or g.cin not in (64, 128) or g.kpad != g.cin:
            bad.append("pw:geometry")
        if not plain:
            bad.append("pw:extras")
    elif cfg in (25, 26):      # conv_p8.hip launch_conv_p8
        if not g.utap:
            bad.append("p8:cin%64")
        if g.nk < 2:
            bad.append("p8:nk<2")
        if g.cout % 256:
            bad.append("p8:cout%256")
        if not plain:
            bad.append("p8:extras")
    elif cfg == 27:            # conv_flat.hip launch_conv_flat, launch_flat_t
        same = g.same and g.pf[0] == 0 and g.pf[1] < kh and g.pf[2] < kw
        if g.cin != 64 or kt != 1 or not g.stride1 or not same or not 2 <= kh * kw <= 32 or g.kpad != kh * kw * 64:
            bad.append("flat:geometry")
        if g.cout > 64:
            bad.append("flat:cout>64")
        if not plain:
            bad.append("flat:extras")
        S = (256 + (kh - 1) * W + (kw - 1) + 1) * 8
        if max((S + 63) // 64 * 64 * 16 + 3 * 8192, 256 * 68 * 4) > LDS_LIMIT:
            bad.append("flat:lds")
    elif cfg in (28, 34):      # conv_flat.hip launch_conv_tflat; conv_patch.hip launch_conv_patch, mode 2 (its halo, T * (256 / T) positions, always fits)
        same = g.same and g.pf[1] == 0 and g.pf[2] == 0 and g.pf[0] < kt
        if g.cin % 64 or kh != 1 or kw != 1 or not 2 <= kt <= 3 or not g.stride1 or not same or g.kpad != kt * g.cin:
            bad.append("temporal:geometry")
        if T > 4:
            bad.append("temporal:T>4")
        if g.cout > (64 if cfg == 28 else 512):
            bad.append("temporal:cout")
        if (not plain) if cfg == 28 else ("ostrided" in ex):
            bad.append("temporal:extras")
    elif cfg in (32, 33):      # conv_patch.hip launch_conv_patch, modes 0 / 1; launch_patch_t (the head / tail split changes no clause: none depends on cout <= 512)
        same = g.same and g.pf[0] < kt and g.pf[1] < kh and g.pf[2] < kw
        kt_ok = g.pf[0] == 0 if kt == 1 else (kt <= 3 and T * H * W * g.cin * g.n < 2 ** 31)
        if g.cin % 64 or not kt_ok or not g.stride1 or not same or not 2 <= kh * kw <= 16 or g.kpad != kt * kh * kw * g.cin:
            bad.append("patch:geometry")
        if g.cout > 512:
            bad.append("patch:cout>512")
        if "ostrided" in ex:
            bad.append("patch:extras")
        NP = (16 + kh - 1) * (16 + kw - 1) if cfg == 32 else 256 + (kh - 1) * W + (kw - 1)
        S = (NP + (1 if cfg == 33 else 0)) * 8
        if ((S + 63) // 64 * 64 + 255) // 256 > 12:
            bad.append("patch:halo>384")
    elif cfg in (38, 40):      # conv_patch.hip launch_conv_patch2; conv_patch3.hip launch_conv_patch3 (cout = 128: two launches of 64), launch_conv_patch3_64
        if (g.cin % (64 if "gathered" in ex else 32) or g.k != (1, 3, 3) or g.pf != (0, 1, 1) or not g.stride1 or not g.same or g.kpad < 9 * g.cin):
            bad.append("patch2:geometry")
        if "ostrided" in ex:
            bad.append("patch2:extras")
        if cfg == 40:
            if not (32 < g.cout <= 64 or g.cout == 128):
                bad.append("patch3:cout")
            if "gathered" in ex and (g.cin <= 64 or "stats" in ex):
                bad.append("patch3:gathered")
    else:
        raise AssertionError(cfg)
    return bad


def fwd_refusals(cfg, case, extras=(), n=None):
    """The failed clauses of PackedConv.__call__ on `case` under the forced tile `cfg`. launch_cfg: cout = 128 k + r with 0 < r <= 64 on a tile with a 64-wide sibling
    runs the last r channels on the sibling first; if the sibling declines them, the conv goes unsplit; if it takes them, the head's verdict is the call's."""
    g = FwdGeo(case, n)
    sib = NARROW_SIBLING.get(cfg, 0)
    if sib and "gathered" not in _extras(extras)[0] and g.cout > 128 and 0 < g.cout % 128 <= 64:
        head = g.cout // 128 * 128
        if not fwd_refusals_one(sib, g.with_cout(g.cout - head), extras):
            return fwd_refusals_one(cfg, g.with_cout(head), extras)
    return fwd_refusals_one(cfg, g, extras)


def fwd_accepts(cfg, case, extras=()):
    """The launcher's acceptance rule for a forced tile, restated from the code's own formulas (as wgrad_form does for the weight gradient)."""
    return not fwd_refusals(cfg, case, extras)


def fwd_is_split(cfg, case):
    """launch_cfg runs the row as a head on `cfg` and a tail on its 64-wide sibling."""
    g = FwdGeo(case)
    sib = NARROW_SIBLING.get(cfg, 0)
    return bool(sib) and g.cout > 128 and 0 < g.cout % 128 <= 64 and not fwd_refusals_one(sib, g.with_cout(g.cout % 128))


FWD_SMALL = Mix(2, 0.5, [(2, 0.5)])
FWD_BIG = Mix(8, 0.5, [(32, 0.5)])


class FwdCase:
    """A FWD_CASES row: the conv and its options. big: x in [-8, 8], w in [-32, 32] (otherwise both in [-2, 2]), density 0.5 either way; residual: integers in
    [-8, 8]; slices: the row also runs on channel slices of wider buffers; rounds: the types whose store the row must really round (condition 4)."""

    def __init__(self, conv, big=False, residual=False, slices=False, rounds=()):
        self.conv, self.name, self.big, self.residual, self.slices = conv, conv.name, big, residual, slices
        self.mix, self.rounds = FWD_BIG if big else FWD_SMALL, tuple(rounds)
        self.stem = conv.kernel_geometry()[0] == 8

    def tensors(self, seed=61):
        c, m = self.conv, self.mix
        n, t, h, w = c.dims
        d = {"x": m.x(seed, c.name + "x", (n, c.cin, t, h, w)), "w": m.w(0, seed, c.name + "w", (c.cout, c.cin) + c.k)}
        d["s"], d["b"] = m.bn(seed, c.name + "bn", c.cout)
        d["res"] = small_ints(seed, c.name + "r", (n, c.cout) + c.out, lo=-8, hi=8, density=1.0) if self.residual else None
        return d

    def stage(self, d):
        c = self.conv
        return (d["w"], c.stride, (c.pf, c.pb), d["s"], d["b"], d["res"], True)


_FWD_REF = {}


def fwd_reference(case, dtype):
    """(tensors, [stage]) of a FwdCase: chain_ref64 with a single stage, rounded once. The float64 convs are computed once per row and shared by both types."""
    if case.name not in _FWD_REF:
        d = case.tensors()
        _FWD_REF[case.name] = (d, chain_ref64(d["x"], [case.stage(d)], "f16")[0])
    d, st = _FWD_REF[case.name]
    return d, [dict(st, y=round_once(st["raw"], dtype))]


def fwd_stats_reference(case, d):
    """(z, per-sample statistics (n, 2, c), step) of a stem row: z = scale * conv + shift before the residual and the ReLU; the gate on the absolute sums in steps."""
    c = case.conv
    _, z = conv_fwd_ref64(d["x"], d["w"], c.stride, c.pf, c.pb, scale=d["s"], shift=d["b"])
    _, zabs = conv_fwd_ref64(d["x"].abs(), d["w"].abs(), c.stride, c.pf, c.pb, scale=d["s"], shift=d["b"].abs())
    step = float(d["s"].abs().min())
    sabs = conv_stats_ref64(z.abs(), 1)[0]             # every partial sum of z and of z^2 is bounded by the sums of |z| and z^2
    assert exact_in_fp32(sabs[0] / step, sabs[1] / step ** 2, stats_z=zabs / step)
    return z, conv_stats_ref64(z, c.dims[0]), step


FWD_CASES = [
    FwdCase(ConvCase("pw_64_136_res", (2, 2, 9, 7), 64, 136, (1, 1, 1)), residual=True),                           # Kpad 64: one K tile, M = 252 < 256, sibling split r = 8; tile 19
    FwdCase(ConvCase("pw_128_256_s2", (2, 2, 15, 14), 128, 256, (1, 1, 1), S2)),                                   # the shortest K the ping-pong takes, strided gather on 25 / 26
    FwdCase(ConvCase("pw_192_256", (1, 1, 5, 7), 192, 256, (1, 1, 1)), slices=True),                               # odd K-tile count, M = 35
    FwdCase(ConvCase("pw_1024_64", (1, 2, 5, 7), 1024, 64, (1, 1, 1))),                                            # Kpad = 1024: the short-K tiles 6, 7, 8, 10 take it ...
    FwdCase(ConvCase("pw_1088_64", (1, 2, 5, 7), 1088, 64, (1, 1, 1))),                                            # ... and refuse Kpad = 1088
    FwdCase(ConvCase("t3_T4_256_64", (3, 4, 9, 11), 256, 64, (3, 1, 1))),                                          # tiles 28 and 34 at T = 4
    FwdCase(ConvCase("t3_T3_64_48_res", (2, 3, 5, 13), 64, 48, (3, 1, 1)), residual=True, slices=True),            # T = 3 (an idle wave), ragged cout
    FwdCase(ConvCase("t3_T2_128_512_res", (2, 2, 9, 11), 128, 512, (3, 1, 1)), big=True, residual=True, rounds=("bf16",)),      # two 256-channel tiles on 25 / 26, tile 34 at cout = 512
    FwdCase(ConvCase("t3_2048_512", (2, 2, 7, 7), 2048, 512, (3, 1, 1)), big=True, rounds=BOTH),                   # K = 6144: 96 K tiles
    FwdCase(ConvCase("t5_kmax_2048_64", (1, 5, 3, 3), 2048, 64, (5, 1, 1))),                                       # Kpad = 10240 = KTAB_MAX_BYTES: a full K table
    FwdCase(ConvCase("k333_s2_tfsame", (2, 4, 9, 9), 64, 64, (3, 3, 3), (2, 2, 2), pf=(0, 1, 1), pb=(1, 1, 1))),   # asymmetric pads, strided in all three dims
    FwdCase(ConvCase("s2_3x3_128_128", (2, 2, 15, 15), 128, 128, (1, 3, 3), S2)),                                  # M = 256 exactly
    FwdCase(ConvCase("3x3_64_40_res", (1, 2, 9, 7), 64, 40, (1, 3, 3)), big=True, residual=True, slices=True, rounds=BOTH),     # frames smaller than a tile on 27, 32, 33, 38, 40
    FwdCase(ConvCase("3x3_256_256", (3, 2, 14, 13), 256, 256, (1, 3, 3)), big=True, rounds=BOTH),                  # 36 K tiles on 25 / 26, ragged M
    FwdCase(ConvCase("k333_96_208_res", (1, 4, 9, 10), 96, 208, (3, 3, 3)), residual=True),                        # cin % 64 != 0 (table tiles only), r = 80 > 64: unsplit
    FwdCase(ConvCase("k333_144_288", (1, 2, 7, 9), 144, 288, (3, 3, 3)), big=True, rounds=("bf16",)),              # sibling split r = 32 on every 128-wide tile, split-K ones included
    FwdCase(ConvCase("k333_64_192", (2, 3, 9, 17), 64, 192, (3, 3, 3)), big=True, rounds=BOTH),                    # patch and flat tiles 32 / 33 with temporal taps, ragged patches
    FwdCase(ConvCase("unet_first_3_64", (3, 1, 20, 37), 3, 64, (1, 3, 3))),                                        # stem halo tiles on K = 72
    FwdCase(ConvCase("stem_large", (2, 8, 32, 32), 3, 64, (5, 7, 7), (2, 2, 2), pf=(2, 3, 3), pair_w=3)),          # the six stem tiles on the largei3d stem
    FwdCase(ConvCase("stem_i3d", (2, 8, 32, 32), 3, 64, (7, 7, 7), (2, 2, 2), pf=(2, 2, 2), pb=(3, 3, 3), pair_w=2)),           # ... on the Inception stem, TF-SAME pads
    FwdCase(ConvCase("k13_64_64", (2, 2, 5, 9), 64, 64, (1, 1, 3))),                                               # a second kernel shape for tile 27 (and 32 / 33): 1 x 1 x 3
    FwdCase(ConvCase("t2_T3_128_64", (2, 3, 5, 9), 128, 64, (2, 1, 1), pf=(1, 0, 0), pb=(0, 0, 0))),               # ... for tiles 28 and 34: 2 x 1 x 1, the pad in front
] + [FwdCase(c) for c, _ in EPILOGUE_CASES]                                                                         # the three epilogue rows with the plain epilogue
FWD_STEM_ROWS = [c for c in FWD_CASES if c.stem]
FWD_SLICE_ROWS = [c for c in FWD_CASES if c.slices]
SINGLE_CLASS_TILES = {19: ((1, 1, 1), (1, 1, 1)), 38: ((1, 3, 3), (1, 1, 1)), 40: ((1, 3, 3), (1, 1, 1))}      # launchers that admit one (kernel, stride) only
GATHER_FWD_CASES = [((2, 1, 12, 20), (64, 64), 64), ((2, 1, 28, 28), (128, 64, 64), 128), ((1, 1, 2, 2), (64, 128), 24)]       # dims, source channels, cout (1 x 3 x 3)


def gather_conv_case(row):
    dims, chans, cout = row
    return ConvCase("gather_%dx%d_%d" % (dims[2], dims[3], cout), dims, sum(chans), cout, (1, 3, 3))


def gather_fwd_reference(row, dtype, seed=67):
    """PackedConv.gather on a GATHER_FWD_CASES row: the sources (n, c_i, t, h, w) -- source 0 at half the height and width --, w, scale, shift, and chain_ref64's
    single stage on the concatenation built in float64 (source 0 through the x2 nearest map)."""
    dims, chans, cout = row
    n, t, h, w = dims
    name = gather_conv_case(row).name
    srcs = [small_ints(seed, "%s_x%d" % (name, i), (n, ci, t) + ((h // 2, w // 2) if i == 0 else (h, w)), density=0.5) for i, ci in enumerate(chans)]
    x = torch.cat([upsample2x_nchw(srcs[0])] + srcs[1:], dim=1)
    d = {"srcs": srcs, "w": small_ints(seed, name + "w", (cout, sum(chans), 1, 3, 3), density=0.5), "s": pow2_scales(cout), "b": nonzero_ints(seed, name + "b", (cout,))}
    return d, chain_ref64(x, [(d["w"], ONE, P011, d["s"], d["b"], None, True)], dtype)


# ---- the inference max-pool forms and the clip layouts (csrc/pool_layout.hip; tests/test_hip_infer_pool.py) --------------------------------------------------
def maxpool_infer_ref(x, k, s, pf, out_dims, pad_zero):
    """x (n, t, h, w, c) -> (n, to, ho, wo, c), float64 / numpy, from tedspad_pool_desc's semantics: the IEEE maxNum (np.fmax: a NaN beside a number is
    dropped, NaNs alone give NaN) over the window taps that lie inside the input; with `pad_zero`, an output with at least one tap outside is additionally
    max'ed with 0. Front padding `pf`; the back padding is whatever `out_dims` implies."""
    x = x.to(D).numpy()
    n, T, H, W, c = x.shape
    To, Ho, Wo = out_dims
    acc = np.full((n, To, Ho, Wo, c), np.nan)
    outside = np.zeros((To, Ho, Wo), bool)
    for dt in range(k[0]):
        it = np.arange(To) * s[0] - pf[0] + dt
        for dh in range(k[1]):
            ih = np.arange(Ho) * s[1] - pf[1] + dh
            for dw in range(k[2]):
                iw = np.arange(Wo) * s[2] - pf[2] + dw
                ok = ((it >= 0) & (it < T))[:, None, None] & ((ih >= 0) & (ih < H))[None, :, None] & ((iw >= 0) & (iw < W))[None, None, :]
                outside |= ~ok
                if not ok.any():
                    continue
                v = x[:, it.clip(0, T - 1)][:, :, ih.clip(0, H - 1)][:, :, :, iw.clip(0, W - 1)]
                acc = np.where(ok[None, ..., None], np.fmax(acc, v), acc)
    if pad_zero:
        acc = np.where(outside[None, ..., None], np.fmax(acc, 0.0), acc)
    return torch.from_numpy(acc)


def pool_border(thw, k, s, pf, out_dims):
    """(to, ho, wo) bool: the outputs whose window has at least one tap outside the input."""
    m = []
    for size, kk, ss, p, o in zip(thw, k, s, pf, out_dims):
        lo = np.arange(o) * ss - p
        m.append((lo < 0) | (lo + kk > size))
    return torch.from_numpy(m[0][:, None, None] | m[1][None, :, None] | m[2][None, None, :])


K3_NL, K3_NO = 10, 8          # pool_layout.hip: input rows / output rows of a frame tile per thread


def maxpool_form(d, idx=False, no_lds=False):
    """The kernel tedspad_maxpool_fwd_idx launches for the descriptor `d` (anything with tedspad_pool_desc's fields), restated clause by clause from the
    launcher: ('idx',) the fp32 compare-and-select kernel, ('lds', geometry) the frame-band kernel, ('walk', dict(segs, seglen)) the column walk,
    ('generic',) the packed generic kernel. `no_lds`: a process started with TEDSPAD_POOL_NO_LDS. In the geometry, rp_host is the launcher's rows per
    pass, rp_last_group what the kernel recomputes for the last (possibly ragged) channel group, live_last_group its number of working threads."""
    if idx:
        return ("idx",)
    C8 = d.c // 8
    k3 = (d.kt, d.kh, d.kw, d.st, d.sh, d.sw, d.pt, d.ph, d.pw) == (3, 3, 3, 1, 1, 1, 1, 1, 1) and (d.to, d.ho, d.wo) == (d.t, d.h, d.w)
    if not k3:
        return ("generic",)
    CG = C8 if C8 < 8 else 8
    while CG * 2 <= C8 and d.w * CG * 2 <= 128 and d.h * d.w * CG * 2 <= 2048:
        CG *= 2
    rp = 256 // (d.w * CG) if d.w * CG <= 256 else 0
    hb = d.h
    while rp and hb > 1 and (-(-hb // rp) > K3_NO or -(-(hb + 2) // rp) > K3_NL):
        hb -= 1
    bands, cgroups = -(-d.h // hb), -(-C8 // CG)
    lds = 2 * (hb + 2) * (d.w + 2) * CG * 16
    wgs = d.n * bands * cgroups
    clauses = {"rp": rp >= 1, "rows": rp >= 1 and -(-hb // rp) <= K3_NO and -(-(hb + 2) // rp) <= K3_NL, "lds": lds <= 150 * 1024, "wgs": wgs < 1 << 30,
               "offsets": d.h * d.w * max(d.ldx, d.ldy) < 1 << 31, "band": hb >= 4 or hb == d.h}
    if not no_lds and all(clauses.values()):
        ncg = C8 - (cgroups - 1) * CG
        rp_last = 256 // (d.w * ncg)
        return ("lds", dict(CG=CG, HB=hb, bands=bands, cgroups=cgroups, rp_host=rp, rp_last_group=rp_last, live_last_group=rp_last * d.w * ncg,
                            last_band_rows=d.h - (bands - 1) * hb, lds_bytes=lds))
    rows = d.n * d.t * ((d.h + 1) // 2) * C8
    segs = 1
    while rows * segs < 256 * 2048 and -(-d.w // segs) > 4:
        segs += 1
    return ("walk", dict(segs=segs, seglen=-(-d.w // segs), refused=[c for c, v in clauses.items() if not v]))


class InferPoolCase:
    """A row of INFER_POOL_CASES: dims (n, t, h, w), channels, kernel, stride, front padding, back padding (-> the explicit output dims) and the form the row
    is meant to reach."""

    def __init__(self, name, form, dims, c, k=(3, 3, 3), s=(1, 1, 1), pf=(1, 1, 1), pb=(1, 1, 1)):
        self.name, self.form, self.dims, self.c, self.k, self.s, self.pf, self.pb = name, form, dims, c, k, s, pf, pb
        self.n, self.thw = dims[0], tuple(dims[1:])
        self.out = conv_out_dims(self.thw, k, s, pf, pb)

    def desc(self, ldx=None, ldy=None):
        """tedspad_pool_desc's geometry fields as a plain object (what maxpool_form reads)."""
        from types import SimpleNamespace
        (t, h, w), (kt, kh, kw), (st, sh, sw), (pt, ph, pw), (to, ho, wo) = self.thw, self.k, self.s, self.pf, self.out
        return SimpleNamespace(n=self.n, t=t, h=h, w=w, c=self.c, ldx=ldx or self.c + 16, ldy=ldy or self.c + 24, kt=kt, kh=kh, kw=kw, st=st, sh=sh, sw=sw,
                               pt=pt, ph=ph, pw=pw, to=to, ho=ho, wo=wo)

    def geo(self):
        return maxpool_form(self.desc())[1]

    def x(self):
        """Signed multiples of 1/64 in [-1.125, 0.125] (81 values, 72 of them negative): exact in f16 and bf16; zero padding beats most border windows'
        own maximum, and most windows of 4 or more taps still hold a positive value."""
        u = synth_tensor(71, "ip_" + self.name, tuple(self.dims) + (self.c,)).to(D)
        return (torch.floor(u * 81).clamp_(0, 80) - 72) / 64


_Z, _S2 = (0, 0, 0), (2, 2, 2)
INFER_POOL_CASES = [
    # the LDS frame-band form: what each row is there for is asserted by test_kernel_refs.py from maxpool_form alone
    InferPoolCase("lds_cg32_ragged", "lds", (2, 2, 3, 4), 320),              # CG doubled twice (8 -> 32); the last group has 8 of 32: rp 2 -> 8
    InferPoolCase("lds_cg64_near_lds_bound", "lds", (2, 3, 16, 2), 512),     # CG doubled three times; 147456 bytes of LDS, the largest the solver can ask for and get
    InferPoolCase("lds_c8_w40", "lds", (2, 3, 5, 40), 8),                    # C8 = 1 with W > 32: CG = 1, rp 6
    InferPoolCase("lds_c24_w9", "lds", (2, 2, 7, 9), 24),                    # C8 = 3: CG = 3
    InferPoolCase("lds_banded_28_t4", "lds", (2, 4, 28, 28), 200),           # rp 1, four bands, the last of 4 rows; last group 1 of 8: rp 9, 252 live threads; T = 4
    InferPoolCase("lds_banded_odd_t3", "lds", (2, 3, 19, 23), 72),           # rp 1, three bands, the last of 3 rows; last group rp 11, 253 live; T = 3
    InferPoolCase("lds_banded_w9_t2", "lds", (2, 2, 30, 9), 72),             # rp 3, HB 24, two bands; last group 1 of 8: rp 28; T = 2
    InferPoolCase("lds_banded_w9_t1", "lds", (3, 1, 30, 9), 64),             # ... T = 1: both temporal neighbours are padding
    InferPoolCase("lds_w32_t5", "lds", (2, 5, 11, 32), 64),                  # W = 32 with C8 = 8: the last width the form takes; two bands, T = 5
    InferPoolCase("lds_odd_7x7_c832", "lds", (2, 2, 7, 7), 832),             # InceptionI3d's last modules: CG 16, ragged last group (8 of 16)
    InferPoolCase("lds_1x1", "lds", (2, 1, 1, 1), 8),                        # every neighbour is padding
    # the column walk
    InferPoolCase("walk_w33", "walk", (2, 3, 6, 33), 64),                    # the first width that falls to it; segs 9 x seglen 4 = 36 > 33
    InferPoolCase("walk_w40_h5", "walk", (2, 2, 5, 40), 64),                 # H odd: the last pair's second row is absent; segs divides W
    InferPoolCase("walk_h1_w35", "walk", (2, 3, 1, 35), 72),                 # H = 1
    InferPoolCase("walk_lds_bound_w1", "walk", (2, 3, 16, 1), 1024),         # CG 128: 221184 bytes of LDS refused; seglen 1
    InferPoolCase("walk_seglen5", "walk", (64, 1, 1, 33), 8192),             # 2^16 rows: segs stops at 8, seglen 5; the eighth run starts past the row. 35 MB, the smallest such
    # the generic packed kernel: every geometry of test_hip_ops.POOLS that is not 3x3x3 / s1 / p1 ...
    InferPoolCase("gen_2x3x3_s2", "generic", (2, 4, 15, 14), 64, (2, 3, 3), _S2, _Z, _Z),
    InferPoolCase("gen_2x1x1_s2", "generic", (2, 4, 9, 9), 256, (2, 1, 1), (2, 1, 1), _Z, _Z),
    InferPoolCase("gen_1x3x3_s2_same", "generic", (2, 3, 14, 14), 64, (1, 3, 3), (1, 2, 2), _Z, (0, 1, 1)),
    InferPoolCase("gen_3x3x3_s2_same", "generic", (2, 8, 14, 14), 32, (3, 3, 3), _S2, _Z, (1, 1, 1)),
    InferPoolCase("gen_2x2x2_s2_odd", "generic", (2, 4, 7, 7), 64, (2, 2, 2), _S2, _Z, (0, 1, 1)),
    InferPoolCase("gen_1x2x2_s2", "generic", (3, 1, 14, 14), 128, (1, 2, 2), (1, 2, 2), _Z, _Z),
    # ... and one that looks like the fast path but pads two frames at the back instead of one on each side
    InferPoolCase("gen_3x3x3_s1_pt0", "generic", (2, 4, 9, 10), 24, (3, 3, 3), (1, 1, 1), (0, 1, 1), (2, 1, 1)),
]
INFER_POOL_SPECIAL = ("lds_banded_odd_t3", "walk_w33", "gen_3x3x3_s1_pt0", "gen_1x3x3_s2_same")       # the rows that also run with non-finite inputs


def special_values(x):
    """x (n, t, h, w, c >= 16) with non-finite values planted: channels 0-1 NaN in the first and the last corner block (windows of NaNs alone that padding reaches), 2-3 NaN in an
    interior block (... that no padding reaches), 4-5 / 6-7 the same with -inf, +inf at two points of channel 8, and single NaNs among the numbers of
    channels 9 and up."""
    x = x.clone()
    assert x.shape[4] >= 16 and x.shape[1] >= 3
    nan, inf = float("nan"), float("inf")
    H, W = x.shape[2], x.shape[3]
    x[:, 0:3, 0:2, 0:4, 0:2] = nan
    x[:, 0:3, H - 2:, W - 4:, 0:2] = nan
    x[:, 0:3, 1:6, 5:10, 2:4] = nan
    x[:, 0:3, 0:2, 0:4, 4:6] = -inf
    x[:, 0:3, H - 2:, W - 4:, 4:6] = -inf
    x[:, 0:3, 1:6, 5:10, 6:8] = -inf
    x[:, 1, 0, 0, 8] = inf
    x[:, 1, x.shape[2] // 2, x.shape[3] // 2, 8] = inf
    hole = synth_tensor(72, "ip_hole", tuple(x.shape[:4]) + (x.shape[4] - 9,)) < 0.15
    x[..., 9:][hole] = nan
    return x


def clip_layout_refusals(c, w, cpad, strides, ptr_mod16):
    """The clauses of tedspad_clip_to_channels_last's dispatch that keep a clip off the W-contiguous fast path; strides (sn, sc, st, sh, sw) in elements."""
    sn, sc, st, sh, sw = strides
    out = []
    if sw != 1:
        out.append("sw")
    if w % 8 != 0:
        out.append("w8")
    if c > 4:
        out.append("c")
    if ptr_mod16 != 0:
        out.append("ptr")
    if sn % 4 or sc % 4 or st % 4 or sh % 4:
        out.append("stride")
    return out


def clip_layout_form(c, w, cpad, strides, ptr_mod16):
    return "generic" if clip_layout_refusals(c, w, cpad, strides, ptr_mod16) else "w8"


def clip_layout_ref(x, cpad):
    """(n, c, t, h, w) -> (n, t, h, w, cpad) float64 with channels [c, cpad) zero (cpad 4: two pixels per 16 bytes, the same memory order)."""
    n, c, t, h, w = x.shape
    y = torch.zeros((n, t, h, w, cpad), dtype=D)
    y[..., :c] = x.to(D).permute(0, 2, 3, 4, 1)
    return y


class LayoutCase:
    """A view (n, c, t, h, w) of a larger contiguous fp32 clip `big`: per dimension (start, size), W optionally with a step, or of a clip stored with H and W
    swapped (`hw_swapped`: the innermost stride is then H's). The strides and the pointer's offset follow from `big` alone."""

    def __init__(self, name, form, cpad, big, n, c, t, h, w, wstep=1, hw_swapped=False):
        self.name, self.form, self.cpad, self.big, self.sl, self.wstep, self.hw_swapped = name, form, cpad, big, (n, c, t, h, w), wstep, hw_swapped

    def view(self, big):
        """`big`: a contiguous tensor of shape self.big (H and W exchanged if hw_swapped)."""
        if self.hw_swapped:
            big = big.permute(0, 1, 2, 4, 3)
        (n0, n), (c0, c), (t0, t), (h0, h), (w0, w) = self.sl
        return big[n0:n0 + n, c0:c0 + c, t0:t0 + t, h0:h0 + h, w0:w0 + w * self.wstep:self.wstep]

    def storage(self):
        N, C, T, H, W = self.big
        return (N, C, T, W, H) if self.hw_swapped else self.big

    def geometry(self):
        """(c, w, strides, pointer offset in bytes mod 16 from a 16-byte aligned allocation): the arguments of clip_layout_form."""
        v = self.view(torch.empty(self.storage(), dtype=torch.float32))
        return v.shape[1], v.shape[4], tuple(v.stride()), (v.storage_offset() * 4) % 16

    def refusals(self):
        c, w, st, pm = self.geometry()
        return clip_layout_refusals(c, w, self.cpad, st, pm)


def _all(n):
    return (0, n)


LAYOUT_CASES = (
    # the fast path: T-slices and H / W crops of a larger clip (every stride a multiple of 4, the crop starting on a 16-byte boundary), w = 8 and 72
    [LayoutCase("w8_c%d_cpad%d" % (c, cpad), "w8", cpad, (3, 4, 6, 12, 80), (1, 2), (0, c), (1, 4), (3, 7), (4, 72)) for cpad in (4, 8) for c in (1, 2, 3, 4)] +
    [LayoutCase("w8_w8_cpad%d" % cpad, "w8", cpad, (2, 3, 3, 5, 16), _all(2), _all(3), (1, 2), (1, 3), (8, 8)) for cpad in (4, 8)] +
    [LayoutCase("w8_whole_cpad%d" % cpad, "w8", cpad, (2, 3, 2, 5, 24), _all(2), _all(3), _all(2), _all(5), _all(24)) for cpad in (4, 8)] +
    # each refusing clause alone
    [LayoutCase("gen_sw2_cpad%d" % cpad, "generic", cpad, (2, 3, 2, 4, 16), _all(2), _all(3), _all(2), _all(4), (0, 8), wstep=2) for cpad in (4, 8)] +
    [LayoutCase("gen_w6_cpad4", "generic", 4, (2, 3, 2, 4, 8), _all(2), _all(3), _all(2), _all(4), (0, 6)),
     LayoutCase("gen_w7_cpad8", "generic", 8, (2, 3, 2, 4, 8), _all(2), _all(3), _all(2), _all(4), (0, 7)),
     LayoutCase("gen_ptr_cpad4", "generic", 4, (2, 3, 2, 4, 12), _all(2), _all(3), _all(2), _all(4), (1, 8)),
     LayoutCase("gen_ptr_cpad8", "generic", 8, (2, 3, 2, 4, 12), _all(2), _all(3), _all(2), _all(4), (3, 8)),
     LayoutCase("gen_stride_cpad4", "generic", 4, (2, 3, 2, 4, 10), _all(2), _all(3), _all(2), _all(4), (0, 8)),
     LayoutCase("gen_stride_cpad8", "generic", 8, (2, 3, 3, 5, 10), _all(2), _all(3), (1, 2), (1, 3), (0, 8)),
     LayoutCase("gen_c5_cpad8", "generic", 8, (2, 5, 2, 4, 8), _all(2), _all(5), _all(2), _all(4), _all(8)),
     LayoutCase("gen_c8_cpad8", "generic", 8, (2, 8, 2, 4, 8), _all(2), _all(8), _all(2), _all(4), _all(8))] +
    # the generic kernel on the remaining channel counts, odd sizes and a clip stored with H and W exchanged
    [LayoutCase("gen_c%d_cpad%d" % (c, cpad), "generic", cpad, (2, 4, 3, 7, 10), (0, 2), (0, c), (1, 2), (2, 5), (1, 6)) for cpad in (4, 8) for c in (1, 2, 3, 4)] +
    [LayoutCase("gen_hw_swapped_cpad%d" % cpad, "generic", cpad, (2, 3, 4, 6, 8), _all(2), _all(3), _all(4), _all(6), _all(8), hw_swapped=True) for cpad in (4, 8)])


# ---- the weight images, folded BatchNorm vectors and gradient unpack of csrc/pack.hip (tests/test_hip_pack_exact.py) ---------------------------------------
# Restated from the layout comment at the top of pack.hip and the header's documentation, in numpy. The 16-bit roundings are written out here (numpy's own
# float16 for f16, integer arithmetic on the fp32 bits for bf16) and test_kernel_refs.py holds them against torch's conversions.
F16_MAX = 65504.0
PK_FLOATS = 64 * (8 * 27 + 1)              # pack.hip: the largest LDS tile, in floats
PK_FWD_FLOATS = 4096                       # pack.hip: a forward tile holds as many whole rows as fit this
PK_MAX_BLOCKS = 256                        # pack.hip: workgroups per job of a multi-job launch
SENTINEL16 = 0x7E7E                        # what destinations and guards hold before a pack


def _np32(t):
    if t is None:
        return None
    return np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float32)


def round16_bits(v32, dtype):
    """fp32 numpy array -> the int16 bit patterns of the 16-bit type: ONE round-to-nearest-even; f16 clamped to +-65504 first, bf16 not clamped. No NaN / Inf."""
    v32 = np.ascontiguousarray(v32, dtype=np.float32)
    assert bool(np.isfinite(v32).all())
    if dtype == "f16":
        return np.clip(v32, np.float32(-F16_MAX), np.float32(F16_MAX)).astype(np.float16).view(np.int16)
    b = v32.view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16).view(np.int16)


def kernel_form(w, cink, kwk, pair_shift):
    """wk of pack.hip's layout comment: (co, cink, kt, kh, kwk) -- channels zero-padded, or the pixel-pair form wk(n, j*4 + c, dt, dh, d) = w(n, c, dt, dh, 2d + j - shift)."""
    co, ci, kt, kh, kw = w.shape
    wk = np.zeros((co, cink, kt, kh, kwk), dtype=w.dtype)
    if pair_shift < 0:
        assert kwk == kw and cink >= ci
        wk[:, :ci] = w
        return wk
    assert ci <= 4 and cink == 8
    for d in range(kwk):
        for j in range(2):
            k = 2 * d + j - pair_shift
            if 0 <= k < kw:
                wk[:, j * 4:j * 4 + ci, :, :, d] = w[..., k]
    return wk


def pack_image_ref(w, scale, *, cink, kwk, pair_shift, mode, rows, rows_pad, kpad, geo, dtype):
    """The (rows_pad, kpad) int16 bit image tedspad_pack_conv_weights / a tedspad_pack_job writes for the fp32 parameter w (co, ci, kt, kh, kw):
    w * scale[co] is ONE fp32 multiply, then one rounding to the 16-bit type (round16_bits); everything outside [rows) x [K) is +0.
    mode 0: out[n][((dt*KH + dh)*KWk + dw)*CINk + c]; mode 1: out[c][((et*Eh + eh)*Ew + ew)*CO8 + n] with tap = c. + s.*(E. - 1 - e.), geo = (Et,Eh,Ew, ct,ch,cw, st,sh,sw)."""
    w, scale = _np32(w), _np32(scale)
    co, ci, kt, kh, kw = w.shape
    p = w if scale is None else w * scale.reshape(co, 1, 1, 1, 1)                  # float32 * float32 -> float32
    assert p.dtype == np.float32
    wk = kernel_form(p, cink, kwk, pair_shift)
    img = np.zeros((rows_pad, kpad), dtype=np.float32)
    if mode == 0:
        K = kt * kh * kwk * cink
        assert K <= kpad and rows <= co and rows <= rows_pad
        img[:rows, :K] = wk.transpose(0, 2, 3, 4, 1).reshape(co, K)[:rows]
    else:
        Et, Eh, Ew, ct, ch, cw, st, sh, sw = geo
        co8 = (co + 7) // 8 * 8
        assert Et * Eh * Ew * co8 <= kpad and rows <= cink and rows <= rows_pad
        for et in range(Et):
            for eh in range(Eh):
                for ew in range(Ew):
                    dt, dh, dw = ct + st * (Et - 1 - et), ch + sh * (Eh - 1 - eh), cw + sw * (Ew - 1 - ew)
                    k0 = ((et * Eh + eh) * Ew + ew) * co8
                    img[:rows, k0:k0 + co] = wk[:, :rows, dt, dh, dw].T
    return round16_bits(img, dtype)


class PkPlan:
    def __init__(self, tiled, per_tile, tiles):
        self.tiled, self.per_tile, self.tiles = tiled, per_tile, tiles

    def blocks(self, rows_pad, kpad):
        """Workgroups the job gets in a multi-job launch."""
        g = self.tiles if self.tiled else (rows_pad * (kpad // 8) + 1023) // 1024
        return max(1, min(PK_MAX_BLOCKS, g))


def pk_plan_ref(mode, pair_shift, kw, kwk, ci, taps, rows_pad, co8):
    """pk_plan of pack.hip restated: does a job of tedspad_pack_multi go through LDS tiles, how many rows (mode 0) / input channels (mode 1) a tile holds and how
    many tiles it has. Not tiled (pack_body, the gather): pixel-pair forms, forward rows longer than the largest tile, data gradients with more than 27 taps.
    `taps` = kt * kh * kw of the whole kernel, in both modes."""
    if pair_shift >= 0 or kwk != kw:
        return PkPlan(False, 0, 0)
    if mode == 0:
        run = ci * taps
        if run > PK_FLOATS:
            return PkPlan(False, 0, 0)
        R = max(1, min(64, PK_FWD_FLOATS // run))
        return PkPlan(True, R, (rows_pad + R - 1) // R)
    if taps > 27:
        return PkPlan(False, 0, 0)
    C = 32 if taps == 1 else 16 if taps <= 3 else 8
    return PkPlan(True, C, ((rows_pad + C - 1) // C) * ((co8 + 63) // 64))


def fold_ref64(gamma, beta, mean, var, eps, conv_bias=None, n=None):
    """Eval-mode BatchNorm folded to (scale, shift) in numpy float64: scale = gamma / sqrt(var + eps), shift = beta - mean*scale (+ conv_bias*scale).
    gamma None: no BatchNorm -- scale = 1 and shift = conv_bias, or 0 (then `n` gives the length)."""
    f = lambda t: None if t is None else (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).astype(np.float64)
    gamma, beta, mean, var, conv_bias = f(gamma), f(beta), f(mean), f(var), f(conv_bias)
    if gamma is None:
        n = len(conv_bias) if conv_bias is not None else n
        return np.ones(n), (conv_bias if conv_bias is not None else np.zeros(n))
    scale = gamma / np.sqrt(var + np.float64(eps))
    shift = beta - mean * scale
    if conv_bias is not None:
        shift = shift + conv_bias * scale
    return scale, shift


def ulp32(x64):
    """The fp32 spacing at |x| (float64 in, float64 out): 2^(e - 23) for 2^e <= |x| < 2^(e+1), never below the subnormal step 2^-149."""
    a = np.abs(np.asarray(x64, dtype=np.float64))
    _, e = np.frexp(a)                                                      # |x| = m * 2^e, m in [0.5, 1)
    return np.ldexp(1.0, np.where(a == 0, -149, np.maximum(e - 24, -149)))


def wgrad_unpack_ref(dw, co, ci, k, cink, kpad, row_scale=None, grad0=None):
    """grad[n, c, tap] = (grad0 or 0) + dw[n, tap*cink + c] * row_scale[n], float64, shaped (co, ci, kt, kh, kw); dw: the packed [>= co][kpad] accumulator."""
    dw = np.asarray(dw, dtype=np.float64)
    taps = k[0] * k[1] * k[2]
    assert dw.shape[1] == kpad and taps * cink <= kpad and ci <= cink
    g = dw[:co, :taps * cink].reshape(co, taps, cink)[:, :, :ci].transpose(0, 2, 1)
    if row_scale is not None:
        g = g * np.asarray(row_scale, dtype=np.float64)[:co].reshape(co, 1, 1)
    if grad0 is not None:
        g = g + np.asarray(grad0, dtype=np.float64).reshape(co, ci, taps)
    return g.reshape(co, ci, *k)


# values planted into every case's weights (fp32): an f16 tie above an even and above an odd mantissa, the same for bf16, f16 subnormals (one inexact, one a tie, one
# half the smallest subnormal), -0.0, values above 65504 (65520 is the tie between 65504 and what would be +inf) and one just below that tie
PACK_PLANTS = np.array([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 3 * 2.0 ** -11), 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 3.3e-6, 2.5 * 2.0 ** -24,
                        2.0 ** -25, -0.0, 70000.0, -1.0e6, 65520.0, 65519.99], dtype=np.float32)


def pack_weights(shape, seed):
    """(w, scale) fp32 numpy: w random in (-1, 1) with PACK_PLANTS written into output channels 0, 4, 8, ... (co >= 8); scale in +-[0.5, 1.5) with every fourth
    entry exactly 1, so the planted values reach the rounding unchanged with and without the scale."""
    co = shape[0]
    per = int(np.prod(shape[1:]))
    w = synth_tensor(seed, "pack_w", shape, -1, 1).numpy().astype(np.float32).reshape(co, per)
    pos = (synth_tensor(seed, "pack_pos", (len(PACK_PLANTS),)).numpy() * per).astype(np.int64).clip(0, per - 1)
    rows4 = (co + 3) // 4
    for i, v in enumerate(PACK_PLANTS):
        r, c = 4 * (i % rows4), int(pos[i])
        while any(r == 4 * (j % rows4) and c == int(pos[j]) for j in range(i)):       # two plants drew the same slot
            c = (c + 1) % per
        pos[i] = c
        w[r, c] = v
    s = synth_tensor(seed, "pack_s", (co,), 0.5, 1.5).numpy().astype(np.float32)
    s[1::2] *= -1
    s[::4] = 1.0
    return w.reshape(shape), s


def _once_from_exact(x64, dtype):
    """float64 -> the 16-bit type in ONE rounding (as int16 bits, f16 clamped): numpy's float64 -> float16 for f16; for bf16 round to odd into fp32 first
    (fp32 keeps 16 more bits than bf16, so the second rounding then sees exactly which side of a tie the value lies on)."""
    if dtype == "f16":
        return np.clip(x64, -F16_MAX, F16_MAX).astype(np.float16).view(np.int16)
    f = x64.astype(np.float32)
    inexact = f.astype(np.float64) != x64
    away = np.abs(f.astype(np.float64)) > np.abs(x64)
    t = np.where(away, np.nextafter(f, np.float32(0)), f)                   # truncated toward zero
    t = np.where(inexact, (t.view(np.uint32) | np.uint32(1)).view(np.float32), t)
    return round16_bits(t, dtype)


def rounding_ingredients(w, scale, dtype):
    """Counts, over the products the pack rounds, of what makes its arithmetic visible: ties over an even / an odd mantissa (normal range of the type), products whose
    fp32 rounding changes the 16-bit result against rounding the exact product once, f16-subnormal magnitudes, -0.0 and magnitudes above 65504."""
    w = _np32(w)
    co = w.shape[0]
    s = np.ones(co, dtype=np.float32) if scale is None else _np32(scale)
    p = (w.reshape(co, -1) * s.reshape(co, 1)).reshape(-1)
    exact = (w.reshape(co, -1).astype(np.float64) * s.reshape(co, 1).astype(np.float64)).reshape(-1)          # 24 x 24 bits: exact in float64
    b = p.view(np.uint32)
    a = np.abs(p)
    drop = 13 if dtype == "f16" else 16
    normal = (a >= 2.0 ** -14) & (a < F16_MAX) if dtype == "f16" else (a >= 2.0 ** -126)
    tie = normal & ((b & ((1 << drop) - 1)) == (1 << (drop - 1)))
    odd = ((b >> drop) & 1) == 1
    return {"tie_even": int((tie & ~odd).sum()), "tie_odd": int((tie & odd).sum()),
            "double_rounding": int((round16_bits(p, dtype) != _once_from_exact(exact, dtype)).sum()),
            "f16_subnormal": int(((a > 0) & (a < 2.0 ** -14)).sum()), "neg_zero": int(((p == 0) & np.signbit(p)).sum()), "above_f16_max": int((a > F16_MAX).sum())}


class PackCase:
    """One convolution of the weight-image tests: the parameter's shape, its stride / front pads, the stem's pair_w, the kernel-form input dims a DgradPlan is built for,
    and the path each of its images must take in a multi-job launch (checked through pk_plan_ref):
      fwd / dgrad = (tiled, per_tile, over_cap): LDS tiles or pack_body, rows / channels per tile, more tiles than the 256 workgroups of a job;
      class_taps: taps of every parity class of the data gradient; last_chunks: 8-channel chunks of the last 64-wide co tile."""

    def __init__(self, name, shape, stride=ONE, pads=(0, 0, 0), pair_w=None, in_dims=(2, 4, 4), fwd=None, dgrad=None, class_taps=(1,), last_chunks=None):
        self.name, self.shape, self.stride, self.pads, self.pair_w, self.in_dims = name, shape, stride, pads, pair_w, in_dims
        self.fwd, self.dgrad, self.class_taps, self.last_chunks = fwd, dgrad, tuple(class_taps), last_chunks
        co, ci, kt, kh, kw = shape
        self.co8 = (co + 7) // 8 * 8
        if pair_w is None:
            self.cink, self.kwk, self.pair_shift = (ci + 7) // 8 * 8, kw, -1
            self.stride_k, self.pads_k = tuple(stride), tuple(pads)
        else:                                                                       # engine.PackedConv: the pixel-pair form, stride 1 along W
            pw2 = (pair_w + 1) // 2
            self.pair_shift = 2 * pw2 - pair_w
            self.cink, self.kwk = 8, (kw + self.pair_shift + 1) // 2
            self.stride_k, self.pads_k = (stride[0], stride[1], 1), (pads[0], pads[1], pw2)
        self.k_k = (kt, kh, self.kwk)
        self.out_dims = conv_out_dims(in_dims, self.k_k, self.stride_k, self.pads_k, (self.pads_k[0], self.pads_k[1], self.k_k[2] - 1 - self.pads_k[2]) if pair_w is not None else self.pads_k)

    def classes(self):
        """geo = (Et,Eh,Ew, ct,ch,cw, st,sh,sw) of every parity class of the data gradient: the taps c, c + s, ... < k of each residue c of (r + front pad) mod s."""
        out = []
        for rt in range(self.stride_k[0]):
            for rh in range(self.stride_k[1]):
                for rw in range(self.stride_k[2]):
                    c = [(r + pf) % s for r, pf, s in zip((rt, rh, rw), self.pads_k, self.stride_k)]
                    E = [len(range(cc, k, s)) for cc, k, s in zip(c, self.k_k, self.stride_k)]
                    if min(E) > 0:
                        out.append(tuple(E) + tuple(c) + self.stride_k)
        return out

    def image_dims(self, mode, geo=None):
        """(rows, rows_pad, kpad) as tedspad_conv_cout_pad / tedspad_conv_kpad pad them: rows to 128, K to 64."""
        rows = self.shape[0] if mode == 0 else self.cink
        K = self.k_k[0] * self.k_k[1] * self.k_k[2] * self.cink if mode == 0 else geo[0] * geo[1] * geo[2] * self.co8
        return rows, (rows + 127) // 128 * 128, (K + 63) // 64 * 64

    def plan(self, mode, geo=None):
        co, ci, kt, kh, kw = self.shape
        return pk_plan_ref(mode, self.pair_shift, kw, self.kwk, ci, kt * kh * kw, self.image_dims(mode, geo)[1], self.co8)

    def pack_args(self, mode, geo=None):
        """The keyword arguments of pack_image_ref for one image of this case."""
        rows, rows_pad, kpad = self.image_dims(mode, geo)
        return dict(cink=self.cink, kwk=self.kwk, pair_shift=self.pair_shift, mode=mode, rows=rows, rows_pad=rows_pad, kpad=kpad, geo=geo)


BODY = (False, 0, False)
PACK_CASES = [
    PackCase("stem_pairs", (64, 3, 5, 7, 7), (2, 2, 2), (2, 3, 3), pair_w=3, in_dims=(4, 16, 8), fwd=BODY, dgrad=BODY, class_taps=(48, 36, 32, 24)),
    # forward tile of several rows; ci a multiple of 8 but co not (co8 = 24); data-gradient tiles of 8 channels; the four parity classes of a strided 3 x 3
    PackCase("rows_per_tile_co20_s2", (20, 40, 1, 3, 3), (1, 2, 2), (0, 1, 1), fwd=(True, 11, False), dgrad=(True, 8, False), class_taps=(1, 2, 2, 4), last_chunks=3),
    # data-gradient tiles of 16 channels with ci < 16 (and no multiple of 8); co8 = 96: a second co tile with 4 chunks
    PackCase("dgrad_c16_two_co_tiles", (96, 12, 3, 1, 1), ONE, (1, 0, 0), in_dims=(2, 2, 2), fwd=(True, 64, False), dgrad=(True, 16, False), class_taps=(3,), last_chunks=4),
    # data-gradient tiles of 32 channels, the last channel tile partly filled (ci = 72), one parity class, a third co tile with one chunk
    PackCase("dgrad_c32_s2", (136, 72, 1, 1, 1), (1, 2, 2), fwd=(True, 56, False), dgrad=(True, 32, False), class_taps=(1,), last_chunks=1),
    # a forward row longer than PK_FWD_FLOATS: one row per tile, 384 tiles on 256 workgroups; data gradient 80 x 5 = 400 tiles on 256 workgroups
    PackCase("long_rows_over_cap", (300, 520, 1, 3, 3), (1, 2, 2), (0, 1, 1), fwd=(True, 1, True), dgrad=(True, 8, True), class_taps=(1, 2, 2, 4), last_chunks=6),
    # the longest forward row that is still tiled (13 887 floats, ci % 8 != 0), and 8 floats more: pack_body inside the multi-job launch
    PackCase("longest_tiled_row", (16, 1543, 1, 3, 3), ONE, (0, 1, 1), fwd=(True, 1, False), dgrad=(True, 8, False), class_taps=(9,), last_chunks=2),
    PackCase("row_too_long", (16, 1544, 1, 3, 3), ONE, (0, 1, 1), fwd=BODY, dgrad=(True, 8, False), class_taps=(9,), last_chunks=2),
    # plain data gradients with 27 taps (the most that is tiled) and with 49 (pack_body)
    PackCase("dgrad_27_taps", (8, 8, 3, 3, 3), ONE, (1, 1, 1), fwd=(True, 18, False), dgrad=(True, 8, False), class_taps=(27,), last_chunks=1),
    PackCase("dgrad_49_taps", (24, 8, 1, 7, 7), ONE, (0, 3, 3), in_dims=(1, 8, 8), fwd=(True, 10, False), dgrad=BODY, class_taps=(49,)),
    # forward rows per tile capped at 64 with more than 256 tiles; the data gradient has 257 co tiles (the last with 2 chunks)
    PackCase("rows_capped_over_cap", (16400, 8, 1, 1, 1), fwd=(True, 64, True), dgrad=(True, 32, True), class_taps=(1,), last_chunks=2),
]
PACK_BIG = "long_rows_over_cap"            # the job the find_job tables spread 256 workgroups at a time
FIND_JOB_SIZES = (1, 2, 63, 64, 65, 4095, 4096, 4097)
FOLD_C = (1, 255, 256, 257, 2048)


def find_job_rounds(n):
    """Rounds of the 64-ary search over a table of n jobs (1 up to 64, 2 up to 4096, ...)."""
    r = 0
    while n > 1:
        n, r = (n + 63) // 64, r + 1
    return r


def fold_inputs(C, seed):
    """(gamma, beta, mean, var, conv_bias) fp32 numpy: some gamma negative, some var exactly 0."""
    g = synth_tensor(seed, "fold_g", (C,), -1.5, 1.5).numpy().astype(np.float32)
    be = synth_tensor(seed, "fold_b", (C,), -0.5, 0.5).numpy().astype(np.float32)
    m = synth_tensor(seed, "fold_m", (C,), -2.0, 2.0).numpy().astype(np.float32)
    v = synth_tensor(seed, "fold_v", (C,), 0.0, 3.0).numpy().astype(np.float32)
    v[::5] = 0.0
    cb = synth_tensor(seed, "fold_cb", (C,), -1.0, 1.0).numpy().astype(np.float32)
    return g, be, m, v, cb


def fold_shift_bound(ref_shift, beta, mean, scale64, conv_bias=None):
    """|shift - ref64| allowed: the fp32 rounding of a value within a few double ulps of the reference -- 1/2 ulp32(ref) + 4 * 2^-52 * (|beta| + |mean*scale| + |b*scale|).
    (The library is built with -ffp-contract=fast: beta - mean*scale may be one FMA or a multiply and an add.)"""
    mag = np.abs(np.asarray(beta, np.float64)) + np.abs(np.asarray(mean, np.float64) * scale64)
    if conv_bias is not None:
        mag = mag + np.abs(np.asarray(conv_bias, np.float64) * scale64)
    return 0.5 * ulp32(ref_shift) + 4 * 2.0 ** -52 * mag


# ---- MGFN kernels (csrc/mgfn.hip, csrc/mgfn_train.hip): float64 references, each with a per-element bound ---------------------------------------------
# Every reference returns (value, bound) -- or a dict of such pairs -- as float64 tensors. A bound is built as tests/test_hip_head_ops.py builds its own:
# (terms in the sum + a small constant) * 2^-24 * sum |terms| of that element, propagated to first order (and rounded up) through the few operations
# around the sum. The order of an MFMA or butterfly sum is the kernel's business: (n + c) * 2^-24 * sum |terms| holds for ANY order of n terms. The
# reductions over tokens have a chain of MT_CHUNK in-chunk terms plus the number of chunks (chain_tokens), the row kernels one of ceil(C / 256) float4
# loads per lane plus a 6-step butterfly (chain_row). Where a kernel is handed fp32 statistics (ln_apply, ln_bwd, bn_bwd, col_reduce, head_bwd), so is its
# reference: the bound then covers that kernel's own roundings only. expf / erff / logf / sqrtf: K_* * 2^-24 relative, K_* = 10x the worst per-element
# ratio of torch's fp32 CPU result against float64 on the same inputs (measured: exp 1.04, erf 1.05, log 1.03, sqrt 1.07 -- test_kernel_refs.py
# test_mgfn_transcendental_constants measures them again). FLOOR32, the smallest normal fp32, is added to every bound: a result below it may be flushed.
U = F32_EPS
K_EXP = K_ERF = K_LOG = K_SQRT = 11.0
FLOOR32 = 2.0 ** -126
MT_CHUNK = 128
SQRT1_2, INV_SQRT_2PI, TWO_OVER_SQRT_PI = 0.5 ** 0.5, 1.0 / (2.0 * np.pi) ** 0.5, 2.0 / np.pi ** 0.5


def f32(v):
    """a float kernel argument as the kernel receives it"""
    return float(np.float32(v))


def chain_tokens(M):
    return MT_CHUNK + (M + MT_CHUNK - 1) // MT_CHUNK


def chain_row(C):
    return 4 * ((C + 255) // 256) + 6


def mgfn_ragged(lengths):
    """sequence offsets (list, nseq + 1) and bounds (M, 2) int64: first / one-past-last token of each token's sequence."""
    L = torch.tensor(list(lengths), dtype=torch.int64)
    off = torch.zeros(len(L) + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(L, 0)
    st = off[:-1].repeat_interleave(L)
    return off.tolist(), torch.stack([st, st + L.repeat_interleave(L)], 1)


# The torch restatements the two older MGFN test files (test_hip_mgfn.py, test_hip_mgfn_train_kernels.py) compare with, in the dtype they are handed; the
# references below are held to them in float64 (test_kernel_refs.py).
def mgfn_seqs(x, off):
    return [x[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def mgfn_conv_seq(x, w, b, taps):
    """x (T, cin) one sequence, w (N, taps, cin) -> Conv1d(padding = taps // 2) over time"""
    return F.conv1d(x.t().unsqueeze(0), w.permute(0, 2, 1), b, padding=taps // 2)[0].t()


def mgfn_conv_tokens(x, off, w, b, taps):
    return torch.cat([mgfn_conv_seq(s, w, b, taps) for s in mgfn_seqs(x, off)])


def mgfn_conv_autograd(x, w, b, taps, off, dy):
    """(dx, dw, db) of sum(conv(x) * dy) by autograd in x's dtype."""
    x, w, b = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    (mgfn_conv_tokens(x, off, w, b, taps) * dy).sum().backward()
    return x.grad, w.grad, b.grad


def mgfn_attention_torch(qkv, off, heads, dt=D, do=None):
    """softmax attention per sequence and head (qkv rows = q | k | v, each heads x 64) in dtype dt; with do: (out, d qkv) by autograd."""
    x = qkv.to(dt).clone().requires_grad_(do is not None)
    inner, outs = 64 * heads, []
    for s in mgfn_seqs(x, off):
        T = s.shape[0]
        q, k, v = (t.reshape(T, heads, 64).transpose(0, 1) for t in s.chunk(3, dim=1))
        outs.append((torch.softmax((q * 0.125) @ k.transpose(1, 2), -1) @ v).transpose(0, 1).reshape(T, inner))
    out = torch.cat(outs)
    if do is None:
        return out.detach()
    (out * do.to(dt)).sum().backward()
    return out.detach(), x.grad


def mgfn_relpos_torch(v, w, b, off, heads, dt=D, do=None):
    """FOCUS rel_pos (utils.py:144-146: 'b (c h) t -> (b c) h t' gives channel ch the filter of head ch % heads) as a grouped Conv1d per sequence in dtype dt;
    with do: (out, dv, dw, db) by autograd."""
    C = v.shape[1]
    vd, wd, bd = (t.to(dt).clone().requires_grad_(do is not None) for t in (v, w, b))
    wf, bf = wd.repeat(C // heads, 1).unsqueeze(1), bd.repeat(C // heads)
    y = torch.cat([F.conv1d(s.t().unsqueeze(0), wf, bf, padding=2, groups=C)[0].t() for s in mgfn_seqs(vd, off)])
    if do is None:
        return y.detach()
    (y * do.to(dt)).sum().backward()
    return y.detach(), vd.grad, wd.grad, bd.grad


def mgfn_window(x, bounds, taps, wrong=None):
    """(M, taps, C): A[m, t] = x[m + t - taps // 2] inside m's sequence, else 0 (bounds None: every token its own sequence). wrong = 'leak': a tap stops at
    the ends of the batch only; 'reversed': tap t reads m - t + taps // 2."""
    x = x.to(D)
    M = x.shape[0]
    m = torch.arange(M)
    lo, hi = (m, m + 1) if bounds is None else (bounds[:, 0].long(), bounds[:, 1].long())
    A = torch.zeros((M, taps, x.shape[1]), dtype=D)
    for t in range(taps):
        src = m + t - taps // 2
        ok = (src >= 0) & (src < M) if wrong == "leak" else (src >= lo) & (src < hi)
        A[ok, taps - 1 - t if wrong == "reversed" else t] = x[src[ok]]
    return A


def mgfn_gelu_ref(v):
    """y = v Phi(v) = 0.5 v (1 + erf(v / sqrt 2)). Bound: the argument v / sqrt 2 carries 2 roundings (the constant, the product): erf moves by at most
    erf'(a) |a| 2u; erff itself K_ERF u |erf|; 1 + erf one rounding; the two products one each (0.5 v is exact)."""
    v = v.to(D)
    a = v * SQRT1_2
    e = torch.erf(a)
    y = 0.5 * v * (1.0 + e)
    de = TWO_OVER_SQRT_PI * torch.exp(-a * a) * a.abs() * 2 * U + K_ERF * U * e.abs() + U * (1.0 + e).abs()
    return y, 0.5 * v.abs() * de + 2 * U * y.abs() + FLOOR32


def mgfn_gelu_bwd_ref(v, dy):
    """dx = dy (Phi(v) + v phi(v)), phi(v) = exp(-v^2 / 2) / sqrt(2 pi). Bound: Phi as in mgfn_gelu_ref; the argument of expf carries 2 roundings
    (|arg| 2u relative in the result), expf K_EXP u, three products; the sum and the product with dy one rounding each."""
    v, dy = v.to(D), dy.to(D)
    a = v * SQRT1_2
    e = torch.erf(a)
    Phi = 0.5 * (1.0 + e)
    dPhi = 0.5 * (TWO_OVER_SQRT_PI * torch.exp(-a * a) * a.abs() * 2 * U + K_ERF * U * e.abs() + U * (1.0 + e).abs()) + U * Phi
    t = v * INV_SQRT_2PI * torch.exp(-0.5 * v * v)
    dt = t.abs() * (K_EXP * U + v * v * U + 3 * U)
    dx = dy * (Phi + t)
    return dx, dy.abs() * (dPhi + dt + U * (Phi + t).abs()) + U * dx.abs() + FLOOR32


def mgfn_gemm_ref(x, bounds, taps, w, bias=None, gelu=False, res=None, stats=None, wrong=None):
    """tedspad_mgfn_gemm: y[m, n] = sum_{t, c} A[m, t, c] w[n, t cin + c] + bias[n], then GELU, then + res. x (M, cin), w (N, taps * cin); stats (M, 2)
    fp32 as handed (taps == 1): A = (x - mean) rs. Bound: z = the sum: (K + 2) u sum |A||w| with K = taps * cin (any order; + 2: the bias add and slack),
    plus, with stats, the two roundings of every A element, u ((|x| + |mean|) |rs| + |A|), through |w|. GELU: its slope is at most 1.13, so 1.14 dz,
    plus its own evaluation (mgfn_gelu_ref). Residual: one rounding of the sum, u (|y| + |res|)."""
    A = mgfn_window(x, bounds, taps, wrong)
    M, K = A.shape[0], taps * A.shape[2]
    Aerr = torch.zeros_like(A)
    if stats is not None:
        mu, rs = stats[:, 0].to(D).view(M, 1, 1), stats[:, 1].to(D).view(M, 1, 1)
        A0 = A
        A = (A0 - mu) * rs
        Aerr = U * ((A0.abs() + mu.abs()) * rs.abs() + A.abs())
    w = w.to(D).reshape(-1, K)
    z = A.reshape(M, K) @ w.t()
    za = A.reshape(M, K).abs() @ w.abs().t()
    if bias is not None:
        z, za = z + bias.to(D), za + bias.to(D).abs()
    b = (K + 2) * U * za + Aerr.reshape(M, K) @ w.abs().t()
    if gelu:
        z, be = mgfn_gelu_ref(z)
        b = 1.14 * b + be
    if res is not None:
        b = b + U * (z.abs() + res.to(D).abs())
        z = z + res.to(D)
    return z, b + FLOOR32


def mgfn_ln_stats_ref(x, eps, torch_ln):
    """tedspad_mgfn_ln_stats: mean, rs = 1 / (std + eps) (MGFN) or 1 / sqrt(var + eps) (nn.LayerNorm), biased variance. Returns mean, rs, dmean, drs.
    n = chain_row(C). dmean = (n + 2) u sum |x| / C. The second pass sums (x - mean~)^2 around the COMPUTED mean: sum (x - mean~)^2 / C = var + (mean -
    mean~)^2 exactly, so dvar = dmean^2 + (n + 4) u (var + dmean^2) (each term: 2 roundings of the difference squared, one of the product). A one-pass
    E[x^2] - mean^2 does not meet this. sqrt: |sqrt a~ - sqrt a| <= min(|a~ - a| / sqrt a, sqrt |a~ - a|), + K_SQRT u; the adds one rounding each; the
    reciprocal: d(1 / den) <= dden / (den (den - dden)) + u / den."""
    x = x.to(D)
    C, n, eps = x.shape[1], chain_row(x.shape[1]), f32(eps)
    mu = x.mean(1)
    dmu = (n + 2) * U * x.abs().sum(1) / C
    var = ((x - mu[:, None]) ** 2).mean(1)
    dvar = dmu ** 2 + (n + 4) * U * (var + dmu ** 2)
    if torch_ln:
        den = (var + eps).sqrt()
        dden = (dvar + U * (var + eps)) / den + K_SQRT * U * den
    else:
        std = var.sqrt()
        den = std + eps
        dden = torch.minimum(dvar / std.clamp_min(1e-300), dvar.sqrt()) + K_SQRT * U * std + U * den
    rs = 1.0 / den
    drs = torch.where(dden < den, dden / (den * (den - dden).clamp_min(1e-300)), torch.full_like(den, float("inf"))) + U * rs
    return mu, rs, dmu, drs


def mgfn_ln_apply_ref(x, stats, g, b):
    """tedspad_mgfn_ln_apply with the fp32 stats it is handed: y = (x - mean) rs g + b. Bound: the difference one rounding, u (|x| + |mean|) |rs g|; two
    products and the add: 3 u |(x - mean) rs g| + u |y|."""
    x, g, b = x.to(D), g.to(D), b.to(D)
    mu, rs = stats[:, 0:1].to(D), stats[:, 1:2].to(D)
    t = (x - mu) * rs * g
    return t + b, U * (x.abs() + mu.abs()) * (rs * g).abs() + 3 * U * t.abs() + U * (t + b).abs() + FLOOR32


def mgfn_ln_bwd_ref(dy, x, stats, g, torch_ln, eps, add=None):
    """tedspad_mgfn_ln_bwd with the fp32 stats it is handed. d = dy g, xh = (x - mean) rs, s1 = mean_c d, s2 = mean_c d xh, k = rs (nn.LayerNorm) or
    1 / (1 / rs - eps) (MGFN: 1 / std), dx = (d - s1) rs - xh s2 k (+ add). Bound, n = chain_row(C): exh = u ((|x| + |mean|) |rs| + |xh|); ds1 = (n + 2) u
    mean |d|; ds2 = (n + 3) u mean |d xh| + mean |d| exh; MGFN: 1 / rs and the subtraction round once each, dsd = u (|1 / rs| + |sd|), dk = |k| (dsd / |sd|)
    / (1 - dsd / |sd|) + u |k|; then every product and difference one rounding. A constant row has sd = 0 in the MGFN flavour: the reference divides by
    zero there as the formula does (inf / nan)."""
    dy, x, g = dy.to(D), x.to(D), g.to(D)
    C, n, eps = x.shape[1], chain_row(x.shape[1]), f32(eps)
    mu, rs = stats[:, 0:1].to(D), stats[:, 1:2].to(D)
    xh = (x - mu) * rs
    exh = U * ((x.abs() + mu.abs()) * rs.abs() + xh.abs())
    d = dy * g
    s1 = d.mean(1, keepdim=True)
    ds1 = (n + 2) * U * d.abs().mean(1, keepdim=True)
    s2 = (d * xh).mean(1, keepdim=True)
    ds2 = (n + 3) * U * (d * xh).abs().mean(1, keepdim=True) + (d.abs() * exh).mean(1, keepdim=True)
    if torch_ln:
        k, dk = rs, torch.zeros_like(rs)
    else:
        inv = 1.0 / rs
        sd = inv - eps
        k = 1.0 / sd
        r = U * (inv.abs() + sd.abs()) / sd.abs()
        dk = k.abs() * r / (1.0 - r) + U * k.abs()
    k2 = s2 * k
    dk2 = ds2 * k.abs() + s2.abs() * dk + U * k2.abs()
    t1 = (d - s1) * rs
    e1 = rs.abs() * (U * d.abs() + ds1 + U * (d - s1).abs()) + U * t1.abs()
    t2 = xh * k2
    e2 = exh * k2.abs() + xh.abs() * dk2 + U * t2.abs()
    dx = t1 - t2
    b = e1 + e2 + U * (t1.abs() + t2.abs())
    if add is not None:
        dx = dx + add.to(D)
        b = b + U * (dx.abs() + add.to(D).abs())
    return dx, b + FLOOR32


def _inv_sqrt(var, dvar, eps):
    """1 / sqrt(var + eps) and its bound (see mgfn_ln_stats_ref)."""
    den = (var + eps).sqrt()
    dden = (dvar + U * (var + eps)) / den + K_SQRT * U * den
    inv = 1.0 / den
    return inv, torch.where(dden < den, dden / (den * (den - dden).clamp_min(1e-300)), torch.full_like(den, float("inf"))) + U * inv


def mgfn_bn_fwd_ref(x, gamma, beta, eps, momentum, running_mean=None, running_var=None, wrong=None):
    """tedspad_mgfn_bn_train_fwd: nn.BatchNorm1d over all M tokens in train mode. M = 1: the kernel's documented rule, running_var takes the biased
    variance (0). Returns a dict of (value, bound): y, mean, invstd, running_mean, running_var. n = chain_tokens(M): dmean = (n + 2) u sum |x| / M;
    dvar = dmean^2 + (n + 5) u (var + dmean^2) (the second pass is centred on the computed mean: see mgfn_ln_stats_ref); invstd: _inv_sqrt; y = xh gamma +
    beta with dxh = (dmean + u (|x| + |mean|)) invstd + |x - mean| dinvstd + u |xh|, then |gamma| dxh + 2 u |xh gamma| + u |y|; the running statistics:
    momentum times the error of the statistic (the variance times M / (M - 1)), plus 3 u on each term. wrong = 'biased_running_var'."""
    x, gamma, beta = x.to(D), gamma.to(D), beta.to(D)
    M, n, eps, mom = x.shape[0], chain_tokens(x.shape[0]), f32(eps), f32(momentum)
    mean = x.mean(0)
    dmu = (n + 2) * U * x.abs().sum(0) / M
    d = x - mean
    var = (d * d).mean(0)
    dvar = dmu ** 2 + (n + 5) * U * (var + dmu ** 2)
    inv, dinv = _inv_sqrt(var, dvar, eps)
    xh = d * inv
    dxh = (dmu + U * (x.abs() + mean.abs())) * inv + d.abs() * dinv + U * xh.abs()
    t = xh * gamma
    out = {"y": (t + beta, gamma.abs() * dxh + 2 * U * t.abs() + U * (t + beta).abs() + FLOOR32), "mean": (mean, dmu + U * mean.abs() + FLOOR32),
           "invstd": (inv, dinv + FLOOR32), "running_mean": None, "running_var": None}
    if running_mean is not None:
        rm, rv = running_mean.to(D), running_var.to(D)
        f = M / (M - 1.0) if (M > 1 and wrong != "biased_running_var") else 1.0
        out["running_mean"] = ((1 - mom) * rm + mom * mean, mom * dmu + 3 * U * ((1 - mom) * rm.abs() + mom * mean.abs()) + FLOOR32)
        out["running_var"] = ((1 - mom) * rv + mom * var * f, mom * f * (dvar + 2 * U * var) + 3 * U * ((1 - mom) * rv.abs() + mom * var * f) + FLOOR32)
    return out


def mgfn_bn_bwd_ref(dy, x, stat, gamma, add=None):
    """tedspad_mgfn_bn_train_bwd with the fp32 stat (mean | invstd, 2 C) it is handed: dbeta = sum dy, dgamma = sum dy xh, dx = gamma invstd (dy - dbeta / M
    - xh dgamma / M) (+ add). Returns a dict of (value, bound). n = chain_tokens(M): ddbeta = (n + 1) u sum |dy|; exh = u ((|x| + |mean|) invstd + |xh|);
    ddgamma = (n + 2) u sum |dy xh| + sum |dy| exh; dx from the COMPUTED sums: their errors / M, exh |dgamma| / M, and 3 u on each of the three terms (1 / M,
    the products, the differences); the outer products 2 u, the add one."""
    dy, x, gamma = dy.to(D), x.to(D), gamma.to(D)
    M, C = x.shape
    n = chain_tokens(M)
    mean, inv = stat[:C].to(D), stat[C:].to(D)
    xh = (x - mean) * inv
    exh = U * ((x.abs() + mean.abs()) * inv.abs() + xh.abs())
    dbeta, ddb = dy.sum(0), (n + 1) * U * dy.abs().sum(0)
    dgamma, ddg = (dy * xh).sum(0), (n + 2) * U * (dy * xh).abs().sum(0) + (dy.abs() * exh).sum(0)
    inner = dy - dbeta / M - xh * dgamma / M
    einner = ddb / M + exh * dgamma.abs() / M + xh.abs() * ddg / M + 3 * U * (dy.abs() + dbeta.abs() / M + (xh * dgamma).abs() / M)
    gi = gamma * inv
    dx = gi * inner
    b = gi.abs() * einner + 2 * U * dx.abs()
    if add is not None:
        dx = dx + add.to(D)
        b = b + U * (dx.abs() + add.to(D).abs())
    return {"dx": (dx, b + FLOOR32), "dgamma": (dgamma, ddg + FLOOR32), "dbeta": (dbeta, ddb + FLOOR32)}


def mgfn_head_ref(x, ln_w, ln_b, fc_w, fc_b, eps):
    """tedspad_mgfn_head: h = nn.LayerNorm(C)(x), logit = h . fc_w + fc_b, score = sigmoid(logit), mag = ||h||_2. Returns a dict of (value, bound).
    Statistics and their errors: mgfn_ln_stats_ref (torch flavour). dxh = (dmean + u (|x| + |mean|)) rs + |x - mean| drs + u |xh|; dh = |ln_w| dxh + u |xh
    ln_w| + u |h|; dlogit = sum dh |fc_w| + (n + 3) u (sum |h fc_w| + |fc_b|); score = 1 / (1 + exp(-z)): a relative error r of the exponential moves it by
    s (1 - s) r, so s (1 - s) (dlogit + K_EXP u) (1 + 2 (dlogit + K_EXP u)) + 3 u s; mag: dn2 = sum (2 |h| dh + dh^2) + (n + 3) u sum h^2, then min(dn2 /
    mag, sqrt dn2) + K_SQRT u mag."""
    x, lw, lb, fw = x.to(D), ln_w.to(D), ln_b.to(D), fc_w.to(D)
    n, fb = chain_row(x.shape[1]), f32(fc_b)
    mu, rs, dmu, drs = mgfn_ln_stats_ref(x, eps, 1)
    mu, rs, dmu, drs = (t[:, None] for t in (mu, rs, dmu, drs))
    d = x - mu
    xh = d * rs
    dxh = (dmu + U * (x.abs() + mu.abs())) * rs + d.abs() * drs + U * xh.abs()
    t = xh * lw
    h = t + lb
    dh = lw.abs() * dxh + U * t.abs() + U * h.abs() + FLOOR32
    z = (h * fw).sum(1) + fb
    dz = (dh * fw.abs()).sum(1) + (n + 3) * U * ((h * fw).abs().sum(1) + abs(fb)) + FLOOR32
    s = torch.sigmoid(z)
    r = dz + K_EXP * U
    ds = s * (1 - s) * r * (1 + 2 * r) + 3 * U * s + FLOOR32
    n2 = (h * h).sum(1)
    dn2 = (2 * h.abs() * dh + dh * dh).sum(1) + (n + 3) * U * n2
    mag = n2.sqrt()
    dmag = torch.minimum(dn2 / mag.clamp_min(1e-300), dn2.sqrt()) + K_SQRT * U * mag + FLOOR32
    return {"h": (h, dh), "logit": (z, dz), "score": (s, ds), "mag": (mag, dmag)}


def mgfn_head_bwd_ref(score, dscore, fc_w, dh):
    """tedspad_mgfn_head_bwd with the fp32 score it is handed: dz = dscore s (1 - s), dh += fc_w dz. Returns (dh, bound), (dz, bound). 1 - s rounds once
    (absolute u |1 - s| <= u): u |dscore s| + 3 u |dz|; dh: |fc_w| ddz + u |fc_w dz| + u |dh|."""
    s, ds, fw, dh = score.to(D), dscore.to(D), fc_w.to(D), dh.to(D)
    z = ds * s * (1 - s)
    dz = U * (ds * s).abs() + 3 * U * z.abs() + FLOOR32
    out = dh + fw * z[:, None]
    return (out, fw.abs() * dz[:, None] + U * (fw * z[:, None]).abs() + U * out.abs() + FLOOR32), (z, dz)


def mgfn_crop_mean_ref(a, seg_off, ncrops):
    """tedspad_mgfn_crop_mean: out[seg_off[v] + t] = mean_c a[ncrops seg_off[v] + c T_v + t]. Bound: (ncrops + 1) u mean |a|."""
    a = a.to(D)
    outs, bs = [], []
    for v in range(len(seg_off) - 1):
        s0, T = seg_off[v], seg_off[v + 1] - seg_off[v]
        blk = a[ncrops * s0:ncrops * s0 + ncrops * T].view(ncrops, T)
        outs.append(blk.mean(0))
        bs.append((ncrops + 1) * U * blk.abs().mean(0) + FLOOR32)
    return torch.cat(outs), torch.cat(bs)


def mgfn_col_reduce_ref(a, mode, scale=1.0, x=None, st=None, wrong=None):
    """tedspad_mgfn_col_reduce, with the fp32 st it is handed. (out0, bound0), (out1, bound1), each (C):
    0: scale sum a | 0;  1: scale sum a | scale sum a (x - st[m, 0]) st[m, 1];  2: the same with the per-column st[c], st[C + c];  3: scale sum (a -
    st[c])^2 | 0 (st None: mode 0);  4: scale sum st[m] a | scale sum st[m]. Bound, n = chain_tokens(M): (n + 2) u |scale| sum |terms| (any order inside the
    chunk and over the chunks; + 2: the scale), plus per term the roundings that make it: xh = (x - mean) rs: u ((|x| + |mean|) |rs| + |xh|) times |a|, and
    u |a xh|; (a - st)^2: 3 u; st[m] a: u. wrong = 'skip_last_chunk': a last partial chunk of MT_CHUNK tokens is left out."""
    a = a.to(D)
    M, C = a.shape
    n, scale = chain_tokens(M), f32(scale)
    if mode == 3 and st is None:
        mode = 0
    zero = torch.zeros_like(a)
    if mode == 0:
        t0, e0, t1, e1 = a, zero, zero, zero
    elif mode in (1, 2):
        st = st.to(D)
        mu, rs = (st[:, 0:1], st[:, 1:2]) if mode == 1 else (st[:C], st[C:])
        xh = (x.to(D) - mu) * rs
        t0, e0, t1 = a, zero, a * xh
        e1 = a.abs() * U * ((x.to(D).abs() + mu.abs()) * rs.abs() + xh.abs()) + U * t1.abs()
    elif mode == 3:
        d = a - st.to(D)[:C]
        t0, e0, t1, e1 = d * d, 3 * U * d * d, zero, zero
    else:
        r = st.to(D)[:M, None]
        t0, e0, t1, e1 = r * a, U * (r * a).abs(), r.expand(M, C), zero
    rows = M - M % MT_CHUNK if (wrong == "skip_last_chunk" and M % MT_CHUNK) else M
    out = []
    for t, e in ((t0, e0), (t1, e1)):
        out.append((scale * t[:rows].sum(0), abs(scale) * ((n + 2) * U * t.abs().sum(0) + e.sum(0)) + FLOOR32))
    return out


def mgfn_transpose_ref(x, bounds, taps, ldo):
    """tedspad_mgfn_transpose: out[(t C + c), m] = x[m + t - taps // 2, c] inside m's sequence, 0 outside and for M <= m < ldo. A copy: exact."""
    A = mgfn_window(x, bounds, taps)
    M, _, C = A.shape
    out = torch.zeros((taps * C, ldo), dtype=D)
    out[:, :M] = A.permute(1, 2, 0).reshape(taps * C, M)
    return out


def mgfn_wgrad_slices(ldk, rows, N):
    """(kslice, nslices) of tedspad_mgfn_wgrad, the launcher's own formula: enough slices for ~2048 waves, at least 128 tokens each."""
    tiles = ((rows + 63) // 64) * (N // 64)
    want = max(1, min((2048 + tiles - 1) // tiles, (ldk + 127) // 128))
    ks = ((ldk + want - 1) // want + 15) // 16 * 16
    return ks, (ldk + ks - 1) // ks


def mgfn_wgrad_ref(at, dyt):
    """tedspad_mgfn_wgrad: dwt (rows, N) = at (rows, ldk) . dyt (N, ldk)^T over the token axis. Bound: (ldk + slices + 2) u sum |at||dyt| (any order)."""
    at, dyt = at.to(D), dyt.to(D)
    ldk = at.shape[1]
    ns = mgfn_wgrad_slices(ldk, at.shape[0], dyt.shape[0])[1]
    return at @ dyt.t(), (ldk + ns + 2) * U * (at.abs() @ dyt.abs().t()) + FLOOR32


def _head_of(C, heads, wrong=None):
    c = torch.arange(C)
    return c // (C // heads) if wrong == "head_block" else c % heads


def mgfn_relpos_ref(v, bounds, heads, w, b, wrong=None):
    """tedspad_mgfn_relpos: out[m, c] = b[c % heads] + sum_t w[c % heads, t] v[m + t - 2, c], zero outside the sequence. Bound: 7 u (|b| + sum |w||v|).
    wrong = 'head_block': the filter of head c / (C / heads); 'leak': taps cross the sequence ends."""
    A = mgfn_window(v, bounds, 5, "leak" if wrong == "leak" else None)
    hd = _head_of(A.shape[2], heads, wrong)
    wc, bc = w.to(D)[hd].t(), b.to(D)[hd]                                   # (5, C), (C)
    return (A * wc).sum(1) + bc, 7 * U * ((A * wc).abs().sum(1) + bc.abs()) + FLOOR32


def mgfn_relpos_bwd_ref(dout, v, bounds, heads, w):
    """tedspad_mgfn_relpos_bwd: dv[m, c] = sum_t w[c % heads, t] dout[m - t + 2, c]; dw[h, j] = sum over m and the channels of head h of dout[m, c]
    v[m + j - 2, c]; db[h] = the same sum of dout. Returns (dv, bound), (dw, bound), (db, bound). dv: 7 u sum |w||dout|. dw, db: the chain is MT_CHUNK
    tokens in a chunk, then ceil(chunks * C / heads / 256) entries per thread and an 8-step tree: (that + 2) u sum |terms|."""
    dout = dout.to(D)
    M, C = dout.shape
    hd = _head_of(C, heads)
    wc = w.to(D)[hd].t()
    B = mgfn_window(dout, bounds, 5).flip(1)                            # B[m, t] = dout[m - t + 2]
    dv = (B * wc).sum(1)
    A = mgfn_window(v, bounds, 5)
    terms = dout[:, None, :] * A                                        # (M, 5, C)
    nch, per = (M + MT_CHUNK - 1) // MT_CHUNK, C // heads
    n = MT_CHUNK + (nch * per + 255) // 256 + 8 + 2
    sel = torch.zeros((C, heads), dtype=D)
    sel[torch.arange(C), hd] = 1.0
    dw, dwa = (terms.sum(0) @ sel).t(), (terms.abs().sum(0) @ sel).t()   # (heads, 5)
    db, dba = dout.sum(0) @ sel, dout.abs().sum(0) @ sel
    return (dv, 7 * U * (B * wc).abs().sum(1) + FLOOR32), (dw, n * U * dwa + FLOOR32), (db, n * U * dba + FLOOR32)


def _att_rows(q, k, wrong=None):
    """Per (sequence, head): logits S = (q / 8) k^T with their bound dS = 66 u sum |q / 8||k| (64 products, any order, + 2), the row maximum, the logit range R
    (+ 2 max dS: the computed logits), the key blocks nb, and row = u (R + K_EXP + nb (K_EXP + R + 3)): the relative error of one unnormalised weight exp(s - m)
    beyond dS: the subtraction (u |s - m| <= u R), expf, and per key block one rescale by exp(m_old - m_new) (argument u R, expf, two products)."""
    T = q.shape[0]
    qs = q * (1.0 if wrong == "no_scale" else 0.125)
    S = qs @ k.t()
    dS = 66 * U * (qs.abs() @ k.abs().t())
    nb = (T + 31) // 32
    R = S.max(1).values - S.min(1).values + 2 * dS.max(1).values
    return qs, S, dS, nb, R, U * (R + K_EXP + nb * (K_EXP + R + 3))


def mgfn_attention_ref(qkv, off, heads, wrong=None):
    """tedspad_mgfn_attention: out[m, h 64 + d] = sum_j softmax_j((q_m / 8) . k_j) v_j[d] over m's sequence; qkv rows = q | k | v, each heads x 64. Bound: with
    eps_ij = expm1(dS_ij) + row_i the relative error of weight j of row i (_att_rows), the numerator sum_j e_j v_jd (T terms on the MFMA) is off by
    sum_j e_j |v_jd| (eps_ij + (T + 2) u), the denominator by sum_j e_j eps_ij + (T + nb + 3) u sum_j e_j; so |out~ - out| <= sum_j p_j |v_jd| (eps_ij + (T + 2) u)
    + (sum_j p_j |v_jd|) (sum_j p_j eps_ij + (T + nb + 3) u), times 1 + 4 max eps for the second order. wrong = 'no_scale': softmax of q . k; 'drop_block':
    the last (partial) key block of a sequence longer than 32 is left out."""
    qkv = qkv.to(D)
    M, inner = qkv.shape[0], 64 * heads
    out, bnd = torch.zeros((M, inner), dtype=D), torch.zeros((M, inner), dtype=D)
    for s in range(len(off) - 1):
        b0, b1 = off[s], off[s + 1]
        T = b1 - b0
        for h in range(heads):
            q, k, v = (qkv[b0:b1, j * inner + h * 64:j * inner + (h + 1) * 64] for j in range(3))
            if wrong == "drop_block" and T > 32:
                keep = (T - 1) // 32 * 32
                k, v = k[:keep], v[:keep]
            _, S, dS, nb, R, row = _att_rows(q, k, wrong)
            p = torch.softmax(S, 1)
            eps = torch.expm1(dS) + row[:, None]
            pv = p @ v.abs()
            b = (p * (eps + (T + 2) * U)) @ v.abs() + pv * ((p * eps).sum(1) + (T + nb + 3) * U)[:, None]
            out[b0:b1, h * 64:(h + 1) * 64] = p @ v
            bnd[b0:b1, h * 64:(h + 1) * 64] = b * (1 + 4 * float(eps.max())) + FLOOR32
    return out, bnd


def mgfn_attention_bwd_ref(qkv, o, dO, off, heads):
    """tedspad_mgfn_attention_bwd with the fp32 forward output o it is handed. P = softmax(S), D_i = dO_i . o_i, dP = dO V^T, dS = P (dP - D), dq = dS K / 8,
    dk = dS^T q / 8, dv = P^T dO; lse (M, heads, 2) = the row's log-sum-exp L and D. Returns (dqkv (M, 3 inner), bound), (lse, bound).
    dL = max_j dS_ij + row_i + (T + 2) u (the sum of the weights) + K_LOG u |log l| + u |L|; the recomputed p~ = exp(s~ - L~): epsP = expm1(dS) + dL +
    u |s - L| + K_EXP u relative; dD = 66 u sum |dO||o|, ddP = 66 u sum |dO||v|; ddS = p (epsP |dP - D| + ddP + dD + u (|dP| + |D|)) + 2 u |dS|; then each
    product over T terms: dq: (sum_j ddS |k| + (T + 3) u sum_j |dS||k|) / 8, dk alike over the queries, dv: sum_i p |dO| (epsP + (T + 3) u); all times
    1 + 4 max epsP."""
    qkv, o, dO = qkv.to(D), o.to(D), dO.to(D)
    M, inner = qkv.shape[0], 64 * heads
    dqkv, bnd = torch.zeros((M, 3 * inner), dtype=D), torch.zeros((M, 3 * inner), dtype=D)
    lse, blse = torch.zeros((M, heads, 2), dtype=D), torch.zeros((M, heads, 2), dtype=D)
    for s in range(len(off) - 1):
        b0, b1 = off[s], off[s + 1]
        T = b1 - b0
        for h in range(heads):
            cs = [slice(j * inner + h * 64, j * inner + (h + 1) * 64) for j in range(3)]
            q, k, v = (qkv[b0:b1, c] for c in cs)
            oh, dh = o[b0:b1, cs[0]], dO[b0:b1, cs[0]]
            qs, S, dS, nb, R, row = _att_rows(q, k)
            L = torch.logsumexp(S, 1)
            logl = L - S.max(1).values
            dL = dS.max(1).values + row + (T + 2) * U + K_LOG * U * logl.abs() + U * L.abs()
            p = torch.exp(S - L[:, None])
            epsP = torch.expm1(dS) + dL[:, None] + U * (S - L[:, None]).abs() + K_EXP * U
            Dr, dD = (dh * oh).sum(1), 66 * U * (dh * oh).abs().sum(1)
            dP, ddP = dh @ v.t(), 66 * U * (dh.abs() @ v.abs().t())
            G = dP - Dr[:, None]
            dSg = p * G
            ddS = p * (epsP * G.abs() + ddP + dD[:, None] + U * (dP.abs() + Dr.abs()[:, None])) + 2 * U * dSg.abs()
            so = 1 + 4 * float(epsP.max())
            dqkv[b0:b1, cs[0]] = dSg @ k * 0.125
            bnd[b0:b1, cs[0]] = 0.125 * (ddS @ k.abs() + (T + 3) * U * (dSg.abs() @ k.abs())) * so + FLOOR32
            dqkv[b0:b1, cs[1]] = dSg.t() @ qs
            bnd[b0:b1, cs[1]] = (ddS.t() @ qs.abs() + (T + 3) * U * (dSg.abs().t() @ qs.abs())) * so + FLOOR32
            dqkv[b0:b1, cs[2]] = p.t() @ dh
            bnd[b0:b1, cs[2]] = ((p * (epsP + (T + 3) * U)).t() @ dh.abs()) * so + FLOOR32
            lse[b0:b1, h, 0], blse[b0:b1, h, 0] = L, dL + FLOOR32
            lse[b0:b1, h, 1], blse[b0:b1, h, 1] = Dr, dD + FLOOR32
    return (dqkv, bnd), (lse, blse)


def worst(got, ref, bound):
    """'' if every element of got is within its bound of ref (and finite), else the number of offenders and the worst one's index, error and bound."""
    got, ref, bound = torch.as_tensor(got).to(D), torch.as_tensor(ref).to(D), torch.as_tensor(bound).to(D)
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    err = (got - ref).abs()
    bad = ~(err <= bound)                                               # a NaN on either side is an offender
    if not bool(bad.any()):
        return ""
    ratio = torch.where(bad, torch.nan_to_num(err / bound, nan=float("inf")), torch.zeros_like(err))
    idx = tuple(int(i) for i in (ratio == ratio.max()).nonzero()[0])
    return "%d of %d out of bound; worst at %s: got %r, want %r, error %.3e, bound %.3e" % (
        int(bad.sum()), bad.numel(), idx, float(got[idx]), float(ref[idx]), float(err[idx]), float(bound[idx]))


# shapes of tests/test_hip_mgfn_edges.py
MGFN_GEMM_M = (1, 63, 64, 65, 255, 256, 257)
MGFN_GEMM_N = (64, 128)
MGFN_GEMM_TAPS_CIN = ((1, 16), (1, 48), (3, 16), (3, 48), (5, 32))
MGFN_ATT_LENGTHS = (1, 31, 32, 33, 64, 65)
MGFN_ROW_C = (4, 252, 256, 260)
MGFN_ROW_M = (1, 3, 4, 5)
MGFN_COL_C = (1, 63, 64, 65, 255, 256, 257)
MGFN_COL_M = (1, 127, 128, 129, 385)
MGFN_WGRAD_M = (1, 15, 16, 17, 128, 129, 300)


def gemm_lengths(M):
    """Sequence lengths summing to M with ends exactly on rows 32, 64 and 256 and one row either side of them (where M reaches), and a run of length-1
    sequences (only the centre tap survives)."""
    ends = sorted({e for e in (1, 2, 3, 4, 31, 32, 33, 63, 64, 65, 255, 256, 257) if e < M} | {M})
    return [b - a for a, b in zip([0] + ends[:-1], ends)]


# ---- the small fp32 kernels that close a step (tests/test_hip_head_exact.py): tedspad_linear_fwd (csrc/head.hip), tedspad_bce_head_fwd_bwd (csrc/bce_head.hip),
# tedspad_vote_accumulate / _vote_finalize / _softmax_ce_eval (csrc/action_eval.hip) ------------------------------------------------------------------------
# Two methods. Where the inputs can be chosen so that every partial sum is exact in fp32 in any order (integers; dyadic gradients), the kernel must EQUAL the
# float64 reference. On realistic magnitudes every element has a bound built as above: (chain + 8) u sum |terms| for a sum, K_* u for a transcendental,
# propagated to first order; a reference that is handed the kernel's own fp32 intermediate (the logits of the BCE head) bounds that kernel's roundings only.
# Every reference takes `wrong=`: a kernel that is subtly wrong in one named way; test_kernel_refs.py shows that each is caught by its table.
def _draw(seed, name, shape, n):
    """integers 0 .. n - 1"""
    return torch.floor(synth_tensor(seed, name, shape).to(D) * n).clamp_(0, n - 1)


def linear_form(B, K, N):
    """(kernel, path) of tedspad_linear_fwd, the launcher's own conditions (csrc/head.hip): K <= 32 and B >= 64: a thread per column with K <= 16 or K <= 32
    weights in registers ('smallk16' | 'smallk32'; path 'full' where K fills them, else 'partial'); else B <= 16 and K >= 256: a wavefront per column over
    8 or 16 rows ('cols8' | 'cols16'); else a wavefront per output ('wave'). The last three: path 'vec' (float4 loads, K % 4 == 0) or 'scalar'."""
    if K <= 32 and B >= 64:
        km = 16 if K <= 16 else 32
        return "smallk%d" % km, "full" if K == km else "partial"
    path = "vec" if K % 4 == 0 else "scalar"
    if B <= 16 and K >= 256:
        return ("cols8" if B <= 8 else "cols16"), path
    return "wave", path


LINEAR_FORMS = {("smallk16", "partial"), ("smallk16", "full"), ("smallk32", "partial"), ("smallk32", "full"), ("cols8", "vec"), ("cols8", "scalar"),
                ("cols16", "vec"), ("cols16", "scalar"), ("wave", "vec"), ("wave", "scalar")}
LINEAR_CASES = [      # the kernel the row is there for, B, K, N
    ("smallk16", 64, 1, 1), ("smallk16", 65, 16, 257), ("smallk16", 97, 7, 256),                   # partial 32-row blocks; N on both sides of a 256-thread block
    ("smallk32", 64, 17, 5), ("smallk32", 96, 32, 300), ("smallk32", 129, 24, 255),
    ("cols8", 1, 256, 1), ("cols8", 8, 256, 5), ("cols8", 3, 260, 4), ("cols8", 8, 2050, 9),      # (3, 260, 4): one live lane in the second sweep
    ("cols16", 9, 256, 3), ("cols16", 16, 2048, 7), ("cols16", 16, 258, 6),
    # the near side of every dispatch boundary; (1, 12, 33): the db product of train_nets._linear_bwd
    ("wave", 63, 16, 9), ("wave", 64, 33, 9), ("wave", 17, 256, 5), ("wave", 16, 255, 5), ("wave", 16, 252, 5), ("wave", 1, 12, 33), ("wave", 2, 4, 1),
    ("wave", 5, 130, 33), ("wave", 24, 2048, 102),
]
LINEAR_EPILOGUES = [(sc, sh, relu) for sc, sh in ((0, 0), (0, 1), (1, 1), (1, 0)) for relu in (0, 1)]       # with scale, with shift, ReLU
LINEAR_WRONG = ("drop_last_k", "row_next", "scale_next", "no_relu", "shift_first")


def linear_chain(B, K, N):
    """terms one output's fp32 sum chains: a float4 per 256 columns and a 6-step butterfly, a scalar per 64 columns and the butterfly, or K in one thread"""
    form, path = linear_form(B, K, N)
    return K if form.startswith("smallk") else chain_row(K) if path == "vec" else (K + 63) // 64 + 6


def linear_exact_inputs(B, K, N, seed=71):
    """x: integers in [-8, 8], w: integers in [-4, 4], scale: powers of two that differ between neighbours, shift: non-zero even integers. Column 0 of both
    is odd; of every later column k one side is even (x for odd k, w for even k): every product but the first is even, so x . w is odd -- never 0, and neither is
    x . w * 2^-e + an EVEN shift: no output sits on the ReLU's edge, under any of the four epilogues."""
    tag = "lin%d_%d_%d" % (B, K, N)
    x, w = _draw(seed, tag + "x", (B, K), 17) - 8, _draw(seed, tag + "w", (N, K), 9) - 4
    k = torch.arange(K)
    x[:, k % 2 == 1] = 2 * _draw(seed, tag + "xe", (B, int((k % 2 == 1).sum())), 9) - 8
    w[:, k % 2 == 0] = 2 * _draw(seed, tag + "we", (N, int((k % 2 == 0).sum())), 5) - 4
    x[:, 0], w[:, 0] = 2 * _draw(seed, tag + "x0", (B,), 8) - 7, 2 * _draw(seed, tag + "w0", (N,), 4) - 3
    return x, w, pow2_scales(N), 2 * nonzero_ints(seed, tag + "b", (N,), lo=-2, hi=2)


def linear_real_inputs(B, K, N, seed=72):
    """the magnitudes of a head: activations of a few units, weights ~ 1 / sqrt(K), BatchNorm scales of either sign, shifts below 1"""
    tag = "linr%d_%d_%d" % (B, K, N)
    x, w = synth_tensor(seed, tag + "x", (B, K), -2, 2), synth_tensor(seed, tag + "w", (N, K), -1, 1) / K ** 0.5
    scale = synth_tensor(seed, tag + "s", (N,), 0.5, 1.5) * torch.where(synth_tensor(seed, tag + "ss", (N,)) < 0.25, -1.0, 1.0)
    return x, w, scale, synth_tensor(seed, tag + "b", (N,), -1, 1)


def linear_ref(x, w, scale=None, shift=None, relu=False, chain=None, wrong=None):
    """tedspad_linear_fwd: y = act(scale[n] sum_k x[b, k] w[n, k] + shift[n]). A dict: y, pre (before the ReLU), abs = sum |x||w|, and with `chain` (the terms
    of one fp32 sum, linear_chain) bound = |scale| (chain + 8) u sum |x||w| + 2 u (|scale z| + |shift|) + FLOOR32: the sum in any order, then the product
    and the add (one rounding where they are fused); the ReLU moves nothing further. wrong: 'drop_last_k': the sum stops one element early; 'row_next': the
    x of row b + 1; 'scale_next': the scale of column n + 1; 'no_relu'; 'shift_first': scale (z + shift)."""
    x, w = x.to(D), w.to(D)
    B, K = x.shape
    N = w.shape[0]
    xx = x.roll(-1, 0) if wrong == "row_next" else x
    kk = K - 1 if wrong == "drop_last_k" else K
    z = xx[:, :kk] @ w[:, :kk].t()
    za = x.abs() @ w.abs().t()
    s = torch.ones(N, dtype=D) if scale is None else torch.as_tensor(scale).to(D)
    s = s.roll(-1) if wrong == "scale_next" else s
    b = torch.zeros(N, dtype=D) if shift is None else torch.as_tensor(shift).to(D)
    pre = (z + b) * s if wrong == "shift_first" else z * s + b
    out = {"y": pre.clamp_min(0.0) if (relu and wrong != "no_relu") else pre, "pre": pre, "abs": za}
    if chain is not None:
        out["bound"] = s.abs() * (chain + 8) * U * za + 2 * U * ((z * s).abs() + b.abs()) + FLOOR32
    return out


# The BCE head. (B, K, N): the smallest sizes; the largest B on one column; one workgroup whose last lane's float4 ends at K; exactly one full workgroup; both
# limits at once (all of the 32 KB logit array; the second workgroup has one live lane); eight workgroups. B N is a power of two in all: 1 / (B N) is exact.
BCE_CASES = [(1, 4, 1), (128, 8, 1), (1, 252, 64), (2, 256, 8), (128, 260, 64), (32, 2048, 8)]
BCE_WRONG = ("bias_next", "div_B", "sigma_neg", "dW_row_next", "loss_scaled")
BCE_EXACT_SCALE, BCE_DENSE_SCALE = 256.0, 3.0           # grad_scale of the two tables: a power of two (exact), and one that rounds


def bce_exact_inputs(B, K, N, seed=5):
    """f, W, bias, targets with every logit in {0} or |z| >= 40 (a multiple of 40): W = 40 x integers, f integers, bias 0 / +-40, targets from {0.25, 0.5, 1}.
    Columns 0 and 1 carry the logits (both sides non-zero: z / 40 in [-3, 3]); of the others the even ones hold f only and the odd ones W only: they fill
    dW and df without moving z. The kernel's own formulas then give sigmoid = 0.5 at 0, 1 for z >= 40 (1 + e rounds to 1) and sigmoid - y = -y for z <= -40
    (e < half an ulp of y), so g = (sigmoid - y) / (B N) is a known dyadic number and df, dW, db are sums of dyadic products: exact in any order.
    (The seed: one at which the single logit of (1, 4, 1) has g != 0 -- test_kernel_refs.py asserts the conditions for every row.)"""
    tag = "bcex%d_%d_%d" % (B, K, N)
    f, W = torch.zeros((B, K), dtype=D), torch.zeros((N, K), dtype=D)
    f[:, :2], W[:, :2] = _draw(seed, tag + "f", (B, 2), 3) - 1, 40.0 * (_draw(seed, tag + "w", (N, 2), 3) - 1)
    k = torch.arange(K)
    fo, wo = (k >= 2) & (k % 2 == 0), (k >= 2) & (k % 2 == 1)
    f[:, fo] = nonzero_ints(seed, tag + "fo", (B, int(fo.sum())), lo=-3, hi=3)
    W[:, wo] = 40.0 * torch.where(_draw(seed, tag + "wo", (N, int(wo.sum())), 2) > 0, 1.0, -1.0) * (1 + _draw(seed, tag + "wm", (N, int(wo.sum())), 2))
    bias = 40.0 * ((torch.arange(N) + 1) % 3 - 1).to(D)
    y = torch.tensor([0.25, 0.5, 1.0], dtype=D)[_draw(seed, tag + "y", (B, N), 3).long()]
    return f, W, bias, y


def bce_dense_inputs(B, K, N, seed=75):
    """Integer f and W that are no multiples of 40, spread over all of K (W the sparser the longer the row: logits of a few tens), integer biases up to 60 in
    magnitude (|z| reaches 80), targets anywhere in [0, 1] with some exactly 0 and 1. The logits are integers: the kernel's forward must return them exactly."""
    tag = "bced%d_%d_%d" % (B, K, N)
    f = small_ints(seed, tag + "f", (B, K), lo=-3, hi=3, density=1.0)
    W = small_ints(seed, tag + "w", (N, K), lo=-2, hi=2, density=min(1.0, 64.0 / K))
    bias = _draw(seed, tag + "b", (N,), 121) - 60
    if N > 1:
        bias[0], bias[-1] = 60.0, -60.0
    y = (synth_tensor(seed, tag + "y", (B, N)).to(D) * 1.5 - 0.25).clamp_(0.0, 1.0).to(torch.float32).to(D)
    return f, W, bias, y


def bce_logit_classes(z):
    """how many logits are 0, >= 40, <= -40 -- and whether there is no other"""
    n = [int((z == 0).sum()), int((z >= 40).sum()), int((z <= -40).sum())]
    return n, sum(n) == z.numel()


def bce_head_ref(f, W, bias, y, grad_scale=1.0, logits=None, wrong=None):
    """tedspad_bce_head_fwd_bwd (the formulas at the top of csrc/bce_head.hip); W None: logits mode, f holds the logits. `logits`: the fp32 logits the kernel
    returned, which everything after them is then derived from (the bounds cover the kernel's roundings after its K reduction only). A dict of (value,
    bound): logits (bound None: compared exactly), loss, g, df, dW, db (the last two None in logits mode). With e = exp(-|z|), sigma = 1 / (1 + e) or
    e / (1 + e): expf K_EXP u, the add, the division, then sigma - y (u (sigma + |y|)) and the exact or once-rounded 1 / (B N):
      g : (K_EXP + 4) u (sigma + |y|) / (B N)
      df: ((N + 8) u sum_n |g||W| + sum_n dg |W| + (N + 2) FLOOR32) grad_scale; dW and db likewise over B; logits mode: (dg + 2 u |g|) grad_scale
          (dg carries FLOOR32: a g below the smallest normal may be flushed -- at z = -80, y = 0 it is e^-80 / (B N) -- and so may each of the N partial sums)
      loss: a term max(z, 0) - z y + log1p(e) cancels, so it is held against m = |max(z, 0)| + |z y| + log1p(e): the product, the difference and the last add one
            rounding each, log1pf K_LOG u, its argument K_EXP u (e / (1 + e) <= log1p(e)): (3 + K_EXP + K_LOG) u m; the sum chains ceil(B N / 1024) terms per
            thread, a 6-step butterfly and the 16 wave sums, + 8 for the mean: that many u sum m, all over B N.
    (Measured on gfx950: the device's expf is off by ~|z| u at large |z| -- DESIGN.md, "What the head, BCE and vote tests pin" -- which the g bound absorbs
    on the dense table only just where y = 0 and z << 0: sigma - y is then e itself.)
    wrong: 'bias_next': the bias of column n + 1; 'div_B': g over B instead of B N; 'sigma_neg': sigmoid(-z); 'dW_row_next': dW from row b + 1 of f;
    'loss_scaled': grad_scale applied to the loss as well."""
    f, y = f.to(D), y.to(D)
    B, N = y.shape
    gs = f32(grad_scale)
    if W is None:
        z = f.clone()
    else:
        W = W.to(D)
        bb = torch.zeros(N, dtype=D) if bias is None else torch.as_tensor(bias).to(D)
        z = f @ W.t() + (bb.roll(-1) if wrong == "bias_next" else bb)
    if logits is not None:
        z = logits.to(D).reshape(B, N)
    e = torch.exp(-z.abs())
    sig = torch.sigmoid(-z if wrong == "sigma_neg" else z)
    g = (sig - y) / (B if wrong == "div_B" else B * N)
    dg = (K_EXP + 4) * U * (sig + y.abs()) / (B * N) + FLOOR32
    m = z.clamp_min(0.0) + (z * y).abs() + torch.log1p(e)
    loss = (z.clamp_min(0.0) - z * y + torch.log1p(e)).sum() / (B * N) * (gs if wrong == "loss_scaled" else 1.0)
    chain = (B * N + 1023) // 1024 + 6 + 16 + 8
    out = {"logits": (z, None), "g": (g, dg), "loss": (loss.reshape(1), ((3 + K_EXP + K_LOG + chain) * U * m.sum() / (B * N) + FLOOR32).reshape(1))}
    if W is None:
        out.update(df=(g * gs, gs * (dg + 2 * U * g.abs()) + FLOOR32), dW=None, db=None)
        return out
    ga, fr = g.abs(), (f.roll(-1, 0) if wrong == "dW_row_next" else f)
    out["df"] = (gs * (g @ W), gs * ((N + 8) * U * (ga @ W.abs()) + dg @ W.abs() + (N + 2) * FLOOR32) + FLOOR32)
    out["dW"] = (gs * (g.t() @ fr), gs * ((B + 8) * U * (ga.t() @ f.abs()) + dg.t() @ f.abs() + (B + 2) * FLOOR32) + FLOOR32)
    out["db"] = (gs * g.sum(0), gs * ((B + 8) * U * ga.sum(0) + dg.sum(0) + (B + 2) * FLOOR32) + FLOOR32)
    return out


def bce_kernel_g32(z, y):
    """g as csrc/bce_head.hip forms it, in torch's fp32 on the CPU: e = expf(-|z|), sigma = z >= 0 ? 1 / (1 + e) : e / (1 + e), (sigma - y) * (1 / (B N))."""
    z, y = z.to(torch.float32), y.to(torch.float32)
    e = torch.exp(-z.abs())
    sig = torch.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    return (sig - y) * (torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(z.numel()), dtype=torch.float32))


# The vote kernels: a sum per (video, class) in ROW order, one fp32 add per row -- which a host loop over float32 numpy rows reproduces bit for bit.
VOTE_C = (2, 255, 256, 257, 1024)             # one workgroup per 256 classes: one partial, exactly one, one class into the second, four
VOTE_B = (1, 7, 1024)
VOTE_V = {1: 2, 7: 4, 1024: 9}                # videos per batch size; the last one is never named
VOTE_FINAL_V = (1, 4, 5, 9)                   # four videos per workgroup of vote_finalize
VOTE_WRONG = ("reverse", "count_reload", "first_tie")


def vote_vids(B):
    """Video index per row: long runs, strict alternation (every flush followed by a reload of what an earlier flush wrote), single rows. V - 1 never occurs."""
    if B == 1:
        return [0]
    if B == 7:
        return [0, 0, 1, 0, 1, 2, 0]
    seq = [0] * 300 + [1, 2] * 100 + [3, 4, 5, 6, 7, 3, 0, 5] * 8 + [1] * 200 + [0, 3] * 80
    seq += [(5 * i) % 8 for i in range(B - len(seq) - 40)] + [7] * 40
    assert len(seq) == B
    return seq


def vote_inputs(B, C, seed=76):
    """probability rows (softmax of logits in [-4, 4], fp32), the video of each row, and sums / counts that already hold something"""
    tag, V = "vote%d_%d" % (B, C), VOTE_V[B]
    probs = torch.softmax(synth_tensor(seed, tag + "z", (B, C), -4, 4), dim=1).numpy()
    sums = synth_tensor(seed, tag + "s", (V, C), 0, 3).numpy()
    counts = (_draw(seed, tag + "c", (V,), 4) + 1).numpy().astype(np.int32)
    return probs, vote_vids(B), sums, counts, V


def vote_accumulate_ref(probs, vid, sums, counts, wrong=None):
    """tedspad_vote_accumulate, the kernel's own walk in float32 numpy: a run of rows of one video starts from what `sums` holds (also what an earlier run of
    this launch wrote back), adds its rows one by one, is written back when the video changes; counts likewise. Returns new (sums, counts).
    wrong = 'reverse': the rows from last to first; 'count_reload': a run of a video that was written back earlier counts one row too many."""
    p, s, c = np.asarray(probs, np.float32), np.array(sums, np.float32, copy=True), np.array(counts, np.int32, copy=True)
    rows = range(len(vid) - 1, -1, -1) if wrong == "reverse" else range(len(vid))
    cur, n, acc, flushed = -1, 0, None, set()
    for b in rows:
        v = int(vid[b])
        if v != cur:
            if cur >= 0:
                s[cur], c[cur] = acc, c[cur] + n
                flushed.add(cur)
            cur, n, acc = v, (1 if wrong == "count_reload" and v in flushed else 0), s[v].copy()
        acc = acc + p[b]                      # float32 + float32: one IEEE add per class
        n += 1
    if cur >= 0:
        s[cur], c[cur] = acc, c[cur] + n
    assert s.dtype == np.float32
    return s, c


def vote_finalize_inputs(V, C, seed=77):
    """sums in [0, 1), counts 1 .. 9, labels; exactly equal maxima (1.5) planted in two neighbouring lanes of video 0, and for V >= 4: in one lane (c, c + 64)
    of video 1 where C allows, in the first and the last class of video 2; video 3 has no rows (count 0). Returns sums, counts, labels, the top-1 wanted."""
    tag = "votef%d_%d" % (V, C)
    sums = synth_tensor(seed, tag + "s", (V, C), 0, 1).numpy()
    counts = (_draw(seed, tag + "c", (V,), 9) + 1).numpy().astype(np.int32)
    c0 = min(C - 2, 130)
    sums[0, c0] = sums[0, c0 + 1] = 1.5
    want = [c0 + 1] + [-2] * (V - 1)
    if V >= 4:
        c1 = min(C - 1, 70)
        sums[1, c1] = sums[1, max(c1 - 64, 0)] = 1.5
        sums[2, 0] = sums[2, C - 1] = 1.5
        counts[3] = 0
        want[1:4] = [c1, C - 1, -1]
    labels = np.array([(7 * v) % C for v in range(V)], np.int64)
    labels[0] = want[0]                       # video 0 is right only under the highest-index rule
    return sums, counts, labels, want


def vote_finalize_ref(sums, counts, labels, wrong=None):
    """tedspad_vote_finalize: mean = sums / float32(count) (IEEE division; a video without rows: zeros, top-1 -1, not correct), top-1 = the HIGHEST index
    among exactly equal maxima of the mean, correct = (top-1 == label). wrong = 'first_tie': the lowest index."""
    s, c = np.asarray(sums, np.float32), np.asarray(counts, np.int32)
    V, C = s.shape
    seen = c > 0
    mean = np.where(seen[:, None], s / np.where(seen, c, 1).astype(np.float32)[:, None], np.float32(0)).astype(np.float32)
    top = np.argmax(mean, axis=1) if wrong == "first_tie" else C - 1 - np.argmax(mean[:, ::-1], axis=1)
    pred = np.where(seen, top, -1).astype(np.int32)
    return mean, pred, (seen & (pred == np.asarray(labels))).astype(np.uint8)


def sce_logits(B, C, seed=78):
    """Rows spread over [-80, 80] as tests/test_hip_action_eval.py draws them: the maximum (80) at a different column per row, a runner-up 0.1 .. 0.5 below
    it, one entry at -80 (C = 2: odd rows negated instead); row 0 is labelled with its top class. Returns logits (fp32), labels (int64)."""
    z = synth_tensor(seed, "sce_z_%d_%d" % (B, C), (B, C), -80.0, 79.0)
    lab = (synth_tensor(seed, "sce_l_%d_%d" % (B, C), (B,)) * C).long().clamp(0, C - 1)
    for r in range(B):
        m = (7 * r + 3) % C
        z[r, m] = 80.0
        z[r, (m + 2) % C if C > 2 else 1 - m] = 80.0 - 0.1 * (1 + r % 5)
        if C > 2:
            z[r, (m + 1) % C] = -80.0
        elif r % 2:
            z[r] = -z[r]
    lab[0] = int(z[0].argmax())
    return z, lab


def softmax_ce_ref(z, labels):
    """tedspad_softmax_ce_eval: softmax over the classes, -log_softmax[label] per row, its mean, the top-1 class (float64 argmax). A dict of (value, bound)
    and pred. The kernel forms d = z - max (one rounding: u |d| in the exponent), e = expf(d) (K_EXP u), rest = the sum of e without the top class over
    n = ceil(C / 64) + 6 chained terms, den = 1 + rest:
      drest = sum e (u |d| + K_EXP u) + (n + 2) u rest;  dden = drest + u den
      probs: p (u |d| + K_EXP u + dden / den + 2 u)      (the division, and slack for the second order)
      row loss = log1p(rest) + (max - z[label]): drest / den + K_LOG u log1p(rest) + u |max - z[label]| + u |loss|
      mean: (sum of the row bounds + (ceil(B / 64) + 6 + 2) u sum |row loss|) / B."""
    z = z.to(D)
    B, C = z.shape
    mx, top = z.max(1)
    d = z - mx[:, None]
    e = torch.exp(d)
    notop = torch.ones_like(e)
    notop[torch.arange(B), top] = 0.0
    rest = (e * notop).sum(1)
    n = (C + 63) // 64 + 6
    drest = (e * notop * (U * d.abs() + K_EXP * U)).sum(1) + (n + 2) * U * rest
    den = 1.0 + rest
    dden = drest + U * den
    p = e / den[:, None]
    dp = p * (U * d.abs() + K_EXP * U + (dden / den)[:, None] + 2 * U) + FLOOR32
    gap = mx - z[torch.arange(B), labels]
    rows = torch.log1p(rest) + gap
    drows = drest / den + K_LOG * U * torch.log1p(rest) + U * gap.abs() + U * rows.abs() + FLOOR32
    dmean = (drows.sum() + ((B + 63) // 64 + 8) * U * rows.abs().sum()) / B + FLOOR32
    return {"probs": (p, dp), "row_loss": (rows, drows), "loss": (rows.mean().reshape(1), dmean.reshape(1)), "pred": top}


def worst_ratio(got, ref, bound):
    """the largest error / bound over the elements: what a bounded test prints per quantity"""
    got, ref, bound = torch.as_tensor(got).to(D), torch.as_tensor(ref).to(D), torch.as_tensor(bound).to(D)
    return float(((got.reshape(ref.shape) - ref).abs() / bound).max())
