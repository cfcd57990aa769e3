"""Host only: inputs for the non-local attention kernels (csrc/nonlocal.hip) whose right answer is known bit for bit, and that answer.

The winners / decoys construction, for n items, q queries, k keys (k <= d), d in {256, 512}:

    H        the d x d Sylvester Hadamard matrix, entries +-1: H[a] . H[b] = d [a == b]
    phi      phi[b, j] = H[(7 j + 3 b) mod d]: distinct rows (7 is odd), so phi[b, j] . phi[b, j'] = d [j == j']
    W(b, i)  the WINNERS of query i, a window {(a + s) mod k, s < m} of m keys, m from 1, 2, 4, 8, 16, 32 cycling with i + b and halved until m <= k; the start
             a walks the keys in steps of max(1, k // q) | 1 from 3 b, so that the windows of a short query list still reach every key tile and wrap past
             k - 1; every fourth query starts AT k - 1
    D(b, i)  0 .. 8 DECOYS, disjoint from W: directly behind the window for even i, directly in front of it for odd i
    theta    theta[b, i] = 8 (2 sum_{j in W} phi[b, j] + sum_{j in D} phi[b, j]): multiples of 8 up to 576, exact in f16 and bf16
    g        32 x integers in [-2, 2]
    dT       one channel of +-1 per query
    scale    2^-4 (d = 256), 2^-5 (d = 512): a power of two

The logits theta . phi are then exact integers -- 16 d on a winner, 8 d on a decoy, 0 elsewhere -- and the scaled logits are 256, 128, 0. exp(-128) is 3e-56 in
float64 and exp2(-184.7) is zero in fp32 (the smallest denormal is 2^-149), so the kernel's P is exactly 1 / m on W and exactly 0 elsewhere: every product and
every sum of the forward and of the three backward launches is exact in fp32 IN ANY ORDER, and each result is the closed form below rounded once.

    T = mean of g over W (an integer),  dg = P^T dT,  dP = dT g^T (an integer, |.| <= 64),  D_i = dT_i . T_i,  dS = P o (dP - D) (at most 8 significant
    bits: it survives the kernel's rounding to the storage type in LDS),  dtheta = scale dS phi,  dphi = scale dS^T theta,  lse = 256 + ln m.
"""
import functools

import torch

from ted_spad_amd.synth import synth_tensor

SEED = 11
N_ITEMS = 2
MS = (1, 2, 4, 8, 16, 32)
WINNER_LOGIT = 256.0                 # scale * 16 d
# every remainder the kernels branch on: k on and next to the multiples of 16 (the forward's wave skip and its pv(1) / pv(3) steps), 32 (`second`, the backward's
# walked / resident tiles) and 64 (the key tile); q one off the multiples of 32 (the last partial query tile), odd (the backward's row pairs) and off the
# multiples of 16 (nl_dsum_kernel's groups straddle the item boundary)
SHAPES = ((1, 1), (2, 3), (15, 16), (16, 15), (17, 17), (31, 33), (32, 32), (33, 31),
          (47, 49), (48, 48), (49, 47), (63, 65), (64, 64), (65, 63), (33, 80), (95, 96),
          (96, 97), (97, 95), (31, 127), (64, 128), (33, 129), (65, 191), (32, 193), (129, 256))
HOST_TAPE_SHAPES = ((2, 3), (33, 31), (49, 47), (96, 97), (33, 129), (65, 191))
STRIDE_SHAPES = ((33, 31), (65, 63), (96, 97), (33, 129))
WIDTHS = (256, 512)
STORAGE = {"f16": torch.float16, "bf16": torch.bfloat16}


def scale_of(d):
    return {256: 2.0 ** -4, 512: 2.0 ** -5}[d]


def hadamard(d):
    h = torch.ones(1, 1, dtype=torch.float64)
    while h.shape[0] < d:
        h = torch.cat([torch.cat([h, h], dim=1), torch.cat([h, -h], dim=1)], dim=0)
    assert h.shape[0] == d
    return h


def sets(n, q, k):
    """(winners (n, q, k) bool, decoys (n, q, k) bool, m (n, q) long)."""
    win, dec = torch.zeros(n, q, k, dtype=torch.bool), torch.zeros(n, q, k, dtype=torch.bool)
    ms = torch.zeros(n, q, dtype=torch.long)
    step = max(1, k // q) | 1
    for b in range(n):
        for i in range(q):
            m = MS[(i + b) % len(MS)]
            while m > k:
                m //= 2
            a = k - 1 if i % 4 == 3 else (i * step + 3 * b) % k
            nd = min((3 * i + 5 * b + 2) % 9, k - m)
            w = [(a + s) % k for s in range(m)]
            dd = [(a + m + s) % k for s in range(nd)] if i % 2 == 0 else [(a - 1 - s) % k for s in range(nd)]
            assert len(set(w)) == m and len(set(dd)) == nd and not set(w) & set(dd)
            win[b, i, w], dec[b, i, dd], ms[b, i] = True, True, m
    return win, dec, ms


def build(q, k, d, h=None, n=N_ITEMS, seed=SEED):
    """The inputs (float64 tensors holding values exact in both storage types) and the sets: dict(theta, phi, g, dt, win, dec, m, scale)."""
    assert 1 <= k <= d and d in WIDTHS
    h = hadamard(d) if h is None else h
    tag = "nl_exact/%d/%d/%d/" % (q, k, d)
    win, dec, ms = sets(n, q, k)
    rows = (7 * torch.arange(k).unsqueeze(0) + 3 * torch.arange(n).unsqueeze(1)) % d
    phi = h[rows]                                                                      # (n, k, d)
    theta = 8.0 * torch.einsum("nqk,nkd->nqd", 2.0 * win.double() + dec.double(), phi)
    g = 32.0 * (torch.floor(synth_tensor(seed, tag + "g", (n, k, d)).double() * 5.0).clamp_(0, 4) - 2.0)
    ch = torch.floor(synth_tensor(seed, tag + "ch", (n, q)).double() * d).long().clamp_(0, d - 1)
    dt = torch.zeros(n, q, d, dtype=torch.float64)
    dt.scatter_(2, ch.unsqueeze(2), torch.where(synth_tensor(seed, tag + "sign", (n, q, 1)) < 0.5, -1.0, 1.0).double())
    return dict(theta=theta, phi=phi, g=g, dt=dt, win=win, dec=dec, m=ms, scale=scale_of(d))


def closed_form(c):
    """The float64 closed form with P = [j in W] / m put in: every product and sum below is one of integers over powers of two far inside 2^53, so each
    value is the exact real number. dict(p, t, lse, dg, dp, dsum, ds, dtheta, dphi)."""
    p = c["win"].double() / c["m"].double().unsqueeze(2)
    t = torch.einsum("nqk,nkd->nqd", p, c["g"])
    dg = torch.einsum("nqk,nqd->nkd", p, c["dt"])
    dp = torch.einsum("nqd,nkd->nqk", c["dt"], c["g"])
    dsum = (c["dt"] * t).sum(dim=2)
    ds = p * (dp - dsum.unsqueeze(2))
    return dict(p=p, t=t, lse=WINNER_LOGIT + torch.log(c["m"].double()), dg=dg, dp=dp, dsum=dsum, ds=ds,
                dtheta=torch.einsum("nqk,nkd->nqd", ds, c["phi"]) * c["scale"], dphi=torch.einsum("nqk,nqd->nkd", ds, c["theta"]) * c["scale"])


@functools.lru_cache(maxsize=None)
def hadamard_of(d):
    return hadamard(d)


@functools.lru_cache(maxsize=None)
def case(q, k, d):
    """(inputs, closed form) of a shape, built once and shared; nobody writes to either."""
    c = build(q, k, d, hadamard_of(d))
    return c, closed_form(c)


def bits(x, dtype):
    """The 16-bit image of float64 values rounded ONCE to the storage type (fp32 holds every value of the closed form exactly): (n * rows, d) int16."""
    x32 = x.float()
    assert torch.equal(x32.double(), x), "a closed-form value is not an fp32 number"
    return x32.to(STORAGE[dtype]).view(torch.int16).reshape(-1, x.shape[-1]).contiguous()


def placements(c):
    """Per (item, query): does a decoy lie in an EARLIER 64-key tile than every winner, in a LATER one, in ANOTHER WAVE's sixteen keys of a tile that holds
    winners (the forward kernel gives wave w keys 16 w .. 16 w + 15 of a tile)? dict of (n, q) bool."""
    n, q, k = c["win"].shape
    res = {key: torch.zeros(n, q, dtype=torch.bool) for key in ("earlier", "later", "other_wave")}
    for b in range(n):
        for i in range(q):
            w = torch.nonzero(c["win"][b, i]).flatten().tolist()
            tiles, groups = {j // 64 for j in w}, {j // 16 for j in w}
            for j in torch.nonzero(c["dec"][b, i]).flatten().tolist():
                res["earlier"][b, i] |= j // 64 < min(tiles)
                res["later"][b, i] |= j // 64 > max(tiles)
                res["other_wave"][b, i] |= j // 64 in tiles and j // 16 not in groups
    return res


def lse_fp32(c):
    """lse as the host tape holds it: the float64 value rounded to fp32."""
    return (WINNER_LOGIT + torch.log(c["m"].double())).float()
