"""Shared by tests/test_optim_host.py (CPU) and tests/test_hip_optim.py (GPU): the inputs of the optimizer-kernel tests, the float64 torch.optim twin they are
compared with, and a restatement of the update with the three mistakes the comparison has to be able to see."""
import math

import torch

# Sizes (elements) against the kernel's chunk of 4096 (tedspad_optim_chunk_elems(); the GPU test asserts that it is 4096): below one 16-byte vector (1, 3), vectors
# + tail in a short chunk (102, 5, 7), exactly one vector (4), exactly one chunk (4096: the all-loads-first path), one chunk + 1 (4097), several chunks + a tail of 3
# (65539 = 16 x 4096 + 3). EXCLUDED is the index of the tensor that takes no part in the step.
SIZES = [1, 3, 102, 4, 6, 5, 7, 4096, 4097, 65539]
EXCLUDED = 4
# two buckets; with both flats 16-byte aligned the slots start at element phases {0, 1, 0, 2, 2, 0} and {0, 3, 3, 0}: every phase occurs, the full chunks of 4096 /
# 4097 read their gradient as dwords (phase 3), those of 65539 as 16-byte vectors (phase 0)
BUCKETS = [[0, 1, 2, 3, 4, 5], [6, 7, 8, 9]]
# the same tensors as three buckets whose flats start at other phases (elements): slot phases {1, 2, 1}, {2, 2, 2, 0, 1}, {3, 2}
# (65539 moves from 16-byte to dword gradient loads, the small tensors to other heads and tails)
BUCKETS3, PHASES3 = [[0, 1, 2], [7, 3, 4, 5, 9], [6, 8]], [1, 2, 3]
LRS = [1e-2, 2e-2, 5e-3, 1.5e-2, 1e-2]
WD = 0.1
SCALE = 65536.0
# rel-L2 per tensor against the float64 twin: measured maxima on MI355X (tests/test_hip_optim.py's docstring) and the bounds, 4 x those
MEASURED_P, MEASURED_M, MEASURED_V = 1.6e-7, 9.3e-8, 1.4e-7
BOUND_P, BOUND_M, BOUND_V = 4 * MEASURED_P, 4 * MEASURED_M, 4 * MEASURED_V
CONFIGS = {     # name -> (opt_type, kwargs of FusedOptimizer / torch.optim)
    "adam": ("adam", dict()),
    "adam_wd": ("adam", dict(weight_decay=WD)),
    "adamw": ("adamw", dict(weight_decay=WD)),
    "sgd_mu": ("sgd", dict(momentum=0.9, weight_decay=WD)),
    "sgd_plain": ("sgd", dict(momentum=0.0, weight_decay=WD)),
}


def make_params(seed=0):
    """fp32 ~N(0,1) with exact zeros at every 7th element."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for n in SIZES:
        p = torch.randn(n, generator=g)
        p[::7] = 0.0
        out.append(p)
    return out


def make_grads(step, seed=100):
    """The TRUE (unscaled) fp32 gradients of one step, by flat index i of each tensor: i % 10 == 0 -> 0, 1 -> 1e-30 (g * g underflows in fp32), 2 -> 1e4,
    3 -> +-3e-8 (sqrt(v) of the size of eps: where a misplaced eps shows), the rest ~N(0,1) drawn anew every step."""
    g = torch.Generator().manual_seed(seed + step)
    out = []
    for n in SIZES:
        x = torch.randn(n, generator=g)
        i = torch.arange(n)
        x[i % 10 == 0] = 0.0
        x[i % 10 == 1] = 1e-30
        x[i % 10 == 2] = 1e4
        x[i % 10 == 3] = torch.where(i[i % 10 == 3] % 20 == 3, 3e-8, -3e-8)
        out.append(x)
    return out


def torch_twin(opt_type, params64, lr, **kw):
    cls = {"adam": torch.optim.Adam, "adamw": torch.optim.AdamW, "sgd": torch.optim.SGD}[opt_type]
    return cls(params64, lr=lr, **kw)


def twin_params(params32):
    """float64 leaf copies; the excluded one never gets a .grad (torch then skips it: no decay, no state)."""
    return [torch.nn.Parameter(p.detach().double().cpu().clone()) for p in params32]


def twin_step(opt, params64, grads_scaled32, scale, lr):
    """One step of the float64 twin on the fp32 gradients the kernel reads, divided by the scale."""
    for g_ in opt.param_groups:
        g_["lr"] = lr
    for i, (p, g) in enumerate(zip(params64, grads_scaled32)):
        p.grad = None if i == EXCLUDED else g.detach().double().cpu() / scale
    opt.step()


def twin_state(opt, p, opt_type):
    st = opt.state.get(p, {})
    if opt_type == "sgd":
        return st.get("momentum_buffer"), None
    return st.get("exp_avg"), st.get("exp_avg_sq")


def rel_l2(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    d = float(b.norm())
    return float((a - b).norm()) / d if d > 0 else float((a - b).norm())


def restated(opt_type, params, grads_per_step, lrs, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, momentum=0.0, mistake=None):
    """float64 restatement of the update the kernel implements (csrc/optim.hip update_elem), optionally with one mistake:
    'eps_inside' (sqrt(v / bc2 + eps)), 'no_bias_correction', 'swap_decay' (coupled where decoupled is meant and the reverse)."""
    ps = [p.detach().double().clone() for p in params]
    ms, vs = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    decoupled = (opt_type == "adamw") != (mistake == "swap_decay")
    b1, b2 = betas
    for t, (grads, lr) in enumerate(zip(grads_per_step, lrs), start=1):
        for i, (p, g) in enumerate(zip(ps, grads)):
            if i == EXCLUDED:
                continue
            g = g.double()
            if opt_type == "sgd":
                g = g + weight_decay * p
                if momentum:
                    ms[i] = momentum * ms[i] + g
                    g = ms[i]
                p -= lr * g
                continue
            if decoupled:
                p -= lr * weight_decay * p
            elif weight_decay:
                g = g + weight_decay * p
            ms[i] = ms[i] + (1 - b1) * (g - ms[i])
            vs[i] = b2 * vs[i] + (1 - b2) * g * g
            bc1, bc2 = (1.0, 1.0) if mistake == "no_bias_correction" else (1 - b1 ** t, 1 - b2 ** t)
            denom = (vs[i] / bc2 + eps).sqrt() if mistake == "eps_inside" else vs[i].sqrt() / math.sqrt(bc2) + eps
            p -= (lr / bc1) * ms[i] / denom
    return ps, ms, vs
