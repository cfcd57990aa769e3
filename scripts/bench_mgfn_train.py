"""One MGFN training iteration on one MI355X at the reference's default shape (main.py / option.py: batch 16 normal + 16 abnormal videos,
10 crops, 32 segments, F = 2048, depths 3 / 3 / 2: M = 10 240 tokens), timed two ways in alternating turns:

  (i)  MGFNTrainStep.step: the train-mode forward, MSNSD, the cost, the backward (csrc/mgfn.hip, csrc/mgfn_train.hip) and Adam
  (ii) the same iteration as plain torch fp32 autograd of the restatement (tests/mgfn_train_restate.py) with torch.optim.Adam, on the same
       GPU, same weights, inputs and masks: what a user would otherwise run

Each iteration is timed with device events; the figure is the median of `--iters` iterations after `--warmup` untimed ones of each. Prints
one JSON line: milliseconds per iteration of both, every sample, and the first costs of both paths.

    python scripts/bench_mgfn_train.py [--iters 20] [--warmup 3] [--batch 16]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from ted_spad_amd.mgfn import MGFN, MGFNTrainStep  # noqa: E402
from ted_spad_amd.synth import synth_mgfn_state_dict, synth_tensor  # noqa: E402

BUFFERS = ("running_mean", "running_var", "num_batches_tracked")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    a = ap.parse_args()
    if a.iters < 20:
        ap.error("--iters must be at least 20: the figure is a median")
    import mgfn_train_restate as R
    torch.cuda.set_device(0)
    n, nc, T, F = a.batch, 10, 32, 2048
    cfg = (F, (3, 3, 2), ("gb", "fb", "fb"), 0.1)
    x = synth_tensor(0, "mgfn_train_bench/x", (2 * n, nc, T, F + 1), 0.0, 2.0, device="cuda")
    ninput, ainput = x[:n].contiguous(), x[n:].contiguous()
    nlabel, alabel = torch.zeros(n, device="cuda"), torch.ones(n, device="cuda")
    masks = tuple((synth_tensor(0, "mgfn_train_bench/mask%d" % i, (n, T), device="cuda") >= 0.7).float() / 0.3 for i in range(2))

    m = MGFN()
    sd0 = synth_mgfn_state_dict(m.state_dict(), 0)
    m.load_state_dict(sd0)
    m = m.cuda()
    drv = MGFNTrainStep(m, n)

    prm = {k: (v.cuda().clone().requires_grad_(True) if not k.endswith(BUFFERS) else v.cuda().clone()) for k, v in sd0.items()}
    opt = torch.optim.Adam([v for v in prm.values() if v.requires_grad], lr=1e-3, weight_decay=5e-4)

    def hip_step():
        return drv.step(ninput, ainput, nlabel, alabel, masks)["cost"]

    def torch_step():
        bn_out = {}
        opt.zero_grad()
        r = R.train_cost(prm, ninput, ainput, nlabel, alabel, masks, cfg, 3, bn_out)
        r["cost"].backward()
        opt.step()
        prm.update(bn_out)
        return float(r["cost"].detach())

    runs = {"hip_step": hip_step, "torch_autograd_fp32": torch_step}
    first = {}
    for k, fn in runs.items():
        for i in range(a.warmup):
            c = fn()
            first.setdefault(k, c)
        torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(a.iters):
        for k, fn in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    res = {"shape": {"batch": [n, n], "ncrops": nc, "segments": T, "feature_size": F, "depths": [3, 3, 2], "tokens": 2 * n * nc * T},
           "iters": a.iters, "warmup": a.warmup, "first_cost": first,
           "ms_per_iteration": {k: statistics.median(v) for k, v in ms.items()}, "ms_min_max": {k: [min(v), max(v)] for k, v in ms.items()},
           "hip_over_torch": statistics.median(ms["hip_step"]) / statistics.median(ms["torch_autograd_fp32"])}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
