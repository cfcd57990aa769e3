"""The optimizer tail of a training step on ft's real parameter set (I3Res50 + heads, 168 tensors, ~28.5 M elements) with random gradients, on 1 MI355X:
  fused     optim.FusedOptimizer.step: tedspad_optim_check + tedspad_optim_update (Adam) + tedspad_optim_finish -- 3 launches
  update    the same without a loss scale: update + finish only (the update kernel's own rate)
  parent    what the step drivers did before it: torch._amp_foreach_non_finite_check_and_unscale_ + torch.optim.Adam(fused=True).step() with its found_inf
Each timed with device events around `--steps` calls, in alternating rounds (a drift of the clock or the box shows in every column); the median round is reported.
GB/s = the bytes the algorithm needs per element (fused: 4 check + 28 update = 32; update: 28; parent: 8 unscale + 28 Adam = 36) x elements / time, next to the
6.3 TB/s measured HBM ceiling. All three are given an inverse scale of 1 (static scale 1.0) so that repeated calls on the same gradients keep their values:
the memory traffic is that of any other scale. Prints one JSON line."""
import argparse
import contextlib
import io
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # the repository root
from ted_spad_amd.grad_reduce import GradBucketReducer
from ted_spad_amd.model_loaders import load_ft_model
from ted_spad_amd.optim import DynamicLossScale, FusedOptimizer
from ted_spad_amd.synth import synth_state_dict
from ted_spad_amd.train_nets import I3DTrainer

HBM_CEILING_GBS = 6300.0

ap = argparse.ArgumentParser()
ap.add_argument('--steps', type=int, default=50)
ap.add_argument('--warmup', type=int, default=10)
ap.add_argument('--rounds', type=int, default=5)
a = ap.parse_args()


def ft_model():
    with contextlib.redirect_stdout(io.StringIO()):
        ft = load_ft_model('largei3d', num_classes=102)
    ft.load_state_dict(synth_state_dict(ft.state_dict(), 0))
    return ft.cuda()


def with_grads(ft):
    red = GradBucketReducer(I3DTrainer(ft).grad_buckets(), None, all_params=list(ft.parameters()))
    red.prepare()
    g = torch.Generator(device='cuda').manual_seed(0)
    for flat in red.flats:
        flat.copy_(torch.randn(flat.numel(), generator=g, device='cuda') * 1e-2)
    return red


def timed(fn):
    for _ in range(2):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / a.steps


ft_new, ft_upd, ft_old = ft_model(), ft_model(), ft_model()
red_new, red_upd, red_old = with_grads(ft_new), with_grads(ft_upd), with_grads(ft_old)
numel = sum(p.numel() for p in ft_new.parameters())
opt_new, opt_upd = FusedOptimizer(red_new, 'adam', lr=1e-5), FusedOptimizer(red_upd, 'adam', lr=1e-5)
scaler = DynamicLossScale.static(1.0)
opt_old = torch.optim.Adam(ft_old.parameters(), lr=1e-5, fused=True)
grads_old = [p.grad for p in ft_old.parameters()]
inv_scale = torch.ones((), device='cuda')


def fused():
    opt_new.step(scaler=scaler)


def update():
    opt_upd.step()


def parent():
    found_inf = torch.zeros((), device='cuda')
    torch._amp_foreach_non_finite_check_and_unscale_(grads_old, found_inf, inv_scale)
    opt_old.grad_scale, opt_old.found_inf = None, found_inf
    try:
        opt_old.step()
    finally:
        del opt_old.grad_scale, opt_old.found_inf


cols = {'fused': (fused, 32), 'update': (update, 28), 'parent': (parent, 36)}
for fn, _ in cols.values():
    for _ in range(a.warmup):
        fn()
torch.cuda.synchronize()
rounds = {k: [] for k in cols}
for _ in range(a.rounds):
    for k, (fn, _) in cols.items():
        rounds[k].append(timed(fn))
res = dict(metric='optimizer_tail', tensors=len(list(ft_new.parameters())), elements=numel, chunks=opt_new._nchunks, steps=a.steps, hbm_ceiling_gbs=HBM_CEILING_GBS)
for k, (_, bytes_per_elem) in cols.items():
    ms = sorted(rounds[k])[len(rounds[k]) // 2]
    res[k + '_ms_rounds'] = [round(m, 4) for m in rounds[k]]
    res[k + '_ms'] = round(ms, 4)
    res[k + '_bytes_per_element'] = bytes_per_elem
    res[k + '_gbs'] = round(bytes_per_elem * numel / ms / 1e6, 1)
    res[k + '_share_of_hbm_ceiling'] = round(res[k + '_gbs'] / HBM_CEILING_GBS, 3)
res['fused_over_parent_time'] = round(res['fused_ms'] / res['parent_ms'], 3)
print(json.dumps(res))
