"""Validation of the action classifier on 1 MI355X: ActionValidator.evaluate at the reference's validation batch shape
(params_anonymization.py: v_batch_size 8, 3 x 16 frames of 224 x 224 from the contrastive loader, unet++ in front of largei3d; --temporal adds
the triplet term of train_anonymized_action.py:158-165 and its two further ft forwards).
Prints a JSON line with ms per batch and clips/s of `evaluate` and of the bare forward composed by hand (fa, ft on the first clip), then the same
line completed by the number of kernel launches of each as the torch profiler counts them -- their difference (less the two further ft forwards of --temporal) is
what `evaluate` adds behind the ft forward."""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # the repository root
from ted_spad_amd.action_eval import ActionValidator
from ted_spad_amd.model_loaders import load_fa_model, load_ft_model
from ted_spad_amd.synth import synth_state_dict, synth_train_video

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=8)
ap.add_argument('--frames', type=int, default=48)
ap.add_argument('--res', type=int, default=224)
ap.add_argument('--fa', default='unet++')
ap.add_argument('--temporal', action='store_true')
ap.add_argument('--steps', type=int, default=10)
ap.add_argument('--warmup', type=int, default=45)   # the tile tuner needs up to ~40 calls per conv geometry
a = ap.parse_args()

with contextlib.redirect_stdout(io.StringIO()):
    fa = load_fa_model(arch=a.fa)
    ft = load_ft_model('largei3d', num_classes=102)
fa.load_state_dict(synth_state_dict(fa.state_dict(), 0))
ft.load_state_dict(synth_state_dict(ft.state_dict(), 0))
fa, ft = fa.cuda().eval(), ft.cuda().eval()
x = synth_train_video(0, 'action_val_probe', (a.batch, a.frames, 3, a.res, a.res), device='cuda')
labels = [i % 102 for i in range(a.batch)]
paths = ['/data/val/v_%03d.avi' % (i // 2) for i in range(a.batch)]                  # two clips per video
val = ActionValidator(ft, fa, temporal_loss=a.temporal)
clip16 = synth_train_video(0, 'action_val_probe_clip', (a.batch, 16, 3, a.res, a.res), device='cuda').permute(0, 2, 1, 3, 4)


def evaluate():
    val.evaluate(x, labels, paths)


def bare():
    with torch.no_grad():
        v = x.permute(0, 2, 1, 3, 4)
        anon = fa(v.reshape(-1, v.shape[1], v.shape[3], v.shape[4])).reshape(v.shape)
        ft(anon[:, :, :16])


def ft_only():
    with torch.no_grad():
        ft(clip16)


def timed(fn):
    for _ in range(a.warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / a.steps


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and 'memcpy' not in e.name.lower() and 'memset' not in e.name.lower())


res = dict(metric='action_val_evaluate', batch=a.batch, frames=a.frames, res=a.res, fa=a.fa, temporal=a.temporal, steps=a.steps)
ms = timed(evaluate)
res['evaluate_ms_per_batch'] = round(ms, 3)
res['evaluate_clips_per_s'] = round(a.batch * 1e3 / ms, 1)
val.reset()
ms = timed(bare)
res['bare_forward_ms_per_batch'] = round(ms, 3)
res['bare_forward_clips_per_s'] = round(a.batch * 1e3 / ms, 1)
print(json.dumps(res), flush=True)
evaluate()                                                            # (the first batch after reset() also zero-fills the new vote buffers)
res['evaluate_launches'] = launches(evaluate)
res['bare_forward_launches'] = launches(bare)
res['ft_forward_launches'] = launches(ft_only)
res['launches_added'] = res['evaluate_launches'] - res['bare_forward_launches'] - (2 * res['ft_forward_launches'] if a.temporal else 0)
print(json.dumps(res))
