"""Reconstruction pre-training of the unet++ anonymizer (fa_pretraining/train_reconstruction.py) on 1 MI355X at parameters.py's batch 32 x 3 x 224^2:
  step      ReconstructionTrainStep.step (16-bit ends, the fused L1 loss / gradient kernel)
  pieces    the same step assembled from what existed before it: tr.forward -> fp32 NCHW, torch's L1 loss, loss.backward(), tr.backward(tape, dy) with
            the same loss scale, the same unscale / fused-Adam tail
  evaluate  ReconstructionTrainStep.evaluate per batch
Prints one JSON line (ms per call, images/s)."""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # the repository root
from ted_spad_amd.model_loaders import load_fa_model
from ted_spad_amd.pretrain import ReconstructionTrainStep
from ted_spad_amd.synth import synth_state_dict, synth_tensor

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=32)
ap.add_argument('--res', type=int, default=224)
ap.add_argument('--steps', type=int, default=10)
ap.add_argument('--warmup', type=int, default=45)   # the tile tuner needs up to ~40 calls per conv geometry
ap.add_argument('--rounds', type=int, default=5)
a = ap.parse_args()


def fa_model():
    with contextlib.redirect_stdout(io.StringIO()):
        fa = load_fa_model(arch='unet++')
    fa.load_state_dict(synth_state_dict(fa.state_dict(), 0))
    return fa.cuda()


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def pieces_step(step, x):
    """`step.step` with the loss outside the library: fp32 NCHW output, torch's sub / abs / mean and their autograd backward, the fp32 gradient converted back."""
    step.fa.train()
    step._begin(x.device, (step.opt,))
    step.red.prepare(exclude=step._off_path)
    step.loss_scale = step.scale_for(x)
    y, tape = step.fa_tr.forward(x)
    y.requires_grad_()
    loss = torch.nn.functional.l1_loss(y, x)
    step._post(dict(loss=loss))
    (loss * step.loss_scale).backward()
    step.fa_tr.backward(tape, y.grad, on_bucket_done=step.red.bucket_ready)
    v, skipped = step._end(step.fa_tr, step.red, step.opt, step.fa)
    return dict(loss=v['loss'], skipped=skipped)


gain = (torch.arange(1, a.batch + 1, device='cuda').float() / a.batch).view(-1, 1, 1, 1)
x = synth_tensor(0, 'bench_recon', (a.batch, 3, a.res, a.res), device='cuda') * gain
res = dict(metric='reconstruction_train_step', batch=a.batch, res=a.res, steps=a.steps)

step, old = ReconstructionTrainStep(fa_model()), ReconstructionTrainStep(fa_model())
res['loss_scale'] = step.scale_for(x)
for _ in range(a.warmup):
    step.step(x)
    pieces_step(old, x)
rounds = {'step': [], 'pieces': []}
for _ in range(a.rounds):                             # alternating rounds: a drift of the clock or the box shows in both columns
    rounds['step'].append(timed(lambda: step.step(x), a.steps, 2))
    rounds['pieces'].append(timed(lambda: pieces_step(old, x), a.steps, 2))
for name, v in rounds.items():
    res[name + '_ms_rounds'] = [round(m, 3) for m in v]
    res[name + '_ms'] = round(sorted(v)[len(v) // 2], 3)
    res[name + '_images_per_s'] = round(a.batch * 1e3 / res[name + '_ms'], 1)
ms = timed(lambda: step.evaluate(x), a.steps, min(a.warmup, 10))
res['evaluate_ms_per_batch'] = round(ms, 3)
res['evaluate_images_per_s'] = round(a.batch * 1e3 / ms, 1)
print(json.dumps(res))
