"""The privacy classifier (privacy_training/train_privacy.py) on 1 MI355X: PrivacyTrainStep.step at params_privacy.py's batch 32 x 3 x 224^2, raw
images (`anon = False`) and behind a frozen unet++ anonymizer (`anon = True`), plus PrivacyTrainStep.evaluate throughput.
Prints one JSON line: ms/step and images/s of each form, and the fb training step's algorithmic TFLOP/s as a fraction of the dense f16 MFMA
peak (ResNet-50 conv + fc MACs x 2 FLOP x 3 for forward, data gradient and weight gradient; the anonymizer's FLOPs are not counted)."""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # the repository root
from ted_spad_amd.model_loaders import load_fa_model, load_fb_model
from ted_spad_amd.privacy import PrivacyTrainStep
from ted_spad_amd.resnet50 import STAGES
from ted_spad_amd.synth import synth_state_dict, synth_tensor

PEAK_F16_TFLOPS = 2500.0          # MI355X dense FP16 / BF16 matrix peak (spec)

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=32)
ap.add_argument('--res', type=int, default=224)
ap.add_argument('--steps', type=int, default=10)
ap.add_argument('--warmup', type=int, default=45)   # the tile tuner needs up to ~40 calls per conv geometry
a = ap.parse_args()


def resnet50_macs(h, w, num_classes=7):
    """Multiply-adds of one (3,h,w) image through ResNet-50 (torchvision layout) + fc."""
    out = lambda n, k, s, p: (n + 2 * p - k) // s + 1
    h, w = out(h, 7, 2, 3), out(w, 7, 2, 3)
    macs = h * w * 64 * 3 * 49
    h, w = out(h, 3, 2, 1), out(w, 3, 2, 1)
    cin = 64
    for planes, blocks, stride in STAGES:
        for i in range(blocks):
            s = stride if i == 0 else 1
            ho, wo = out(h, 3, s, 1), out(w, 3, s, 1)
            macs += h * w * cin * planes + ho * wo * planes * planes * 9 + ho * wo * planes * planes * 4
            if i == 0:
                macs += ho * wo * cin * planes * 4
            h, w, cin = ho, wo, planes * 4
    return macs + cin * num_classes


def fb_model():
    with contextlib.redirect_stdout(io.StringIO()):
        fb = load_fb_model(arch='r50', ssl=False, pretrained=False, num_pa=7)
    fb.load_state_dict(synth_state_dict(fb.state_dict(), 0))
    return fb.cuda()


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


gain = (torch.arange(1, a.batch + 1, device='cuda').float() / a.batch).view(-1, 1, 1, 1)
x = synth_tensor(0, 'bench_vispr', (a.batch, 3, a.res, a.res), device='cuda') * gain
y = (synth_tensor(0, 'bench_pa', (a.batch, 7), device='cuda') > 0.7).float()
train_flop = 3 * 2 * resnet50_macs(a.res, a.res) * a.batch
res = dict(metric='privacy_train_step', batch=a.batch, res=a.res, steps=a.steps, train_tflop_per_step=round(train_flop / 1e12, 4))

step = PrivacyTrainStep(fb_model())
ms = timed(lambda: step.step(x, y), a.steps, a.warmup)
res['plain_ms_per_step'] = round(ms, 3)
res['plain_images_per_s'] = round(a.batch * 1e3 / ms, 1)
res['plain_tflops'] = round(train_flop / ms / 1e9, 1)
res['plain_mfma_fraction'] = round(train_flop / ms / 1e9 / PEAK_F16_TFLOPS, 4)
ms = timed(lambda: step.evaluate(x, y), a.steps, a.warmup)
res['evaluate_ms_per_batch'] = round(ms, 3)
res['evaluate_images_per_s'] = round(a.batch * 1e3 / ms, 1)

with contextlib.redirect_stdout(io.StringIO()):
    fa = load_fa_model(arch='unet++')
fa.load_state_dict(synth_state_dict(fa.state_dict(), 0))
for p in fa.parameters():
    p.requires_grad = False
step = PrivacyTrainStep(fb_model(), fa_model=fa.cuda().eval())
ms = timed(lambda: step.step(x, y), a.steps, a.warmup)
res['anon_unetpp_ms_per_step'] = round(ms, 3)
res['anon_unetpp_images_per_s'] = round(a.batch * 1e3 / ms, 1)
print(json.dumps(res))
