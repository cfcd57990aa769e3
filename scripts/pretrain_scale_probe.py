"""Which binade should the L1 gradient g = loss_scale / numel live in? (pretrain.GRAD_BINADE; DESIGN.md "Reconstruction pre-training")

Stage 1, 6 x 3 x 64 x 64, smooth weights, deterministic mode: for k in --ks the fused forward / loss / backward with loss_scale = the power of two that puts g
into [2^-k, 2^(1-k)), its unscaled parameter gradients against the fp32 oracle's (oracle/unetpp_ref.py) for dy = sign(yy - x) / numel, yy the device's own output.
Stage 2, 32 x 3 x 224 x 224: one ReconstructionTrainStep.step per k (and with the constant scale 256): skipped? how many on-path parameter gradients are all zero?
Prints one JSON line."""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # the repository root
from oracle import unetpp_ref
from ted_spad_amd import engine as E, train_engine as TE
from ted_spad_amd.losses import l1_train
from ted_spad_amd.model_loaders import load_fa_model
from ted_spad_amd.pretrain import ReconstructionTrainStep
from ted_spad_amd.synth import synth_state_dict, synth_tensor
from ted_spad_amd.train_nets import UNetPPTrainer

ap = argparse.ArgumentParser()
ap.add_argument('--ks', type=int, nargs='+', default=[4, 6, 8, 10])
a = ap.parse_args()


def model(smooth):
    with contextlib.redirect_stdout(io.StringIO()):
        fa = load_fa_model()
    sd = synth_state_dict(fa.state_dict(), 0)
    if smooth:            # every BatchNorm bias +4: the ReLUs are (nearly) the identity, so the fp32 oracle takes the device's branches
        for k in sd:
            if k.rsplit('.', 1)[0] + '.running_mean' in sd and k.endswith('.bias'):
                sd[k] = torch.full_like(sd[k], 4.0)
    fa.load_state_dict(sd)
    return fa.cuda(), sd


def scale_for_k(numel, k):
    return 2.0 ** ((numel - 1).bit_length() - k)


res = dict(metric='pretrain_loss_scale', small=[], full=[])
shape = (6, 3, 64, 64)
numel = int(np.prod(shape))
x = synth_tensor(0, 'recon', shape)
E.set_deterministic(True)
ref = None
for k in a.ks:
    fa, sd = model(True)
    scale = scale_for_k(numel, k)
    TE.ARENA.reset(torch.device('cuda'))
    tr = UNetPPTrainer(fa.train())
    y, tape = tr.forward(x.cuda(), nchw=False)
    loss, dl, yy = l1_train(y, x.cuda(), scale, want_y32=True)
    tr.backward(tape, dl=dl)
    tr.flush_grads()
    if ref is None:       # the forward does not depend on the scale: one oracle pass serves every k
        sdg = {n: (v.clone().requires_grad_() if v.is_floating_point() and 'running' not in n else v) for n, v in sd.items()}
        yr = unetpp_ref.forward(x, sdg, train=True)
        yr.backward(torch.sign(yy.cpu() - x) / numel)
        ref = {n: v.grad for n, v in sdg.items() if v.requires_grad and v.grad is not None}
    errs = []
    for n, p in fa.named_parameters():
        if n in ref and float(ref[n].norm()) > 1e-4:
            g = (p.grad / scale).cpu().double()
            errs.append(float((g - ref[n].double()).norm() / ref[n].double().norm()))
    res['small'].append(dict(k=k, loss_scale=scale, g=scale / numel, median_rel_l2=float(np.median(errs)), max_rel_l2=max(errs), finite=bool(all(np.isfinite(errs)))))
assert E.deterministic_giveups() == 0
E.set_deterministic(False)

shape = (32, 3, 224, 224)
numel = int(np.prod(shape))
x = (synth_tensor(0, 'recon224', shape) * (torch.arange(1, 33).float() / 32).view(-1, 1, 1, 1)).cuda()
for k in list(a.ks) + [None]:
    fa, _ = model(False)
    scale = 256.0 if k is None else scale_for_k(numel, k)
    step = ReconstructionTrainStep(fa, loss_scale=scale)
    out = step.step(x)
    off = {id(p) for p in step.fa_tr.off_path_params()}
    on = [(n, p) for n, p in fa.named_parameters() if id(p) not in off]
    dead = [n for n, p in on if p.grad is None or not bool((p.grad != 0).any())]
    gmax = max(float(p.grad.abs().max()) for n, p in on if p.grad is not None)
    res['full'].append(dict(k=k, loss_scale=scale, g=scale / numel, loss=out['loss'], skipped=bool(out['skipped']), all_zero_grads=len(dead), on_path=len(on),
                            max_abs_unscaled_grad=gmax))
print(json.dumps(res))
