"""Generate the non-local fixture by RUNNING THE REFERENCE's I3Res50(use_nl=True) and NonLocalBlock in the authoring container.

    python tests/golden/make_nl_golden.py            # writes tests/golden/nl_golden.npz / nl_golden_meta.json

The reference is imported in place (never copied); outputs and settings only are stored. Weights and clips are regenerated on both sides from
`ted_spad_amd.synth` through tests/nl_ref.nl_state_dict.

Default-initialised (and plainly synth-filled) non-local blocks are useless as a fixture: from layer3.1 on every softmax is a one-hot argmax (scaled
logits with a standard deviation in the hundreds), any 16-bit rounding flips its winner, and the activations grow past f16. So the weights are
CALIBRATED on the fp32 reference: in one pass over the fixture clip, block by block, theta's and phi's weights and biases are scaled by one gain
per block until the scaled logits have the standard deviation LOGIT_STD; nl.bn.weight is drawn from [0.1, 0.3]. The gains, the resulting logit
statistics and the mean largest probability per block go into the meta JSON; the tests rebuild the same weights from the gains.

What is captured:
  nl_feat_112         fp32 feature (1, 2048) of the non-local network on the 16x112^2 synth clip; meta: (mean, abs-mean) of the five nl outputs
  nl_block512_out     NonLocalBlock(512, 512, 256) on a synth (2, 512, 2, 7, 7) input, full output
  nl_block1024_out    NonLocalBlock(1024, 1024, 512) on a synth (1, 1024, 2, 7, 7) input, full output
"""
import json
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from _refimport import REFERENCE_ROOT, import_reference  # noqa: E402
import nl_ref  # noqa: E402
from ted_spad_amd.synth import synth_clips, synth_tensor  # noqa: E402

SEED = 0
LOGIT_STD = 2.0      # calibration target: std of the scaled logits of every block
BLOCKS = {"nl_block512": ((512, 512, 256), (2, 512, 2, 7, 7)), "nl_block1024": ((1024, 1024, 512), (1, 1024, 2, 7, 7))}


def calibrate(mod, x, target):
    """Scale theta / phi of the reference block `mod` in place so that its scaled logits on input `x` have std `target`; returns the gain (an fp32 value)."""
    with torch.no_grad():
        n = x.shape[0]
        th = mod.theta(x).view(n, mod.dim_inner, -1)
        ph = mod.phi(mod.maxpool(x)).view(n, mod.dim_inner, -1)
        s = torch.bmm(th.transpose(1, 2), ph) * (mod.dim_inner ** -.5)
        gain = float(np.float32((target / float(s.double().std())) ** 0.5))
        for p in (mod.theta.weight, mod.theta.bias, mod.phi.weight, mod.phi.bias):
            p.mul_(torch.tensor(gain, dtype=torch.float32))
    return gain


def main():
    torch.set_num_threads(os.cpu_count())
    import_reference()
    from aux_code.models import large_i3d as ref
    meta = {"seed": SEED, "torch": torch.__version__, "reference": REFERENCE_ROOT, "logit_std_target": LOGIT_STD}
    out = {}

    # ---- the network: weights under the wrapper's key names (`i3d.` prefix), as the other fixtures' ----
    net = ref.I3Res50(num_classes=102, use_nl=True)
    keys = list(net.state_dict().keys())
    meta["state_dict"] = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    meta["nl_blocks"] = [n[:-3] for n, m in net.named_modules() if isinstance(m, ref.NonLocalBlock)]
    tmpl = OrderedDict(("i3d." + k, v) for k, v in net.state_dict().items())
    strip = lambda sd: OrderedDict((k[4:], v) for k, v in sd.items())
    net.load_state_dict(strip(nl_ref.nl_state_dict(tmpl, SEED)), strict=True)
    net.eval()
    x = synth_clips(SEED, 1, (3, 16, 112, 112))
    gains = {}
    nls = [(n, m) for n, m in net.named_modules() if isinstance(m, ref.NonLocalBlock)]
    hs = [m.register_forward_pre_hook(lambda m, i, n=n: gains.__setitem__("i3d." + n + ".", calibrate(m, i[0], LOGIT_STD))) for n, m in nls]
    with torch.no_grad():
        net.extract_features(x)                       # the calibration pass: every block is scaled before it runs, so later blocks see calibrated inputs
    for h in hs:
        h.remove()
    sd = nl_ref.nl_state_dict(tmpl, SEED, gains)      # what the tests rebuild
    for k, v in net.state_dict().items():
        assert torch.equal(v, sd["i3d." + k]), k
    stats, taps = {}, {}
    hs = [m.register_forward_pre_hook(lambda m, i, n=n: stats.__setitem__(n, nl_ref.logit_stats(i[0], sd, "i3d." + n + "."))) for n, m in nls]
    hs += [m.register_forward_hook(lambda m, i, o, n=n: taps.__setitem__(n, [float(o.double().mean()), float(o.double().abs().mean()), float(o.abs().max())]))
           for n, m in nls]
    with torch.no_grad():
        f = net.extract_features(x)
    for h in hs:
        h.remove()
    out["nl_feat_112"] = f.reshape(1, 2048).numpy()
    meta["gains"] = gains
    meta["logit_std"] = {n: s[0] for n, s in stats.items()}
    meta["mean_max_prob"] = {n: s[1] for n, s in stats.items()}
    meta["taps_112"] = {n: t[:2] for n, t in taps.items()}
    meta["tap_abs_max"] = {n: t[2] for n, t in taps.items()}
    assert keys == [k for k, _ in meta["state_dict"]]

    # ---- the two block shapes on their own ----
    meta["blocks"] = {}
    for name, (dims, xshape) in BLOCKS.items():
        blk = ref.NonLocalBlock(*dims).eval()
        tb = OrderedDict((name + ".nl." + k, v) for k, v in blk.state_dict().items())
        unp = lambda sd_: OrderedDict((k[len(name) + 4:], v) for k, v in sd_.items())
        blk.load_state_dict(unp(nl_ref.nl_state_dict(tb, SEED)), strict=True)
        xb = synth_tensor(SEED, name + "/in", xshape, -1.0, 1.0)
        gain = calibrate(blk, xb, LOGIT_STD)
        sdb = nl_ref.nl_state_dict(tb, SEED, {name + ".nl.": gain})
        for k, v in blk.state_dict().items():
            assert torch.equal(v, sdb[name + ".nl." + k]), k
        with torch.no_grad():
            yb = blk(xb)
        st = nl_ref.logit_stats(xb, sdb, name + ".nl.")
        out[name + "_out"] = yb.numpy()
        meta["blocks"][name] = {"dims": list(dims), "input": list(xshape), "gain": gain, "logit_std": st[0], "mean_max_prob": st[1]}

    np.savez_compressed(os.path.join(HERE, "nl_golden.npz"), **out)
    with open(os.path.join(HERE, "nl_golden_meta.json"), "w") as fh:
        json.dump(meta, fh, indent=1, sort_keys=True)
    print("wrote", {k: v.shape for k, v in out.items()})
    print(json.dumps({k: meta[k] for k in ("gains", "logit_std", "mean_max_prob", "tap_abs_max", "blocks")}, indent=1))


if __name__ == "__main__":
    main()
