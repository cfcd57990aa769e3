"""Generate the non-local TRAINING fixture by RUNNING THE REFERENCE's NonLocalBlock in train() under torch autograd in the authoring container.

    python tests/golden/make_nl_train_golden.py      # writes tests/golden/nl_train_golden.npz / nl_train_golden_meta.json

The reference is imported in place (never copied); recorded results only are stored. The two block cases, their inputs and their weights are those of
nl_golden_meta.json (tests/golden/make_nl_golden.py), rebuilt from `ted_spad_amd.synth` through tests/nl_ref.nl_state_dict with the stored gains; the
upstream gradient is synth_tensor(seed, name + "/dy", shape, -1, 1).

Stored per case and tensor -- the output, d(input), the running statistics after the forward, the ten parameter gradients -- as `<case>/<tensor>/norm`
(L2 norm, float64) and `<case>/<tensor>/sample` (the fixed strided sample of tests/nl_grad_ref.sample_index, fp32 as the reference computed it).
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

from _refimport import import_reference  # noqa: E402
import nl_grad_ref  # noqa: E402
import nl_ref  # noqa: E402
from ted_spad_amd.synth import synth_tensor  # noqa: E402


def main():
    torch.set_num_threads(os.cpu_count())
    import_reference()
    from aux_code.models import large_i3d as ref
    with open(os.path.join(HERE, "nl_golden_meta.json")) as fh:
        src = json.load(fh)
    seed = src["seed"]
    out, meta = {}, {"seed": seed, "torch": torch.__version__, "cases": {}}

    def put(key, t):
        t = t.detach().flatten()
        out[key + "/norm"] = np.float64(float(t.double().norm()))
        out[key + "/sample"] = t[nl_grad_ref.sample_index(t.numel())].float().numpy()

    for name, b in src["blocks"].items():
        p = name + ".nl."
        blk = ref.NonLocalBlock(*b["dims"])
        tmpl = OrderedDict((p + k, v) for k, v in blk.state_dict().items())
        sd = nl_ref.nl_state_dict(tmpl, seed, {p: b["gain"]})
        blk.load_state_dict(OrderedDict((k[len(p):], v) for k, v in sd.items()), strict=True)
        blk.train()
        x = synth_tensor(seed, name + "/in", tuple(b["input"]), -1.0, 1.0).requires_grad_()
        dy = synth_tensor(seed, name + "/dy", tuple(b["input"]), -1.0, 1.0)
        y = blk(x)
        y.backward(dy)
        put(name + "/out", y)
        put(name + "/dx", x.grad)
        put(name + "/running_mean", blk.bn.running_mean)
        put(name + "/running_var", blk.bn.running_var)
        for k in nl_grad_ref.PARAMS:
            mod, leaf = k.split(".")
            put(name + "/grad/" + k, getattr(getattr(blk, mod), leaf).grad)
        assert int(blk.bn.num_batches_tracked) == 1
        meta["cases"][name] = {"dims": b["dims"], "input": b["input"], "gain": b["gain"], "momentum": blk.bn.momentum, "eps": blk.bn.eps,
                               "dy_abs_sum": float(dy.double().abs().sum())}

    np.savez_compressed(os.path.join(HERE, "nl_train_golden.npz"), **out)
    with open(os.path.join(HERE, "nl_train_golden_meta.json"), "w") as fh:
        json.dump(meta, fh, indent=1, sort_keys=True)
    print("wrote %d entries, %d bytes" % (len(out), os.path.getsize(os.path.join(HERE, "nl_train_golden.npz"))))


if __name__ == "__main__":
    main()
