"""Shared by tests/test_hip_resume.py (MI355X) and tests/test_resume_host.py (CPU): what a training run's state IS, collected into one flat
`name -> value` dict, and the bit-for-bit comparison of two such dicts that names everything that differs.

    step_record(result)                      a step driver's result dict as plain Python values (floats, bools, tuples)
    losses(records, first)                   {"loss/step<i>/<key>": value}
    snapshot(modules, optimizers, scaler)    parameters, buffers, optimizer state, learning rate, loss scale -- cloned, on their device
    differences(got, want)                   one message per name that differs (kernel_refs.first_mismatch's words for tensors)
    assert_same / assert_differs             the whole list in one assertion message / "this part must NOT be equal" (the `wrong=` habit)
    bias_words_running / bias_words_loaded   the two ways ted_spad_amd.optim forms Adam's bias-correction words, restated

Names: "<module>/param/<name>", "<module>/buffer/<name>", "<optimizer>/state/<parameter name>/<key>", "<optimizer>/lr",
"<optimizer>/steps_applied", "<optimizer>/words[0:4]", "scaler/<key>", "loss/step<i>/<key>".
"""
import numpy as np
import torch

from kernel_refs import first_mismatch


def _plain(v):
    if torch.is_tensor(v):
        return float(v) if v.dim() == 0 else tuple(v.detach().cpu().reshape(-1).tolist())
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if isinstance(v, (np.floating, np.integer)):
        return v.item()
    return bool(v)                                                    # train_step.DeviceFlag


def step_record(result: dict) -> dict:
    """Every entry of a step's result as a plain Python value: a loss stays the float the driver read back, `skipped` becomes a bool, a device tensor
    (`pred`, `grad_scale`, MGFN's scores and indices) its exact values."""
    return {k: _plain(v) for k, v in result.items()}


def losses(records, first=0) -> dict:
    return {"loss/step%d/%s" % (first + i, k): v for i, r in enumerate(records) for k, v in r.items()}


def _clone(t):
    return t.detach().clone()


def snapshot(modules: dict, optimizers: dict, scaler=None, steps_base: int = 0) -> dict:
    """modules: name -> nn.Module; optimizers: name -> (optimizer, the module whose `parameters()` order its state indices follow).

    Optimizer state is read through `state_dict()` (torch's layout, which optim.FusedOptimizer writes too): every tensor of every entry, under the
    parameter's name. A FusedOptimizer adds `steps_applied()` and words 0..3 of its device state -- the found-inf flag, the step count and the two fp32 bias
    corrections the update kernel reads.

    Words 4..7 are left out: they are the double powers beta^(t+1), which a running optimizer forms by repeated multiplication (optim_finish_kernel) and
    a loaded one as `beta ** (t + 1)` (FusedOptimizer._write_state); the two doubles differ in their last bits from t = 3 on, and nothing but words 2
    and 3 is ever derived from them (tests/test_resume_host.py::test_bias_correction_words_do_not_depend_on_how_the_powers_were_formed).

    An SGD FusedOptimizer has no step count in torch's layout (torch.optim.SGD keeps none), so its counter restarts at 0 on a load and its Adam words are
    unused: for `opt_type == 'sgd'` the snapshot holds the steps applied since `steps_base` (the count at the save, 0 for a loaded optimizer) and the
    found-inf word alone."""
    out = {}
    for mname, m in modules.items():
        for k, p in m.named_parameters():
            out["%s/param/%s" % (mname, k)] = _clone(p)
        for k, b in m.named_buffers():
            out["%s/buffer/%s" % (mname, k)] = _clone(b)
    for oname, (opt, module) in optimizers.items():
        names = [k for k, _ in module.named_parameters()]
        sd = opt.state_dict()
        if len(sd["param_groups"]) != 1 or list(sd["param_groups"][0]["params"]) != list(range(len(names))):
            raise ValueError("snapshot: %s is not one parameter group over %d parameters" % (oname, len(names)))
        out["%s/lr" % oname] = float(sd["param_groups"][0]["lr"])
        for i, st in sd["state"].items():
            for key, v in st.items():
                out["%s/state/%s/%s" % (oname, names[int(i)], key)] = _clone(v) if torch.is_tensor(v) else v
        if hasattr(opt, "steps_applied"):                             # optim.FusedOptimizer
            sgd = opt.opt_type == "sgd"
            out["%s/steps_applied" % oname] = opt.steps_applied() - (steps_base if sgd else 0)
            words = None if opt._state is None else _clone(opt._state[:1] if sgd else opt._state[:4])
            out["%s/words[0:%d]" % (oname, 1 if sgd else 4)] = words
    if scaler is not None:
        for k, v in scaler.state_dict().items():
            out["scaler/%s" % k] = v
    return out


def differences(got: dict, want: dict) -> list:
    """One message per name whose value is not the same bits on both sides (or that only one side has)."""
    msgs = []
    for k in list(want) + [k for k in got if k not in want]:
        if k not in got or k not in want:
            msgs.append("%s: only in %s" % (k, "the reference run" if k in want else "this run"))
            continue
        a, b = got[k], want[k]
        if torch.is_tensor(a) != torch.is_tensor(b):
            msgs.append("%s: got %s, want %s" % (k, type(a).__name__, type(b).__name__))
        elif torch.is_tensor(a):
            if a.shape != b.shape or a.dtype != b.dtype:
                msgs.append("%s: got %s %s, want %s %s" % (k, a.dtype, tuple(a.shape), b.dtype, tuple(b.shape)))
                continue
            a = a.to(b.device)
            msg = first_mismatch(a.reshape(-1), b.reshape(-1)) if a.numel() else ""
            if not msg and not torch.equal(a, b):
                msg = "not torch.equal"
            if msg:
                msgs.append("%s: %s" % (k, msg))
        elif not (a == b):
            msgs.append("%s: got %r, want %r" % (k, a, b))
    return msgs


def assert_same(got: dict, want: dict, what: str, show: int = 40):
    msgs = differences(got, want)
    assert not msgs, "%s: %d of %d items differ\n  %s%s" % (what, len(msgs), len(want), "\n  ".join(msgs[:show]),
                                                             "\n  ... and %d more" % (len(msgs) - show) if len(msgs) > show else "")


def part(snap: dict, *needles) -> dict:
    """The entries whose name contains one of `needles` ("/param/", "/buffer/", "loss/", "scaler/", ...)."""
    sub = {k: v for k, v in snap.items() if any(n in k for n in needles)}
    assert sub, "no entry named like %s" % (needles,)
    return sub


def assert_differs(got: dict, want: dict, what: str, *needles):
    """The run that produced `got` left a piece of the state out: the part of the result named by `needles` must NOT be equal. If it is, the case does
    not exercise that piece of state and the equality tests beside it cannot see it being lost."""
    g, w = part(got, *needles), part(want, *needles)
    n = len(differences(g, w))
    print("%s: %d of %d items named like %s differ" % (what, n, len(w), needles))
    assert n > 0, "%s: every item named like %s is the same bits with and without it: the case does not exercise this state" % (what, needles)


# ---- Adam's bias-correction words: the two ways ted_spad_amd.optim forms them, restated ----------------------------------------------------
def bias_words_loaded(t: int, betas=(0.9, 0.999)):
    """FusedOptimizer._write_state(t): (p1, p2) as Python doubles `beta ** (t + 1)`, and the two fp32 words derived from them, as their bits."""
    p1, p2 = betas[0] ** (t + 1), betas[1] ** (t + 1)
    return (p1, p2), (np.float32(1.0 - p1).view(np.uint32).item(), np.float32((1.0 - p2) ** 0.5).view(np.uint32).item())


def bias_words_running(t: int, betas=(0.9, 0.999)):
    """optim_finish_kernel after t applied steps from a fresh state: the powers by repeated double multiplication, the words as
    (float)(1.0 - b1) and (float)sqrt(1.0 - b2) (a correctly rounded double square root)."""
    p1, p2 = np.float64(betas[0]), np.float64(betas[1])              # _write_state(0): beta ** 1
    for _ in range(t):
        p1, p2 = p1 * np.float64(betas[0]), p2 * np.float64(betas[1])
    return (float(p1), float(p2)), (np.float32(1.0 - p1).view(np.uint32).item(), np.float32(np.sqrt(1.0 - p2)).view(np.uint32).item())
