"""-m gpu: a training run that is stopped, written to a file, read back and continued gives the bits of the run that never stopped -- for every step driver
(AnonymizerTrainStep, ActionTrainStep, ReconstructionTrainStep, PrivacyTrainStep, MGFNTrainStep) and both ways of loading:

    A  uninterrupted   K steps, the checkpoint is written (the project's own writer where one exists), M more steps (K = M = 2)
    B  restart         fresh models through model_loaders.load_*_model(saved_model_file=...), a fresh driver, load_state_dict on its optimizer(s) / scaler, M steps
    C  rollback        load_state_dict on A's LIVE modules, optimizers and scaler after its M steps, the same M steps again

A == B and A == C under torch.equal (resume_helpers.snapshot: every loss, parameter, buffer, optimizer tensor, learning rate, the scaler, a FusedOptimizer's
step count and bias-correction words). No tolerance: in deterministic mode with the tile tuner off two runs from the same state execute the same arithmetic in
the same order (test_hip_train_step.py::test_deterministic_mode_repeats_bit_for_bit), MGFN training is deterministic by construction, and a weight image
refreshed in place equals a fresh pack (test_hip_refresh.py). What a load can lose without anything in `state_dict()` showing it -- stale weight images and
BatchNorm folds, data-gradient plans, a restarted step counter, a loss scale without its growth tracker -- shows as a differing bit here.

Every step index has its own input batch (a run that replays the wrong step shows), dropout masks are passed in (no RNG takes part). The learning rates are
1e-3 where the drivers' defaults are 1e-5: a step then moves every element of the 16-bit weight images (a weight of 0.05 has an f16 spacing of 3e-5), so an
image that was not rebuilt after a load cannot go unnoticed. Shapes are the smallest the suite already runs each driver at.

The `omit` cases run arm B once more with one piece of the state left out, for one step, and assert that the named part of the result is NOT equal: the
comparison can fail, and each case does exercise that piece."""
import time
from types import SimpleNamespace

import pytest
import torch

import resume_helpers as H
from ted_spad_amd.synth import synth_mgfn_state_dict, synth_state_dict, synth_tensor, synth_train_video

pytestmark = pytest.mark.gpu

_A = {}                    # case name -> arm A's record (one uninterrupted run per case, shared by the tests of that case)


@pytest.fixture(scope="module")
def ckpt_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("resume")
    yield d
    _A.clear()                                                        # the live models of every arm A, and their files (up to 0.8 GB each)
    for f in d.iterdir():
        f.unlink()
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def wall_time(request):
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    print("wall time %s: %.2f s" % (request.node.name, time.perf_counter() - t0))


def _smooth(sd, beta=4.0):
    for k in sd:
        if k.rsplit(".", 1)[0] + ".running_mean" in sd and k.endswith(".bias"):
            sd[k] = torch.full_like(sd[k], beta)
    return sd


def _synth_into(model, smooth=False):
    sd = synth_state_dict(model.state_dict(), 0)
    model.load_state_dict(_smooth(sd) if smooth else sd)
    return model.cuda()


def _without_buffers(sd):
    return {k: v for k, v in sd.items() if not k.endswith(("running_mean", "running_var", "num_batches_tracked"))}


def _load_models(builders: dict, keys: dict, path, ckpt, omit):
    """name -> module on the device. builders[name](saved_model_file) is the project's loader; with "buffers" in `omit` the module is built without a file and
    loaded non-strictly from the file's entry with the running statistics and `num_batches_tracked` dropped."""
    out = {}
    for name, build in builders.items():
        if "buffers" in omit:
            m = build(None)
            missing, unexpected = m.load_state_dict(_without_buffers(ckpt[keys[name]]), strict=False)
            assert missing and not unexpected and all(k.endswith(("running_mean", "running_var", "num_batches_tracked")) for k in missing)
        else:
            m = build(path)
        out[name] = m.cuda()
    return out


def _labels(b, n=4):
    return torch.tensor([(5 + 7 * b) % 102, (77 + b) % 102, (101 - b) % 102, (1 + 3 * b) % 102][:n]).cuda()


def _drop_masks(b, n, count):
    """`count` dropout masks for the (n, 2048) pooled feature in front of ft's classifier: 0 / 1 (I3DTrainer applies the 1 / (1 - p))."""
    return [(synth_tensor(b, "resume_drop%d" % i, (n, 2048)) >= 0.5).float().cuda() for i in range(count)]


class Case:
    """One driver at one configuration: how its objects are built (fresh, from a file, loaded live), saved and stepped."""
    name, omissions, smooth = None, (), False
    K, M = 2, 2                                                       # steps before the save, steps after it
    model_keys = {}                                                  # module name -> its key in the checkpoint
    opt_keys = {}                                                     # optimizer name -> its key in the checkpoint

    def builders(self):
        """name -> build(saved_model_file or None): the project's loader for that module."""
        raise NotImplementedError

    def driver(self, models):
        """-> SimpleNamespace(driver, opts: name -> (optimizer, module), scaler, ...) over `models`."""
        raise NotImplementedError

    def save(self, o, path):
        """Writes the checkpoint; returns the dict that was written."""
        raise NotImplementedError

    def step(self, o, s, batch=None):
        """Step `s` of the run on batch `s` (or on `batch`, for the wrong-batch omission). Returns the driver's result dict."""
        raise NotImplementedError

    def fresh(self):
        models = {name: _synth_into(build(None), smooth=self.smooth) for name, build in self.builders().items()}
        return self._objs(models)

    def _objs(self, models):
        o = self.driver(models)
        o.modules = models
        if not hasattr(o, "scaler"):
            o.scaler = None
        return o

    def restart(self, path, omit=frozenset()):
        ckpt = torch.load(path)
        o = self._objs(_load_models(self.builders(), self.model_keys, path, ckpt, omit))
        self.load_driver_state(o, ckpt, omit)
        return o

    def rollback(self, o, path):
        ckpt = torch.load(path)
        for name, m in o.modules.items():
            m.load_state_dict(ckpt[self.model_keys[name]])
        self.load_driver_state(o, ckpt, frozenset())

    def load_driver_state(self, o, ckpt, omit):
        if "optimizer" not in omit:
            for name, (opt, _) in o.opts.items():
                opt.load_state_dict(ckpt[self.opt_keys[name]])
        if o.scaler is not None and "scaler" not in omit:
            o.scaler.load_state_dict(ckpt["amp_scaler"])

    def steps_at_save(self, o):
        return 0

    def snap(self, o, base=0):
        # Everything a run's state is, EXCEPT words 4..7 of FusedOptimizer._state: the double powers beta^(t+1), which a running optimizer forms by repeated
        # multiplication (optim_finish_kernel) and a loaded one as beta ** (t + 1) (_write_state). The doubles differ in their last bits from t = 3 on; the
        # two fp32 bias corrections derived from them -- words 2 and 3, which ARE compared -- do not (tests/test_resume_host.py).
        return H.snapshot(o.modules, o.opts, o.scaler, steps_base=base)

    def verify(self, a):
        """Things that must have happened in arm A for the case to test what it is for."""


def _anon_params():
    from ted_spad_amd.train_step import DEFAULT_PARAMS
    return SimpleNamespace(**{**vars(DEFAULT_PARAMS), "learning_rate_fa": 1e-3, "learning_rate_fb": 1e-3, "learning_rate_ft": 1e-3})


class AnonymizerCase(Case):
    """AnonymizerTrainStep; one step = step_fa then step_ft. Video (4,48,3,64,64) -- the shape the suite runs phase 2 at (test_hip_fb.py,
    test_hip_train_step.py) -- and with fb two VISPR views (4,3,128,128). with_fb: UNet fa, the I3D wrapper, fb and three Adams: the rollback lands on
    trainers whose images the other phase's step rewrote in place, and on fb's train-mode statistics. Without: the default unet++ fa (UNetPPTrainer,
    `encoder.layer4` off the gradient path and without optimizer state)."""
    model_keys = {"fa": "fa_model_state_dict", "fb": "fb_model_state_dict", "ft": "ft_model_state_dict"}
    opt_keys = {"opt_fa": "optimizer_fa", "opt_fb": "optimizer_fb", "opt_ft": "optimizer_ft"}

    def __init__(self, with_fb):
        self.with_fb = with_fb
        self.name = "anonymizer_unet_fb" if with_fb else "anonymizer_unetpp"
        self.omissions = ("optimizer", "buffers", "batch") if with_fb else ()

    def builders(self):
        from ted_spad_amd.model_loaders import load_fa_model, load_fb_model, load_ft_model
        b = {"fa": lambda f: load_fa_model(saved_model_file=f, arch="unet" if self.with_fb else "unet++")}
        if self.with_fb:
            b["fb"] = lambda f: load_fb_model(arch="r50", saved_model_file=f, ssl=True)
        b["ft"] = lambda f: load_ft_model("largei3d", saved_model_file=f, num_classes=102)
        return b

    def driver(self, m):
        from ted_spad_amd.train_step import AnonymizerTrainStep
        d = AnonymizerTrainStep(m["fa"], m["ft"], params=_anon_params(), fb_model=m.get("fb"))
        opts = {"opt_fa": (d.opt_fa, m["fa"]), "opt_ft": (d.opt_ft, m["ft"])}
        if self.with_fb:
            opts["opt_fb"] = (d.opt_fb, m["fb"])
        return SimpleNamespace(driver=d, opts=opts)

    def save(self, o, path):
        from ted_spad_amd.checkpoint import save_anonymizer_checkpoint
        d = o.driver
        assert d.iteration % 2 == 0                                   # the phase parity starts afresh on a restart: the save is at an even iteration
        return save_anonymizer_checkpoint(path, self.K, o.modules["fa"], o.modules.get("fb"), o.modules["ft"], optimizers=(d.opt_fa, d.opt_fb, d.opt_ft))

    def step(self, o, s, batch=None):
        b = s if batch is None else batch
        video = synth_train_video(b, "resume_video64", (4, 48, 3, 64, 64)).cuda()
        labels = _labels(b)
        vispr = None
        if self.with_fb:
            gain = (torch.arange(1, 5).float() / 4).view(4, 1, 1, 1)
            vispr = [(synth_tensor(b, "resume_vispr%d" % i, (4, 3, 128, 128)) * gain).cuda() for i in range(2)]
        r1 = o.driver.step_fa(video, labels, vispr)
        r2 = o.driver.step_ft(video, labels, drop_masks=_drop_masks(b, 4, 3), inputs_vispr=vispr)
        return {**{"fa." + k: v for k, v in r1.items()}, **{"ft." + k: v for k, v in r2.items()}}

    def verify(self, a):
        assert not any(r["fa.skipped"] or r["ft.skipped"] for r in a.recs)
        off = [k for k in a.end if "/param/encoder.layer4." in k]
        if not self.with_fb:                                          # unet++: layer4 never had a gradient, torch keeps no state for it
            assert off and not any("opt_fa/state/encoder.layer4." in k for k in a.end)


def _action_params(**kw):
    from ted_spad_amd.train_step import DEFAULT_ACTION_PARAMS
    return SimpleNamespace(**{**vars(DEFAULT_ACTION_PARAMS), **kw})


# Measured with static scales at the synthetic weights: the f16 activation gradients of the raw-clip step first overflow at 2^21 on batches 0 and 1 and at 2^20 on
# batches 2 and 3; 2^19 passes on all four. The run starts a factor 2 above the first and backs off (x 1/16) to a factor 2 below the second.
# ActionRawCase.verify holds the run to the skip, the back-off and the growth this is meant to give.
ACTION_INIT_SCALE, ACTION_BACKOFF = 2.0 ** 22, 1.0 / 16


class ActionRawCase(Case):
    """ActionTrainStep on raw clips (4,16,3,64,64), AdamW with weight decay, a DynamicLossScale(growth_interval=3) that starts too high: step 0 overflows and is
    skipped (scale x backoff, tracker 0), step 1 is applied (tracker 1), the save; steps 2 and 3 are applied and the scale doubles after step 3. A restart that
    forgot the tracker would not grow; one that forgot the step count would redo Adam's first bias corrections. The mlp head and the frozen BatchNorm
    parameters are excluded from the step: no state, no decay, on either side of the load. Learning rate 1e-4 (the f16 spacing of a weight of 0.1, and most weights are
    smaller): at 1e-3 the loss of this case jumps by a factor 7 within two steps, and with it the scale that overflows."""
    name, omissions = "action_raw_adamw_dynamic", ("optimizer", "buffers", "batch", "scaler")
    model_keys, opt_keys = {"ft": "ft_model_state_dict"}, {"opt": "optimizer"}

    def builders(self):
        from ted_spad_amd.model_loaders import load_ft_model
        return {"ft": lambda f: load_ft_model("largei3d", saved_model_file=f, num_classes=102)}

    def driver(self, m):
        from ted_spad_amd.optim import DynamicLossScale
        from ted_spad_amd.train_step import ActionTrainStep
        d = ActionTrainStep(m["ft"], None, params=_action_params(opt_type="adamw", learning_rate=1e-4, weight_decay=0.1),
                            loss_scale=DynamicLossScale(init_scale=ACTION_INIT_SCALE, backoff_factor=ACTION_BACKOFF, growth_interval=3))
        return SimpleNamespace(driver=d, opts={"opt": (d.opt, m["ft"])}, scaler=d.scaler)

    def save(self, o, path):
        from ted_spad_amd.checkpoint import save_action_checkpoint
        return save_action_checkpoint(path, self.K, o.modules["ft"], o.driver.opt, None, scaler=o.driver.scaler)

    def step(self, o, s, batch=None):
        b = s if batch is None else batch
        video = synth_train_video(b, "resume_video64", (4, 48, 3, 64, 64))[:, :16].contiguous().cuda()
        return o.driver.step(video, _labels(b), drop_masks=_drop_masks(b, 4, 1)[0])

    def steps_at_save(self, o):
        return o.driver.opt.steps_applied()

    def verify(self, a):
        S, low = ACTION_INIT_SCALE, ACTION_INIT_SCALE * ACTION_BACKOFF
        print("action raw: skipped %s, grad_scale %s, scaler at the save %s, at the end %s" % (
            [r["skipped"] for r in a.recs], [r["grad_scale"] for r in a.recs], a.saved["amp_scaler"], {k: v for k, v in a.end.items() if k.startswith("scaler/")}))
        assert [r["skipped"] for r in a.recs] == [True, False, False, False]
        assert a.saved["amp_scaler"]["scale"] == low and a.saved["amp_scaler"]["_growth_tracker"] == 1, "at the save: backed off once, tracker non-zero"
        assert a.saved["amp_scaler"]["backoff_factor"] == ACTION_BACKOFF
        assert [r["grad_scale"] for r in a.recs] == [S, low, low, low]
        assert a.end["scaler/scale"] == 2 * low and a.end["scaler/_growth_tracker"] == 0, "the scale grew inside the steps after the load"
        assert a.base == 1 and a.end["opt/steps_applied"] == 3
        names = set(a.end)
        assert "opt/state/i3d.fc.weight/exp_avg" in names and not any(k.startswith("opt/state/mlp.") or k.startswith("opt/state/i3d.bn1.") for k in names)


class ActionTripCase(Case):
    """ActionTrainStep in the anonymised triplet form (4,48,3,64,64): a frozen UNet fa in front (not in the file: the scripts load it from its own), the mlp
    head inside the step, SGD with momentum, static scale 256."""
    name = "action_trip_sgd"
    model_keys, opt_keys = {"ft": "ft_model_state_dict"}, {"opt": "optimizer"}

    def builders(self):
        from ted_spad_amd.model_loaders import load_ft_model
        return {"ft": lambda f: load_ft_model("largei3d", saved_model_file=f, num_classes=102)}

    def driver(self, m):
        from ted_spad_amd.model_loaders import load_fa_model
        from ted_spad_amd.train_step import ActionTrainStep
        fa = _synth_into(load_fa_model(arch="unet"))
        d = ActionTrainStep(m["ft"], fa, params=_action_params(temporal_loss="trip", opt_type="sgd", learning_rate=1e-3), loss_scale=256.0)
        return SimpleNamespace(driver=d, opts={"opt": (d.opt, m["ft"])}, scaler=d.scaler, fa=fa)

    def save(self, o, path):
        from ted_spad_amd.checkpoint import save_action_checkpoint
        return save_action_checkpoint(path, self.K, o.modules["ft"], o.driver.opt, None, scaler=o.driver.scaler)

    def step(self, o, s, batch=None):
        b = s if batch is None else batch
        video = synth_train_video(b, "resume_video64", (4, 48, 3, 64, 64)).cuda()
        return o.driver.step(video, _labels(b), drop_masks=_drop_masks(b, 4, 3))

    def steps_at_save(self, o):
        return o.driver.opt.steps_applied()

    def verify(self, a):
        assert not any(r["skipped"] for r in a.recs) and a.base == self.K and a.end["opt/steps_applied"] == self.M
        assert "opt/state/mlp.fc1.weight/momentum_buffer" in a.end and all(r["loss_temporal"] is not None for r in a.recs)


class ReconstructionCase(Case):
    """ReconstructionTrainStep, 6 x 3 x 64 x 64, the smooth unet++ weights of test_hip_pretrain.py. Every step is one epoch of ReconstructionSchedule (epochs
    1..4 are warm-up epochs: a different learning rate each), whose `lr_counter` goes into the file as the script's does."""
    name, omissions, smooth = "reconstruction", ("optimizer", "buffers", "batch"), True
    model_keys, opt_keys = {"fa": "fa_model_state_dict"}, {"opt": "optimizer"}

    def builders(self):
        from ted_spad_amd.model_loaders import load_fa_model
        return {"fa": lambda f: load_fa_model(saved_model_file=f)}

    def driver(self, m):
        from ted_spad_amd.pretrain import ReconstructionSchedule, ReconstructionTrainStep
        d = ReconstructionTrainStep(m["fa"], learning_rate=1e-3)
        return SimpleNamespace(driver=d, opts={"opt": (d.opt, m["fa"])}, sched=ReconstructionSchedule())

    def save(self, o, path):
        from ted_spad_amd.checkpoint import save_reconstruction_checkpoint
        return save_reconstruction_checkpoint(path, self.K, o.sched.lr_counter, o.modules["fa"], o.driver.opt)

    def load_driver_state(self, o, ckpt, omit):
        super().load_driver_state(o, ckpt, omit)
        from ted_spad_amd.pretrain import ReconstructionSchedule
        o.sched = ReconstructionSchedule()                            # train_reconstruction.py builds its schedule variables anew; the file carries lr_counter
        o.sched.lr_counter = ckpt["lr_counter"]
        if "optimizer" not in omit:
            o.sched.lr = ckpt["optimizer"]["param_groups"][0]["lr"]

    def step(self, o, s, batch=None):
        b = s if batch is None else batch
        lr = o.sched.lr_for_epoch(s + 1)
        o.driver.set_lr(lr)
        r = o.driver.step(synth_tensor(b, "resume_recon", (6, 3, 64, 64)).cuda())
        o.sched.after_train_epoch(r["loss"])
        return dict(r, lr=lr, lr_counter=o.sched.lr_counter)

    def verify(self, a):
        from ted_spad_amd.pretrain import DEFAULT_PARAMS
        assert not any(r["skipped"] for r in a.recs)
        assert [r["lr"] for r in a.recs] == [DEFAULT_PARAMS.warmup_array[e] * 1e-3 for e in range(1, self.K + self.M + 1)]
        assert a.saved["lr_counter"] == a.recs[self.K - 1]["lr_counter"] and a.saved["optimizer"]["param_groups"][0]["lr"] == a.recs[self.K - 1]["lr"]
        assert a.end["opt/lr"] == a.recs[-1]["lr"]


class PrivacyCase(Case):
    """PrivacyTrainStep, (6,3,64,64), a frozen eval-mode UNet in front (not in the file). The driver has no checkpoint writer: plain torch.save."""
    name = "privacy"
    model_keys, opt_keys = {"fb": "fb_model_state_dict"}, {"opt": "optimizer"}

    def builders(self):
        from ted_spad_amd.model_loaders import load_fb_model
        return {"fb": lambda f: load_fb_model(arch="r50", saved_model_file=f, num_pa=7, ssl=False, pretrained=False)}

    def driver(self, m):
        from ted_spad_amd.model_loaders import load_fa_model
        from ted_spad_amd.privacy import PrivacyTrainStep
        fa = _synth_into(load_fa_model(arch="unet")).eval()
        for p in fa.parameters():
            p.requires_grad = False
        d = PrivacyTrainStep(m["fb"], fa_model=fa, learning_rate=1e-3)
        return SimpleNamespace(driver=d, opts={"opt": (d.opt, m["fb"])}, fa=fa)

    def save(self, o, path):
        states = {"fb_model_state_dict": o.modules["fb"].state_dict(), "optimizer": o.driver.opt.state_dict()}
        torch.save(states, path)
        return states

    def step(self, o, s, batch=None):
        b = s if batch is None else batch
        gain = (torch.arange(1, 7).float() / 6).view(6, 1, 1, 1)
        x = (synth_tensor(b, "resume_prv_x", (6, 3, 64, 64)) * gain).cuda()
        y = (synth_tensor(b, "resume_prv_y", (6, 7)) > 0.6).float().cuda()
        return o.driver.step(x, y)

    def verify(self, a):
        assert not any(r["skipped"] for r in a.recs)


class MGFNCase(Case):
    """MGFNTrainStep on case "a" of the mgfn_train_golden fixture (its model, shapes and masks; the features of step s are drawn with their own salt).
    torch.optim.Adam, unfused; deterministic by construction. No writer and no loader: torch.save, a fresh MGFN + load_state_dict."""
    name = "mgfn"
    model_keys, opt_keys = {"model": "model"}, {"opt": "optimizer"}

    def _fixture(self):
        import test_hip_mgfn_train as T
        return T._meta() + (T.G,)

    def builders(self):
        from ted_spad_amd.mgfn import MGFN
        meta, _, _ = self._fixture()
        c = meta["cases"]["a"]

        def build(f):
            m = MGFN(feature_size=meta["feature_size"], depths=tuple(c["depths"]), mgfn_types=tuple(c["types"]))
            if f is not None:
                m.load_state_dict(torch.load(f)["model"])
            return m
        return {"model": build}

    def fresh(self):
        meta, _, _ = self._fixture()
        m = self.builders()["model"](None)
        m.load_state_dict(synth_mgfn_state_dict(m.state_dict(), meta["seed"]))
        return self._objs({"model": m.cuda()})

    def driver(self, m):
        from ted_spad_amd.mgfn import MGFNTrainStep
        meta, _, _ = self._fixture()
        d = MGFNTrainStep(m["model"], meta["batch_size"], lr=1e-3, weight_decay=5e-4, dropout_rate=meta["dropout_rate"], k=meta["k"])
        return SimpleNamespace(driver=d, opts={"opt": (d.opt, m["model"])})

    def save(self, o, path):
        states = {"model": o.modules["model"].state_dict(), "optimizer": o.driver.opt.state_dict()}
        torch.save(states, path)
        return states

    def step(self, o, s, batch=None):
        b = s if batch is None else batch
        meta, gold, G = self._fixture()
        ni, ai, nl, al, masks = G.make_inputs("a", torch.float32, (gold["a/mask_abn"], gold["a/mask_nor"]), 1000 + b)
        return o.driver.step(ni.cuda(), ai.cuda(), nl.cuda(), al.cuda(), masks=tuple(t.cuda() for t in masks))


CASES = {c.name: c for c in (AnonymizerCase(True), AnonymizerCase(False), ActionRawCase(), ActionTripCase(), ReconstructionCase(), PrivacyCase(), MGFNCase())}
CONV_CASES = [n for n in CASES if n != "mgfn"]                        # the drivers whose float-atomic sections need the deterministic mode
ROLLBACK_CASES = ["anonymizer_unet_fb", "action_raw_adamw_dynamic", "reconstruction", "privacy"]


def arm_a(case, ckpt_dir):
    """The uninterrupted run, once per case: K steps, the file, M steps; a snapshot after the last step (after each of the M steps where the case has
    omission tests, which compare after one)."""
    if case.name not in _A:
        K, M = case.K, case.M
        t = [time.perf_counter()]

        def lap():
            torch.cuda.synchronize()
            t.append(time.perf_counter())
            return t[-1] - t[-2]
        o = case.fresh()
        t_build = lap()
        recs = [H.step_record(case.step(o, s)) for s in range(K)]
        t_steps = lap()
        path = str(ckpt_dir / (case.name + ".pth"))
        base = case.steps_at_save(o)
        saved = case.save(o, path)                                    # (the writer's dict: its scalars are looked at, the tensors come back through the file)
        t_save = lap()
        snaps = {}
        for s in range(K, K + M):
            recs.append(H.step_record(case.step(o, s)))
            if s == K + M - 1 or case.omissions:
                snaps[s - K + 1] = case.snap(o, base)
        print("wall time %s arm A: build %.2f s, %d steps %.2f s, save %.2f s, %d steps + snapshots %.2f s" % (case.name, t_build, K, t_steps, t_save, M, lap()))
        a = SimpleNamespace(o=o, recs=recs, snaps=snaps, end=snaps[M], path=path, base=base, saved=saved)
        for i, r in enumerate(recs):
            print("%s step %d: %s" % (case.name, i, {k: v for k, v in r.items() if not isinstance(v, tuple)}))
        case.verify(a)                                                # before anything is compared
        _A[case.name] = a
    return _A[case.name]


def expected(case, a, steps=None):
    """Arm A's losses of the first `steps` steps after the save and its state after them."""
    steps = case.M if steps is None else steps
    return {**H.losses(a.recs[case.K:case.K + steps], case.K), **a.snaps[steps]}


def continued(case, o, steps=None, first_batch=None):
    """`steps` steps after the save on `o`, then its state: what `expected` is compared with."""
    steps = case.M if steps is None else steps
    recs = [H.step_record(case.step(o, case.K + i, batch=first_batch if i == 0 else None)) for i in range(steps)]
    return {**H.losses(recs, case.K), **case.snap(o, 0)}


def _restart_test(case, ckpt_dir):
    a = arm_a(case, ckpt_dir)
    t0 = time.perf_counter()
    o = case.restart(a.path)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    got = continued(case, o)
    torch.cuda.synchronize()
    print("wall time %s arm B: load %.2f s, %d steps + snapshot %.2f s" % (case.name, t1 - t0, case.M, time.perf_counter() - t1))
    H.assert_same(got, expected(case, a), "%s: restart from the file vs the uninterrupted run" % case.name)


def _rollback_test(case, ckpt_dir):
    a = arm_a(case, ckpt_dir)
    case.rollback(a.o, a.path)
    got = continued(case, a.o)
    H.assert_same(got, expected(case, a), "%s: rollback of the live objects vs the uninterrupted run" % case.name)
    return a


@pytest.mark.parametrize("name", CONV_CASES)
def test_uninterrupted_run_does_what_the_case_is_for(name, ckpt_dir, deterministic, monkeypatch):
    """Arm A, which the tests below share, and the case's own conditions on it (`verify`): no step skipped -- or, for the dynamic loss scale, exactly the
    skip, back-off and growth the case is built around."""
    from ted_spad_amd import engine
    monkeypatch.setattr(engine, "AUTOTUNE", False)
    arm_a(CASES[name], ckpt_dir)


@pytest.mark.parametrize("name", CONV_CASES)
def test_restart_continues_bit_for_bit(name, ckpt_dir, deterministic, monkeypatch):
    from ted_spad_amd import engine
    monkeypatch.setattr(engine, "AUTOTUNE", False)
    _restart_test(CASES[name], ckpt_dir)


@pytest.mark.parametrize("name", ROLLBACK_CASES)
def test_rollback_continues_bit_for_bit(name, ckpt_dir, deterministic, monkeypatch):
    from ted_spad_amd import engine
    monkeypatch.setattr(engine, "AUTOTUNE", False)
    _rollback_test(CASES[name], ckpt_dir)


def test_mgfn_restart_continues_bit_for_bit(ckpt_dir):
    _restart_test(CASES["mgfn"], ckpt_dir)


def test_mgfn_rollback_continues_bit_for_bit_and_eval_sees_the_loaded_weights(ckpt_dir):
    """... and a live load UNDER existing packed eval weights: `score` equals a fresh model's on the same `state_dict`."""
    case = CASES["mgfn"]
    a = _rollback_test(case, ckpt_dir)
    model = a.o.modules["model"]
    meta = case._fixture()[0]
    v = synth_tensor(3, "resume_mgfn_eval_video", (7, 10, meta["feature_size"] + 1), 0.0, 2.0).cuda()
    packed_before = model.eval().score([v])[0]                        # builds the packed eval weights, at the state after arm C
    case.rollback(a.o, a.path)
    got = model.eval().score([v])[0]
    fresh = case.builders()["model"](None)
    fresh.load_state_dict(model.state_dict())
    want = fresh.cuda().eval().score([v])[0]
    H.assert_same({"score": got}, {"score": want}, "mgfn: eval scores after a live load vs a fresh model on the same state_dict")
    assert not torch.equal(got, packed_before), "the load did not move the scores: stale packed weights would not show"
    got = continued(case, a.o)                                        # (and arm A's objects are left where its record says they are)
    H.assert_same(got, expected(case, a), "mgfn: second rollback vs the uninterrupted run")


OMISSIONS = [(c.name, om) for c in CASES.values() for om in c.omissions]


@pytest.mark.parametrize("name,omit", OMISSIONS, ids=["%s-%s" % p for p in OMISSIONS])
def test_a_restart_that_leaves_something_out_is_seen(name, omit, ckpt_dir, deterministic, monkeypatch):
    """Arm B for ONE step with one piece left out; the part of the result that piece feeds must differ from arm A's after the same step."""
    from ted_spad_amd import engine
    monkeypatch.setattr(engine, "AUTOTUNE", False)
    case = CASES[name]
    a = arm_a(case, ckpt_dir)
    want = expected(case, a, steps=1)
    o = case.restart(a.path, frozenset([omit]))
    got = continued(case, o, steps=1, first_batch=0 if omit == "batch" else None)
    what = "%s without %s" % (name, omit)
    if omit == "optimizer":
        H.assert_differs(got, want, what, "/param/")
    elif omit == "buffers":
        H.assert_differs(got, want, what, "/buffer/")
        if name == "anonymizer_unet_fb":                             # phase 1 runs ft in eval mode: on the running statistics
            H.assert_differs(got, want, what, "/fa.loss_ft")
    elif omit == "batch":
        H.assert_differs(got, want, what, "loss/")
    elif omit == "scaler":                                            # (not the parameters: a power-of-two scale divides out exactly)
        H.assert_differs(got, want, what, "scaler/")
        H.assert_differs(got, want, what, "/grad_scale")
    else:
        raise AssertionError(omit)

