"""-m gpu: the optimizer kernels (csrc/optim.hip) on their own, through optim.FusedOptimizer over a hand-made GradBucketReducer (inputs: tests/optim_ref.py).

Tolerance. The kernel's arithmetic is fp32 rounding of about ten operations per element against a float64 torch.optim twin fed the same fp32 gradients divided by
the scale. Measured maxima over the five configurations, five steps and all tensors (rel-L2 per tensor): parameters 1.60e-7 (adamw), exp_avg / momentum_buffer
9.2e-8 (sgd), exp_avg_sq 1.33e-7 (adam + weight decay). The bounds are 4 x those (optim_ref.BOUND_*: 6.4e-7, 3.7e-7, 5.6e-7), far below the 1e-5 the inputs are built for (tests/test_optim_host.py: a misplaced eps, a missing bias
correction or coupled-for-decoupled decay each move the float64 result by more than 1e-4 in every tensor of 100 elements or more)."""
import pytest
import torch

import optim_ref as R

pytestmark = pytest.mark.gpu

BOUND_P, BOUND_M, BOUND_V = R.BOUND_P, R.BOUND_M, R.BOUND_V
GUARD, SENTINEL = 64, 12345.678


def _guarded(n, phase=0):
    """n fp32 elements `phase` elements past a 16-byte boundary inside a sentinel-filled buffer: (buffer, view)"""
    buf = torch.full((GUARD + 4 + n + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf, buf[GUARD + phase:GUARD + phase + n]


def _guards_intact(buf, view):
    lo = (view.data_ptr() - buf.data_ptr()) // 4
    return bool((buf[:lo] == SENTINEL).all()) and bool((buf[lo + view.numel():] == SENTINEL).all())


class Rig:
    """Parameters (each 16-byte aligned in one guarded buffer, sentinels between them), a GradBucketReducer whose flats are guarded views at chosen phases, the
    optimizer over it, and the float64 twin."""

    def __init__(self, name, buckets=R.BUCKETS, phases=None, scaler="dynamic", twin=True, **scaler_kw):
        from ted_spad_amd.grad_reduce import GradBucketReducer
        from ted_spad_amd.optim import DynamicLossScale, FusedOptimizer
        self.opt_type, self.kw = R.CONFIGS[name]
        p0 = R.make_params()
        offs, off = [], 0
        for n in R.SIZES:
            offs.append(off)
            off += (n + 3) // 4 * 4 + 4                         # at least 4 sentinel elements between two tensors
        self.pbuf, pview = _guarded(off)
        self.params = []
        for p, o, n in zip(p0, offs, R.SIZES):
            pview[o:o + n].copy_(p)
            self.params.append(torch.nn.Parameter(pview[o:o + n]))
        self.pview, self.offs = pview, offs
        self.red = GradBucketReducer([[self.params[i] for i in b] for b in buckets])
        self.gbufs = []
        for b, ph in zip(buckets, phases or [0] * len(buckets)):
            n = sum(R.SIZES[i] for i in b)
            buf, flat = _guarded(n, ph)
            flat.zero_()
            views, o = [], 0
            for i in b:
                views.append(flat[o:o + R.SIZES[i]].view_as(self.params[i]))
                o += R.SIZES[i]
            self.red.flats.append(flat)
            self.red.views.append(views)
            self.gbufs.append((buf, flat))
        self.excluded = self.params[R.EXCLUDED]
        self.opt = FusedOptimizer(self.red, self.opt_type, lr=R.LRS[0], exclude=[self.excluded], **self.kw)
        self.opt.set_params_order(self.params)
        self.scaler = DynamicLossScale(**scaler_kw) if scaler == "dynamic" else (None if scaler is None else DynamicLossScale.static(scaler))
        self.p64 = R.twin_params(p0) if twin else None
        self.twin = R.torch_twin(self.opt_type, self.p64, R.LRS[0], **self.kw) if twin else None

    def step(self, t, lr, poison=None, twin=True):
        """gradients of step t times the current scale into the buckets (poison: (tensor index, element, value)), one optimizer step, the twin's step unless skipped"""
        scale = 1.0 if self.scaler is None else self.scaler.get_scale()
        self.red.prepare(exclude=[self.excluded])
        grads = [g * scale for g in R.make_grads(t)]
        if poison is not None:
            grads[poison[0]][poison[1]] = poison[2]
        for p, g in zip(self.params, grads):
            if p is not self.excluded:
                p.grad.copy_(g)
        found, used = self.opt.step(lr=lr, scaler=self.scaler)
        found, used = float(found), float(used)
        assert used == scale
        if twin and self.twin is not None and not found:
            R.twin_step(self.twin, self.p64, grads, scale, lr)
        return found

    def snapshot(self):
        o = self.opt
        return (self.pbuf.clone(), None if o._m is None else o._m.clone(), None if o._v is None else o._v.clone(), o._state.clone())

    def state_of(self, i):
        o, p = self.opt, self.params[i]
        return (o._state_view(o._m, p) if o.has_m else None), (o._state_view(o._v, p) if o.has_v else None)

    def check_guards(self):
        assert _guards_intact(self.pbuf, self.pview), "parameter guard zones"
        for i, (o, n) in enumerate(zip(self.offs, R.SIZES)):                       # the sentinels between two tensors
            end = self.offs[i + 1] if i + 1 < len(self.offs) else self.pview.numel()
            assert bool((self.pview[o + n:end] == SENTINEL).all()), "sentinels behind parameter %d" % i
        for buf, flat in self.gbufs:
            assert _guards_intact(buf, flat), "gradient guard zones"
        o = self.opt
        used = torch.zeros(o._m.numel() if o._m is not None else 0, dtype=torch.bool, device="cuda")
        for off, n in o._slots.values():
            used[off:off + n] = True
        for f in (o._m, o._v):
            if f is not None:
                assert not bool(f[~used].any()), "padding of the state flats"
        assert id(self.excluded) not in o._slots


def _equal(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", sorted(R.CONFIGS))
def test_five_steps_against_the_float64_torch_twin(name):
    from ted_spad_amd import _lib
    assert _lib.lib().tedspad_optim_chunk_elems() == 4096, "tests/optim_ref.py's sizes bracket a chunk of 4096"
    rig = Rig(name)
    excl_before = rig.excluded.detach().clone()
    worst = dict(p=0.0, m=0.0, v=0.0)
    for t, lr in enumerate(R.LRS):
        assert rig.step(t, lr) == 0.0
        for i in range(len(R.SIZES)):
            if i == R.EXCLUDED:
                continue
            m, v = rig.state_of(i)
            m64, v64 = R.twin_state(rig.twin, rig.p64[i], rig.opt_type)
            worst["p"] = max(worst["p"], R.rel_l2(rig.params[i], rig.p64[i]))
            if m is not None:
                worst["m"] = max(worst["m"], R.rel_l2(m, m64))
            if v is not None:
                worst["v"] = max(worst["v"], R.rel_l2(v, v64))
    print("optim %s: worst rel-L2 per tensor over 5 steps: p %.3e  m %.3e  v %.3e" % (name, worst["p"], worst["m"], worst["v"]))
    assert rig.opt.steps_applied() == 5
    assert torch.equal(rig.excluded.detach(), excl_before), "the excluded tensor is not touched (no decay either)"
    assert any(not torch.equal(p.detach().cpu(), q) for p, q in zip(rig.params, R.make_params()))
    rig.check_guards()
    assert worst["p"] < BOUND_P and worst["m"] < BOUND_M and worst["v"] < BOUND_V, worst


@pytest.mark.parametrize("name", ["adam_wd", "adamw", "sgd_mu"])
def test_bitwise_repeatable_and_independent_of_the_bucket_layout(name):
    """Two runs are identical; the same tensors packed as three buckets at other phases (other heads, tails, 16-byte vs dword gradient loads) give the same bits:
    an element's result depends on the element, not on the path that handled it."""
    runs = []
    for buckets, phases in ((R.BUCKETS, None), (R.BUCKETS, None), (R.BUCKETS3, R.PHASES3)):
        rig = Rig(name, buckets, phases, twin=False)
        for t, lr in enumerate(R.LRS[:3]):
            rig.step(t, lr)
        rig.check_guards()
        runs.append(([p.detach().clone() for p in rig.params], [rig.state_of(i) for i in range(len(R.SIZES)) if i != R.EXCLUDED]))
    for other in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(runs[0][0], other[0]))
        assert all(_equal(a, b) for a, b in zip(runs[0][1], other[1]))


@pytest.mark.parametrize("poison", [(0, 0, float("nan")), (9, 65538, float("inf")), (1, 1, float("-inf")), (8, 4096, float("nan"))],
                         ids=["first-element", "last-element-of-the-last-tail", "inside-a-sub-vector-tensor", "one-chunk-plus-one"])
def test_a_non_finite_gradient_skips_the_step(poison):
    rig = Rig("adamw")
    rig.step(0, R.LRS[0])
    before = rig.snapshot()
    assert rig.step(1, R.LRS[1], poison=poison) == 1.0
    after = rig.snapshot()
    assert _equal(before[:3], after[:3]), "parameters and state keep their bits"
    assert torch.equal(before[3], after[3]), "step counter and bias corrections keep theirs; found_inf is cleared again"
    assert rig.opt.steps_applied() == 1
    assert rig.scaler.state_dict()["scale"] == R.SCALE / 2 and rig.scaler.state_dict()["_growth_tracker"] == 0
    assert rig.step(1, R.LRS[1]) == 0.0                      # the next clean step is step t = 2 of the twin, which never saw the skipped one
    assert rig.opt.steps_applied() == 2 and rig.scaler.state_dict()["_growth_tracker"] == 1
    for i in range(len(R.SIZES)):
        if i != R.EXCLUDED:
            assert R.rel_l2(rig.params[i], rig.p64[i]) < BOUND_P
            assert R.rel_l2(rig.state_of(i)[0], R.twin_state(rig.twin, rig.p64[i], "adamw")[0]) < BOUND_M
    rig.check_guards()


def test_the_scale_grows_after_growth_interval_clean_steps():
    rig = Rig("adam", twin=False, growth_interval=3)
    sd = lambda: (rig.scaler.state_dict()["scale"], rig.scaler.state_dict()["_growth_tracker"])
    seen = []
    for t, poison in enumerate([None, None, (2, 50, float("inf")), None, None, None, None]):
        rig.step(t, 1e-2, poison=poison)
        seen.append(sd())
    S = R.SCALE
    assert seen == [(S, 1), (S, 2), (S / 2, 0), (S / 2, 1), (S / 2, 2), (S, 0), (S, 1)], seen
    assert rig.opt.steps_applied() == 6


def test_a_static_scale_neither_grows_nor_backs_off_and_still_skips():
    rig = Rig("adam", scaler=256.0)
    assert rig.step(0, 1e-2) == 0.0
    before = rig.snapshot()
    assert rig.step(1, 1e-2, poison=(7, 4095, float("nan"))) == 1.0
    assert _equal(before[:3], rig.snapshot()[:3]) and rig.scaler.get_scale() == 256.0
    for t in range(1, 4):
        assert rig.step(t, 1e-2) == 0.0
    assert rig.scaler.state_dict()["scale"] == 256.0 and rig.scaler.state_dict()["_growth_tracker"] == 0 and rig.opt.steps_applied() == 4
    assert max(R.rel_l2(p, q) for i, (p, q) in enumerate(zip(rig.params, rig.p64)) if i != R.EXCLUDED) < BOUND_P


def test_no_scaler_means_no_check_and_no_scaling():
    rig = Rig("sgd_mu", scaler=None)
    for t, lr in enumerate(R.LRS[:2]):
        assert rig.step(t, lr) == 0.0
    assert max(R.rel_l2(p, q) for i, (p, q) in enumerate(zip(rig.params, rig.p64)) if i != R.EXCLUDED) < BOUND_P


@pytest.mark.parametrize("name", ["adam_wd", "sgd_mu"])
def test_state_dict_round_trip_with_the_torch_twin(name):
    """Three steps here -> state_dict -> a fresh float64 torch.optim on the CPU; and three steps of torch -> state_dict -> a fresh FusedOptimizer. One more step on
    both sides agrees under the same bound."""
    rig = Rig(name)
    for t, lr in enumerate(R.LRS[:3]):
        rig.step(t, lr)
    # ours -> torch
    p64 = [torch.nn.Parameter(p.detach().double().cpu().clone()) for p in rig.params]
    fresh = R.torch_twin(rig.opt_type, p64, 1.0, **rig.kw)
    fresh.load_state_dict(rig.opt.state_dict())
    assert fresh.param_groups[0]["lr"] == R.LRS[2]
    if rig.opt_type != "sgd":
        assert float(fresh.state[p64[0]]["step"]) == 3.0 and fresh.state[p64[0]]["exp_avg"].dtype == torch.float64
    # torch -> ours (the running twin's state into a new optimizer over the twin's parameters, rounded to fp32)
    rig2 = Rig(name, twin=False)
    for p, q in zip(rig2.params, rig.p64):
        p.data.copy_(q.detach().float())
    rig2.opt.load_state_dict(rig.twin.state_dict())
    assert rig2.opt.steps_applied() == (0 if rig.opt_type == "sgd" else 3)
    rig2.p64, rig2.twin = rig.p64, rig.twin
    scale = rig.scaler.get_scale()
    grads = [g * scale for g in R.make_grads(3)]
    rig.step(3, R.LRS[3], twin=False)
    R.twin_step(fresh, p64, grads, scale, R.LRS[3])
    for i in range(len(R.SIZES)):
        if i != R.EXCLUDED:
            assert R.rel_l2(rig.params[i], p64[i]) < BOUND_P, i
    rig2.step(3, R.LRS[3])                                   # steps rig.twin as well
    for i in range(len(R.SIZES)):
        if i != R.EXCLUDED:
            assert R.rel_l2(rig2.params[i], rig.p64[i]) < BOUND_P, i


def test_null_and_bad_arguments_are_refused_on_the_host():
    from ted_spad_amd import _lib
    L = _lib.lib()
    assert L.tedspad_optim_update(None, 1, 0, None, None, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.0, None) != 0 and b"tedspad_optim_update" in L.tedspad_last_error()
    st = torch.zeros(8, dtype=torch.int32, device="cuda")
    assert L.tedspad_optim_update(st.data_ptr(), 1, 7, st.data_ptr(), None, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.0, None) != 0 and b"mode" in L.tedspad_last_error()
    assert L.tedspad_optim_check(st.data_ptr(), 0, st.data_ptr(), None) != 0 and L.tedspad_optim_finish(None, None, 0.9, 0.999, 2.0, 0.5, 0, None, None) != 0
