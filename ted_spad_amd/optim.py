"""The optimizer tail of a training step on MI355X: `scaler.step(optimizer); scaler.update()` of the action scripts
(action_training/train_action.py:79-81, train_anonymized_action.py:86-88) as at most three HIP launches per network (csrc/optim.hip).

    FusedOptimizer(reducer_or_params, opt_type, lr, ...)    torch.optim.Adam / AdamW / SGD as train_action.py:251-259 builds them
    DynamicLossScale(init_scale=65536., ...)                torch.amp.GradScaler: scale and growth tracker live on the device

The gradients of a network sit in the flat buckets of grad_reduce.GradBucketReducer; the optimizer keeps its own state (exp_avg / exp_avg_sq or
momentum_buffer) in flats of the same kind, every tensor's slot 16-byte aligned, and describes the whole step to the kernels by ONE device-resident
table of chunk records (parameter, gradient slot, state slots, element count; a chunk never spans two tensors, an excluded tensor has no chunk and
no state). The table is built once -- again only if a gradient bucket moved -- so a step costs the same launches and the same host work for 3 tensors
and for ft's 168.

    check   (only with a loss scale) any gradient not finite -> found_inf, on the device
    update  g / scale and the update; nothing at all is written when found_inf is set
    finish  step counter (applied steps only), GradScaler.update(), found_inf = 0

No host synchronisation anywhere: `step` returns two 0-d device tensors (found_inf as 0. / 1., the scale the gradients carried). The unscale happens
inside the update, so `.grad` keeps the SCALED gradients after a step.

`state_dict()` / `load_state_dict()` speak the layout of the matching torch.optim class (per-parameter 'step' / 'exp_avg' / 'exp_avg_sq' or
'momentum_buffer', `param_groups` with torch's own keys, indices in `parameters()` order, no entry for an excluded parameter -- as torch has none for
a parameter that never had a gradient): the reference's scripts resume from a checkpoint written here and the reverse. SGD's momentum buffers start
as zeros, which is torch's `buf = grad` on the first step (mu * 0 + g), and is what a torch state without a buffer loads as.
"""
from __future__ import annotations

import struct

import numpy as np
import torch

from . import _lib
from ._lib import TedSpadHipError
from . import train_engine as TE
from .grad_reduce import GradBucketReducer

OPT_TYPES = {"adam": 0, "adamw": 1, "sgd": 2}


def _stream():
    return torch.cuda.current_stream().cuda_stream


class DynamicLossScale:
    """torch.amp.GradScaler's state and `update()` rule (defaults 65536, 2.0, 0.5, 2000), on the device: {fp32 scale, int32 growth tracker}.
    `dynamic=False` (or `DynamicLossScale.static(s)`) never changes the scale: the static loss scale of the other step drivers; the non-finite
    check and the skip work the same."""

    def __init__(self, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, dynamic=True, device=None):
        if not (growth_factor > 1.0 and 0.0 < backoff_factor < 1.0 and int(growth_interval) >= 1 and float(init_scale) > 0.0):
            raise ValueError("DynamicLossScale: needs init_scale > 0, growth_factor > 1, 0 < backoff_factor < 1, growth_interval >= 1")
        self.growth_factor, self.backoff_factor, self.growth_interval = float(growth_factor), float(backoff_factor), int(growth_interval)
        self.dynamic = bool(dynamic)
        self._host = (float(init_scale), 0)         # until the device copy exists, and what it is (re)built from
        self._dev = None
        if device is not None:
            self.device_state(device)

    @classmethod
    def static(cls, scale, device=None):
        return cls(init_scale=float(scale), dynamic=False, device=device)

    def device_state(self, device) -> torch.Tensor:
        """The 2-word device state {fp32 scale, int32 tracker} (created on first use)."""
        device = torch.device(device)
        if device.type != "cuda":
            raise TedSpadHipError("DynamicLossScale: the loss scale lives on the GPU (got device %s); there is no CPU path" % device)
        if self._dev is None or self._dev.device != device:
            scale, tracker = self._read()
            host = torch.frombuffer(bytearray(struct.pack("<fi", scale, tracker)), dtype=torch.float32)
            self._dev = host.to(device)
        return self._dev

    def _read(self):
        if self._dev is None:
            return self._host
        raw = self._dev.cpu().numpy().tobytes()
        return struct.unpack("<fi", raw)

    def scale_tensor(self, device) -> torch.Tensor:
        """0-d view of the current scale on the device (what the loss gradients are multiplied with; no sync)."""
        return self.device_state(device)[0]

    def get_scale(self) -> float:
        return float(self._read()[0])

    def state_dict(self) -> dict:
        """The keys of torch.amp.GradScaler.state_dict()."""
        scale, tracker = self._read()
        return {"scale": float(scale), "growth_factor": self.growth_factor, "backoff_factor": self.backoff_factor,
                "growth_interval": self.growth_interval, "_growth_tracker": int(tracker)}

    def load_state_dict(self, sd: dict):
        self.growth_factor, self.backoff_factor = float(sd["growth_factor"]), float(sd["backoff_factor"])
        self.growth_interval = int(sd["growth_interval"])
        self._host = (float(sd["scale"]), int(sd["_growth_tracker"]))
        dev = None if self._dev is None else self._dev.device
        self._dev = None
        if dev is not None:
            self.device_state(dev)


class FusedOptimizer:
    def __init__(self, reducer_or_params, opt_type="adam", lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=None, momentum=0.0, exclude=()):
        """reducer_or_params: the GradBucketReducer that owns the network's gradient buckets (indices of the state_dict then follow the order given
        by `params_order`, by default the reducer's own) or a parameter list (the optimizer then owns a one-bucket reducer and `zero_grad` prepares it).
        weight_decay: None = the torch class's default (0 for adam / sgd, 1e-2 for adamw). exclude: parameters that take no part in the step: no
        gradient is read, no state is kept, nothing is decayed."""
        if opt_type not in OPT_TYPES:
            raise NotImplementedError("Optimizer %s not yet implemented." % opt_type)          # train_action.py:259
        self.opt_type = opt_type
        if isinstance(reducer_or_params, GradBucketReducer):
            self.reducer, self._own_reducer = reducer_or_params, False
            self.params = [p for b in self.reducer.buckets for p in b]
        else:
            self.params = [p for p in reducer_or_params]
            self.reducer, self._own_reducer = GradBucketReducer([self.params]), True
            if len(self.params) != sum(len(b) for b in self.reducer.buckets):
                raise ValueError("FusedOptimizer: every parameter must require a gradient")
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.weight_decay = float(weight_decay) if weight_decay is not None else (1e-2 if opt_type == "adamw" else 0.0)
        self.momentum = float(momentum) if opt_type == "sgd" else 0.0
        self._excluded = {id(p) for p in exclude}
        self.exclude = [p for p in self.params if id(p) in self._excluded]
        self.active = [p for p in self.params if id(p) not in self._excluded]
        if not self.active:
            raise ValueError("FusedOptimizer: no parameter left to update")
        self._steps0 = 0                         # applied steps a loaded state starts from (until the device state exists)
        self._state = None                       # 8 int32 words, tedspad_hip.h
        self._m = self._v = None                 # state flats
        self._slots = None                       # id(p) -> (offset, numel) in the state flats
        self._table = self._table_key = None
        self._nchunks = 0
        self._pending = None                     # state tensors of load_state_dict until the flats exist

    # ---- layout ---------------------------------------------------------------------------------------------------------------
    def set_params_order(self, params):
        """The order `state_dict` numbers the parameters in: `model.parameters()` (the reducer's buckets follow the backward pass)."""
        params = list(params)
        if {id(p) for p in params} != {id(p) for p in self.params}:
            raise ValueError("FusedOptimizer.set_params_order: not the same parameters")
        self.params = params
        self.exclude = [p for p in params if id(p) in self._excluded]
        self.active = [p for p in params if id(p) not in self._excluded]

    @property
    def has_m(self):
        return self.opt_type != "sgd" or self.momentum != 0.0

    @property
    def has_v(self):
        return self.opt_type != "sgd"

    def _device(self):
        return self.active[0].device

    def _require_cuda(self):
        for p in self.params:
            if p.device.type != "cuda":
                raise TedSpadHipError("FusedOptimizer: parameters must be on the GPU (got %s); the HIP kernels are the only update path" % p.device)

    def _alloc_state(self):
        """State flats: every active tensor's slot starts at a multiple of 4 elements (16 bytes; torch's allocations are 256-byte aligned)."""
        dev, off, slots = self._device(), 0, {}
        for p in self.active:
            slots[id(p)] = (off, p.numel())
            off += (p.numel() + 3) // 4 * 4
        self._slots = slots
        self._m = torch.zeros(off, dtype=torch.float32, device=dev) if self.has_m else None
        self._v = torch.zeros(off, dtype=torch.float32, device=dev) if self.has_v else None
        self._write_state(self._steps0)
        if self._pending is not None:
            for p, (m, v) in self._pending.items():
                o, n = slots[p]
                if m is not None and self._m is not None:
                    self._m[o:o + n].copy_(m.reshape(-1).to(dev, torch.float32))
                if v is not None and self._v is not None:
                    self._v[o:o + n].copy_(v.reshape(-1).to(dev, torch.float32))
            self._pending = None

    def _write_state(self, t: int):
        b1, b2 = self.betas
        p1, p2 = b1 ** (t + 1), b2 ** (t + 1)          # Python floats: torch's `beta ** step`
        raw = struct.pack("<iiffdd", 0, int(t), float(np.float32(1.0 - p1)), float(np.float32((1.0 - p2) ** 0.5)), p1, p2)
        self._state = torch.frombuffer(bytearray(raw), dtype=torch.int32).to(self._device())

    def _state_view(self, flat, p):
        o, n = self._slots[id(p)]
        return flat[o:o + n].view_as(p)

    def _build_table(self):
        """One record per run of at most tedspad_optim_chunk_elems() elements of one active tensor: {p, g, m, v, n, 0} as int64."""
        red = self.reducer
        if not red.flats or any(f.device != b[0].device for f, b in zip(red.flats, red.buckets)):
            red._allocate()
        if any(not p.is_contiguous() or p.dtype != torch.float32 for p in self.active):
            raise TedSpadHipError("FusedOptimizer: parameters must be contiguous fp32 tensors")
        chunk = int(_lib.lib().tedspad_optim_chunk_elems())
        recs = []
        mbase = self._m.data_ptr() if self._m is not None else 0
        vbase = self._v.data_ptr() if self._v is not None else 0
        for b, views in zip(red.buckets, red.views):
            for p, gview in zip(b, views):
                if id(p) in self._excluded:
                    continue
                o, n = self._slots[id(p)]
                pp, gp = p.data_ptr(), gview.data_ptr()
                k = np.arange(0, n, chunk, dtype=np.int64)
                r = np.zeros((len(k), 6), dtype=np.int64)
                r[:, 0] = pp + 4 * k
                r[:, 1] = gp + 4 * k
                r[:, 2] = mbase + 4 * (o + k) if mbase else 0
                r[:, 3] = vbase + 4 * (o + k) if vbase else 0
                r[:, 4] = np.minimum(chunk, n - k)
                recs.append(r)
        table = np.concatenate(recs, axis=0)
        self._nchunks = int(table.shape[0])
        self._table = torch.from_numpy(table.reshape(-1)).to(self._device())
        self._table_key = self._key()

    def _key(self):
        return tuple(f.data_ptr() for f in self.reducer.flats)      # per bucket, not per tensor

    def rebuild(self):
        """Call after the parameters were re-allocated (`module.to(...)`, `p.data = ...`): the chunk table holds their addresses."""
        self._table = None

    # ---- the step -------------------------------------------------------------------------------------------------------------
    def zero_grad(self, set_to_none=True):
        """A no-op next to `reducer.prepare(...)`, which the step driver calls; with the optimizer's own reducer (built from a parameter list) it IS that call."""
        if self._own_reducer:
            self.reducer.prepare(exclude=self.exclude)

    def step(self, lr=None, scaler: DynamicLossScale = None):
        """One optimizer step on the reducer's (reduced) gradients. lr: this step's learning rate (the scripts set it per epoch); None = the last one.
        scaler: None = the gradients carry no scale and are not checked. Returns (found_inf, grad_scale): 0-d fp32 device tensors, nothing is read back."""
        if lr is not None:
            self.lr = float(lr)
        if self._state is None:
            self._require_cuda()                 # once: the per-step host work does not grow with the number of tensors
            self._alloc_state()
        if self._table is None or self._table_key != self._key():
            self._build_table()
        L, s = _lib.lib(), _stream()
        dev = self._device()
        out = torch.empty(2, dtype=torch.float32, device=dev)
        sc = None if scaler is None else scaler.device_state(dev)
        scp = 0 if sc is None else sc.data_ptr()
        tp, st = self._table.data_ptr(), self._state.data_ptr()
        if sc is not None:
            _lib.check(L.tedspad_optim_check(tp, self._nchunks, st, s), "tedspad_optim_check")
        _lib.check(L.tedspad_optim_update(tp, self._nchunks, OPT_TYPES[self.opt_type], st, scp, self.lr, self.betas[0], self.betas[1], self.eps,
                                          self.weight_decay, self.momentum, s), "tedspad_optim_update")
        dyn = sc is not None and scaler.dynamic
        _lib.check(L.tedspad_optim_finish(st, scp, self.betas[0], self.betas[1], scaler.growth_factor if dyn else 1.0, scaler.backoff_factor if dyn else 1.0,
                                          scaler.growth_interval if dyn else 0, out.data_ptr(), s), "tedspad_optim_finish")
        TE.mark_updated(self.active)
        return out[0], out[1]

    def steps_applied(self) -> int:
        """Applied (not skipped) steps so far: one device read."""
        return self._steps0 if self._state is None else int(self._state[1].item())

    # ---- torch.optim's state_dict layout --------------------------------------------------------------------------------------
    def _twin(self, params):
        if self.opt_type == "adam":
            return torch.optim.Adam(params, lr=self.lr, betas=self.betas, eps=self.eps, weight_decay=self.weight_decay)
        if self.opt_type == "adamw":
            return torch.optim.AdamW(params, lr=self.lr, betas=self.betas, eps=self.eps, weight_decay=self.weight_decay)
        return torch.optim.SGD(params, lr=self.lr, momentum=self.momentum, weight_decay=self.weight_decay)

    def state_dict(self) -> dict:
        groups = self._twin(self.params).state_dict()["param_groups"]          # torch's own keys and defaults for this torch version
        t = self.steps_applied()
        state = {}
        for i, p in enumerate(self.params):
            if id(p) in self._excluded:
                continue
            if self._state is not None:
                m = self._state_view(self._m, p).clone() if self.has_m else None
                v = self._state_view(self._v, p).clone() if self.has_v else None
            elif self._pending is not None and id(p) in self._pending:
                m, v = self._pending[id(p)]
            else:
                m = torch.zeros_like(p, dtype=torch.float32) if self.has_m else None
                v = torch.zeros_like(p, dtype=torch.float32) if self.has_v else None
            if self.opt_type == "sgd":
                state[i] = {"momentum_buffer": m}
            else:
                state[i] = {"step": torch.tensor(float(t), dtype=torch.float32), "exp_avg": m, "exp_avg_sq": v}
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd: dict):
        g = sd["param_groups"][0]
        if len(sd["param_groups"]) != 1 or list(g["params"]) != list(range(len(self.params))):
            raise ValueError("FusedOptimizer.load_state_dict: expects one parameter group over the same %d parameters" % len(self.params))
        if g.get("amsgrad") or g.get("maximize") or g.get("nesterov") or g.get("dampening"):
            raise NotImplementedError("FusedOptimizer: amsgrad / maximize / nesterov / dampening are not implemented")
        self.lr, self.weight_decay = float(g["lr"]), float(g["weight_decay"])
        if self.opt_type == "sgd":
            self.momentum = float(g["momentum"])
        else:
            self.betas, self.eps = (float(g["betas"][0]), float(g["betas"][1])), float(g["eps"])
        pending, steps = {}, 0
        for i, st in sd["state"].items():
            p = self.params[int(i)]
            if id(p) in self._excluded:
                raise ValueError("FusedOptimizer.load_state_dict: parameter %d has state but is excluded from the step" % int(i))
            if self.opt_type == "sgd":
                pending[id(p)] = (st.get("momentum_buffer"), None)
            else:
                pending[id(p)] = (st["exp_avg"], st["exp_avg_sq"])
                steps = max(steps, int(float(st["step"])))
        self._steps0, self._pending = steps, pending
        self._state = self._m = self._v = self._slots = self._table = None
        if self._device().type == "cuda":
            self._alloc_state()
