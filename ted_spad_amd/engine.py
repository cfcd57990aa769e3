"""Host-side plumbing between torch tensors (device memory, streams) and the C-ABI HIP
library: channels-last activation views, weight packing / BatchNorm folding, launchers.

torch is used here for device memory and the current HIP stream only; every arithmetic
op of the hot path is a kernel of libtedspad_hip.so. Nothing in this file computes on the
CPU and nothing falls back to torch ops: CPU tensors are rejected.
"""
from __future__ import annotations

import ctypes as C
import os
import weakref
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import ConvDesc, PoolDesc, check

DTYPES = {"f16": (torch.float16, _lib.F16), "bf16": (torch.bfloat16, _lib.BF16)}
DEFAULT_DTYPE = "f16"  # DESIGN.md "precision": bf16 operands cannot meet the 1e-3 feature gate

# Tile autotuning (the reference sets cudnn.benchmark = True, train_anonymizer.py:28): during the first
# calls of a conv on a new geometry the tile configurations of the kernel take turns, timed in context with
# HIP events, and the fastest is kept (PackedConv._launch_tuned). Same arithmetic for every configuration
# (K order per output is fixed), so results do not depend on the choice. Off inside hipGraph capture.
BNECK_FRAME = os.environ.get("TEDSPAD_BNECK_FRAME", "1") != "0"   # layer3's plain blocks as one launch per block, a workgroup per 14 x 14 frame (BneckFrame); 0: three launches (A/B)
BNECK_TAIL = os.environ.get("TEDSPAD_BNECK_TAIL", "1") != "0"   # layer1: conv2 -> conv3 (+ residual / downsample) in one launch (BneckTail); 0: separate launches (A/B)
BNECK_TAIL128 = os.environ.get("TEDSPAD_BNECK_TAIL128", "1") != "0"   # layer2's plain blocks (128 mid channels) on the fused tail as well; 0: conv2 + conv3 launches (A/B)
BNECK_TAIL_POOL = os.environ.get("TEDSPAD_BNECK_TAIL_POOL", "1") != "0"   # layer1's last block: the fused tail with maxpool2 inside; 0: conv2 + (conv3 + pool) launches (A/B)
L1_FOLD = os.environ.get("TEDSPAD_L1_FOLD", "1") != "0"   # layer1 on four-frame clips: a plain block's tail also emits the next block's conv1 (BneckTailFold); 0: tail + temporal-conv launches (A/B)
L1_FOLD_DUAL = os.environ.get("TEDSPAD_L1_FOLD_DUAL", "1") != "0"   # ... and so does layer1.0's downsample tail (BneckTailFoldDual; needs L1_FOLD); 0: the two-source tail + the temporal-conv launch (A/B)
TPAIR_MIN_COUT =int(os.environ.get("TEDSPAD_TPAIR_MIN_COUT", "128"))   # smallest cout that takes the folded form (256: layer2's 128-channel temporal convs stay on the temporal chunk-major tile)
TPAIR = os.environ.get("TEDSPAD_TPAIR", "1") != "0"   # 3x1x1 convs on two-frame tensors as one K = 2*cin GEMM over both frames (TPairConv); 0: K = 3*cin with zero taps (A/B)
STEM_POOL = os.environ.get("TEDSPAD_STEM_POOL", "1") != "0"   # the spatial half of maxpool1 inside the stem kernel too (StemPT.conv_pool); 0: separate (1,3,3) max-pool (A/B)
UPP_TAIL = os.environ.get("TEDSPAD_UPP_TAIL", "1") != "0"              # unet++: x_0_3 + segmentation head as one launch (tedspad_unetpp_tail_fwd)
GATHER_CAT = os.environ.get("TEDSPAD_GATHER_CAT", "1") != "0"          # unet++ decoder blocks read upsample + concat in place (PackedConv.gather)
STEM_CLIP = os.environ.get("TEDSPAD_STEM_CLIP", "1") != "0"   # the stem kernel reads the fp32 clip itself (StemPT.conv_pool_clip); 0: tedspad_clip_to_tp layout pass in front of it (A/B)
STEM_NWG = int(os.environ.get("TEDSPAD_STEM_NWG", "0"))   # persistent stem on fewer workgroups than CUs (a multiple of 8): its workgroups take a CU each ALONE (160 KB of LDS), the CUs it leaves free run the other stream's HBM-bound kernels meanwhile (A/B)
STEM_PT = os.environ.get("TEDSPAD_STEM_PT", "1") != "0"   # persistent temporal-unfolded stem with the temporal max-pool fused (StemPT); 0: pixel-pair stem + full max-pool (A/B)
SKIP_TILE_CFGS = {int(c) for c in os.environ.get("TEDSPAD_SKIP_CFGS", "").split(",") if c.strip()}   # A/B: tile configurations the tuner must not try
AUTOTUNE = os.environ.get("TEDSPAD_AUTOTUNE", "1") != "0"
DETERMINISTIC = False        # set_deterministic() below; TEDSPAD_DETERMINISTIC=1 switches it on when the first training object is built
_DET_SAVED = None


def set_deterministic(on: bool) -> None:
    """Bit-identical training from run to run (the reference has no such switch; round-2 review item 4 ii). On: the library's float-atomic sections
    (BatchNorm batch statistics, channel sums, the weight-gradient flush) are passed by one workgroup at a time in blockIdx order (csrc/det_gate.h); the tile tuner
    is off (one K-order-preserving tile per conv); the weight gradients stay on the main stream; conv bias gradients come from the channel-sum kernel instead of
    tedspad_bn_bwd_apply's fused accumulation (train_engine reads `DETERMINISTIC`). Slower -- those sections are serialised -- and meant for tests and debugging.
    `deterministic_giveups()` must stay 0."""
    global DETERMINISTIC, AUTOTUNE, _DET_SAVED
    from . import _lib
    _lib.check(_lib.lib().tedspad_set_deterministic(1 if on else 0), "tedspad_set_deterministic")
    if on and not DETERMINISTIC:
        _DET_SAVED = AUTOTUNE
        AUTOTUNE = False
    elif not on and DETERMINISTIC and _DET_SAVED is not None:
        AUTOTUNE = _DET_SAVED
    DETERMINISTIC = bool(on)


def deterministic_giveups() -> int:
    from . import _lib
    return int(_lib.lib().tedspad_deterministic_giveups())


def apply_env_determinism() -> None:
    """TEDSPAD_DETERMINISTIC=1: called where training objects are built (the library is loaded and a GPU is present by then)."""
    if os.environ.get("TEDSPAD_DETERMINISTIC", "0") == "1" and not DETERMINISTIC:
        set_deterministic(True)

PREFER_TILE_CFG = int(os.environ.get("TEDSPAD_PREFER_CFG", "0"))
FORCE_TILE_CFG = None   # tests: run every conv with this tile configuration (error if it does not apply)
# The kernels index with 32-bit element offsets (and the weight gradient decodes < 2^23 pixels): larger tensors
# (cfg5: 384 frames of 224x224) are processed in chunks of whole samples along n, transparently to the callers.
MAX_ELEMS = (1 << 31) - (1 << 20)
MAX_WGRAD_PIXELS = (1 << 23) - 64


def batch_chunk(n: int, per_sample_sizes, limit: int) -> int:
    """Largest number of samples per launch so that every per-sample size x samples stays below `limit`."""
    worst = max(int(v) for v in per_sample_sizes)
    if worst >= limit:
        raise _lib.TedSpadHipError("a single sample has %d elements: too large for the 32-bit offsets of the kernels" % worst)
    return max(1, min(n, limit // worst))


def sample_chunks(n: int, per_sample_sizes, limit: int, *more):
    """The batch as ranges (n0, n1) of whole samples, each small enough for `batch_chunk(n, per_sample_sizes, limit)` -- and for every further
    (sizes, limit) pair in `more`. A batch that fits one launch comes back as (0, n) alone, for which `Act.samples` is the Act itself. Callers pass
    the limit they read from this module when they call (MAX_ELEMS, MAX_WGRAD_PIXELS): tests lower those."""
    nc = batch_chunk(n, per_sample_sizes, limit)
    for i in range(0, len(more), 2):
        nc = min(nc, batch_chunk(n, more[i], more[i + 1]))
    for first in range(0, n, nc):
        yield first, min(n, first + nc)


def dtype_code(t: torch.Tensor) -> int:
    """The library's storage-type code of a 16-bit tensor."""
    return _lib.F16 if t.dtype == torch.float16 else _lib.BF16


class _Cfgs(dict):
    """geometry key -> chosen tile configuration (int) or the tuner's in-progress state (dict). One instance per convolution,
    SHARED by the PackedConv objects that succeed each other when the weights are re-packed after an optimizer step
    (train_engine.ConvLayer.fwd_conv), so it -- not the PackedConv -- is the identity of a tuning job."""
    __slots__ = ("__weakref__",)


TILE_PICKS = {}         # tile_cfg -> geometries the tuner has settled on it in this process (which of the 39 configurations earn their place: bench.py --tile-picks)
_TUNING = {}            # (id(_Cfgs), geometry key) -> weakref to the _Cfgs whose configurations are still taking turns
_CLOCK = [0]            # conv launches so far (a tuning job that has not been touched for TUNE_STALE launches no longer holds anybody up)
TUNE_STALE = 20000


def tuning_pending() -> bool:
    """True while any conv geometry seen so far is still being tuned. Callers that overlap forwards on several
    streams stay on ONE stream until this is False: a candidate timed while other streams' kernels share the CUs
    is measured with their interference and can lose to a slower configuration. Jobs whose convolution was dropped
    (a model re-packed from scratch) or already decided are pruned here."""
    pending = False
    for k, ref in list(_TUNING.items()):
        cfgs = ref()
        st = cfgs.get(k[1]) if cfgs is not None else None
        if not isinstance(st, dict):
            del _TUNING[k]
        elif _CLOCK[0] - st.get("tick", 0) <= TUNE_STALE:      # a geometry that stopped coming (a one-off batch size): its job waits, nobody waits for it
            pending = True
    return pending


def _tuned_objects(packed: dict):
    """(name, object holding a `_cfgs` table) for every tunable launch of a network's `packed()` dict."""
    for name, obj in packed.items():
        for suffix, o in (("", obj), (".pc", getattr(obj, "pc", None)), (".conv2", getattr(obj, "conv2", None))):
            if o is not None and isinstance(getattr(o, "_cfgs", None), _Cfgs):
                yield name + suffix, o


def export_tile_table(packed: dict) -> dict:
    """{launch name: {geometry key: tile configuration}} of every DECIDED choice of a packed network -- what rank 0 broadcasts after its tuning
    pass so that every rank of a multi-GPU job runs the same tiles (bench.py, extraction.extract_video_sharded): tiles that re-associate the K sum
    differ in the last bit, so ranks that tuned on their own would not produce bit-identical features for the same clip."""
    return {name: {k: v for k, v in o._cfgs.items() if isinstance(v, int)} for name, o in _tuned_objects(packed)}


def import_tile_table(packed: dict, table: dict) -> int:
    """Adopt the choices of `export_tile_table` (same network, same geometries); pending tuning jobs for those geometries are dropped.
    Returns the number of choices taken over."""
    n = 0
    for name, o in _tuned_objects(packed):
        for k, v in table.get(name, {}).items():
            o._cfgs[k] = int(v)
            _TUNING.pop((id(o._cfgs), k), None)
            n += 1
    return n


_raw_stream, _cur_device = torch._C._cuda_getCurrentRawStream, torch._C._cuda_getDevice


def _stream_ptr():
    # the raw handle of torch's current HIP stream on the current device: `torch.cuda.current_stream().cuda_stream` builds a Stream object and resolves the device
    # through three Python layers (9 us a call under the profiler, 500 calls per training step: a third of phase 2's host time)
    return C.c_void_p(_raw_stream(_cur_device()))


def require_cuda(t: torch.Tensor, what: str):
    if not t.is_cuda:
        raise _lib.TedSpadHipError(
            "%s: got a %s tensor. ted_spad_amd runs only on MI355X through libtedspad_hip.so; "
            "there is no CPU path (use oracle/ for a CPU reference in tests)." % (what, t.device))


@dataclass
class Act:
    """A channels-last activation: `buf` is (n, t, h, w, ld) 16-bit; this view covers
    channels [coff, coff + c) of every pixel (concat slices share one buffer). `cpad`: set on a network's INPUT activation only
    (clip_to_act, preprocess.crop_resize_act): the channel count every pixel was padded to, 4 = the pixel-pair buffer; 0 anywhere else."""
    buf: torch.Tensor
    c: int
    coff: int = 0
    cpad: int = 0

    @property
    def dims(self) -> Tuple[int, int, int, int]:
        return tuple(self.buf.shape[:4])

    @property
    def ld(self) -> int:
        return self.buf.shape[4]

    @property
    def ptr(self) -> int:
        return self.buf.data_ptr() + self.coff * 2

    def slice(self, coff: int, c: int) -> "Act":
        assert coff % 8 == 0 and c % 8 == 0 and coff + c <= self.c
        return Act(self.buf, c, self.coff + coff)

    def samples(self, n0: int, n1: int) -> "Act":
        """Samples [n0, n1) of the same channel view (a chunk of `sample_chunks`); the whole batch is this Act itself: nothing is sliced or re-wrapped."""
        if n0 == 0 and n1 == self.buf.shape[0]:
            return self
        return Act(self.buf[n0:n1], self.c, self.coff, self.cpad)

    @staticmethod
    def empty(n, t, h, w, c, dtype, device) -> "Act":
        return Act(torch.empty((n, t, h, w, c), dtype=dtype, device=device), c)


class _Geo:
    """Pixel grid of a gathered input (PackedConv.gather): what the conv descriptor needs of an Act, without a tensor."""

    def __init__(self, dims, c):
        self.dims, self.c, self.ld, self.ptr = tuple(dims), c, c, None


def conv_out(size, k, s, pf, pb):
    return (size + pf + pb - k) // s + 1


def same_pads(size, k, s):
    """TF-SAME front/back zero padding of one dim (reference rule: i3d.py:82-86,101-106)."""
    total = max(k - s, 0) if size % s == 0 else max(k - (size % s), 0)
    return total // 2, total - total // 2


def fold_bn(gamma, beta, mean, var, eps, conv_bias=None):
    """y = gamma*(x + b - mean)/sqrt(var+eps) + beta  ==  x*scale + shift   (fp64 -> fp32).
    On the GPU one launch of tedspad_bn_fold; host tensors (weight-layout tests, before .cuda()) use the same formula."""
    if gamma.is_cuda:
        g, b, m, v = (t.detach().float().contiguous() for t in (gamma, beta, mean, var))
        cb = conv_bias.detach().float().contiguous() if conv_bias is not None else None
        n = g.numel()
        store = torch.zeros((2, (n + 127) // 128 * 128), dtype=torch.float32, device=g.device)
        scale, shift = store[0, :n], store[1, :n]
        # zero-padded to the conv kernels' row padding: a PackedConv built from these takes them as its own scale / shift vectors (no copy),
        # so a later in-place re-fold (FoldRefresh / tedspad_fold_multi) is all a changed BatchNorm needs
        scale._tedspad_padded = shift._tedspad_padded = store.shape[1]
        check(_lib.lib().tedspad_bn_fold(g.data_ptr(), b.data_ptr(), m.data_ptr(), v.data_ptr(), cb.data_ptr() if cb is not None else None,
                                         C.c_double(eps), n, scale.data_ptr(), shift.data_ptr(), _stream_ptr()), "tedspad_bn_fold")
        return scale, shift
    inv = gamma.double() / torch.sqrt(var.double() + eps)
    shift = beta.double() - mean.double() * inv
    if conv_bias is not None:
        shift = shift + conv_bias.double() * inv
    return inv.float(), shift.float()


_CONST_VECS = {}


def _padded_vec(v, n, npad, device, fill):
    """fp32 [npad] = v[:n] then zeros; `v` None -> a cached constant vector of `fill` (no launch)."""
    if v is None:
        key = (str(device), npad, n, fill)
        t = _CONST_VECS.get(key)
        if t is None:
            t = torch.zeros(npad, dtype=torch.float32, device=device)
            t[:n] = fill
            _CONST_VECS[key] = t
        return t
    if getattr(v, "_tedspad_padded", 0) >= npad and v.device == torch.device(device) and v.numel() >= n:
        return torch.as_strided(v, (npad,), (1,), v.storage_offset())                    # fold_bn output: already zero-padded storage
    v = v.detach().to(device=device, dtype=torch.float32)
    return v.contiguous() if npad == n else torch.nn.functional.pad(v, (0, npad - n))     # at most one launch


class JobTable:
    """A static job table of one of the multi-job launches (tedspad_pack_multi / _fold_multi / _wgrad_unpack_multi): built once from ctypes
    job structs, uploaded by its first launch, then re-launched as is (every address in it is persistent)."""
    FN = {_lib.PackJob: "tedspad_pack_multi", _lib.FoldJob: "tedspad_fold_multi", _lib.WgradUnpackJob: "tedspad_wgrad_unpack_multi"}

    def __init__(self, jobs, keep=()):
        self.n = len(jobs)
        self.keep = list(keep)                      # tensors the jobs point at
        if self.n:
            kind = type(jobs[0])
            self.fn = self.FN[kind]
            self.arr = (kind * self.n)(*jobs)
            self.dev = None

    def launch(self, device):
        if not self.n:
            return
        upload = self.dev is None
        if upload:
            self.dev = torch.empty(C.sizeof(self.arr), dtype=torch.uint8, device=device)
        check(getattr(_lib.lib(), self.fn)(C.cast(self.arr, C.c_void_p), self.n, self.dev.data_ptr(), int(upload), _stream_ptr()), self.fn)


class PackedRefresh:
    """In-place refresh of the images of an eval-mode network (`packed()` of unet.py / unetpp.py) after its parameters changed: the folds
    and weight images recorded while the network was packed are rewritten by one tedspad_fold_multi + one tedspad_pack_multi launch; the
    PackedConv objects -- buffers, gather tables, tuned tile choices -- stay."""

    def __init__(self):
        self.fj, self.pj, self.keep, self.tabs = [], [], [], None

    def fold(self, bn, conv_bias, scale, shift):
        self.fj.append(fold_job(bn, conv_bias, scale, shift))
        self.keep += [scale, shift]

    def bias(self, pc: "PackedConv", bias):
        """A conv without BatchNorm whose shift vector is (a padded copy of) its bias."""
        assert bias.is_cuda and bias.dtype == torch.float32 and bias.is_contiguous()
        self.fj.append(_lib.FoldJob(gamma=None, beta=None, mean=None, var=None, conv_bias=bias.data_ptr(), scale=None, shift=pc.shift.data_ptr(),
                                    scale2=None, shift2=None, eps=0.0, C=bias.numel(), n=pc.shift.numel(), n2=0, reserved=0))
        self.keep.append(pc)

    def pack(self, pc: "PackedConv", weight, wscale=None):
        self.pj.append(pc.pack_job(weight.detach(), wscale))
        self.keep.append(pc)

    def run(self, device):
        if self.tabs is None:
            self.tabs = (JobTable(self.fj), JobTable(self.pj))
        for t in self.tabs:
            t.launch(device)


def same_storage(sig_a, sig_b) -> bool:
    """Two `params_signature`s that differ in version counters only (in-place updates: an optimizer step, running statistics)."""
    return len(sig_a) == len(sig_b) and all(a[0] == b[0] and a[2] == b[2] for a, b in zip(sig_a, sig_b))


def fold_job(bn, conv_bias, scale, shift):
    """FoldJob re-folding `bn` (+ conv bias) into the zero-padded (scale, shift) vectors `fold_bn` returned for it."""
    ts = [bn.weight, bn.bias, bn.running_mean, bn.running_var] + ([conv_bias] if conv_bias is not None else [])
    for t in ts:
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), "fold refresh needs contiguous fp32 CUDA BatchNorm tensors"
    n = int(getattr(scale, "_tedspad_padded", scale.numel()))
    return _lib.FoldJob(gamma=bn.weight.data_ptr(), beta=bn.bias.data_ptr(), mean=bn.running_mean.data_ptr(), var=bn.running_var.data_ptr(),
                        conv_bias=conv_bias.data_ptr() if conv_bias is not None else None, scale=scale.data_ptr(), shift=shift.data_ptr(),
                        scale2=None, shift2=None, eps=float(bn.eps), C=bn.weight.numel(), n=n, n2=0, reserved=0)


def stem_pair_form(w: torch.Tensor, pair_w: int):
    """(co, ci<=4, kt, kh, kw) stride-2-along-W weights with FRONT pad `pair_w` -> the equivalent
    (co, 8, kt, kh, kw') weights over pixel PAIRS (2 pixels x 4 channels, stride 1): tap k of the
    original lands on pair-tap d = (k + shift) // 2, half j = (k + shift) % 2."""
    co, ci, kt, kh, kw = w.shape
    assert ci <= 4
    pw2 = (pair_w + 1) // 2
    shift_k = 2 * pw2 - pair_w
    kw2 = (kw + shift_k + 1) // 2
    w2 = torch.zeros((co, 8, kt, kh, kw2), dtype=w.dtype, device=w.device)
    for k in range(kw):
        d, j = divmod(k + shift_k, 2)
        w2[:, j * 4:j * 4 + ci, :, :, d] = w[:, :, :, :, k]
    return w2, kw2, pw2


def stem_pair_grad(dw2: torch.Tensor, ci: int, kw: int, pair_w: int):
    """Inverse gather of `stem_pair_form` for gradients: (co, 8, kt, kh, kw') -> (co, ci, kt, kh, kw)."""
    pw2 = (pair_w + 1) // 2
    shift_k = 2 * pw2 - pair_w
    cols = []
    for k in range(kw):
        d, j = divmod(k + shift_k, 2)
        cols.append(dw2[:, j * 4:j * 4 + ci, :, :, d])
    return torch.stack(cols, dim=4)


class PackedConv:
    """One convolution resident on the device in the kernel's layout:
    weights [cout_pad][kpad] 16-bit with K ordered (dt, dh, dw, ci); fp32 scale/shift;
    per-input-geometry K-chunk gather tables."""

    nosat = False       # True on the training path (train_engine.ConvLayer): tedspad_conv_extras.nosat

    def __init__(self, weight: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, stride=(1, 1, 1),
                 dtype: str = DEFAULT_DTYPE, device="cuda", pair_w: Optional[int] = None):
        """weight: (cout, cin, kt, kh, kw) fp32 (2-D convs: kt = 1).
        pair_w: if not None, the conv has cin <= 4 and stride 2 along W with FRONT pad `pair_w`:
        it is rewritten over pixel PAIRS (cin' = 8 = 2 pixels x 4 channels, kw' = ceil((kw+shift)/2),
        stride_w' = 1), so the Cin=3 stems run on the generic 8-channel-chunk gather."""
        device = torch.device(device)
        w = weight.detach().to(device=device, dtype=torch.float32)
        cout, cin, kt, kh, kw = w.shape
        st, sh, sw = stride
        self.pair = pair_w is not None
        pair_shift = -1
        if self.pair:
            assert cin <= 4 and sw == 2
            self.pair_pw = (pair_w + 1) // 2
            pair_shift = 2 * self.pair_pw - pair_w
            cin_k, kw_k, sw = 8, (kw + pair_shift + 1) // 2, 1
        else:
            cin_k, kw_k = (cin + 7) // 8 * 8, kw
        self.cout_real = cout
        self.cout = (cout + 7) // 8 * 8
        self.cin, self.k, self.stride = cin_k, (kt, kh, kw_k), (st, sh, sw)
        self.torch_dtype, self.dtype_code = DTYPES[dtype]
        d = self._desc(1, 1, 1, 1, cin_k, (0, 0, 0), (1, 1, 1), self.cout, 0, True)
        self.kpad = _lib.lib().tedspad_conv_kpad(d)
        self.cpad = _lib.lib().tedspad_conv_cout_pad(d)
        self.K = kt * kh * kw_k * cin_k
        if device.type == "cuda":      # one pack launch (csrc/pack.hip)
            self.w = torch.empty((self.cpad, self.kpad), dtype=self.torch_dtype, device=device)
            wc = w.contiguous()
            check(_lib.lib().tedspad_pack_conv_weights(wc.data_ptr(), None, self.w.data_ptr(), cout, cin, kt, kh, kw, cin_k, kw_k, pair_shift,
                                                       0, cout, self.cpad, self.kpad, None, self.dtype_code, _stream_ptr()),
                  "tedspad_pack_conv_weights")
            self._pack_args = dict(co=cout, ci=cin, kt=kt, kh=kh, kw=kw, cink=cin_k, kwk=kw_k, pair_shift=pair_shift, mode=0, rows=cout, geo=(0,) * 9)
        else:                          # host packing (CPU tests of the layout)
            if self.pair:
                w, _, _ = stem_pair_form(w, pair_w)
            elif cin % 8:
                w = torch.nn.functional.pad(w, (0, 0, 0, 0, 0, 0, 0, cin_k - cin))
            self.w = torch.zeros(self.cpad, self.kpad, dtype=self.torch_dtype, device=device)
            self.w[:cout, :self.K] = w.permute(0, 2, 3, 4, 1).reshape(cout, self.K).to(self.torch_dtype)
        self.scale = _padded_vec(scale, cout, self.cpad, device, 1.0)
        self.shift = _padded_vec(shift, cout, self.cpad, device, 0.0)
        self.device = device
        self._ktabs = {}
        self._cfgs = _Cfgs()

    @classmethod
    def dgrad_sub(cls, w5: torch.Tensor, wscale, geo, pair_w, dtype):
        """The data-gradient matrix of one parity class, packed on the device in one launch.
        w5: the (co, ci, kt, kh, kw) fp32 CUDA parameter; wscale: per-co fp32 scale folded into the weights or None;
        geo = (Et,Eh,Ew, ct,ch,cw, st,sh,sw)."""
        self = cls.__new__(cls)
        co, ci, kt, kh, kw = w5.shape
        self.pair = False
        pair_shift, cin_k, kw_k = -1, (ci + 7) // 8 * 8, kw
        if pair_w is not None:
            pw2 = (pair_w + 1) // 2
            pair_shift = 2 * pw2 - pair_w
            cin_k, kw_k = 8, (kw + pair_shift + 1) // 2
        co8 = (co + 7) // 8 * 8
        self.cout_real = self.cout = cin_k
        self.cin, self.k, self.stride = co8, tuple(geo[:3]), (1, 1, 1)
        self.torch_dtype, self.dtype_code = DTYPES[dtype]
        d = self._desc(1, 1, 1, 1, co8, (0, 0, 0), (1, 1, 1), self.cout, 0, False)
        self.kpad = _lib.lib().tedspad_conv_kpad(d)
        self.cpad = _lib.lib().tedspad_conv_cout_pad(d)
        self.K = geo[0] * geo[1] * geo[2] * co8
        dev = w5.device
        self.w = torch.empty((self.cpad, self.kpad), dtype=self.torch_dtype, device=dev)
        g = (C.c_int32 * 9)(*geo)
        wc = w5.detach().contiguous()
        check(_lib.lib().tedspad_pack_conv_weights(wc.data_ptr(), wscale.data_ptr() if wscale is not None else None, self.w.data_ptr(), co, ci,
                                                   kt, kh, kw, cin_k, kw_k, pair_shift, 1, cin_k, self.cpad, self.kpad, g, self.dtype_code,
                                                   _stream_ptr()), "tedspad_pack_conv_weights")
        self._pack_args = dict(co=co, ci=ci, kt=kt, kh=kh, kw=kw, cink=cin_k, kwk=kw_k, pair_shift=pair_shift, mode=1, rows=cin_k, geo=tuple(geo))
        self.scale = _padded_vec(None, cin_k, self.cpad, dev, 1.0)
        self.shift = _padded_vec(None, cin_k, self.cpad, dev, 0.0)
        self.device = dev
        self._ktabs, self._cfgs = {}, _Cfgs()
        return self

    def pack_job(self, w: torch.Tensor, wscale=None) -> "_lib.PackJob":
        """The PackJob that rewrites this object's weight image in place from the fp32 parameter `w` (the tensor -- or one of the same shape --
        it was built from) and the per-output-channel scale folded into it (data-gradient images of a frozen BatchNorm)."""
        a = getattr(self, "_pack_args", None)
        if a is None:
            raise _lib.TedSpadHipError("PackedConv.pack_job: this image was not packed on the device")
        assert w.is_cuda and w.dtype == torch.float32 and w.is_contiguous() and w.numel() == a["co"] * a["ci"] * a["kt"] * a["kh"] * a["kw"], \
            "pack_job needs the contiguous fp32 CUDA parameter this image was built from"
        j = _lib.PackJob(w=w.data_ptr(), scale=wscale.data_ptr() if wscale is not None else None, out=self.w.data_ptr(),
                         co=a["co"], ci=a["ci"], kt=a["kt"], kh=a["kh"], kw=a["kw"], cink=a["cink"], kwk=a["kwk"], pair_shift=a["pair_shift"],
                         mode=a["mode"], rows=a["rows"], rows_pad=self.cpad, kpad=self.kpad, dtype=self.dtype_code, block0=0, nblocks=0)
        for i, g in enumerate(a["geo"]):
            j.geo[i] = g
        return j

    def _desc(self, n, t, h, w, ldx, pads, out, ldy, ldres, relu):
        kt, kh, kw = self.k
        st, sh, sw = self.stride
        return ConvDesc(n=n, t=t, h=h, w=w, cin=self.cin, ldx=ldx, cout=self.cout, ldy=ldy, ldres=ldres,
                        kt=kt, kh=kh, kw=kw, st=st, sh=sh, sw=sw, pt=pads[0], ph=pads[1], pw=pads[2],
                        to=out[0], ho=out[1], wo=out[2], relu=int(relu), dtype=self.dtype_code, tile_cfg=0)

    def _ktab(self, d: ConvDesc):
        key = (d.t, d.h, d.w, d.ldx)
        tab = self._ktabs.get(key)
        if tab is None:
            n = _lib.lib().tedspad_conv_ktab_entries(d)
            host = (C.c_int32 * (2 * n))()
            check(_lib.lib().tedspad_conv_build_ktab(d, host), "tedspad_conv_build_ktab")
            tab = torch.frombuffer(host, dtype=torch.int32).clone().to(self.device)
            self._ktabs[key] = tab
        return tab

    # ---- in-context tile tuning -------------------------------------------------------------------------------
    # Every call during the tuning phase IS a real call (any tile configuration gives the same result), launched
    # with the next candidate and bracketed by HIP events; after TUNE_REPS passes over the candidates the
    # fastest (median) is kept. Timing each configuration inside the running network -- cold caches, the other
    # stream's kernels alongside -- ranks them as they will actually run; replaying one launch in isolation
    # (first version) favoured L2-hungry configurations that lose in context.
    TUNE_REPS = int(os.environ.get("TEDSPAD_TUNE_REPS", "3"))

    def _launch_tuned(self, key, d, args):
        L = _lib.lib()
        stream = _stream_ptr()
        _CLOCK[0] += 1
        if FORCE_TILE_CFG is not None:
            d.tile_cfg = FORCE_TILE_CFG
            check(L.tedspad_conv_fwd_ex(*args, stream), "tedspad_conv_fwd(cfg %d)" % FORCE_TILE_CFG)
            return
        if PREFER_TILE_CFG:          # experiments: use this configuration wherever it applies
            d.tile_cfg = PREFER_TILE_CFG
            if L.tedspad_conv_fwd_ex(*args, stream) == 0:
                self._cfgs[key] = PREFER_TILE_CFG
                return
        st = self._cfgs.get(key)
        if AUTOTUNE and isinstance(st, int):
            d.tile_cfg = st
            check(L.tedspad_conv_fwd_ex(*args, stream), "tedspad_conv_fwd")
            return
        if not AUTOTUNE or torch.cuda.is_current_stream_capturing():     # built-in heuristic: only K-order-preserving tiles
            d.tile_cfg = 0
            check(L.tedspad_conv_fwd_ex(*args, stream), "tedspad_conv_fwd")
            return
        if st is None:
            st = {"cands": [c for c in range(0, L.tedspad_conv_num_tile_cfgs() + 1) if c not in SKIP_TILE_CFGS], "pos": 0, "rep": 0, "rec": {}}
            self._cfgs[key] = st
            _TUNING[(id(self._cfgs), key)] = weakref.ref(self._cfgs)
        st["tick"] = _CLOCK[0]
        while True:
            cfg = st["cands"][st["pos"]]
            d.tile_cfg = cfg
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = L.tedspad_conv_fwd_ex(*args, stream)
            if rc != 0:                                   # configuration not applicable to this conv: drop it
                st["cands"].pop(st["pos"])
                if not st["cands"]:
                    check(rc, "tedspad_conv_fwd")
                if st["pos"] >= len(st["cands"]):
                    st["pos"] = 0
                    st["rep"] += 1
                continue
            e1.record()
            st["rec"].setdefault(cfg, []).append((e0, e1))
            break
        st["pos"] += 1
        if st["pos"] >= len(st["cands"]):
            st["pos"] = 0
            st["rep"] += 1
            # after every full pass keep only the candidates within 1.3x of the best so far: the later passes
            # (which decide) cost a handful of calls instead of one per configuration
            med = {}
            for cfg in st["cands"]:
                ts = []
                for a, b in st["rec"].get(cfg, []):
                    b.synchronize()
                    ts.append(a.elapsed_time(b))
                ts.sort()
                med[cfg] = ts[len(ts) // 2] if ts else float("inf")
            lo = min(med.values())
            st["cands"] = [c for c in st["cands"] if med[c] <= 1.3 * lo]
            st["med"] = med
        if st["rep"] >= self.TUNE_REPS or (st["rep"] >= 1 and len(st["cands"]) == 1):
            med = st.get("med") or {c: 0.0 for c in st["cands"]}
            best, best_ms = st["cands"][0], float("inf")
            for cfg in st["cands"]:
                if med[cfg] < best_ms * 0.98:
                    best, best_ms = cfg, med[cfg]
            self._cfgs[key] = best
            TILE_PICKS[best] = TILE_PICKS.get(best, 0) + 1
            _TUNING.pop((id(self._cfgs), key), None)

    def pool_t2_supported(self, x: Act) -> bool:
        return self.k == (1, 1, 1) and self.stride == (1, 1, 1) and self.cin in (64, 128) and x.dims[1] >= 2

    def call_pool_t2(self, x: Act, residual: Optional[Act] = None, relu=True) -> Act:
        """conv (1x1x1) + scale/shift + residual + ReLU + MaxPool3d((2,1,1),(2,1,1)) in one persistent launch
        (tedspad_conv_pool_t2_fwd): the un-pooled tensor is never written."""
        n, t, h, w = x.dims
        assert self.pool_t2_supported(x) and x.c == self.cin
        if residual is not None:
            assert residual.dims == x.dims and residual.c == self.cout
        out = Act.empty(n, t // 2, h, w, self.cout, self.torch_dtype, x.buf.device)
        worst = max(t * h * w * x.ld, t * h * w * (residual.ld if residual is not None else self.cout))
        for n0, n1 in sample_chunks(n, [worst], MAX_ELEMS):
            xs, rs, os_ = (a.samples(n0, n1) if a is not None else None for a in (x, residual, out))
            d = self._desc(n1 - n0, t, h, w, xs.ld, (0, 0, 0), (t, h, w), os_.ld, rs.ld if rs is not None else 0, relu)
            check(_lib.lib().tedspad_conv_pool_t2_fwd(C.byref(d), xs.ptr, self.w.data_ptr(), self.scale.data_ptr(), self.shift.data_ptr(),
                                                      rs.ptr if rs is not None else None, os_.ptr, _stream_ptr()), "tedspad_conv_pool_t2_fwd")
        return out

    def dual_supported(self, other: "PackedConv", x: Act, x2: Act) -> bool:
        return (os.environ.get("TEDSPAD_DUAL_PW", "1") != "0" and self.k == (1, 1, 1) and other.k == (1, 1, 1) and self.stride == (1, 1, 1) and other.stride == (1, 1, 1) and
                self.cin == 64 and other.cin == 64 and self.cout == other.cout and x.dims == x2.dims and self.dtype_code == other.dtype_code)

    def call_dual(self, x: Act, other: "PackedConv", x2: Act, relu=True) -> Act:
        """act(self(x) + other(x2)): two 1x1x1 convs with cin = 64 summed in one persistent launch
        (tedspad_conv_pw_dual_fwd) -- conv3 + bn3 and the downsample branch of the first layer1 bottleneck."""
        assert self.dual_supported(other, x, x2) and x.c == 64 and x2.c == 64
        n, t, h, w = x.dims
        out = Act.empty(n, t, h, w, self.cout, self.torch_dtype, x.buf.device)
        worst = t * h * w * max(x.ld, x2.ld, self.cout)
        for n0, n1 in sample_chunks(n, [worst], MAX_ELEMS):
            xs, x2s, os_ = (a.samples(n0, n1) for a in (x, x2, out))
            d = self._desc(n1 - n0, t, h, w, xs.ld, (0, 0, 0), (t, h, w), os_.ld, 0, relu)
            check(_lib.lib().tedspad_conv_pw_dual_fwd(C.byref(d), xs.ptr, self.w.data_ptr(), self.scale.data_ptr(), self.shift.data_ptr(),
                                                      x2s.ptr, x2s.ld, other.w.data_ptr(), other.scale.data_ptr(), other.shift.data_ptr(),
                                                      os_.ptr, _stream_ptr()), "tedspad_conv_pw_dual_fwd")
        return out

    @classmethod
    def fused_pair(cls, w1: torch.Tensor, s1, b1, w2: torch.Tensor, s2, b2, dtype: str = DEFAULT_DTYPE, device="cuda") -> "PackedConv":
        """[W1*s1 | W2*s2] as ONE 1x1x1 matrix over the concatenated input channels (shift = b1 + b2, scale = 1): the
        K-concatenated form of `act(bn(conv1(x)) + bn(conv2(x2)))` that `call_dual_p8` runs as a single GEMM."""
        assert tuple(w1.shape[2:]) == (1, 1, 1) and tuple(w2.shape[2:]) == (1, 1, 1) and w1.shape[0] == w2.shape[0]
        dev = torch.device(device)
        wc = torch.cat([w1.detach().to(dev, torch.float32) * s1.to(dev).view(-1, 1, 1, 1, 1),
                        w2.detach().to(dev, torch.float32) * s2.to(dev).view(-1, 1, 1, 1, 1)], dim=1)
        pc = cls(wc, torch.ones(w1.shape[0], device=dev), (b1.to(dev) + b2.to(dev)), dtype=dtype, device=dev)
        pc.cin1, pc.cin2 = int(w1.shape[1]), int(w2.shape[1])
        return pc

    def dual_p8_supported(self, x: Act, x2: Act, stride2) -> bool:
        n, t, h, w = x.dims
        n2, t2, h2, w2 = x2.dims
        return (os.environ.get("TEDSPAD_DUAL_P8", "1") != "0" and getattr(self, "cin1", 0) > 0 and self.cin1 % 64 == 0 and self.cin2 % 64 == 0 and
                self.cout % 256 == 0 and x.c == self.cin1 and x2.c == self.cin2 and n2 == n and t2 == t and
                (h - 1) * stride2[0] < h2 and (w - 1) * stride2[1] < w2 and n * t * h2 * w2 * x2.ld < MAX_ELEMS and n * t * h * w * max(x.ld, self.cout) < MAX_ELEMS)

    def call_dual_p8(self, x: Act, x2: Act, stride2=(2, 2), relu=True) -> Act:
        """act([W1*s1 | W2*s2] . [x ; x2 sampled with spatial stride stride2] + shift) on the ping-pong kernel
        (tedspad_conv_p8_dual_fwd): conv3 + bn3 and the strided downsample branch of layer2.0 / 3.0 / 4.0 as one GEMM."""
        assert self.dual_p8_supported(x, x2, stride2)
        n, t, h, w = x.dims
        out = Act.empty(n, t, h, w, self.cout, self.torch_dtype, x.buf.device)
        d = self._desc(n, t, h, w, x.ld, (0, 0, 0), (t, h, w), out.ld, 0, relu)
        d.cin = self.cin1
        check(_lib.lib().tedspad_conv_p8_dual_fwd(C.byref(d), x.ptr, x2.ptr, self.cin2, x2.ld, x2.dims[2], x2.dims[3], stride2[0], stride2[1],
                                                  self.w.data_ptr(), self.scale.data_ptr(), self.shift.data_ptr(), out.ptr, _stream_ptr()),
              "tedspad_conv_p8_dual_fwd")
        return out

    def _run(self, x, pads, o, out, residual, mask, stats, out_map, z32, relu, sigmoid, sources=None):
        """One launch (through the tuner) on tensors small enough for the kernel's 32-bit offsets."""
        n, t, h, w = x.dims
        y32 = z32 is not None
        d = self._desc(n, t, h, w, x.ld, pads, o, out.ld, residual.ld if residual is not None else 0, relu)
        ex = None
        if mask is not None or stats is not None or out_map is not None or y32 or self.nosat or sources is not None:
            ex = _lib.ConvExtras()
            ex.nosat = int(self.nosat)
            if sources is not None:      # gathered concatenation: one descriptor per 64-channel chunk (tedspad_conv_extras.nchunk_src)
                k = 0
                for a, up in sources:
                    for j in range(a.c // 64):
                        ex.chunk_src[k], ex.chunk_ld[k] = a.ptr + j * 128, a.ld
                        ex.chunk_up |= int(bool(up)) << k
                        k += 1
                ex.nchunk_src = k
            if y32:
                ex.y32, ex.ldy32 = z32.data_ptr(), self.cout
            if mask is not None:
                ex.mask, ex.ldmask = mask.ptr, mask.ld
            if stats is not None:
                assert stats.dtype == torch.float32 and stats.is_contiguous() and stats.shape[-2] == 2 and stats.shape[-1] >= self.cout
                ex.stats, ex.stats_ld = stats.data_ptr(), stats.shape[-1]
                if stats.dim() == 3 and stats.shape[0] > 1:          # (G, 2, ld): G groups of consecutive samples with their own statistics
                    rows = n * o[0] * o[1] * o[2]
                    assert n % stats.shape[0] == 0 and rows // stats.shape[0] >= 256, "grouped batch statistics need >= 256 output rows per group"
                    ex.stats_rows = rows // stats.shape[0]
            if out_map is not None:
                (ex.ost, ex.osh, ex.osw), (ex.oot, ex.ooh, ex.oow) = out_map
                ex.out_strided = 1
                _, ex.tf, ex.hf, ex.wf = out.dims
        args = (C.byref(d), None if sources is not None else x.ptr, self.w.data_ptr(), self._ktab(d).data_ptr(), self.scale.data_ptr(), self.shift.data_ptr(),
                residual.ptr if residual is not None else None, None if y32 else out.ptr, int(sigmoid),
                C.byref(ex) if ex is not None else None)
        key = (n, t, h, w, x.ld, tuple(pads), o, out.ld, residual is not None, mask is not None, stats is not None, out_map, y32,
               None if sources is None else tuple((a.c, a.ld, bool(up)) for a, up in sources))
        self._launch_tuned(key, d, args)

    def gather(self, sources, pads=(0, 0, 0), out: Optional[Act] = None, relu=True) -> Act:
        """The conv on `torch.cat([s (nearest x2 upsampled if up) for s, up in sources], dim=1)` without that tensor: every source (an Act with a multiple
        of 64 channels; `up` sources at half the height and width) is read in place by the patch / flat halo kernels (tile_cfg 32 / 33,
        tedspad_conv_extras.nchunk_src) -- the decoder blocks of the default anonymizer (unet++: smp DecoderBlock.forward = interpolate + cat + conv).
        Stride-1 'same' convs with kt = 1; same sums, in the same order, as the conv on the materialised concat buffer under the same tile_cfg."""
        assert sources and all(a.c % 64 == 0 for a, _ in sources) and sum(a.c for a, _ in sources) == self.cin and self.cin <= 512 and self.k[0] == 1
        full = [a.dims if not up else (a.dims[0], a.dims[1], 2 * a.dims[2], 2 * a.dims[3]) for a, up in sources]
        assert all(f == full[0] for f in full), "gather: the sources' pixel grids differ: %s" % (full,)
        n, t, h, w = full[0]
        kt, kh, kw = self.k
        o = (t, conv_out(h, kh, 1, pads[1], pads[1]), conv_out(w, kw, 1, pads[2], pads[2]))
        assert self.stride == (1, 1, 1) and o == (t, h, w), "gather: stride-1 'same' convolutions only"
        if out is None:
            out = Act.empty(n, t, h, w, self.cout, self.torch_dtype, sources[0][0].buf.device)
        assert out.dims == (n, t, h, w) and out.c == self.cout
        worst = t * h * w * max(max(a.ld // (4 if up else 1) for a, up in sources), out.ld)
        for n0, n1 in sample_chunks(n, [worst], MAX_ELEMS):
            sub = [(a.samples(n0, n1), up) for a, up in sources]
            geo = _Geo((n1 - n0, t, h, w), self.cin)
            self._run(geo, pads, o, out.samples(n0, n1), None, None, None, None, None, relu, False, sources=sub)
        return out

    def __call__(self, x: Act, pads=(0, 0, 0), pads_back=None, out: Optional[Act] = None,
                 residual: Optional[Act] = None, relu=True, sigmoid=False, mask: Optional[Act] = None,
                 stats: Optional[torch.Tensor] = None, out_dims=None, out_map=None, y32: bool = False):
        """pads: FRONT zero padding (t,h,w); pads_back defaults to pads (symmetric, as nn.Conv3d).
        out_dims: explicit output extent (instead of the one implied by pads_back).
        out_map = ((ost,osh,osw), (oot,ooh,oow)): output pixel (to,ho,wo) lands at (to*ost+oot, ...) of `out`
        (which then is the full, larger tensor; residual / mask are indexed the same way).
        mask: out = mask > 0 ? out : 0.  stats: fp32 (2, >=cout) batch-statistics accumulator.
        y32=True: the result is returned as an fp32 (n,to,ho,wo,cout) tensor instead of a 16-bit Act."""
        n, t, h, w = x.dims
        assert x.c == self.cin, "conv expects %d input channels, got %d" % (self.cin, x.c)
        pb = pads if pads_back is None else pads_back
        kt, kh, kw = self.k
        st, sh, sw = self.stride
        o = tuple(out_dims) if out_dims is not None else (
            conv_out(t, kt, st, pads[0], pb[0]), conv_out(h, kh, sh, pads[1], pb[1]), conv_out(w, kw, sw, pads[2], pb[2]))
        z32 = None
        if y32:
            assert out is None and out_map is None and residual is None and mask is None
            z32 = torch.empty((n,) + o + (self.cout,), dtype=torch.float32, device=x.buf.device)
            out = Act(z32, self.cout)      # geometry carrier only; the 16-bit pointer is not passed
        if out is None:
            assert out_map is None
            out = Act.empty(n, o[0], o[1], o[2], self.cout, self.torch_dtype, x.buf.device)
        if out_map is None:
            assert out.dims == (n,) + o, (out.dims, (n,) + o)
        assert out.c == self.cout, (out.c, self.cout)
        for other in (residual, mask):
            if other is not None:
                assert other.dims == out.dims and other.c == self.cout
        od = out.dims
        worst = max(t * h * w * x.ld, od[1] * od[2] * od[3] * max(out.ld, self.cout if residual is None else residual.ld,
                                                                  0 if mask is None else mask.ld))
        for n0, n1 in sample_chunks(n, [worst], MAX_ELEMS):               # the common case: one launch on the arguments as they are
            assert n1 - n0 == n or stats is None or stats.dim() == 2 or stats.shape[0] == 1, "grouped batch statistics: the batch must fit one launch"
            xs, os_, rs, ms = (a.samples(n0, n1) if a is not None else None for a in (x, out, residual, mask))
            self._run(xs, pads, o, os_, rs, ms, stats, out_map, os_.buf if y32 else None, relu, sigmoid)
        return z32 if y32 else out


class TPairConv:
    """A kt x 1 x 1 = 3 x 1 x 1 'same' (pad 1, stride 1) convolution + BN + ReLU on a TWO-frame tensor -- conv1 of the temporal bottlenecks of
    I3Res50's layer3 / layer4 after maxpool2 (large_i3d.py:61-68 with T = 2) -- as ONE GEMM over both frames with K = 2 * cin:
        out[0] = W1 . x[0] + W2 . x[1],    out[1] = W0 . x[0] + W1 . x[1]
    (the third tap of either frame multiplies zero padding: a third of the K = 3 * cin products of the plain form). The kernel sees a
    kt = 2, pad 0 conv with 2 * cout output channels [W1 W2 ; W0 W1] whose two channel halves are the two output frames
    (tedspad_conv_extras.fold_hw, ping-pong kernel): the rows of a pixel's two frames are gathered once and feed both frames' outputs."""

    def __init__(self, weight: torch.Tensor, scale, shift, dtype: str = DEFAULT_DTYPE, device="cuda"):
        assert self.supported(weight)
        co = weight.shape[0]
        w = weight.detach()
        wf = torch.cat([torch.stack([w[:, :, 1], w[:, :, 2]], dim=2), torch.stack([w[:, :, 0], w[:, :, 1]], dim=2)], dim=0)    # (2co, ci, 2, 1, 1)
        rep = lambda v: None if v is None else torch.cat([v.detach().float(), v.detach().float()])
        self.pc = PackedConv(wf, rep(scale), rep(shift), dtype=dtype, device=device)
        self.cout = co

    @staticmethod
    def supported(weight: torch.Tensor) -> bool:
        co, ci, kt, kh, kw = weight.shape
        return (kt, kh, kw) == (3, 1, 1) and ci % 64 == 0 and co % 128 == 0

    def applies(self, x: Act, pads) -> bool:
        n, t, h, w = x.dims
        return (TPAIR and self.cout >= TPAIR_MIN_COUT and t == 2 and tuple(pads) == (1, 0, 0) and x.c == self.pc.cin and
                n * 2 * h * w * max(x.ld, self.cout) < MAX_ELEMS)

    def __call__(self, x: Act, relu=True) -> Act:
        n, t, h, w = x.dims
        assert t == 2
        pc = self.pc
        out = Act.empty(n, 2, h, w, self.cout, pc.torch_dtype, x.buf.device)
        d = pc._desc(n, 2, h, w, x.ld, (0, 0, 0), (1, h, w), pc.cout, 0, relu)
        ex = _lib.ConvExtras()
        ex.fold_hw, ex.fold_c, ex.fold_ldy = h * w, self.cout, out.ld
        args = (C.byref(d), x.ptr, pc.w.data_ptr(), pc._ktab(d).data_ptr(), pc.scale.data_ptr(), pc.shift.data_ptr(), None, out.ptr, 0, C.byref(ex))
        pc._launch_tuned((n, h, w, x.ld, out.ld, "tpair"), d, args)
        return out


class BneckTail:
    """conv2 (1x3x3, 64 -> 64) + bn2 + ReLU -> conv3 (1x1x1, 64 -> cout3) + bn3 (+ residual | + downsample branch) + ReLU of a layer1
    bottleneck (large_i3d.py:49-54,69-84) as ONE launch (csrc/conv_bneck.hip): the 64-channel tensor between the two convolutions stays in
    registers (an MFMA accumulator tile is the next MFMA's operand; the conv3 weight columns are stored in that k order)."""

    # column kk = ((a*2 + s)*2 + h)*8 + j of the conv3 weight image <- input channel 32 a + 16 s + 8 (j >> 2) + 4 h + (j & 3)
    PERM = [32 * a + 16 * s + 8 * (j >> 2) + 4 * h + (j & 3) for a in range(4) for s in range(2) for h in range(2) for j in range(8)]   # first 64: the 64-channel form

    def __init__(self, conv2: "PackedConv", w3: torch.Tensor, scale3, shift3, wd: Optional[torch.Tensor] = None, scale_d=None, shift_d=None):
        assert self.supported(conv2, w3, wd)
        dev = conv2.device
        self.conv2 = conv2
        self.cout3 = int(w3.shape[0])
        self.cmid = conv2.cin                        # 64 (layer1) or 128 (layer2's plain blocks: chunk-major stage A, conv3 weights streamed)
        w3m = w3.detach().to(dev, torch.float32).reshape(self.cout3, self.cmid)[:, torch.tensor(self.PERM[:self.cmid], device=dev)]
        self.dual = wd is not None
        if self.dual:
            w3m = torch.cat([w3m, wd.detach().to(dev, torch.float32).reshape(self.cout3, 64)], dim=1)
        self.w3p = w3m.to(conv2.torch_dtype).contiguous()
        self.scale3 = scale3.detach().to(dev, torch.float32).contiguous()
        sh = shift3.detach().to(dev, torch.float32)
        self.shift3 = (sh + shift_d.detach().to(dev, torch.float32)).contiguous() if self.dual else sh.contiguous()
        self.scale_d = scale_d.detach().to(dev, torch.float32).contiguous() if self.dual else None

    @staticmethod
    def supported(conv2: "PackedConv", w3: torch.Tensor, wd=None) -> bool:
        kt, kh, kw = conv2.k
        return (conv2.cin in (64, 128) and conv2.cout == conv2.cin and kt == 1 and 2 <= kh * kw <= 32 and conv2.stride == (1, 1, 1) and not conv2.pair and
                tuple(w3.shape[1:]) == (conv2.cin, 1, 1, 1) and w3.shape[0] % 64 == 0 and w3.shape[0] <= 512 and
                (wd is None or (conv2.cin == 64 and tuple(wd.shape) == tuple(w3.shape))))

    def applies(self, x: Act, pads) -> bool:
        n, t, h, w = x.dims
        kt, kh, kw = self.conv2.k
        flat_halo = (256 + (kh - 1) * w + (kw - 1) + 1 + 8) * 128 + (4 * 8192 + 512 if self.cmid == 64 else 2 * 16384)   # halo (rounded up to 1 KB) + weight ring (+ bn2 vectors)
        return (x.c == self.cmid and pads[0] == 0 and pads[1] < kh and pads[2] < kw and 2 * pads[1] == kh - 1 and 2 * pads[2] == kw - 1 and
                flat_halo <= 80 * 1024 and n * t * h * w * max(x.ld, self.cout3) < MAX_ELEMS)

    def __call__(self, x: Act, pads=(0, 1, 1), residual: Optional[Act] = None, x2: Optional[Act] = None, relu=True, pool_t2=False, out: Optional[Act] = None) -> Act:
        """pool_t2: MaxPool3d((2,1,1), (2,1,1)) of the block's output fused (large_i3d.py:139): result (n, t // 2, h, w, cout3)."""
        n, t, h, w = x.dims
        assert self.applies(x, pads) and (x2 is not None) == self.dual and not (self.dual and residual is not None)
        assert not pool_t2 or (not self.dual and t % 2 == 0 and self.cmid == 64), "BneckTail: the temporal pool goes with the plain 64-channel block and an even frame count"
        odims = (n, t // 2 if pool_t2 else t, h, w)
        if out is None:
            out = Act.empty(*odims, self.cout3, self.conv2.torch_dtype, x.buf.device)
        assert out.dims == odims and out.c == self.cout3 and out.coff == 0
        for o in (residual, x2):
            if o is not None:
                assert o.dims == x.dims
        if residual is not None:
            assert residual.c == self.cout3
        if x2 is not None:
            assert x2.c == 64
        c2 = self.conv2
        d = c2._desc(n, t, h, w, x.ld, pads, (t, h, w), self.cmid, 0, True)
        check(_lib.lib().tedspad_bneck_tail_fwd(C.byref(d), x.ptr, c2.w.data_ptr(), c2.scale.data_ptr(), c2.shift.data_ptr(), self.w3p.data_ptr(),
                                                self.scale3.data_ptr(), self.shift3.data_ptr(), self.cout3,
                                                residual.ptr if residual is not None else None, residual.ld if residual is not None else 0,
                                                x2.ptr if x2 is not None else None, x2.ld if x2 is not None else 0,
                                                self.scale_d.data_ptr() if self.dual else None, out.ptr, out.ld, int(relu),
                                                4 if pool_t2 else 0, _stream_ptr()),
              "tedspad_bneck_tail_fwd")
        return out


class _BneckFold:
    """What the two folded layer1 tails share: a BneckTail AND the next block's conv1 (3x1x1, pads (1,0,0), 256 -> 64) + bn1 + ReLU as ONE launch on
    four-frame clips (large_i3d.py:61-84). A workgroup owns an 8 x 8 patch (a partial one at the frame's right / bottom edge: layer1 is 55 x 55 at
    224 x 224 clips) across the four frames, one frame per wave, so the temporal neighbours of a pixel sit in sibling waves and the 256-channel block
    output is not read again only to make the next block's 64-channel h. Held here: the conv1 weight image, the output allocation, the checks and the
    argument lists around the tail's second source. A subclass says which tail it takes (`supported`), which switches it obeys (`applies`) and which
    entry point gets which second source (`__call__`); it returns (y, h_next), y bit-identical to its BneckTail's."""

    def __init__(self, tail: "BneckTail", conv1: "PackedConv", w1: torch.Tensor):
        """conv1: the next block's PackedConv (its folded scale / shift are used); w1: that conv's (64, 256, 3, 1, 1) weight."""
        assert self.supported(tail, w1)
        dev = tail.conv2.device
        self.tail, self.conv1 = tail, conv1
        w = w1.detach().to(dev, torch.float32).reshape(64, 4, 64, 3).permute(1, 3, 0, 2).contiguous()      # [group][dt][co][k]
        w[:, 1] = w[:, 1][:, :, torch.tensor(BneckTail.PERM[:64], device=dev)]                                # dt = 0 tap: accumulator k order
        self.w1p = w.to(tail.conv2.torch_dtype).contiguous()

    @staticmethod
    def _foldable(tail: "BneckTail", w1: torch.Tensor) -> bool:
        return tuple(w1.shape) == (64, 256, 3, 1, 1) and tail.cmid == 64 and tail.cout3 == 256 and tail.conv2.k == (1, 3, 3)

    def _applies(self, x: Act, pads, src: Optional[Act]) -> bool:
        n, t, h, w = x.dims
        return (t == 4 and tuple(pads) == (0, 1, 1) and x.buf.dtype == self.tail.conv2.torch_dtype == self.conv1.torch_dtype and
                (src is None or src.buf.dtype == x.buf.dtype) and self.tail.applies(x, pads))

    def _args(self, x: Act, src: Act, src_c: int, pads, relu, out: Optional[Act], out_h: Optional[Act]):
        """(out, out_h, the entry point's arguments in front of the second source, those behind it); src: the second source, of src_c channels."""
        n, t, h, w = x.dims
        tl, c2 = self.tail, self.tail.conv2
        assert self.applies(x, pads, src) and src.dims == x.dims and src.c == src_c
        if out is None:
            out = Act.empty(n, t, h, w, 256, c2.torch_dtype, x.buf.device)
        if out_h is None:
            out_h = Act.empty(n, t, h, w, 64, c2.torch_dtype, x.buf.device)
        assert out.dims == x.dims and out.c == 256 and out_h.dims == x.dims and out_h.c == 64
        assert n * t * h * w * max(x.ld, out.ld, out_h.ld, src.ld) < MAX_ELEMS
        d = c2._desc(n, t, h, w, x.ld, pads, (t, h, w), 64, 0, True)
        front = (C.byref(d), x.ptr, c2.w.data_ptr(), c2.scale.data_ptr(), c2.shift.data_ptr(), tl.w3p.data_ptr(), tl.scale3.data_ptr(), tl.shift3.data_ptr())
        back = (out.ptr, out.ld, int(relu), self.w1p.data_ptr(), self.conv1.scale.data_ptr(), self.conv1.shift.data_ptr(), out_h.ptr, out_h.ld, _stream_ptr())
        return out, out_h, front, back


class BneckTailFold(_BneckFold):
    """A plain layer1 block's BneckTail and the next block's conv1 (csrc/conv_bneck_fold.hip). The two-source (downsample) tail has its own folded form,
    BneckTailFoldDual: this class refuses it (`supported`)."""

    @staticmethod
    def supported(tail: "BneckTail", w1: torch.Tensor) -> bool:
        return _BneckFold._foldable(tail, w1) and not tail.dual

    def applies(self, x: Act, pads, residual: Optional[Act] = None) -> bool:
        return L1_FOLD and self._applies(x, pads, residual)

    def __call__(self, x: Act, residual: Act, pads=(0, 1, 1), relu=True, out: Optional[Act] = None, out_h: Optional[Act] = None):
        out, out_h, front, back = self._args(x, residual, 256, pads, relu, out, out_h)
        check(_lib.lib().tedspad_bneck_tail_fold_fwd(*front, residual.ptr, residual.ld, *back), "tedspad_bneck_tail_fold_fwd")
        return out, out_h


class BneckTailFoldDual(_BneckFold):
    """layer1.0's two-source BneckTail (conv3 + bn3 + the downsample branch on x2) and layer1.1's conv1 (csrc/conv_bneck_fold_dual.hip): BneckTailFold's
    tile and fold with the downsample branch in place of the residual. The wave's LDS row image holds its frame's 64 channels of x2, fetched again for
    each of the four output groups (L2 hits), so the second source costs no registers beside the fold's tile. Reuses the tail's w3p / scale3 / shift3 /
    scale_d. Runs when both TEDSPAD_L1_FOLD and TEDSPAD_L1_FOLD_DUAL are on."""

    @staticmethod
    def supported(tail: "BneckTail", w1: torch.Tensor) -> bool:
        return _BneckFold._foldable(tail, w1) and tail.dual

    def applies(self, x: Act, pads, x2: Optional[Act] = None) -> bool:
        return L1_FOLD and L1_FOLD_DUAL and self._applies(x, pads, x2)

    def __call__(self, x: Act, x2: Act, pads=(0, 1, 1), relu=True, out: Optional[Act] = None, out_h: Optional[Act] = None):
        out, out_h, front, back = self._args(x, x2, 64, pads, relu, out, out_h)
        check(_lib.lib().tedspad_bneck_tail_fold2_fwd(*front, x2.ptr, x2.ld, self.tail.scale_d.data_ptr(), *back), "tedspad_bneck_tail_fold2_fwd")
        return out, out_h


class BneckFrame:
    """A whole plain bottleneck of I3Res50's layer3 -- conv1 (1x1x1 | 3x1x1) + bn1 + ReLU -> conv2 (1x3x3) + bn2 + ReLU -> conv3 (1x1x1) + bn3 + residual +
    ReLU (large_i3d.py:61-84, blocks without `downsample`) -- as ONE launch (csrc/conv_bneck_frame.hip): a workgroup owns a whole 14 x 14 frame, both
    256-channel tensors between the convolutions stay in LDS. The weights are packed here into the kernel's stream of 16 KB slot images
    (include/tedspad_hip.h, tedspad_bneck_frame_fwd)."""

    def __init__(self, w1: torch.Tensor, s1, b1, w2: torch.Tensor, s2, b2, w3: torch.Tensor, s3, b3, dtype: str = DEFAULT_DTYPE, device="cuda"):
        assert self.supported(w1, w2, w3)
        dev = torch.device(device)
        self.torch_dtype, self.dtype_code = DTYPES[dtype]
        self.cin, self.cmid = int(w1.shape[1]), int(w1.shape[0])
        f = lambda w: w.detach().to(dev, torch.float32)
        w1, w2, w3 = f(w1), f(w2), f(w3)
        self.temporal = w1.shape[2] == 3
        if self.temporal:       # folded two-frame form (TPairConv): frame 0 = W1 . x0 + W2 . x1, frame 1 = W0 . x0 + W1 . x1
            m1 = [torch.cat([w1[:, :, 1, 0, 0], w1[:, :, 2, 0, 0]], dim=1), torch.cat([w1[:, :, 0, 0, 0], w1[:, :, 1, 0, 0]], dim=1)]
        else:
            m1 = [w1[:, :, 0, 0, 0]]
        self.w1 = [self.slot_images(m).to(self.torch_dtype).contiguous() for m in m1]
        m2 = w2[:, :, 0].permute(0, 2, 3, 1).reshape(self.cmid, 9 * self.cmid)          # K = (dh*3 + dw) * cmid + ci
        pad = torch.zeros(2, 4, 4, 64, 8, device=dev)         # the kernel's ring keeps fetching two steps past the end
        self.w23 = torch.cat([self.slot_images(m2), self.slot_images(w3[:, :, 0, 0, 0], cols=True), pad]).to(self.torch_dtype).contiguous()
        self.steps1 = self.w1[0].shape[0]
        vec = lambda v: v.detach().to(dev, torch.float32).contiguous().clone()
        self.bn = [vec(v) for v in (s1, b1, s2, b2, s3, b3)]

    @staticmethod
    def slot_images(wm: torch.Tensor, cols: bool = False) -> torch.Tensor:
        """(rows, K) matrix -> (rows / 256 * K / 32, 4, 4, 64, 8): slot image of (row block rb, K step ks) at index rb * (K / 32) + ks;
        img[wc][j][lane][kk] = wm[256 rb + 64 wc + r(j, lane & 15)][32 ks + 8 (lane >> 4) + kk] with r(j, i) = 16 (i >> 2) + 4 j + (i & 3) (weights as the MFMA A
        operand: a lane ends with 16 consecutive channels of one pixel) or, cols=True, r(j, i) = 4 i + j (weights as the B operand, stage 3: a lane ends with 4
        consecutive channels of 4 pixels, consecutive lanes with consecutive channels)."""
        rows, K = wm.shape
        assert rows % 256 == 0 and K % 32 == 0
        dev = wm.device
        lane = torch.arange(64, device=dev)
        i, kg = lane & 15, lane >> 4
        j = torch.arange(4, device=dev).view(1, 4, 1)
        rin = (4 * i).view(1, 1, 64) + j if cols else 4 * j + (16 * (i >> 2) + (i & 3)).view(1, 1, 64)
        r = 64 * torch.arange(4, device=dev).view(4, 1, 1) + rin                          # (4,4,64)
        kk = 8 * kg.view(64, 1) + torch.arange(8, device=dev).view(1, 8)                  # (64,8)
        w4 = wm.reshape(rows // 256, 256, K // 32, 32).permute(0, 2, 1, 3)              # (rb, ks, 256, 32)
        g = w4[:, :, r]                                                                  # (rb, ks, 4, 4, 64, 32)
        img = torch.gather(g, 5, kk.view(1, 1, 1, 1, 64, 8).expand(g.shape[0], g.shape[1], 4, 4, 64, 8))
        return img.reshape(-1, 4, 4, 64, 8)

    @staticmethod
    def supported(w1, w2, w3) -> bool:
        return (tuple(w1.shape[:2]) == (256, 1024) and tuple(w1.shape[2:]) in ((1, 1, 1), (3, 1, 1)) and tuple(w2.shape) == (256, 256, 1, 3, 3) and
                tuple(w3.shape) == (1024, 256, 1, 1, 1))

    def applies(self, x: Act) -> bool:
        n, t, h, w = x.dims
        return (BNECK_FRAME and (h, w) == (14, 14) and x.c == self.cin and x.coff == 0 and x.ld == self.cin and (not self.temporal or t == 2) and x.buf.dtype == self.torch_dtype and
                n * t * h * w * x.ld < MAX_ELEMS)

    def __call__(self, x: Act, relu=True) -> Act:
        assert self.applies(x)
        n, t, h, w = x.dims
        out = Act.empty(n, t, h, w, self.cin, self.torch_dtype, x.buf.device)
        w1e, w1o = self.w1[0], self.w1[-1]
        check(_lib.lib().tedspad_bneck_frame_fwd(x.ptr, x.ld, out.ptr, out.ld, n, t, h, w, self.cin, self.cmid, w1e.data_ptr(), w1o.data_ptr(), self.steps1,
                                                 self.w23.data_ptr(), *[v.data_ptr() for v in self.bn], int(relu), self.dtype_code, _stream_ptr()),
              "tedspad_bneck_frame_fwd")
        return out


def maxpool(x: Act, k, s, pads=(0, 0, 0), pads_back=None, pad_zero=False, out: Optional[Act] = None, return_idx=False):
    n, t, h, w = x.dims
    pb = pads if pads_back is None else pads_back
    o = tuple(conv_out(sz, kk, ss, pf, pbk) for sz, kk, ss, pf, pbk in zip((t, h, w), k, s, pads, pb))
    if out is None:
        out = Act.empty(n, o[0], o[1], o[2], x.c, x.buf.dtype, x.buf.device)
    code = dtype_code(x.buf)
    d = PoolDesc(n=n, t=t, h=h, w=w, c=x.c, ldx=x.ld, ldy=out.ld, kt=k[0], kh=k[1], kw=k[2], st=s[0], sh=s[1], sw=s[2],
                 pt=pads[0], ph=pads[1], pw=pads[2], to=o[0], ho=o[1], wo=o[2], pad_zero=int(pad_zero), dtype=code)
    idx = torch.empty((n, o[0], o[1], o[2], x.c), dtype=torch.uint8, device=x.buf.device) if return_idx else None
    check(_lib.lib().tedspad_maxpool_fwd_idx(C.byref(d), x.ptr, out.ptr, idx.data_ptr() if return_idx else None, _stream_ptr()),
          "tedspad_maxpool_fwd")
    return (out, idx) if return_idx else out


def nl_attention(theta: Act, phi: Act, g: Act, scale: float, out: Optional[Act] = None, lse: Optional[torch.Tensor] = None) -> Act:
    """out[b, i, :] = sum_j softmax_j(scale * theta[b, i, :] . phi[b, j, :]) g[b, j, :] over the pixels of a batch item (large_i3d.py:112-119), one launch of
    tedspad_nl_attention_fwd: the score matrix is never written. theta (n, t, h, w, d) are the queries; phi and g (n, t, h', w', d) the keys and values, each
    an Act with its own row stride and channel offset (two slices of one buffer). d: 256 or 512 -- any other width is the library's error, never a torch path.
    lse: an fp32 (n, q) tensor that receives the log-sum-exp of the scaled logits (tedspad_nl_attention_fwd_lse, the tape of `nl_attention_bwd`); `out` is
    bit-identical with and without it."""
    n, t, h, w = theta.dims
    assert phi.dims == g.dims and phi.dims[0] == n and theta.c == phi.c == g.c, "nl_attention: theta %s x %d, phi %s x %d, g %s x %d" % (
        theta.dims, theta.c, phi.dims, phi.c, g.dims, g.c)
    assert theta.buf.dtype == phi.buf.dtype == g.buf.dtype
    if out is None:
        out = Act.empty(n, t, h, w, theta.c, theta.buf.dtype, theta.buf.device)
    assert out.dims == theta.dims and out.c == theta.c and out.buf.dtype == theta.buf.dtype
    q, k = t * h * w, phi.dims[1] * phi.dims[2] * phi.dims[3]
    code = dtype_code(theta.buf)
    assert lse is None or (lse.dtype == torch.float32 and lse.is_contiguous() and tuple(lse.shape) == (n, q))
    for n0, n1 in sample_chunks(n, [q * max(theta.ld, out.ld), k * max(phi.ld, g.ld)], MAX_ELEMS):
        ts, ps, gs, os_ = (a.samples(n0, n1) for a in (theta, phi, g, out))
        if lse is None:
            check(_lib.lib().tedspad_nl_attention_fwd(ts.ptr, ts.ld, ps.ptr, ps.ld, gs.ptr, gs.ld, os_.ptr, os_.ld, n1 - n0, q, k, theta.c, C.c_float(scale), code,
                                                      _stream_ptr()), "tedspad_nl_attention_fwd")
        else:                                               # row n0 of the contiguous (n, q) fp32 tensor
            check(_lib.lib().tedspad_nl_attention_fwd_lse(ts.ptr, ts.ld, ps.ptr, ps.ld, gs.ptr, gs.ld, os_.ptr, os_.ld, lse.data_ptr() + 4 * q * n0, n1 - n0, q, k,
                                                          theta.c, C.c_float(scale), code, _stream_ptr()), "tedspad_nl_attention_fwd_lse")
    return out


def nl_attention_lse(theta: Act, phi: Act, g: Act, scale: float):
    """`nl_attention` with its tape: (T, lse), lse (n, q) fp32."""
    n, t, h, w = theta.dims
    lse = torch.empty((n, t * h * w), dtype=torch.float32, device=theta.buf.device)
    return nl_attention(theta, phi, g, scale, lse=lse), lse


def nl_attention_bwd(theta: Act, phi: Act, g: Act, t: Act, lse: torch.Tensor, dt: Act, scale: float):
    """Backward of `nl_attention` (tedspad_nl_attention_bwd): (dtheta, dphi, dg) as Acts of the inputs' shapes from the forward's inputs, its output `t`, its
    `lse` and the upstream gradient `dt`. P is recomputed from lse; neither it nor dS is written. dt is expected SCALED (train_engine.GRAD_SCALE, a loss
    scale): the matrix cores flush f16 subnormal operands, and nothing is clamped -- an overflow comes back as inf / NaN."""
    n, tt, h, w = theta.dims
    d = theta.c
    assert phi.dims == g.dims and t.dims == theta.dims == dt.dims and phi.c == g.c == t.c == dt.c == d
    q, k = tt * h * w, phi.dims[1] * phi.dims[2] * phi.dims[3]
    assert lse.dtype == torch.float32 and lse.is_contiguous() and tuple(lse.shape) == (n, q)
    tdt, dev = theta.buf.dtype, theta.buf.device
    code = dtype_code(theta.buf)
    dtheta = Act.empty(n, tt, h, w, d, tdt, dev)
    dphi, dg = Act.empty(*phi.dims, d, tdt, dev), Act.empty(*phi.dims, d, tdt, dev)
    nbytes = C.c_int64(0)
    check(_lib.lib().tedspad_nl_attention_bwd_workspace(n, q, C.byref(nbytes)), "tedspad_nl_attention_bwd_workspace")
    ws = torch.empty(nbytes.value // 4, dtype=torch.float32, device=dev)
    acts = (theta, phi, g, t, dt, dtheta, dphi, dg)
    for n0, n1 in sample_chunks(n, [q * max(a.ld for a in (theta, t, dt, dtheta)), k * max(a.ld for a in (phi, g, dphi, dg))], MAX_ELEMS):
        s = [a.samples(n0, n1) for a in acts]
        check(_lib.lib().tedspad_nl_attention_bwd(s[0].ptr, s[0].ld, s[1].ptr, s[1].ld, s[2].ptr, s[2].ld, s[3].ptr, s[3].ld, s[4].ptr, s[4].ld,
                                                  lse.data_ptr() + 4 * q * n0, s[5].ptr, s[5].ld, s[6].ptr, s[6].ld, s[7].ptr, s[7].ld, ws.data_ptr(), n1 - n0, q, k, d,
                                                  C.c_float(scale), code, _stream_ptr()), "tedspad_nl_attention_bwd")
    return dtheta, dphi, dg


def global_avgpool(x: Act) -> torch.Tensor:
    """(n,t,h,w,c) -> fp32 (n, c): mean over all pixels."""
    n, t, h, w = x.dims
    y = torch.empty((n, x.c), dtype=torch.float32, device=x.buf.device)
    code = dtype_code(x.buf)
    check(_lib.lib().tedspad_global_avgpool_fwd(x.ptr, y.data_ptr(), n, t * h * w, x.c, x.ld, code, _stream_ptr()),
          "tedspad_global_avgpool_fwd")
    return y


def count_saturated(x: Act, counter: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Adds to `counter` (uint32-as-int32 x 2 on the device; made if None): elements of `x` at the largest finite f16 value -- what a clamped (saturated) inference
    store writes -- and non-finite elements (tedspad_count_saturated). No host sync: read it when convenient."""
    if counter is None:
        counter = torch.zeros(2, dtype=torch.int32, device=x.buf.device)
    n, t, h, w = x.dims
    code = dtype_code(x.buf)
    check(_lib.lib().tedspad_count_saturated(x.ptr, n * t * h * w, x.c, x.ld, code, counter.data_ptr(), _stream_ptr()), "tedspad_count_saturated")
    return counter


def avgpool3d_stride1(x: Act, k) -> torch.Tensor:
    """nn.AvgPool3d(k, stride 1): (n,t,h,w,c) -> fp32 (n, c, t-kt+1, h-kh+1, w-kw+1)."""
    n, t, h, w = x.dims
    y = torch.empty((n, x.c, t - k[0] + 1, h - k[1] + 1, w - k[2] + 1), dtype=torch.float32, device=x.buf.device)
    code = dtype_code(x.buf)
    check(_lib.lib().tedspad_avgpool3d_s1_fwd(x.ptr, y.data_ptr(), n, t, h, w, x.c, x.ld, k[0], k[1], k[2], code, _stream_ptr()),
          "tedspad_avgpool3d_s1_fwd")
    return y


def clip_to_act(x: torch.Tensor, cpad: int, dtype: str = DEFAULT_DTYPE) -> Act:
    """fp32 (n,c,t,h,w) (any strides) -> channels-last 16-bit Act. cpad=4 returns the
    pixel-pair view (n,t,h,w/2,8) the stems consume; cpad=8 returns (n,t,h,w,8)."""
    require_cuda(x, "clip_to_act")
    if x.dtype != torch.float32:
        x = x.float()
    n, c, t, h, w = x.shape
    tdt, code = DTYPES[dtype]
    wv = w // 2 if cpad == 4 else w
    buf = torch.empty((n, t, h, wv, 8), dtype=tdt, device=x.device)
    sn, sc, st, sh, sw = x.stride()
    check(_lib.lib().tedspad_clip_to_channels_last(x.data_ptr(), buf.data_ptr(), n, c, t, h, w, sn, sc, st, sh, sw,
                                                   cpad, code, _stream_ptr()), "tedspad_clip_to_channels_last")
    return Act(buf, 8, 0, cpad)


class StemPT:
    """conv1 5x7x7 / 2 / pad (2,3,3) + bn1 + ReLU of I3Res50 (large_i3d.py:133-137,229-231) on the persistent stem kernel
    (csrc/conv_stem_pt.hip), inference only, with the TEMPORAL half of maxpool1 (large_i3d.py:138,232) fused: the result is
    max(frame 2k, frame 2k+1) of the stem output, (n, To // 2, ho, wo, 64); `engine.maxpool(., (1,3,3), (1,2,2))` finishes the pool.
    K = 7*7*16 = 784 (temporal taps x channels folded into one 32-byte position), all weights resident in LDS."""
    VARIANT = int(os.environ.get("TEDSPAD_STEM_PT_VARIANT", "6"))      # bit 1: 8 waves per workgroup; bit 2 (pool-fused entry, 8 waves): 16x16x32 MFMAs
    # tap pairs of the 16x16x32 form, in the kernel's order (csrc/conv_stem_pt.hip, stem_pt_phase16): ((dh, dw), (dh, dw) | None)
    PAIRS = ([((2 * (i // 3), 1 + 2 * (i % 3)), (2 * (i // 3), 2 + 2 * (i % 3))) for i in range(12)] + [((0, 0), (2, 0)), ((4, 0), (6, 0))] +
             [((2 * (i // 3) + 1, 1 + 2 * (i % 3)), (2 * (i // 3) + 1, 2 + 2 * (i % 3))) for i in range(9)] + [((1, 0), (3, 0)), ((5, 0), None)])

    def __init__(self, weight: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, stride=(2, 2, 2), pads=(2, 3, 3),
                 dtype: str = DEFAULT_DTYPE, device="cuda"):
        co, ci, kt, kh, kw = weight.shape
        assert self.supported(weight, stride, pads), "StemPT: 64 x (<=3) x (<=5) x 7 x 7 weights, spatial stride 2 / pad 3, even temporal stride"
        device = torch.device(device)
        self.kt, self.stride_t, self.pad_t = kt, int(stride[0]), int(pads[0])
        self.torch_dtype, self.dtype_code = DTYPES[dtype]
        w = weight.detach().to(device=device, dtype=torch.float32)
        if ci < 3:
            w = torch.nn.functional.pad(w, (0, 0, 0, 0, 0, 0, 0, 3 - ci))
        w = w.permute(3, 4, 0, 2, 1).reshape(49, 64, kt * 3)                      # [tap = dh*7 + dw][co][dt*3 + ci]
        w = torch.nn.functional.pad(w, (0, 16 - kt * 3)).reshape(49, 64, 2, 8)
        swap = ((torch.arange(64, device=device) >> 4) & 1).bool().view(1, 64, 1, 1)
        self.wimg = torch.where(swap, w.flip(2), w).to(self.torch_dtype).contiguous()   # halves of a row swapped when (co >> 4) & 1
        assert self.wimg.numel() * 2 == _lib.lib().tedspad_stem_pt_wimg_bytes()
        # 16x16x32 form: [pair][co][chunk q = 2 * (tap of the pair) + half][8]; chunk q of row co is stored at chunk q ^ (2 * ((co >> 3) & 1))
        zero = torch.zeros(64, 2, 8, device=device)
        L = torch.stack([torch.cat([w[a[0] * 7 + a[1]], w[b[0] * 7 + b[1]] if b is not None else zero], dim=1) for a, b in self.PAIRS])   # (25, 64, 4, 8)
        src = torch.arange(4, device=device).view(1, 4) ^ (2 * ((torch.arange(64, device=device).view(64, 1) >> 3) & 1))                # physical chunk p <- logical p ^ ...
        self.wimg16 = torch.gather(L, 2, src.view(1, 64, 4, 1).expand(len(self.PAIRS), 64, 4, 8)).to(self.torch_dtype).contiguous()
        assert self.wimg16.numel() * 2 == _lib.lib().tedspad_stem_pt_wimg16_bytes()
        self.scale = _padded_vec(scale, co, 64, device, 1.0)
        self.shift = _padded_vec(shift, co, 64, device, 0.0)
        self.nwg = torch.cuda.get_device_properties(device).multi_processor_count if device.type == "cuda" else 256
        if STEM_NWG:
            self.nwg = min(self.nwg, STEM_NWG)

    @staticmethod
    def supported(weight: torch.Tensor, stride, pads) -> bool:
        co, ci, kt, kh, kw = weight.shape
        return (co == 64 and ci <= 3 and kt <= 5 and (kh, kw) == (7, 7) and tuple(stride[1:]) == (2, 2) and tuple(pads[1:]) == (3, 3) and
                stride[0] % 2 == 0)

    def frame_pairs(self, t: int) -> int:
        return conv_out(t, self.kt, self.stride_t, self.pad_t, self.pad_t) // 2

    def applies(self, x: torch.Tensor) -> bool:
        n, c, t, h, w = x.shape
        return (x.is_cuda and c <= 3 and x.stride(4) == 1 and w % 2 == 0 and self.stride_t == 2 and self.frame_pairs(t) >= 1 and
                h * w * 48 < (1 << 31))

    def layout(self, x: torch.Tensor) -> torch.Tensor:
        """fp32 (n, c, t, h, w) clip batch -> X[n][tp][h][b][w/2][24]: per output-frame pair one 48-byte record per pixel."""
        require_cuda(x, "StemPT")
        if x.dtype != torch.float32:
            x = x.float()
        n, c, t, h, w = x.shape
        tp = self.frame_pairs(t)
        xtp = torch.empty((n, tp, h, 2, w // 2, 24), dtype=self.torch_dtype, device=x.device)
        sn, sc, st, sh, sw = x.stride()
        check(_lib.lib().tedspad_clip_to_tp(x.data_ptr(), xtp.data_ptr(), n, c, t, h, w, sn, sc, st, sh, sw, self.pad_t, self.stride_t, tp,
                                            self.dtype_code, _stream_ptr()), "tedspad_clip_to_tp")
        return xtp

    def conv(self, xtp: torch.Tensor, relu=True, variant=None) -> Act:
        n, tp, h, _, wq, _ = xtp.shape
        w = 2 * wq
        ho, wo = (h + 1) // 2, wq
        out = Act.empty(n, tp, ho, wo, 64, self.torch_dtype, xtp.device)
        check(_lib.lib().tedspad_stem_pt_fwd(xtp.data_ptr(), self.wimg.data_ptr(), self.scale.data_ptr(), self.shift.data_ptr(), out.ptr, n, tp, h, w,
                                             ho, wo, out.ld, int(relu), self.nwg, (self.VARIANT if variant is None else variant) & ~4,
                                             self.dtype_code, _stream_ptr()), "tedspad_stem_pt_fwd")
        return out

    def conv_pool(self, xtp: torch.Tensor, variant=None) -> Act:
        """conv1 + bn1 + ReLU + MaxPool3d((2,3,3), 2) (large_i3d.py:229-232) in one pass over the frame-pair layout:
        Act (n, To // 2, (ho - 3) // 2 + 1, (wo - 3) // 2 + 1, 64)."""
        n, tp, h, _, wq, _ = xtp.shape
        w = 2 * wq
        ho, wo = (h + 1) // 2, wq
        assert ho >= 3 and wo >= 3, "StemPT.conv_pool: the stem output must hold one 3x3 window"
        hp, wp = (ho - 3) // 2 + 1, (wo - 3) // 2 + 1
        out = Act.empty(n, tp, hp, wp, 64, self.torch_dtype, xtp.device)
        side = torch.empty(_lib.lib().tedspad_stem_pt_side_bytes(n, tp, h, w), dtype=torch.uint8, device=xtp.device)
        v = self.VARIANT if variant is None else variant
        if v & 4:
            v |= 2                                          # the 16x16x32 form is the 8-wave kernel
        check(_lib.lib().tedspad_stem_pt_pool_fwd(xtp.data_ptr(), (self.wimg16 if v & 4 else self.wimg).data_ptr(), self.scale.data_ptr(), self.shift.data_ptr(),
                                                  out.ptr, side.data_ptr(), n, tp, h, w, hp, wp, out.ld, self.nwg, v, self.dtype_code, _stream_ptr()),
              "tedspad_stem_pt_pool_fwd")
        return out

    def direct_applies(self, x: torch.Tensor) -> bool:
        """The stem can read this fp32 clip batch itself (16-byte aligned rows)."""
        if not (self.applies(x) and x.dtype == torch.float32 and x.shape[4] % 4 == 0 and x.data_ptr() % 16 == 0):
            return False
        n, c, t, h, w = x.shape
        sn, sc, st, sh, _ = x.stride()
        return (all(s_ % 4 == 0 and s_ >= 0 for s_ in (sn, sc, st, sh)) and (c - 1) * sc + (t + 8) * st + (h + 32) * sh + w + 64 < (1 << 31) and
                (h + 1) // 2 >= 3 and w // 2 >= 3)

    PER_LANE_LOADER = 8      # conv_pool_clip variant bit 3: the loader waves deal their tasks per lane (the form before the wave-uniform deal; TEDSPAD_STEM_UNIFORM=0 sets it for every call)

    def conv_pool_clip(self, x: torch.Tensor, variant=0) -> Act:
        """conv1 + bn1 + ReLU + MaxPool3d((2,3,3), 2) (large_i3d.py:229-232) straight from the fp32 (n, c, t, h, w) clip batch: no layout pass.
        variant: StemPT.PER_LANE_LOADER selects the loader waves' per-lane task deal (same results, A/B); bits 8..10 are the kernel's timing ablations."""
        require_cuda(x, "StemPT")
        n, c, t, h, w = x.shape
        tp = self.frame_pairs(t)
        ho, wo = (h + 1) // 2, w // 2
        hp, wp = (ho - 3) // 2 + 1, (wo - 3) // 2 + 1
        out = Act.empty(n, tp, hp, wp, 64, self.torch_dtype, x.device)
        side = torch.empty(_lib.lib().tedspad_stem_pt_side_bytes(n, tp, h, w), dtype=torch.uint8, device=x.device)
        sn, sc, st, sh, sw = x.stride()
        check(_lib.lib().tedspad_stem_pt_pool_clip_fwd(x.data_ptr(), n, c, t, h, w, sn, sc, st, sh, sw, self.pad_t, self.stride_t, tp, self.wimg16.data_ptr(),
                                                       self.scale.data_ptr(), self.shift.data_ptr(), out.ptr, side.data_ptr(), hp, wp, out.ld, self.nwg,
                                                       variant, self.dtype_code, _stream_ptr()), "tedspad_stem_pt_pool_clip_fwd")
        return out

    def __call__(self, x: torch.Tensor, relu=True) -> Act:
        """x: fp32 (n, c, t, h, w) -> max over output-frame pairs of act(bn(conv(x))): Act (n, To // 2, ho, wo, 64)."""
        return self.conv(self.layout(x), relu)


def act_to_nchw(x: Act, c: Optional[int] = None) -> torch.Tensor:
    n, t, h, w = x.dims
    c = x.c if c is None else c
    y = torch.empty((n, c, t, h, w), dtype=torch.float32, device=x.buf.device)
    code = dtype_code(x.buf)
    check(_lib.lib().tedspad_channels_last_to_nchw(x.ptr, y.data_ptr(), n, c, t, h, w, x.ld, code, _stream_ptr()),
          "tedspad_channels_last_to_nchw")
    return y


def upsample2x_into(x: Act, out: Act, pad_top=0, pad_left=0):
    """Bilinear x2 (align_corners=True) of `x` (t == 1) into the channel slice `out`, zero-padded to out's size."""
    n, t, h, w = x.dims
    no, to, ho, wo = out.dims
    assert t == 1 and to == 1 and no == n and out.c == x.c
    code = dtype_code(x.buf)
    check(_lib.lib().tedspad_upsample_bilinear2x_fwd(x.ptr, out.ptr, n, h, w, x.c, x.ld, out.ld, ho, wo, pad_top, pad_left,
                                                     code, _stream_ptr()), "tedspad_upsample_bilinear2x_fwd")
    return out
