"""What I3Res50._trunk (ted_spad_amd/i3res50.py) must launch, and compute, on clip geometries other than 16 x 112^2 / 16 x 224^2 -- shared by
tests/test_i3res50_geometry_host.py (CPU) and tests/test_hip_i3res50_geometry.py (-m gpu). Importing this needs no GPU.

    GEOMETRIES, REACHES, RUNS     the table of clips, the launch labels each entry is in the table for, and the (entry, use_nl, input form) runs of the GPU file
    stage_dims(geometry)          (t, h, w) behind maxpool1 and behind each layer, from the conv / pool size rules
    expected_sequence(...)        the ordered launch labels, a plain restatement of _trunk's predicates with their constants as literals
    BRANCHES                      every launch form (labels without the block name); the host file demands that RUNS reaches each
    record_launches(monkeypatch)  pass-through recorders on the engine's entry points
    oracle(...)                   oracle/i3res50_ref.py's trunk in fp32 and with the device's rounding points, with tests/nl_ref's non-local block for use_nl
    rel_l2 / worst_position       the two distances of the stage rule

A label is "<block>:<form>" ("layer1.0:tail_dual+fold2", "stem:conv_pool_clip", "layer2.1:nl_attention") or a bare "maxpool1" / "maxpool2" / "avgpool".
"""
import functools
import inspect
import json
import os
from collections import OrderedDict

import torch
import torch.nn.functional as F

import nl_ref
from oracle import i3res50_ref as R

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# name -> (n, T, H, W)
GEOMETRIES = OrderedDict([
    ("t8", (2, 8, 64, 64)),          # layer1 t = 2: no folds, the pool fused in the last tail; t = 1 from layer2 on; two clips
    ("t12", (1, 12, 72, 56)),        # layer1 t = 3: the last block unfused + call_pool_t2 on an odd t
    ("t20", (1, 20, 66, 50)),        # layer1 t = 5 -> t = 2: TPairConv; W % 4 == 2
    ("t7", (1, 7, 40, 42)),          # the shortest clip the reference takes; layout stem; layer3 frames 3 x 3
    ("t15", (1, 15, 40, 40)),        # odd T with layer1 t = 4: fold2 in layer1.0, fold in layer1.1
    ("t32", (1, 32, 40, 40)),        # layer1 t = 8; t = 4 behind maxpool2
    ("wide", (1, 16, 48, 256)),      # layer1 frames 63 wide: the 64-channel tail refused
    ("wider", (1, 8, 40, 480)),      # layer2 frames 60 wide: the 128-channel tail refused
    ("f14_t1", (1, 8, 214, 214)),    # 14 x 14 frames at t = 1: BneckFrame only on the non-temporal blocks
    ("f14_t2", (1, 16, 216, 216)),   # the production sequence
])

# the labels each entry is in the table for (use_nl=False, the contiguous clip): the host file checks that expected_sequence holds them
REACHES = {
    "t8": ["stem:conv_pool_clip", "layer1.0:tail_dual", "layer1.1:conv1", "layer1.1:tail", "layer1.2:tail+pool_t2", "layer2.0:conv1", "layer3.2:conv1"],
    "t12": ["layer1.0:tail_dual", "layer1.2:conv2", "layer1.2:conv3+pool_t2", "layer2.0:conv1"],
    "t20": ["stem:layout", "stem:conv_pool", "layer1.2:conv3+pool_t2", "layer2.0:conv1_tpair", "layer3.2:conv1_tpair", "layer4.1:conv1_tpair"],
    "t7": ["stem:layout", "stem:conv_pool", "layer1.2:tail+pool_t2", "layer4.2:conv3"],
    "t15": ["layer1.0:tail_dual+fold2", "layer1.1:tail+fold", "layer1.2:tail+pool_t2", "layer2.0:conv1_tpair"],
    "t32": ["layer1.0:tail_dual", "layer1.1:tail", "layer1.2:tail+pool_t2", "layer2.0:conv1", "layer2.1:tail", "layer3.2:conv1"],
    "wide": ["layer1.0:conv3+dual", "layer1.1:conv3", "layer1.2:conv3+pool_t2", "layer2.1:tail"],
    "wider": ["layer1.0:conv3+dual", "layer1.2:conv3+pool_t2", "layer2.0:dual_p8", "layer2.1:conv2", "layer2.1:conv3"],
    "f14_t1": ["layer3.1:frame", "layer3.2:conv1", "layer3.2:conv3", "layer3.3:frame", "layer3.4:conv2", "layer3.5:frame"],
    "f14_t2": ["stem:conv_pool_clip", "layer1.0:tail_dual+fold2", "layer1.1:tail+fold", "layer1.2:tail+pool_t2", "layer2.0:conv1_tpair", "layer2.3:tail",
               "layer3.1:frame", "layer3.2:frame", "layer3.5:frame", "layer4.1:conv1_tpair"],
}

# input forms of expected_sequence: "clip" a contiguous fp32 clip batch (the stem form follows from W % 4); "tslice" T frames out of a longer clip;
# "offset4" a clip 4 bytes off a 16-byte boundary; "records" StemPT.layout's records through extract_features_records; "wstride" a W stride of 2;
# "taps" _trunk(x, taps=...), the generic sequence
INPUT_FORMS = ("clip", "tslice", "offset4", "records", "wstride", "taps")

NL_ENTRIES = ("t8", "t20", "t7")
BF16_ENTRIES = ("t8", "wide")
FORM_ENTRIES = ("t8", "t7")

# every (entry, use_nl, input form) the GPU file runs and asserts the sequence of
RUNS = ([(g, False, "clip") for g in GEOMETRIES] + [(g, False, "taps") for g in GEOMETRIES] + [(g, True, "clip") for g in NL_ENTRIES] +
        [(g, False, f) for g in FORM_ENTRIES for f in ("tslice", "offset4", "records", "wstride")])

# clips the reference cannot process (name -> ((n, T, H, W), use_nl, what the ValueError names))
REFUSED = OrderedDict([
    ("six_frames", ((1, 6, 40, 40), False, "at least 7 frames")),         # one frame behind maxpool1: MaxPool3d((2,1,1)) raises (large_i3d.py:139)
    ("four_frames", ((1, 4, 64, 64), False, "at least 7 frames")),
    ("conv1_two_rows", ((1, 8, 4, 40), False, "at least 5 x 5")),         # conv1 output 2 x 20: MaxPool3d((2,3,3)) raises (large_i3d.py:138)
    ("nl_layer3_1x1", ((1, 8, 16, 16), True, "at least 2 x 2")),          # layer2 frames 2 x 2, layer3 frames 1 x 1: the block's (1,2,2) pool raises (large_i3d.py:95)
])

BRANCHES = frozenset([
    "conv_pool_clip", "layout", "conv_pool", "pair", "maxpool1", "maxpool2",
    "conv1", "conv1_tpair", "conv2", "conv3", "down", "conv3+dual", "dual_p8", "conv3+pool_t2",
    "tail", "tail_dual", "tail+pool_t2", "tail+fold", "tail_dual+fold2", "frame",
    "nl_theta", "nl_pool", "nl_phi_g", "nl_attention", "nl_out", "avgpool",
])

STAGES = ("maxpool1", "layer1", "layer2", "layer3", "layer4")


def form(label: str) -> str:
    return label.split(":", 1)[-1]


# ---- sizes ---------------------------------------------------------------------------------------------------------------------------------------

def _out(size, k, s, p):
    """nn.Conv3d / nn.MaxPool3d output size of one dim (floor mode)."""
    return (size + 2 * p - k) // s + 1


def stage_dims(geometry):
    """{"maxpool1" | "layer1".."layer4": (t, h, w)} of an (n, T, H, W) clip batch (large_i3d.py:133-145,229-238)."""
    n, t, h, w = geometry
    t, h, w = _out(t, 5, 2, 2), _out(h, 7, 2, 3), _out(w, 7, 2, 3)          # conv1 5x7x7 / 2, pad (2,3,3)
    t, h, w = _out(t, 2, 2, 0), _out(h, 3, 2, 0), _out(w, 3, 2, 0)          # maxpool1 (2,3,3) / 2
    d = OrderedDict(maxpool1=(t, h, w))
    d["layer1"] = (t, h, w)
    t = _out(t, 2, 2, 0)                                                    # maxpool2 (2,1,1) / (2,1,1)
    for name in ("layer2", "layer3", "layer4"):
        h, w = _out(h, 3, 2, 1), _out(w, 3, 2, 1)                           # block 0's conv2 1x3x3 / 2, pad 1
        d[name] = (t, h, w)
    return d


# ---- the launch sequence ----------------------------------------------------------------------------------------------------------------------------

LAYERS = ((64, 3, 1, (1, 1, 1)), (128, 4, 2, (1, 0, 1, 0)), (256, 6, 2, (1, 0, 1, 0, 1, 0)), (512, 3, 2, (0, 1, 0)))      # i3res50.LAYER_PLAN
NL_AT = {2: (1, 3), 3: (1, 3, 5)}                                                                                         # I3Res50.__init__: nonlocal_mod = 2 on layer2 / layer3


def expected_sequence(geometry, use_nl=False, input_form="clip", layers=4):
    """The launch labels of extract_features (of _trunk alone for "taps") on an (n, T, H, W) clip batch, in order. `layers`: a prefix network whose layers
    behind `layers` are empty. Restates I3Res50._stem / _trunk / _bottleneck and the `applies` / `supported` predicates of engine.py with the default switches."""
    assert input_form in INPUT_FORMS
    n, T, H, W = geometry
    generic = input_form == "taps"
    seq = []
    # the stem (I3Res50._stem)
    if input_form == "records":
        seq += ["stem:conv_pool"]                                           # _stem: the records form
    elif input_form in ("wstride", "taps"):
        seq += ["stem:pair", "maxpool1"]                                    # StemPT.applies: x.stride(4) == 1 fails / _stem: taps is None fails
    elif W % 4 == 0 and input_form != "offset4":                            # StemPT.direct_applies: W % 4 == 0 and a 16-byte aligned base
        seq += ["stem:conv_pool_clip"]
    else:
        seq += ["stem:layout", "stem:conv_pool"]
    t, h, w = stage_dims(geometry)["maxpool1"]
    pooled, h_next = False, False
    for li in range(1, layers + 1):
        planes, blocks, stride, tc = LAYERS[li - 1]
        if li == 2:
            if not pooled:
                seq += ["maxpool2"]                                         # _trunk: maxpool2 unless fused
            t = t // 2
        for i in range(blocks):
            b = "layer%d.%d" % (li, i)
            nl = ["%s:%s" % (b, f) for f in ("nl_theta", "nl_pool", "nl_phi_g", "nl_attention", "nl_out")] if use_nl and i in NL_AT.get(li, ()) else []
            s = stride if i == 0 else 1
            last_l1 = li == 1 and i == blocks - 1                           # _trunk: last_l1
            # BneckFrame.supported: 1024 -> 256 -> 1024 without downsample = layer3.1..5; BneckFrame.applies: (h, w) == (14, 14), a temporal block t == 2
            if not generic and li == 3 and i > 0 and (h, w) == (14, 14) and (not tc[i] or t == 2):
                seq += [b + ":frame"] + nl
                continue
            if h_next:
                h_next = False                                              # _bottleneck: h_next taken
            # I3Res50._pack_block: conv1_tp behind maxpool2 only; TPairConv.supported: cout % 128 == 0; TPairConv.applies: cout >= TPAIR_MIN_COUT = 128 and t == 2
            elif not generic and li >= 2 and tc[i] and planes % 128 == 0 and planes >= 128 and t == 2:
                seq += [b + ":conv1_tpair"]
            else:
                seq += [b + ":conv1"]
            # I3Res50._pack_block: a tail in layer1 / layer2 on stride-1 conv2 (BneckTail.supported): layer1.0 the two-source form, layer2.0 none
            has_tail = not generic and li in (1, 2) and s == 1
            # BneckTail.applies: flat_halo <= 80 KB: (256 + 2 w + 11) * 128 + 33280 (64 channels) or + 32768 (128) <= 81920, i.e. w <= 56 or w <= 58
            fits = w <= (56 if planes == 64 else 58)
            dual = li == 1 and i == 0
            if has_tail and fits and (not last_l1 or t % 2 == 0):           # _bottleneck: `h.dims[1] % 2 == 0` (the last block's tail is never dual)
                if dual and t == 4:                                         # BneckTailFoldDual.applies
                    seq += [b + ":tail_dual+fold2"]
                    h_next = True
                elif dual:
                    seq += [b + ":tail_dual"]
                elif li == 1 and not last_l1 and t == 4:                    # BneckTailFold.applies (I3Res50.packed: layer1's plain blocks but the last)
                    seq += [b + ":tail+fold"]
                    h_next = True
                elif last_l1:
                    seq += [b + ":tail+pool_t2"]
                    pooled = True
                else:
                    seq += [b + ":tail"]
                seq += nl
                continue
            seq += [b + ":conv2"]
            h, w = _out(h, 3, s, 1), _out(w, 3, s, 1)
            if not generic and i == 0 and li == 1:                          # PackedConv.dual_supported: both 1x1x1 stride 1 with cin == 64
                seq += [b + ":conv3+dual"] + nl
                continue
            if not generic and i == 0 and s == 2:                           # I3Res50._pack_block `dual` + PackedConv.dual_p8_supported: layer2.0 / 3.0 / 4.0 at any size here
                seq += [b + ":dual_p8"] + nl
                continue
            if i == 0:
                seq += [b + ":down"]                                        # _bottleneck: the downsample branch on its own
            if not generic and last_l1 and t >= 2:                          # PackedConv.pool_t2_supported: cin 64 and t >= 2, odd t included
                seq += [b + ":conv3+pool_t2"]
                pooled = True
            else:
                seq += [b + ":conv3"]
            seq += nl
    if layers < 2 and not pooled:
        seq += ["maxpool2"]                                                 # an empty layer2 is still entered (_trunk's layer loop)
    if not generic:
        seq += ["avgpool"]
    return seq


# ---- recording -------------------------------------------------------------------------------------------------------------------------------------

class LaunchRecorder:
    """The outermost calls of the engine's entry points since the last clear(), as (kind, object, detail)."""

    def __init__(self):
        self.events, self.depth = [], 0

    def clear(self):
        self.events = []

    def labels(self, net):
        """The recorded calls as labels, the blocks named after the keys of `net.packed()`."""
        names = {id(v): k for k, v in net.packed().items()}
        out, block = [], None
        for kind, obj, detail in self.events:
            key = names.get(id(obj)) if obj is not None else None
            if kind in ("maxpool", "nl_attention", "avgpool"):
                if kind == "maxpool":
                    fixed = {(2, 3, 3): "maxpool1", (1, 3, 3): "maxpool1:spatial", (2, 1, 1): "maxpool2"}.get(detail)
                    out.append(fixed if fixed is not None else "%s:nl_pool" % block if detail == (1, 2, 2) else "maxpool%s" % (detail,))
                else:
                    out.append("avgpool" if kind == "avgpool" else "%s:nl_attention" % block)
                continue
            assert key is not None, "a %s launch on an object that is not in packed()" % kind
            if key in ("stem", "stem_pt"):
                out.append("stem:" + ("pair" if key == "stem" else kind))
                continue
            if ".nl." in key:
                block, part = key.split(".nl.")
                out.append("%s:nl_%s" % (block, part))
                continue
            block, part = key.rsplit(".", 1)
            if kind == "conv":
                f = part
            elif kind == "tail":
                f = "tail_dual" if detail[0] else "tail+pool_t2" if detail[1] else "tail"
            else:
                f = {"call_dual": "conv3+dual", "call_dual_p8": "dual_p8", "call_pool_t2": "conv3+pool_t2", "tpair": "conv1_tpair", "fold": "tail+fold",
                     "fold2": "tail_dual+fold2", "frame": "frame"}[kind]
            out.append("%s:%s" % (block, f))
        return out


def record_launches(monkeypatch) -> LaunchRecorder:
    """Wraps the engine's entry points with pass-through recorders (undone with `monkeypatch`): arguments and results go through untouched, only calls
    made while no other recorded call is running are kept."""
    from ted_spad_amd import engine as E
    rec = LaunchRecorder()

    def wrap(owner, name, kind, detail=None, method=True):
        orig = getattr(owner, name)
        sig = inspect.signature(orig)

        @functools.wraps(orig)
        def recorder(*args, **kwargs):
            if rec.depth == 0:
                rec.events.append((kind, args[0] if method else None, detail(sig.bind(*args, **kwargs).arguments) if detail else None))
            rec.depth += 1
            try:
                return orig(*args, **kwargs)
            finally:
                rec.depth -= 1
        monkeypatch.setattr(owner, name, recorder)

    wrap(E.StemPT, "__call__", "pt")
    wrap(E.StemPT, "layout", "layout")
    wrap(E.StemPT, "conv_pool", "conv_pool")
    wrap(E.StemPT, "conv_pool_clip", "conv_pool_clip")
    wrap(E.PackedConv, "__call__", "conv")
    wrap(E.PackedConv, "call_dual", "call_dual")
    wrap(E.PackedConv, "call_dual_p8", "call_dual_p8")
    wrap(E.PackedConv, "call_pool_t2", "call_pool_t2")
    wrap(E.TPairConv, "__call__", "tpair")
    wrap(E.BneckTail, "__call__", "tail", lambda a: (a.get("x2") is not None, bool(a.get("pool_t2", False))))
    wrap(E.BneckTailFold, "__call__", "fold")
    wrap(E.BneckTailFoldDual, "__call__", "fold2")
    wrap(E.BneckFrame, "__call__", "frame")
    wrap(E, "maxpool", "maxpool", lambda a: tuple(a["k"]), method=False)
    wrap(E, "nl_attention", "nl_attention", method=False)
    wrap(E, "global_avgpool", "avgpool", method=False)
    return rec


# ---- weights, clips, oracles ------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def weights(use_nl=False):
    """(the wrapper's state dict, the same under the reference I3Res50's key names) with the seed-0 synthetic weights -- for use_nl the non-local fixture's
    calibration on top (tests/nl_ref.nl_state_dict with the stored gains, as tests/test_hip_nl.py takes them)."""
    from ted_spad_amd.model_loaders import wrapper_i3d
    from ted_spad_amd.synth import synth_state_dict
    tmpl = wrapper_i3d(num_classes=102, use_nl=use_nl).state_dict()
    if use_nl:
        with open(os.path.join(GOLDEN_DIR, "nl_golden_meta.json")) as f:
            meta = json.load(f)
        assert meta["seed"] == 0
        sd = nl_ref.nl_state_dict(tmpl, meta["seed"], meta["gains"])
    else:
        sd = synth_state_dict(tmpl, 0)
    return sd, OrderedDict((k[4:], v) for k, v in sd.items() if k.startswith("i3d."))


def clip(geometry):
    """The fp32 (n, 3, T, H, W) clip batch of a table entry, on the host."""
    from ted_spad_amd.synth import synth_clips
    n, t, h, w = geometry
    return synth_clips(0, n, (3, t, h, w))


def nl_block(x, sd, p, q=R._id):
    """NonLocalBlock.forward (large_i3d.py:102-125) in eval mode: tests/nl_ref.block's float64 arithmetic with the reference's own MaxPool3d, and the
    rounding hook `q` where the launch sequence stores 16-bit values -- the weights, theta, phi, g, the attention output, the block output."""
    x64 = x.double()
    rq = lambda t: q(t.float(), "act").double()
    wq = lambda k: q(sd[p + k], "w")
    rows = lambda t: t.flatten(2).transpose(1, 2)
    mp = F.max_pool3d(x64, (1, 2, 2), (1, 2, 2))                            # :95,106
    th = rq(rows(nl_ref._pw(x64, wq("theta.weight"), sd[p + "theta.bias"])))
    ph = rq(rows(nl_ref._pw(mp, wq("phi.weight"), sd[p + "phi.bias"])))
    g = rq(rows(nl_ref._pw(mp, wq("g.weight"), sd[p + "g.bias"])))
    d = th.shape[2]
    t = rq(nl_ref.attention(th, ph, g, float(d) ** -0.5))                   # :112-118
    t = t.transpose(1, 2).reshape(x.shape[0], d, *x.shape[2:])              # :119
    o = nl_ref._pw(t, wq("out.weight"), sd[p + "out.bias"])                 # :121
    v = lambda k: sd[p + k].double().view(1, -1, 1, 1, 1)
    o = (o - v("bn.running_mean")) / torch.sqrt(v("bn.running_var") + R.BN_EPS) * v("bn.weight") + v("bn.bias")     # :122
    return q((o + x64).float(), "res")                                      # :124


def oracle_trunk(x, sd, q=R._id, taps=None, use_nl=False):
    """oracle/i3res50_ref.trunk; for use_nl the same walk with `nl_block` behind layer2.{1,3} and layer3.{1,3,5} (large_i3d.py:57-58,81-82)."""
    if not use_nl:
        return R.trunk(x, sd, q=q, taps=taps)
    x = F.conv3d(q(x, "act"), q(sd["conv1.weight"], "w"), stride=(2, 2, 2), padding=(2, 3, 3))
    x = q(F.relu(R._bn_eval(x, sd, "bn1.")), "act")
    taps["stem"] = x
    x = F.max_pool3d(x, kernel_size=(2, 3, 3), stride=(2, 2, 2))
    taps["maxpool1"] = x
    for name, planes, blocks, stride, tc in R.LAYER_PLAN:
        if name == "layer2":
            x = F.max_pool3d(x, kernel_size=(2, 1, 1), stride=(2, 1, 1))
        for i in range(blocks):
            p = "%s.%d." % (name, i)
            x = R.bottleneck(x, sd, p, stride if i == 0 else 1, tc[i], i == 0, q=q)
            if p[:-1] in nl_ref.NL_BLOCKS:
                x = nl_block(x, sd, p + "nl.", q)
        taps[name] = x
    return x


def oracle_on(x, dtype=None, use_nl=False):
    """{"stem", "maxpool1", "layer1".."layer4", "feature"} of the oracle on the host clip batch `x`: exact fp32 (dtype None), or rounding the weights and
    every stored activation once to `dtype` (oracle/i3res50_ref.device_rounding)."""
    q = R._id if dtype is None else R.device_rounding(dtype)[0]
    taps = {}
    with torch.no_grad():
        y = oracle_trunk(x, weights(use_nl)[1], q=q, taps=taps, use_nl=use_nl)
    taps["feature"] = y.mean(dim=(2, 3, 4), keepdim=True)
    return taps


@functools.lru_cache(maxsize=None)
def oracle(name, dtype=None, use_nl=False):
    """`oracle_on` of a table entry, computed once per process; nobody writes to the result."""
    return oracle_on(clip(GEOMETRIES[name]), dtype, use_nl)


def stage_ref(taps, stage):
    """The oracle's map to set against a `layers`-prefix network's _trunk output: the tap, for maxpool1 / layer1 behind maxpool2 (which _trunk runs, or fuses,
    before it enters layer2 -- an empty one too)."""
    t = taps[stage]
    return F.max_pool3d(t, (2, 1, 1), (2, 1, 1)) if stage in ("maxpool1", "layer1") else t


# ---- distances -------------------------------------------------------------------------------------------------------------------------------------

def rel_l2(a, ref):
    a, ref = a.double(), ref.double()
    return float((a - ref).norm() / ref.norm().clamp_min(1e-30))


def worst_position(a, ref):
    """The largest rel-L2 over the channels of one (n, t, h, w) position of an (n, c, t, h, w) map."""
    a, ref = a.double(), ref.double()
    return float(((a - ref).norm(dim=1) / ref.norm(dim=1).clamp_min(1e-30)).max())
