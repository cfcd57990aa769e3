"""-m gpu: I3Res50's dispatcher off the 16 x 112^2 / 16 x 224^2 clips -- per entry of tests/i3res50_geometry.GEOMETRIES the recorded launch sequence is
the one the predicates imply, and every stage map, on the fused and on the generic path, is as close to the fp32 oracle as an oracle that rounds where
the device stores 16-bit values.

The stage rule: rel-L2 over the whole map and the worst per-position rel-L2 over channels, each at most RATIO = 1.5 x the same distance of the
matched-rounding oracle (oracle/i3res50_ref.device_rounding) from the fp32 oracle, computed here from the oracle alone. The device rounds at a subset of
that oracle's rounding points (the fused forms keep intermediates in fp32 or in registers), so its distance is expected at or below the oracle's; 1.5
covers another realisation of the rounding noise on maps this small. The tuner is off in every test: no tuning job, fixed tile picks.

Worst ratios measured on an MI355X (whole map / worst position; the entry in brackets), over all entries that run the case:
    f16, fused path    layer1 0.975 / 1.014 (t7 / t12)   layer2 0.981 / 1.037 (t20 / wide)   layer3 1.002 / 1.070 (f14_t2 / t12)   layer4 0.983 / 1.017 (f14_t2)
                       feature 1.060 (f14_t2); the smallest ratio anywhere is 0.884
    f16, generic path  stem 1.000 / 1.001   maxpool1 1.001 / 1.000   layer1 1.006 / 1.037   layer2 1.016 / 1.085 (t7 / wide)   layer3 1.033 / 1.049
                       layer4 1.038 / 1.045
    bf16 (t8, wide)    layer1 0.976 / 0.998   layer2 0.980 / 0.929   layer3 0.983 / 1.001   layer4 0.982 / 1.032   feature 1.054
    use_nl (t8, t20, t7)   layer2 0.953 / 1.007   layer3 1.013 / 1.071 (t20 / t7)   feature 1.065 (t20)
    W stride 2 (t8, t7)    feature 0.943
f16 features against the fp32 oracle: 3.9e-4 (t32) .. 6.2e-4 (t8), use_nl 5.4e-4 .. 6.4e-4, against the gate of 1e-3.
"""
import copy
from collections import OrderedDict

import pytest
import torch
import torch.nn as nn

import i3res50_geometry as G

pytestmark = pytest.mark.gpu
TOL = 1e-3        # the feature gate (tests/test_hip_i3res50.py)
RATIO = 1.5


@pytest.fixture(autouse=True)
def tuner_off(monkeypatch):
    from ted_spad_amd import engine as E
    monkeypatch.setattr(E, "AUTOTUNE", False)


@pytest.fixture(scope="module")
def networks():
    """networks(dtype, use_nl, layers): I3Res50 on the seed-0 weights; layers < 4 the prefix network -- the same parameters, the layers behind `layers`
    replaced by an empty nn.Sequential() (_trunk and packed() loop over whatever blocks are there)."""
    from ted_spad_amd.i3res50 import I3Res50
    cache = {}

    def get(dtype="f16", use_nl=False, layers=4):
        key = (dtype, use_nl, layers)
        if key not in cache:
            if layers == 4:
                m = I3Res50(num_classes=102, use_nl=use_nl, dtype=dtype)
                m.load_state_dict(G.weights(use_nl)[1], strict=True)
                cache[key] = m.cuda().eval()
            else:
                m = copy.copy(get(dtype, use_nl, 4))
                m._modules = OrderedDict(m._modules)
                m._packed = m._packed_sig = None
                for li in range(layers + 1, 5):
                    setattr(m, "layer%d" % li, nn.Sequential())
                cache[key] = m
        return cache[key]
    yield get
    cache.clear()


@pytest.fixture(scope="module")
def clips():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = G.clip(G.GEOMETRIES[name]).cuda()
        return cache[name]
    yield get
    cache.clear()


def nchw(a):
    from ted_spad_amd import engine as E
    return E.act_to_nchw(a).cpu()


def check_rule(what, got, ref, matched):
    """Both distances of `got` from the fp32 oracle's `ref` against RATIO x the matched-rounding oracle's; every ratio is printed."""
    assert tuple(got.shape) == tuple(ref.shape), (what, tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), what
    ok = True
    for kind, dist in (("map", G.rel_l2), ("pos", G.worst_position)):
        d, m = dist(got, ref), dist(matched, ref)
        print("RATIO %-40s %s device %.3e matched %.3e ratio %.3f" % (what, kind, d, m, d / m))
        ok = ok and d <= RATIO * m
    assert ok, "%s: farther from the fp32 oracle than %.1f x the matched-rounding oracle" % (what, RATIO)


# ---- the fused path -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(G.GEOMETRIES))
def test_launch_sequence(name, networks, clips, monkeypatch):
    net = networks()
    rec = G.record_launches(monkeypatch)
    net.extract_features(clips(name))
    assert rec.labels(net) == G.expected_sequence(G.GEOMETRIES[name])


@pytest.mark.parametrize("layers", [1, 2, 3, 4])
@pytest.mark.parametrize("name", list(G.GEOMETRIES))
def test_stage_map(name, layers, networks, clips, monkeypatch):
    net = networks(layers=layers)
    rec = G.record_launches(monkeypatch)
    got = nchw(net._trunk(clips(name)))
    assert rec.labels(net) == G.expected_sequence(G.GEOMETRIES[name], layers=layers)[:-1]          # _trunk alone: no avgpool
    stage = "layer%d" % layers
    check_rule("%s %s" % (name, stage), got, G.stage_ref(G.oracle(name), stage), G.stage_ref(G.oracle(name, torch.float16), stage))


@pytest.mark.parametrize("name", list(G.GEOMETRIES))
def test_feature(name, networks, clips):
    f = networks().extract_features(clips(name)).cpu()
    ref, matched = G.oracle(name)["feature"], G.oracle(name, torch.float16)["feature"]
    assert f.dtype == torch.float32 and tuple(f.shape) == (G.GEOMETRIES[name][0], 2048, 1, 1, 1)
    per_clip = G.worst_position(f, ref)
    print("%s: feature rel-L2 vs the fp32 oracle, worst clip %.3e" % (name, per_clip))
    assert per_clip < TOL
    check_rule("%s feature" % name, f, ref, matched)


@pytest.mark.parametrize("name", list(G.GEOMETRIES))
def test_generic_path(name, networks, clips, monkeypatch):
    """_trunk(x, taps=...): the pixel-pair stem, both pools and three or four plain launches per block, every tap under the stage rule."""
    net = networks()
    rec = G.record_launches(monkeypatch)
    taps = {}
    net._trunk(clips(name), taps=taps)
    assert rec.labels(net) == G.expected_sequence(G.GEOMETRIES[name], input_form="taps")
    ref, matched = G.oracle(name), G.oracle(name, torch.float16)
    assert sorted(taps) == sorted(("stem",) + G.STAGES)
    for tap in ("stem",) + G.STAGES:
        check_rule("%s generic %s" % (name, tap), nchw(taps[tap]), ref[tap], matched[tap])


@pytest.mark.parametrize("name", G.BF16_ENTRIES)
def test_bf16(name, networks, clips, monkeypatch):
    """bf16 storage misses the 1e-3 gate by design (DESIGN.md "precision"): the sequence and the stage rule against the bf16 matched-rounding oracle only."""
    ref, matched = G.oracle(name), G.oracle(name, torch.bfloat16)
    rec = G.record_launches(monkeypatch)
    for layers in (1, 2, 3, 4):
        net = networks("bf16", layers=layers)
        rec.clear()
        got = nchw(net._trunk(clips(name)))
        assert rec.labels(net) == G.expected_sequence(G.GEOMETRIES[name], layers=layers)[:-1]
        stage = "layer%d" % layers
        check_rule("%s bf16 %s" % (name, stage), got, G.stage_ref(ref, stage), G.stage_ref(matched, stage))
    check_rule("%s bf16 feature" % name, networks("bf16").extract_features(clips(name)).cpu(), ref["feature"], matched["feature"])


# ---- input forms, batch ----------------------------------------------------------------------------------------------------------------------------------

def input_form(x, form):
    """The clip batch `x` (contiguous, on the device) handed over in another form that holds the same values."""
    n, c, t, h, w = x.shape
    if form == "tslice":                # T frames out of a longer clip whose other frames hold other values
        big = torch.full((n, c, t + 5, h, w), 0.75, device=x.device)
        big[:, :, 2:2 + t] = x
        y = big[:, :, 2:2 + t]
        assert not y.is_contiguous()
    elif form == "offset4":             # 4 bytes off a 16-byte boundary
        y = torch.empty(x.numel() + 1, device=x.device)[1:].view(x.shape)
        y.copy_(x)
        assert y.data_ptr() % 16 == 4 and y.is_contiguous()
    elif form == "wstride":             # W stride 2
        big = torch.full((n, c, t, h, 2 * w), 0.75, device=x.device)
        big[..., ::2] = x
        y = big[..., ::2]
        assert y.stride(4) == 2
    else:
        raise KeyError(form)
    assert torch.equal(y, x)
    return y


@pytest.mark.parametrize("form", ["tslice", "offset4", "records", "wstride"])
@pytest.mark.parametrize("name", G.FORM_ENTRIES)
def test_input_form(name, form, networks, clips, monkeypatch):
    net, x = networks(), clips(name)
    plain = net.extract_features(x)
    rec = G.record_launches(monkeypatch)
    if form == "records":
        records = net.packed()["stem_pt"].layout(x)
        rec.clear()
        f = net.extract_features_records(records)
    else:
        f = net.extract_features(input_form(x, form))
    want = G.expected_sequence(G.GEOMETRIES[name], input_form=form)
    assert rec.labels(net) == want
    print("%s %s: %s" % (name, form, [l for l in want if l.startswith("stem") or l == "maxpool1"]))
    if form == "wstride":               # the pixel-pair stem stores the conv1 output in 16 bits before the pool: other arithmetic, same tolerance
        assert G.worst_position(f.cpu(), G.oracle(name)["feature"]) < TOL
        check_rule("%s wstride feature" % name, f.cpu(), G.oracle(name)["feature"], G.oracle(name, torch.float16)["feature"])
    else:
        assert torch.equal(f, plain)


def test_clips_one_by_one_give_the_batch_bits(networks, clips):
    net, x = networks(), clips("t8")
    assert x.shape[0] == 2
    assert torch.equal(torch.cat([net.extract_features(x[i:i + 1]) for i in range(2)]), net.extract_features(x))


# ---- non-local -----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", G.NL_ENTRIES)
def test_nonlocal(name, networks, clips, monkeypatch):
    """use_nl=True on maps down to 3 x 3 frames (one key per frame) and 4 x 3 frames (pooled to 2 x 1)."""
    ref, matched = G.oracle(name, None, True), G.oracle(name, torch.float16, True)
    rec = G.record_launches(monkeypatch)
    for layers in (2, 3):
        net = networks(use_nl=True, layers=layers)
        rec.clear()
        got = nchw(net._trunk(clips(name)))
        assert rec.labels(net) == G.expected_sequence(G.GEOMETRIES[name], use_nl=True, layers=layers)[:-1]
        check_rule("%s nl layer%d" % (name, layers), got, ref["layer%d" % layers], matched["layer%d" % layers])
    net = networks(use_nl=True)
    rec.clear()
    f = net.extract_features(clips(name)).cpu()
    seq = G.expected_sequence(G.GEOMETRIES[name], use_nl=True)
    assert rec.labels(net) == seq and sum(l.endswith(":nl_attention") for l in seq) == 5
    print("%s: use_nl=True feature rel-L2 vs the fp32 oracle, worst clip %.3e" % (name, G.worst_position(f, ref["feature"])))
    assert G.worst_position(f, ref["feature"]) < TOL
    check_rule("%s nl feature" % name, f, ref["feature"], matched["feature"])


# ---- what the reference cannot take ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["clip", "records"])
@pytest.mark.parametrize("name", list(G.REFUSED))
def test_refused_before_any_launch(name, form, networks, monkeypatch):
    geometry, use_nl, what = G.REFUSED[name]
    net = networks(use_nl=use_nl)
    x = G.clip(geometry).cuda()
    if form == "records":
        x = net.packed()["stem_pt"].layout(x)
        if name == "conv1_two_rows":
            what = "5 x 6"              # the records form's own frame-size message
    rec = G.record_launches(monkeypatch)
    with pytest.raises(ValueError, match=what):
        net.extract_features_records(x) if form == "records" else net.extract_features(x)
    assert rec.events == []
