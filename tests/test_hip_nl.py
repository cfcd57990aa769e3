"""-m gpu: the non-local blocks of I3Res50 (use_nl=True) -- the fused attention kernel through the C ABI against the float64 restatement with a DERIVED
bound, the packed block against the reference's stored outputs, and the network against the non-local fixture.

The kernel bound. theta and phi are drawn from a coarse grid (multiples of 2^-4), so every product and every partial sum of a logit is exact in fp32
whatever the order: the kernel's logits are the reference's up to the one rounding of `* scale * log2(e)` (relative 2^-24). What is left is the rounding
of the probabilities to the storage type for the second product, at most u per p (u = 2^-11 for f16, 2^-8 for bf16: half an ulp, relative) and so at
most u * max_j |g[j, c]| in a weighted mean whose weights sum to one, and the rounding of the output, again u * |out| <= u * max_j |g[j, c]|; v_exp_f32
and the fp32 sums over at most 392 keys add a few 2^-22. Asserted: |err| <= 4 u max_j |g[j, c]| per element, twice the two terms."""
import ctypes as C
import functools
import json
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

import nl_ref
from conftest import GOLDEN_DIR, rel_l2
from ted_spad_amd.synth import synth_clips, synth_tensor

pytestmark = pytest.mark.gpu
TOL = 1e-3                     # the project's feature gate (tests/test_hip_i3res50.py)
U = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}
SENTINEL = 0x7A5A              # a finite 16-bit pattern in both types, written nowhere by the kernel
GUARD_ROWS = 8

# name: (n, t, h, w, d, phi and g as slices of one (n, k, 2d) buffer)
SHAPES = {
    "k1": (1, 1, 2, 2, 256, False),
    "k32": (1, 2, 8, 8, 256, False),
    "odd7": (2, 2, 7, 7, 512, True),
    "rect": (1, 1, 6, 10, 256, False),
    "layer3": (3, 2, 14, 14, 512, True),
    "layer2": (1, 2, 28, 28, 256, False),
}


def qk(shape):
    n, t, h, w, d, _ = shape
    return t * h * w, t * (h // 2) * (w // 2)


@functools.lru_cache(maxsize=None)
def case(name, variant, dtype):
    """(theta (n,q,d), phi (n,k,d), g (n,k,d)) as fp32 tensors holding values of the storage type, and the float64 reference (n,q,d)."""
    shape = SHAPES[name]
    n, t, h, w, d, _ = shape
    q, k = qk(shape)
    tdt = torch.float16 if dtype == "f16" else torch.bfloat16
    grid = lambda tag, rows: torch.floor(synth_tensor(7, "%s/%s/%s" % (name, variant, tag), (n, rows, d)) * 65.0 - 32.0) / 16.0     # multiples of 2^-4 in [-2, 2]
    theta, phi = grid("theta", q), grid("phi", k)
    g = synth_tensor(7, "%s/%s/g" % (name, variant), (n, k, d), -1.0, 1.0).to(tdt).float()
    scale = float(d) ** -0.5
    if variant == "equal":                       # all logits equal, g small integers: the mean over 32 keys is exactly representable
        theta.zero_()
        g = torch.floor(synth_tensor(7, name + "/gint", (n, k, d)) * 9.0 - 4.0) * 4.0
    elif variant == "spike":                     # one query's logit spike (4 d scale ~ 90) on the LAST key of the last partial tile
        sign = torch.where(synth_tensor(7, name + "/sign", (d,)) < 0.5, -2.0, 2.0)
        theta[:, q // 3] = sign
        phi[:, k - 1] = sign
    elif variant in ("plus200", "minus200"):     # 72 channels of 8 * (+-8): every logit moves by -+ 4608 scale = 203.6 (d = 512)
        theta[:, :, :72] = 8.0
        phi[:, :, :72] = 8.0 if variant == "plus200" else -8.0
    elif variant == "poison":                    # items other than `clean`: phi rows that score ~ +100 against the clean item's queries, g = +-1000
        clean = n // 2
        for b in range(n):
            if b == clean:
                theta[b, :, :144] = 2.0
                phi[b, :, :144] = 0.0
            else:
                phi[b, :, :144] = 8.0            # 2 * 8 * 144 scale = 101.8
                g[b] = torch.where(g[b] < 0, -1000.0, 1000.0)
    else:
        assert variant == "plain"
    return theta, phi, g, nl_ref.attention(theta, phi, g, scale)


def run_kernel(name, variant, dtype):
    """One call of tedspad_nl_attention_fwd on fresh buffers with guard records behind the output and a padded output row; returns (out (n,q,d) float64, ref, g)."""
    from ted_spad_amd import _lib
    from ted_spad_amd.engine import _stream_ptr
    shape = SHAPES[name]
    n, t, h, w, d, sliced = shape
    q, k = qk(shape)
    tdt, code = (torch.float16, _lib.F16) if dtype == "f16" else (torch.bfloat16, _lib.BF16)
    theta, phi, g, ref = case(name, variant, dtype)
    th = theta.to(tdt).cuda()
    if sliced:
        pg = torch.cat([phi, g], dim=2).to(tdt).cuda().contiguous()                # (n, k, 2d): phi at channel 0, g at channel d
        pp, gp, ldp, ldg = pg.data_ptr(), pg.data_ptr() + 2 * d, 2 * d, 2 * d
    else:
        ph, gg = phi.to(tdt).cuda(), g.to(tdt).cuda()
        pp, gp, ldp, ldg = ph.data_ptr(), gg.data_ptr(), d, d
    ldo = d + 8
    out = torch.full((n * q + GUARD_ROWS, ldo), SENTINEL, dtype=torch.int16, device="cuda")
    _lib.check(_lib.lib().tedspad_nl_attention_fwd(th.data_ptr(), d, pp, ldp, gp, ldg, out.data_ptr(), ldo, n, q, k, d, C.c_float(float(d) ** -0.5), code,
                                                   _stream_ptr()), "tedspad_nl_attention_fwd")
    torch.cuda.synchronize()
    host = out.cpu()
    assert bool((host[n * q:] == SENTINEL).all()), "guard rows behind the output were written"
    assert bool((host[:n * q, d:] == SENTINEL).all()), "the padding of an output row was written"
    got = host[:n * q, :d].contiguous().view(tdt).double().reshape(n, q, d)
    return got, ref, g


def fwd_bound(g, dtype):
    return 4.0 * U[dtype] * g.double().abs().amax(dim=1, keepdim=True)           # per batch item and channel


def check_bound(got, ref, g, dtype, what):
    bound = fwd_bound(g, dtype)
    err = (got - ref).abs()
    worst = float((err / bound.clamp_min(1e-30)).max())
    print("%s %s: max |err| / (4 u max|g|) = %.3f, max |err| = %.3e" % (what, dtype, worst, float(err.max())))
    assert torch.isfinite(got).all(), what
    assert bool((err <= bound).all()), "%s: |err| up to %.3f of the bound 4 u max|g|" % (what, worst)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("name", ["odd7", "rect", "layer3", "layer2"])
def test_kernel_within_the_derived_bound(name, dtype):
    got, ref, g = run_kernel(name, "plain", dtype)
    check_bound(got, ref, g, dtype, name)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_one_key_returns_g_bit_for_bit(dtype):
    got, ref, g = run_kernel("k1", "plain", dtype)
    assert torch.equal(got, g.double().expand(-1, got.shape[1], -1))
    assert torch.equal(got, ref)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_equal_logits_give_the_exact_mean(dtype):
    got, ref, g = run_kernel("k32", "equal", dtype)
    assert torch.equal(ref, g.double().mean(dim=1, keepdim=True).expand_as(ref))      # multiples of 1/8 up to 16: exact in both types
    assert torch.equal(got, ref)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("variant", ["spike", "plus200", "minus200", "poison"])
@pytest.mark.parametrize("name", ["odd7", "layer3"])
def test_hard_inputs(name, variant, dtype):
    got, ref, g = run_kernel(name, variant, dtype)
    if variant == "spike":                                  # the spiked query's row IS the last key's g row
        q = got.shape[1]
        assert float((ref[:, q // 3] - g[:, -1].double()).abs().max()) < 1e-12
    check_bound(got, ref, g, dtype, name + "/" + variant)


def test_other_widths_are_refused():
    from ted_spad_amd import _lib, engine as E
    for d in (128, 384, 1024):
        th = E.Act(torch.zeros((1, 1, 2, 2, d), dtype=torch.float16, device="cuda"), d)
        kv = E.Act(torch.zeros((1, 1, 1, 1, d), dtype=torch.float16, device="cuda"), d)
        with pytest.raises(_lib.TedSpadHipError, match="no kernel for d = %d" % d):
            E.nl_attention(th, kv, kv, 1.0)


# ---- the block through the packed launch sequence ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def nl_golden():
    return dict(np.load(os.path.join(GOLDEN_DIR, "nl_golden.npz")))


@pytest.fixture(scope="module")
def nl_meta():
    with open(os.path.join(GOLDEN_DIR, "nl_golden_meta.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("name", ["nl_block512", "nl_block1024"])
def test_block_launch_sequence_vs_reference(name, dtype, nl_golden, nl_meta):
    """theta, pool, phi | g, attention, out + bn + residual (i3res50.nonlocal_forward) on the two stored block cases, at the rel-L2 the per-op tests hold a
    chain of convolutions to (tests/test_hip_ops.py, the whole-bottleneck chain: 5e-4 f16, 4e-3 bf16)."""
    from ted_spad_amd import engine as E
    from ted_spad_amd.i3res50 import NonLocalBlock, nonlocal_forward, pack_nonlocal
    b = nl_meta["blocks"][name]
    p = name + ".nl."
    blk = NonLocalBlock(*b["dims"])
    tmpl = OrderedDict((p + k, v) for k, v in blk.state_dict().items())
    sd = nl_ref.nl_state_dict(tmpl, nl_meta["seed"], {p: b["gain"]})
    blk.load_state_dict(OrderedDict((k[len(p):], v) for k, v in sd.items()), strict=True)
    blk = blk.cuda().eval()
    x = synth_tensor(nl_meta["seed"], name + "/in", tuple(b["input"]), -1.0, 1.0)
    a = E.Act(x.permute(0, 2, 3, 4, 1).contiguous().to(E.DTYPES[dtype][0]).cuda(), x.shape[1])
    P = {}
    pack_nonlocal(P, "", blk, dtype, torch.device("cuda"))
    y = nonlocal_forward(P, "", blk, a)
    got = E.act_to_nchw(y).cpu()
    r = rel_l2(got, nl_golden[name + "_out"])
    print("%s %s: rel-L2 vs the reference block %.3e" % (name, dtype, r))
    assert r < (5e-4 if dtype == "f16" else 4e-3)
    assert torch.equal(nonlocal_forward(P, "", blk, a).buf, y.buf)


# ---- the network ------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def nets(nl_meta):
    """(the non-local wrapper, the default wrapper) on the fixture's weights; the default network's are the same tensors without the nl keys."""
    from ted_spad_amd.model_loaders import wrapper_i3d
    w = wrapper_i3d(num_classes=102, use_nl=True)
    sd = nl_ref.nl_state_dict(w.state_dict(), nl_meta["seed"], nl_meta["gains"])
    w.load_state_dict(sd, strict=True)
    plain = wrapper_i3d(num_classes=102)
    plain.load_state_dict(OrderedDict((k, v) for k, v in sd.items() if ".nl." not in k), strict=True)
    return w.cuda().eval(), plain.cuda().eval()


def test_feature_112_vs_fixture(nets, nl_golden):
    """The network gate: rel-L2 of the 16x112^2 feature against the fp32 reference <= 1e-3 in f16 (TOL of tests/test_hip_i3res50.py), on the fixture
    calibrated to a logit std of 2."""
    x = synth_clips(0, 1, (3, 16, 112, 112), device="cuda")
    f = nets[0].i3d.extract_features(x)
    assert f.shape == (1, 2048, 1, 1, 1) and f.dtype == torch.float32
    r = rel_l2(f.cpu().reshape(1, 2048), nl_golden["nl_feat_112"])
    print("use_nl=True feature 16x112^2 vs the fixture: rel-L2 %.3e" % r)
    assert r < TOL


def test_tap_checksums_vs_fixture(nets, nl_meta):
    x = synth_clips(0, 1, (3, 16, 112, 112), device="cuda")
    taps = {}
    nets[0].i3d._trunk(x, taps=taps)
    assert sorted(k for k in taps if k.endswith(".nl")) == sorted(nl_meta["taps_112"])
    for name, (mean, absmean) in nl_meta["taps_112"].items():
        t = taps[name].buf.double()
        print("%s: mean %.6f (ref %.6f), abs-mean %.6f (ref %.6f)" % (name, float(t.mean()), mean, float(t.abs().mean()), absmean))
        assert abs(float(t.abs().mean()) - absmean) < 2e-3 * absmean, name          # the bounds of test_stage_checksums_vs_golden
        assert abs(float(t.mean()) - mean) < 2e-3 * abs(mean) + 1e-4, name


def test_batch_invariance(nets, monkeypatch):
    """A clip's feature is bit-identical alone and in a batch of three (tuner off: only tiles that sum K in one order, as test_hip_i3res50 does)."""
    from ted_spad_amd import engine as E
    monkeypatch.setattr(E, "AUTOTUNE", False)
    x = synth_clips(0, 3, (3, 16, 112, 112), device="cuda")
    f3 = nets[0].i3d.extract_features(x)
    f1 = torch.cat([nets[0].i3d.extract_features(x[i:i + 1]) for i in range(3)])
    assert torch.equal(f3, f1)


def test_records_path_is_bit_identical(nets, monkeypatch):
    from ted_spad_amd import engine as E
    monkeypatch.setattr(E, "AUTOTUNE", False)
    i3d = nets[0].i3d
    x = synth_clips(0, 2, (3, 16, 112, 112), device="cuda")
    rec = i3d.packed()["stem_pt"].layout(x)
    assert torch.equal(i3d.extract_features_records(rec), i3d.extract_features(x))
    logits, feat = i3d(x)
    assert logits.shape == (2, 102) and torch.equal(feat, i3d.extract_features(x).squeeze())


def test_default_network_on_the_same_weights_is_the_existing_golden(nets, golden):
    x = synth_clips(0, 1, (3, 16, 112, 112), device="cuda")
    f = nets[1].i3d.extract_features(x)
    assert rel_l2(f.cpu().reshape(1, 2048), golden["i3res50_feat_112"]) < TOL


def test_factory_round_trip(nets, tmp_path, nl_golden):
    from ted_spad_amd.model_loaders import load_ft_model
    path = str(tmp_path / "nl.pth")
    torch.save({"ft_model_state_dict": OrderedDict((k, v.cpu()) for k, v in nets[0].state_dict().items())}, path)
    ft = load_ft_model("largei3d", saved_model_file=path, num_classes=102, use_nl=True).cuda().eval()
    x = synth_clips(0, 1, (3, 16, 112, 112), device="cuda")
    assert rel_l2(ft.i3d.extract_features(x).cpu().reshape(1, 2048), nl_golden["nl_feat_112"]) < TOL
    pred, emb = ft(synth_clips(0, 2, (3, 16, 112, 112), device="cuda"))
    assert pred.shape == (2, 102) and emb.shape == (2, 128)
