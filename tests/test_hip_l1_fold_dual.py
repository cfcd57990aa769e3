"""-m gpu: engine.BneckTailFoldDual (csrc/conv_bneck_fold_dual.hip) -- layer1.0's two-source tail (conv3 + bn3 + the downsample branch on x2) that also emits
layer1.1's conv1 (3x1x1) + bn1 + ReLU on four-frame clips; the tile and the fold of test_hip_l1_fold.py's kernel with the downsample branch in place of the residual.

1. Exact arithmetic on the integer grid of tests/kernel_refs.py: BneckTailCase's 'dual' chain extended by one stage (temporal conv -> bn -> ReLU -> one rounding);
   both outputs torch.equal to the float64 reference, dense and with h, x2, y and h' each a channel slice of its own wider buffer; the outputs sit between
   guard regions, so a store of a partial patch outside the frame shows.
2. Realistic magnitudes: y bit-equal to the two-source BneckTail's, h' against oracle/conv_ref.py with the bound test_hip_l1_fold.py holds the temporal conv to.
3. Refusals: other frame counts, pads, mixed dtypes, either switch off, a plain tail, other conv1 shapes; the C entry for t = 3 and a null x2.
4. The network on 64 x 64 clips (layer1 is 15 x 15) with the new switch on and off against oracle/i3res50_ref; at 2, 3 and 8 frames the same bits."""
import pytest
import torch

import kernel_refs as R
from conftest import rel_l2
from kernel_refs import cl, nc
from ted_spad_amd.synth import synth_clips, synth_state_dict, synth_tensor

pytestmark = pytest.mark.gpu
DTYPES = ("f16", "bf16")
SENTINEL = 12288.0             # exact in f16 and bf16
PT = ((1, 0, 0), (1, 0, 0))
FOLD_DIMS = [(1, 4, 8, 8),     # one patch: every pixel on a frame border, both temporal pads
             (2, 4, 16, 24),   # patch seams in both directions and a clip boundary
             (2, 4, 15, 12),   # partial patches: 7 of 8 rows at the bottom edge, 4 of 8 columns at the right edge, a clip boundary
             (1, 4, 3, 5)]     # a frame smaller than a patch
FOLD_W1 = (2, 0.1)             # the next conv1's integer weights: [-2, 2] at density 0.1 (768 products per output). The dual stage's grid is a quarter of the mid
#                                stage's (BneckTailCase.reference), so its values count four times as many steps as the residual chain's; the conditions below
#                                (every absolute-value sum below 2^24 steps, the stages alive) hold on the reference alone with these, checked without a GPU.
_REF = {}


@pytest.fixture(autouse=True)
def folds_switched_on(monkeypatch):
    """The tests run both folds whatever the switches' defaults are (the tests that compare settings set them themselves)."""
    from ted_spad_amd import engine as E
    monkeypatch.setattr(E, "L1_FOLD", True)
    monkeypatch.setattr(E, "L1_FOLD_DUAL", True)


def fold_reference(dims, dtype):
    """(tensors, [mid, y, h']) -- BneckTailCase's 'dual' chain, then the next block's conv1 (64 <- 256, 3x1x1, pads (1,0,0)) + bn + ReLU + one rounding.
    Computed once per (dims, dtype); the conditions that make every summation order exact are asserted on it."""
    key = (tuple(dims), dtype)
    if key not in _REF:
        case = R.BneckTailCase(dims, 64, R.TAIL_BIG)
        d = case.tensors()
        d["w1"] = R.small_ints(29, case.name + "w1n", (64, 256, 3, 1, 1), lo=-FOLD_W1[0], hi=FOLD_W1[0], density=FOLD_W1[1])
        d["s1"], d["b1"] = case.mix.bn(29, case.name + "bn1n", 64)
        mid, y = case.reference(d, dtype)["dual"]
        hn = R.chain_ref64(y["y"], [(d["w1"], R.ONE, PT, d["s1"], d["b1"], None, True)], dtype, step=y["step"])[0]
        stages = [mid, y, hn]
        R.fused_conditions(stages, dtype, "l1_fold_dual " + case.name, case.mix)
        assert R.bn_is_telling(d["s1"], d["b1"]) and R.bn_is_telling(d["s2"], d["b2"]) and R.bn_is_telling(d["s3"], d["b3"]) and R.bn_is_telling(d["sd"], d["bd"])
        _REF[key] = (d, stages)
    return _REF[key]


def f32(*ts):
    return tuple(t.float() for t in ts)


def build_fold(d, dtype, w1=None):
    from ted_spad_amd import engine as E
    c2 = E.PackedConv(d["w2"].float(), *f32(d["s2"], d["b2"]), dtype=dtype, device="cuda")
    tail = E.BneckTail(c2, d["w3"].float(), *f32(d["s3"], d["b3"]), d["wd"].float(), *f32(d["sd"], d["bd"]))
    w1 = d["w1"].float() if w1 is None else w1
    c1 = E.PackedConv(w1, *f32(d["s1"], d["b1"]), dtype=dtype, device="cuda")
    return tail, c1, E.BneckTailFoldDual(tail, c1, w1)


def guarded_out(dims, c, coff, extra, dtype):
    """An output Act inside a larger allocation: two pixel rows of sentinels before and behind it, and sentinels in the buffer's other channels."""
    from ted_spad_amd import engine as E
    n, t, h, w = dims
    ld = coff + c + extra
    guard, numel = 2 * w * ld, n * t * h * w * ld
    flat = torch.full((guard + numel + guard,), SENTINEL, dtype=R.TDT[dtype], device="cuda")
    return E.Act(flat[guard:guard + numel].view(n, t, h, w, ld), c, coff), flat, guard


def sentinels_intact(out, flat, guard, what, fails):
    keep = torch.ones(out.ld, dtype=torch.bool, device=out.buf.device)
    keep[out.coff:out.coff + out.c] = False
    rest = out.buf[..., keep]
    if not bool((rest == SENTINEL).all()):
        fails.append("%s: %d elements of the output buffer's other channels were overwritten" % (what, int((rest != SENTINEL).sum())))
    for name, g in (("before", flat[:guard]), ("behind", flat[flat.numel() - guard:])):
        if not bool((g == SENTINEL).all()):
            fails.append("%s: %d elements of the guard %s the output were overwritten" % (what, int((g != SENTINEL).sum()), name))


# ---- 1. exact arithmetic ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sliced", [False, True], ids=["dense", "slices"])
@pytest.mark.parametrize("dims", FOLD_DIMS, ids=["%dx%dx%dx%d" % d for d in FOLD_DIMS])
def test_dual_fold_equals_the_three_stage_chain(dims, sliced, dtype):
    """conv2 (576 products) -> 16 bits (registers) -> conv3 + the downsample conv on x2 (64 + 64, two BatchNorm scales) -> 16 bits (y, stored AND the fold's
    operand) -> temporal conv over the sibling waves' frames (768, 512 at the first and last frame) -> 16 bits. An x2 fragment of the wrong pixel or k step, a
    downsample weight column out of natural order, scale_d of another channel, x2 rows of a previous group's results left in the image change a bit of y."""
    d, (mid, y, hn) = fold_reference(dims, dtype)
    tail, c1, fold = build_fold(d, dtype)
    xa = cl(d["x"], dtype, **(dict(ld=64 + 16, coff=8, seed=5) if sliced else {}))
    x2a = cl(d["x2"], dtype, **(dict(ld=64 + 24, coff=16, seed=7) if sliced else {}))
    assert fold.applies(xa, (0, 1, 1), x2a)
    out, flat_y, gy_ = guarded_out(dims, 256, *((8, 16) if sliced else (0, 0)), dtype)
    out_h, flat_h, gh_ = guarded_out(dims, 64, *((16, 8) if sliced else (0, 0)), dtype)
    gy, gh = fold(xa, x2=x2a, out=out, out_h=out_h)
    assert gy.dims == tuple(dims) and gh.dims == tuple(dims) and gy.c == 256 and gh.c == 64 and (gy.ld > 256) == sliced and (gh.ld > 64) == sliced
    tag = "l1_fold_dual %s %s %s" % ("x".join(map(str, dims)), "slices" if sliced else "dense", dtype)
    fails = []
    R.same(nc(gy), y["y"], tag + " y", fails)
    R.same(nc(gh), hn["y"], tag + " h'", fails)
    sentinels_intact(gy, flat_y, gy_, tag + " y", fails)
    sentinels_intact(gh, flat_h, gh_, tag + " h'", fails)
    assert not fails, "\n".join(fails)


# ---- 2. the launches it replaces ----------------------------------------------------------------------------------------------------------------------------
def _round(t, dt):
    return t.to(dt).float()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dims", [(2, 4, 16, 24), (2, 4, 15, 12), (1, 4, 55, 55)], ids=["2x4x16x24", "2x4x15x12", "1x4x55x55"])
def test_dual_fold_vs_tail_and_temporal_conv(dims, dtype):
    """Inputs at the magnitudes of test_hip_ops.py. y: the same tap order, k order, MFMA shape and value expression as the two-source BneckTail -> bit-equal.
    h': the fold sums its 768 products group by group, the temporal-conv launch tap by tap -- fp32 summation order only; held against oracle.conv_ref.conv_cl on
    the stored y with the bound of test_hip_l1_fold.py (one 16-bit step relative + 1e-3 per element; rel-L2 4e-4 in f16, 3e-3 in bf16)."""
    from oracle.conv_ref import conv_cl
    from ted_spad_amd import engine as E
    tdt = E.DTYPES[dtype][0]
    n, t, h, w = dims
    name = "fold2_%d" % h
    g = lambda nm, shape, lo, hi: synth_tensor(8, name + nm, shape, lo, hi)
    x = _round(g("x", (n, t, h, w, 64), -1, 1), tdt)
    x2 = _round(g("x2", (n, t, h, w, 64), -1, 1), tdt)
    d = {"w2": _round(g("w2", (64, 64, 1, 3, 3), -1, 1) * (2.0 / 576) ** 0.5, tdt), "w3": _round(g("w3", (256, 64, 1, 1, 1), -1, 1) * (2.0 / 64) ** 0.5, tdt),
         "wd": _round(g("wd", (256, 64, 1, 1, 1), -1, 1) * (2.0 / 64) ** 0.5, tdt), "w1": _round(g("w1", (64, 256, 3, 1, 1), -1, 1) * (2.0 / 768) ** 0.5, tdt),
         "s2": g("s2", (64,), 0.5, 1.5), "b2": g("b2", (64,), -0.3, 0.3), "s3": g("s3", (256,), 0.5, 1.5), "b3": g("b3", (256,), -0.3, 0.3),
         "sd": g("sd", (256,), 0.5, 1.5), "bd": g("bd", (256,), -0.3, 0.3), "s1": g("s1", (64,), 0.5, 1.5), "b1": g("b1", (64,), -0.3, 0.3)}
    tail, c1, fold = build_fold(d, dtype)
    xa, x2a = E.Act(x.to(tdt).cuda(), 64), E.Act(x2.to(tdt).cuda(), 64)
    assert fold.applies(xa, (0, 1, 1), x2a)
    gy, gh = fold(xa, x2=x2a)
    want_y = tail(xa, x2=x2a)
    torch.cuda.synchronize()
    assert torch.equal(gy.buf, want_y.buf), "y differs from the two-source BneckTail's in %d elements" % int((gy.buf != want_y.buf).sum())
    ref = conv_cl(gy.buf.float().cpu(), d["w1"], d["s1"], d["b1"], (1, 1, 1), (1, 0, 0), (1, 0, 0), None, relu=True)
    got = gh.buf.float().cpu()
    assert got.shape == ref.shape
    tol = 2.0 ** -10 if dtype == "f16" else 2.0 ** -7
    err = (got - ref).abs()
    print("l1_fold_dual %s %s: h' max err %g (ref max %g), rel-L2 %.3e" % (dims, dtype, float(err.max()), float(ref.abs().max()), rel_l2(got, ref)))
    assert bool((err <= tol * ref.abs() + 1e-3).all()), "max err %g at ref %g" % (float(err.max()), float(ref.abs().max()))
    assert rel_l2(got, ref) < (4e-4 if dtype == "f16" else 3e-3)


# ---- 3. refusals --------------------------------------------------------------------------------------------------------------------------------------------
def test_dual_fold_refuses_other_geometries(monkeypatch):
    import ctypes as C
    from ted_spad_amd import _lib
    from ted_spad_amd import engine as E
    d, _ = fold_reference(FOLD_DIMS[0], "f16")
    tail, c1, fold = build_fold(d, "f16")
    act = lambda n, t, h, w, c=64, dt=torch.float16: E.Act(torch.zeros((n, t, h, w, c), dtype=dt, device="cuda"), c)
    assert fold.applies(act(1, 4, 8, 16), (0, 1, 1))
    for t in (2, 3, 8):
        assert not fold.applies(act(1, t, 8, 8), (0, 1, 1))
    assert fold.applies(act(1, 4, 12, 8), (0, 1, 1)) and fold.applies(act(1, 4, 8, 12), (0, 1, 1))      # partial patches run
    assert not fold.applies(act(1, 4, 8, 8, dt=torch.bfloat16), (0, 1, 1))
    assert not fold.applies(act(1, 4, 8, 8), (0, 1, 1), act(1, 4, 8, 8, 64, torch.bfloat16))
    assert not fold.applies(act(1, 4, 8, 8), (0, 0, 1)) and not fold.applies(act(1, 4, 8, 8), (1, 1, 1))
    for shape in ((64, 256, 1, 1, 1), (128, 256, 3, 1, 1), (64, 128, 3, 1, 1)):
        assert not E.BneckTailFoldDual.supported(tail, torch.zeros(shape))
    plain = E.BneckTail(tail.conv2, d["w3"].float(), *f32(d["s3"], d["b3"]))
    assert not E.BneckTailFoldDual.supported(plain, d["w1"].float()) and E.BneckTailFold.supported(plain, d["w1"].float())
    assert not E.BneckTailFold.supported(tail, d["w1"].float())
    for name in ("L1_FOLD", "L1_FOLD_DUAL"):
        monkeypatch.setattr(E, name, False)
        assert not fold.applies(act(1, 4, 8, 16), (0, 1, 1))
        monkeypatch.setattr(E, name, True)
    # the C entry refuses what the host class would not send
    c2 = tail.conv2
    entry = _lib.lib().tedspad_bneck_tail_fold2_fwd

    def call(t, x2_ptr):
        x, y, hn = act(1, t, 8, 8), act(1, t, 8, 8, 256), act(1, t, 8, 8)
        desc = c2._desc(1, t, 8, 8, 64, (0, 1, 1), (t, 8, 8), 64, 0, True)
        return entry(C.byref(desc), x.ptr, c2.w.data_ptr(), c2.scale.data_ptr(), c2.shift.data_ptr(), tail.w3p.data_ptr(), tail.scale3.data_ptr(),
                     tail.shift3.data_ptr(), x2_ptr, 64, tail.scale_d.data_ptr(), y.ptr, 256, 1, fold.w1p.data_ptr(), c1.scale.data_ptr(), c1.shift.data_ptr(),
                     hn.ptr, 64, None)

    x2 = act(1, 4, 8, 8)
    assert call(3, x2.ptr) == -1 and b"t == 4" in _lib.lib().tedspad_last_error()
    assert call(4, None) == -1 and b"null pointer" in _lib.lib().tedspad_last_error()
    torch.cuda.synchronize()


# ---- 4. the network -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net():
    from ted_spad_amd.model_loaders import wrapper_i3d
    w = wrapper_i3d(num_classes=102)
    w.load_state_dict(synth_state_dict(w.state_dict(), 0), strict=True)
    return w.cuda().eval()


@pytest.mark.parametrize("shape", [(3, 8, 64, 64), (3, 12, 64, 64), (3, 32, 64, 64)], ids=["t2", "t3", "t8"])
def test_network_takes_todays_launches_where_the_dual_fold_does_not_apply(net, shape, monkeypatch):
    """layer1 at 2, 3 and 8 frames: the new switch on and off are the same launches, so the same bits (tuner off: one tile choice)."""
    from ted_spad_amd import engine as E
    monkeypatch.setattr(E, "AUTOTUNE", False)
    x = synth_clips(0, 2, shape, device="cuda")
    monkeypatch.setattr(E, "L1_FOLD_DUAL", True)
    on = net.i3d.extract_features(x)
    monkeypatch.setattr(E, "L1_FOLD_DUAL", False)
    off = net.i3d.extract_features(x)
    assert torch.equal(on, off)


def test_network_with_the_dual_fold_meets_the_feature_gate(net, monkeypatch):
    """Two 3 x 16 x 64 x 64 clips: layer1 is 4 frames of 15 x 15. With the new switch on, BneckTailFoldDual runs once (layer1.0 -> layer1.1.conv1) and
    BneckTailFold once (layer1.1 -> layer1.2.conv1); off, only the latter. Features within the project's 1e-3 rel-L2 of oracle/i3res50_ref either way; their
    mutual rel-L2 is printed (summation order of layer1.1.conv1 only)."""
    from oracle import i3res50_ref
    from ted_spad_amd import engine as E
    monkeypatch.setattr(E, "AUTOTUNE", False)
    x = synth_clips(0, 2, (3, 16, 64, 64))
    sd = {k[4:]: v.cpu() for k, v in net.state_dict().items() if k.startswith("i3d.")}
    with torch.no_grad():
        ref = i3res50_ref.extract_features(x, sd).reshape(2, -1)
    calls = {"dual": 0, "plain": 0}
    real_d, real_p = E.BneckTailFoldDual.__call__, E.BneckTailFold.__call__
    monkeypatch.setattr(E.BneckTailFoldDual, "__call__", lambda self, *a, **k: (calls.__setitem__("dual", calls["dual"] + 1), real_d(self, *a, **k))[1])
    monkeypatch.setattr(E.BneckTailFold, "__call__", lambda self, *a, **k: (calls.__setitem__("plain", calls["plain"] + 1), real_p(self, *a, **k))[1])
    monkeypatch.setattr(E, "L1_FOLD_DUAL", True)
    on = net.i3d.extract_features(x.cuda()).cpu().reshape(2, -1)
    assert calls == {"dual": 1, "plain": 1}, calls
    monkeypatch.setattr(E, "L1_FOLD_DUAL", False)
    off = net.i3d.extract_features(x.cuda()).cpu().reshape(2, -1)
    assert calls == {"dual": 1, "plain": 2}, calls
    r_on, r_off, r_mut = rel_l2(on, ref), rel_l2(off, ref), rel_l2(on, off)
    print("l1_fold_dual network: rel-L2 vs oracle on %.3e, off %.3e; on vs off %.3e" % (r_on, r_off, r_mut))
    assert r_on < 1e-3 and r_off < 1e-3
