"""-m gpu: engine.BneckTailFold (csrc/conv_bneck_fold.hip) -- a plain layer1 block's fused tail that also emits the next block's conv1 (3x1x1) + bn1 + ReLU
on four-frame clips, a workgroup per 8 x 8 patch with one frame per wave.

1. Exact arithmetic on the integer grid of tests/kernel_refs.py: the bottleneck-tail chain extended by one stage (temporal conv -> bn -> ReLU -> one rounding);
   both outputs torch.equal to the float64 reference, dense and on channel slices of wider buffers.
2. Realistic magnitudes: y bit-equal to BneckTail's, h' against oracle/conv_ref.py with the bound test_hip_ops.py::test_conv_fused holds the temporal conv to.
3. Refusals: other frame counts, another conv1 shape, the two-source tail; the network then runs today's launches bit for bit. (Frames that are not whole
   patches are NOT refused: behind maxpool1 a 224 x 224 clip is 55 x 55, a 112 x 112 clip 27 x 27, so a fold of whole patches only would never run on the
   project's clips; partial patches are computed and tested exactly in 1.)
4. The network on 64 x 64 clips (layer1 is 15 x 15: 2 x 2 patches) with the switch on and off against oracle/i3res50_ref."""
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
             (2, 4, 15, 12),   # partial patches: 7 of 8 rows at the bottom edge, 4 of 8 columns at the right edge (layer1 is 55 x 55 at 224 x 224 clips), a clip boundary
             (1, 4, 3, 5)]     # a frame smaller than a patch
FOLD_W1 = (2, 0.1)             # the next conv1's integer weights: [-2, 2] at density 0.1 (768 products per output)
_REF = {}


@pytest.fixture(autouse=True)
def fold_switched_on(monkeypatch):
    """The tests run the fold whatever TEDSPAD_L1_FOLD's default is (the tests that compare both settings set it themselves)."""
    from ted_spad_amd import engine as E
    monkeypatch.setattr(E, "L1_FOLD", True)


def fold_case(dims):
    return R.BneckTailCase(dims, 64, R.TAIL_BIG)


def fold_reference(dims, dtype):
    """(tensors, [mid, y, h']) -- BneckTailCase's residual chain, then the next block's conv1 (64 <- 256, 3x1x1, pads (1,0,0)) + bn + ReLU + one rounding.
    Computed once per (dims, dtype); the conditions that make every summation order exact are asserted on it."""
    key = (tuple(dims), dtype)
    if key not in _REF:
        case = fold_case(dims)
        d = case.tensors()
        d["w1"] = R.small_ints(29, case.name + "w1n", (64, 256, 3, 1, 1), lo=-FOLD_W1[0], hi=FOLD_W1[0], density=FOLD_W1[1])
        d["s1"], d["b1"] = case.mix.bn(29, case.name + "bn1n", 64)
        mid, y = case.reference(d, dtype)["residual"]
        hn = R.chain_ref64(y["y"], [(d["w1"], R.ONE, PT, d["s1"], d["b1"], None, True)], dtype, step=y["step"])[0]
        stages = [mid, y, hn]
        R.fused_conditions(stages, dtype, "l1_fold " + case.name, case.mix)      # TAIL_BIG: both intermediates are really rounded, ties included, in f16 and bf16
        assert R.bn_is_telling(d["s1"], d["b1"]) and R.bn_is_telling(d["s2"], d["b2"]) and R.bn_is_telling(d["s3"], d["b3"])
        _REF[key] = (d, stages)
    return _REF[key]


def f32(*ts):
    return tuple(t.float() for t in ts)


def build_fold(d, dtype, w1=None):
    from ted_spad_amd import engine as E
    c2 = E.PackedConv(d["w2"].float(), *f32(d["s2"], d["b2"]), dtype=dtype, device="cuda")
    tail = E.BneckTail(c2, d["w3"].float(), *f32(d["s3"], d["b3"]))
    w1 = d["w1"].float() if w1 is None else w1
    c1 = E.PackedConv(w1, *f32(d["s1"], d["b1"]), dtype=dtype, device="cuda")
    return tail, c1, E.BneckTailFold(tail, c1, w1)


def wide_out(dims, c, coff, extra, dtype):
    from ted_spad_amd import engine as E
    buf = torch.full(tuple(dims) + (coff + c + extra,), SENTINEL, dtype=R.TDT[dtype], device="cuda")
    return E.Act(buf, c, coff)


def sentinel_intact(out, what, fails):
    keep = torch.ones(out.ld, dtype=torch.bool, device=out.buf.device)
    keep[out.coff:out.coff + out.c] = False
    rest = out.buf[..., keep]
    if not bool((rest == SENTINEL).all()):
        fails.append("%s: %d elements of the output buffer's other channels were overwritten" % (what, int((rest != SENTINEL).sum())))


# ---- 1. exact arithmetic ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sliced", [False, True], ids=["dense", "slices"])
@pytest.mark.parametrize("dims", FOLD_DIMS, ids=["%dx%dx%dx%d" % d for d in FOLD_DIMS])
def test_fold_equals_the_three_stage_chain(dims, sliced, dtype):
    """conv2 (576 products) -> 16 bits (registers) -> conv3 + residual (64) -> 16 bits (y, stored AND the fold's operand) -> temporal conv over the sibling
    waves' frames (768, 512 at the first and last frame) -> 16 bits. A neighbour frame read from the wrong wave, a tap multiplied on temporal padding, a
    weight column out of the accumulator k order, a halo pixel from across a frame border or a patch seam changes a bit of y or h'."""
    d, (mid, y, hn) = fold_reference(dims, dtype)
    tail, c1, fold = build_fold(d, dtype)
    xa = cl(d["x"], dtype, **(dict(ld=64 + 16, coff=8, seed=5) if sliced else {}))
    ra = cl(d["res"], dtype, **(dict(ld=256 + 24, coff=16, seed=6) if sliced else {}))
    assert fold.applies(xa, (0, 1, 1), ra)
    out = wide_out(dims, 256, 8, 16, dtype) if sliced else None
    out_h = wide_out(dims, 64, 16, 8, dtype) if sliced else None
    gy, gh = fold(xa, residual=ra, out=out, out_h=out_h)
    assert gy.dims == tuple(dims) and gh.dims == tuple(dims) and gy.c == 256 and gh.c == 64 and (gy.ld > 256) == sliced and (gh.ld > 64) == sliced
    tag = "l1_fold %s %s %s" % ("x".join(map(str, dims)), "slices" if sliced else "dense", dtype)
    fails = []
    R.same(nc(gy), y["y"], tag + " y", fails)
    R.same(nc(gh), hn["y"], tag + " h'", fails)
    if sliced:
        sentinel_intact(gy, tag + " y", fails)
        sentinel_intact(gh, tag + " h'", fails)
    assert not fails, "\n".join(fails)


# ---- 2. the launches it replaces ----------------------------------------------------------------------------------------------------------------------------
def _round(t, dt):
    return t.to(dt).float()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dims", [(2, 4, 16, 24), (1, 4, 56, 56), (2, 4, 55, 55)], ids=["2x4x16x24", "1x4x56x56", "2x4x55x55"])
def test_fold_vs_tail_and_temporal_conv(dims, dtype):
    """Inputs at the magnitudes of test_hip_ops.py. y: the same tap order, k order and MFMA shape as BneckTail -> bit-equal. h': the fold sums its 768 products
    group by group, the temporal-conv launch tap by tap -- fp32 summation order only; held against oracle.conv_ref.conv_cl on the stored y with
    test_conv_fused's bound for the temporal conv (one 16-bit step relative + 1e-3 per element; rel-L2 4e-4 in f16, 3e-3 in bf16)."""
    from oracle.conv_ref import conv_cl
    from ted_spad_amd import engine as E
    tdt = E.DTYPES[dtype][0]
    n, t, h, w = dims
    name = "fold%d" % h
    g = lambda nm, shape, lo, hi: synth_tensor(8, name + nm, shape, lo, hi)
    x = _round(g("x", (n, t, h, w, 64), -1, 1), tdt)
    res = _round(g("r", (n, t, h, w, 256), -1, 1), tdt)
    d = {"w2": _round(g("w2", (64, 64, 1, 3, 3), -1, 1) * (2.0 / 576) ** 0.5, tdt), "w3": _round(g("w3", (256, 64, 1, 1, 1), -1, 1) * (2.0 / 64) ** 0.5, tdt),
         "w1": _round(g("w1", (64, 256, 3, 1, 1), -1, 1) * (2.0 / 768) ** 0.5, tdt),
         "s2": g("s2", (64,), 0.5, 1.5), "b2": g("b2", (64,), -0.3, 0.3), "s3": g("s3", (256,), 0.5, 1.5), "b3": g("b3", (256,), -0.3, 0.3),
         "s1": g("s1", (64,), 0.5, 1.5), "b1": g("b1", (64,), -0.3, 0.3)}
    tail, c1, fold = build_fold(d, dtype)
    xa, ra = E.Act(x.to(tdt).cuda(), 64), E.Act(res.to(tdt).cuda(), 256)
    assert fold.applies(xa, (0, 1, 1), ra)
    gy, gh = fold(xa, residual=ra)
    want_y = tail(xa, residual=ra)
    torch.cuda.synchronize()
    assert torch.equal(gy.buf, want_y.buf), "y differs from BneckTail's in %d elements" % int((gy.buf != want_y.buf).sum())
    ref = conv_cl(gy.buf.float().cpu(), d["w1"], d["s1"], d["b1"], (1, 1, 1), (1, 0, 0), (1, 0, 0), None, relu=True)
    got = gh.buf.float().cpu()
    assert got.shape == ref.shape
    tol = 2.0 ** -10 if dtype == "f16" else 2.0 ** -7
    err = (got - ref).abs()
    print("l1_fold %s %s: h' max err %g (ref max %g), rel-L2 %.3e" % (dims, dtype, float(err.max()), float(ref.abs().max()), rel_l2(got, ref)))
    assert bool((err <= tol * ref.abs() + 1e-3).all()), "max err %g at ref %g" % (float(err.max()), float(ref.abs().max()))
    assert rel_l2(got, ref) < (4e-4 if dtype == "f16" else 3e-3)


# ---- 3. refusals --------------------------------------------------------------------------------------------------------------------------------------------
def test_fold_refuses_other_geometries(monkeypatch):
    from ted_spad_amd import engine as E
    d, _ = fold_reference(FOLD_DIMS[0], "f16")
    tail, c1, fold = build_fold(d, "f16")
    act = lambda n, t, h, w, c=64, dt=torch.float16: E.Act(torch.zeros((n, t, h, w, c), dtype=dt, device="cuda"), c)
    assert fold.applies(act(1, 4, 8, 16), (0, 1, 1))
    for t in (2, 3, 8):
        assert not fold.applies(act(1, t, 8, 8), (0, 1, 1))
    assert fold.applies(act(1, 4, 12, 8), (0, 1, 1)) and fold.applies(act(1, 4, 8, 12), (0, 1, 1))      # partial patches run (see the module docstring)
    assert not fold.applies(act(1, 4, 8, 8, dt=torch.bfloat16), (0, 1, 1))
    assert not fold.applies(act(1, 4, 8, 8), (0, 1, 1), act(1, 4, 8, 8, 256, torch.bfloat16))
    assert not fold.applies(act(1, 4, 8, 8), (0, 0, 1))
    for shape in ((64, 256, 1, 1, 1), (128, 256, 3, 1, 1), (64, 128, 3, 1, 1)):
        assert not E.BneckTailFold.supported(tail, torch.zeros(shape))
    dual = E.BneckTail(tail.conv2, d["w3"].float(), *f32(d["s3"], d["b3"]), d["wd"].float(), *f32(d["sd"], d["bd"]))
    assert not E.BneckTailFold.supported(dual, d["w1"].float())
    monkeypatch.setattr(E, "L1_FOLD", False)
    assert not fold.applies(act(1, 4, 8, 16), (0, 1, 1))
    # the C entry refuses what the host class would not send
    x, r = act(1, 3, 8, 8), act(1, 3, 8, 8, 256)
    y, hn = act(1, 3, 8, 8, 256), act(1, 3, 8, 8)
    c2 = tail.conv2
    desc = c2._desc(1, 3, 8, 8, 64, (0, 1, 1), (3, 8, 8), 64, 0, True)
    import ctypes as C
    from ted_spad_amd import _lib
    rc = _lib.lib().tedspad_bneck_tail_fold_fwd(C.byref(desc), x.ptr, c2.w.data_ptr(), c2.scale.data_ptr(), c2.shift.data_ptr(), tail.w3p.data_ptr(),
                                               tail.scale3.data_ptr(), tail.shift3.data_ptr(), r.ptr, 256, y.ptr, 256, 1, fold.w1p.data_ptr(),
                                               c1.scale.data_ptr(), c1.shift.data_ptr(), hn.ptr, 64, None)
    assert rc == -1 and b"t == 4" in _lib.lib().tedspad_last_error()
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def net():
    from ted_spad_amd.model_loaders import wrapper_i3d
    w = wrapper_i3d(num_classes=102)
    w.load_state_dict(synth_state_dict(w.state_dict(), 0), strict=True)
    return w.cuda().eval()


@pytest.mark.parametrize("shape", [(3, 8, 64, 64), (3, 12, 64, 64), (3, 32, 64, 64)], ids=["t2", "t3", "t8"])
def test_network_takes_todays_launches_where_the_fold_does_not_apply(net, shape, monkeypatch):
    """layer1 at 2, 3 and 8 frames: switch on and off are the same launches, so the same bits (tuner off: one tile choice)."""
    from ted_spad_amd import engine as E
    monkeypatch.setattr(E, "AUTOTUNE", False)
    x = synth_clips(0, 2, shape, device="cuda")
    monkeypatch.setattr(E, "L1_FOLD", True)
    on = net.i3d.extract_features(x)
    monkeypatch.setattr(E, "L1_FOLD", False)
    off = net.i3d.extract_features(x)
    assert torch.equal(on, off)


# ---- 4. the network -----------------------------------------------------------------------------------------------------------------------------------------
def test_network_with_the_fold_meets_the_feature_gate(net, monkeypatch):
    """Two 3 x 16 x 64 x 64 clips: layer1 is 4 frames of 15 x 15, 2 x 2 patches per frame, the second row and column 7 wide. Features with the switch on and off within the project's 1e-3
    rel-L2 of oracle/i3res50_ref each; their mutual rel-L2 is printed (summation order of layer1.2.conv1 only)."""
    from oracle import i3res50_ref
    from ted_spad_amd import engine as E
    monkeypatch.setattr(E, "AUTOTUNE", False)
    x = synth_clips(0, 2, (3, 16, 64, 64))
    sd = {k[4:]: v.cpu() for k, v in net.state_dict().items() if k.startswith("i3d.")}
    with torch.no_grad():
        ref = i3res50_ref.extract_features(x, sd).reshape(2, -1)
    calls = []
    real = E.BneckTailFold.__call__
    monkeypatch.setattr(E.BneckTailFold, "__call__", lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    monkeypatch.setattr(E, "L1_FOLD", True)
    on = net.i3d.extract_features(x.cuda()).cpu().reshape(2, -1)
    assert len(calls) == 1, "the fold did not run (layer1.1 -> layer1.2.conv1)"
    monkeypatch.setattr(E, "L1_FOLD", False)
    off = net.i3d.extract_features(x.cuda()).cpu().reshape(2, -1)
    assert len(calls) == 1
    r_on, r_off, r_mut = rel_l2(on, ref), rel_l2(off, ref), rel_l2(on, off)
    print("l1_fold network: rel-L2 vs oracle on %.3e, off %.3e; on vs off %.3e" % (r_on, r_off, r_mut))
    assert r_on < 1e-3 and r_off < 1e-3
