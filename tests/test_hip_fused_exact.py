"""-m gpu: the fused forward kernels of the inference path -- engine.BneckFrame (csrc/conv_bneck_frame.hip), engine.BneckTail with 64 and 128 mid channels
(csrc/conv_bneck.hip), tedspad_unetpp_tail_fwd (csrc/conv_upp_tail.hip), engine.StemPT (csrc/conv_stem_pt.hip), engine.TPairConv, PackedConv.call_dual,
call_dual_p8 and call_pool_t2 -- against the float64 chain references of tests/kernel_refs.py on INTEGER inputs, in f16 and bf16.

Integer activations and weights, power-of-two BatchNorm scales and integer shifts keep every value of every stage on a dyadic grid and every fp32 partial sum
exact in any order; the one rounding of each 16-bit intermediate is round-to-nearest-even of an exactly known number, which the reference reproduces
(kernel_refs.round_once), and a rounded grid value is still on the grid. So a whole fused kernel must equal its reference BIT FOR BIT: every comparison here
is torch.equal. The conditions that make this true (kernel_refs.fused_conditions: sums below 2^24 steps, stored values below 65504, every stage alive; plus,
per kernel with an intermediate and per type, cases whose intermediates are really rounded, ties included: Mix.rounds) are asserted on the reference before anything from
the GPU is compared, and over every case table on the CPU in test_kernel_refs.py. The tolerance tests of test_hip_ops.py keep covering realistic magnitudes."""
import types

import pytest
import torch

import kernel_refs as R
from test_hip_conv_exact import cl, nc

pytestmark = pytest.mark.gpu
D = torch.float64
DTYPES = ("f16", "bf16")
SENTINEL = 12288.0             # exact in f16 and bf16


def where(got, want):
    """For R.same: the first differing element of (n, c, t, h, w) tensors named as sample / frame / pixel / channel, and the output channels that differ."""
    bad = (got != want) & ~(torch.isnan(got) & torch.isnan(want))
    n, c, t, h, w = (int(i) for i in bad.nonzero()[0])
    chans = bad.any(0).flatten(1).any(1).nonzero().flatten().tolist()
    return " -- sample %d frame %d pixel (%d, %d) channel %d; %d output channels differ: %s%s" % (
        n, t, h, w, c, len(chans), chans[:16], " ..." if len(chans) > 16 else "")


def same(got, want, what, fails):
    return R.same(got, want, what, fails, detail=where)


def telling(d, *pairs):
    """Condition 5 on a test's own tensors: power-of-two scales that differ between neighbours, non-zero integer shifts."""
    for s, b in pairs:
        assert R.bn_is_telling(None if s is None else d[s], d[b])


def f32(*ts):
    return tuple(t.float() for t in ts)


def wide_out(dims, c, extra, dtype):
    """An output Act of c channels at offset 0 of a buffer `extra` channels wider, all of it the sentinel."""
    from ted_spad_amd import engine as E
    buf = torch.full(tuple(dims) + (c + extra,), SENTINEL, dtype=R.TDT[dtype], device="cuda")
    return E.Act(buf, c, 0)


def sentinel_intact(out, what, fails):
    rest = out.buf[..., out.c:]
    if not bool((rest == SENTINEL).all()):
        fails.append("%s: %d elements of the output buffer's other channels were overwritten" % (what, int((rest != SENTINEL).sum())))


# ---- 1. the whole bottleneck per frame ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", R.BNECK_FRAME_CASES, ids=[c.name for c in R.BNECK_FRAME_CASES])
def test_bneck_frame_equals_the_three_stage_chain(case, dtype):
    """engine.BneckFrame, plain blocks at (n, t) = (1, 3) and (3, 2), temporal blocks at (2, 2) and (1, 2), 14 x 14 x 1024: conv1 (1024 or 2048 products per
    output) -> 16 bits -> conv2 (2304) -> 16 bits -> conv3 (256) + the input as residual -> 16 bits. One dropped or misplaced product, a wrong pixel at a frame
    corner, a stale ring slot on the last K step or an intermediate kept in fp32 changes a bit."""
    from ted_spad_amd import engine as E
    x, ws, bn = case.tensors()
    assert all(R.bn_is_telling(s, b) for s, b in bn)
    ref = R.chain_ref64(x, case.stages(x, ws, bn), dtype)
    R.fused_conditions(ref, dtype, "bneck_frame " + case.name, case.mix)
    bf = E.BneckFrame(ws[0].float(), *f32(*bn[0]), ws[1].float(), *f32(*bn[1]), ws[2].float(), *f32(*bn[2]), dtype=dtype, device="cuda")
    xa = cl(x, dtype)
    assert bf.applies(xa) and bf.temporal == case.temporal
    fails = []
    same(nc(bf(xa)), ref[2]["y"], "bneck_frame %s %s" % (case.name, dtype), fails)
    assert not fails, "\n".join(fails)


# ---- 2, 3. the bottleneck tail ------------------------------------------------------------------------------------------------------------------------------
def run_bneck_tail(case, dtype):
    from ted_spad_amd import engine as E
    d = case.tensors()
    telling(d, ("s2", "b2"), ("s3", "b3"), *((("sd", "bd"),) if case.cmid == 64 else ()))
    refs = case.reference(d, dtype)
    for form, st in refs.items():
        R.fused_conditions(st, dtype, "bneck_tail %s %s" % (case.name, form), case.mix)
    c, co = case.cmid, case.cout3
    c2 = E.PackedConv(d["w2"].float(), *f32(d["s2"], d["b2"]), dtype=dtype, device="cuda")
    plain = E.BneckTail(c2, d["w3"].float(), *f32(d["s3"], d["b3"]))
    dual = E.BneckTail(c2, d["w3"].float(), *f32(d["s3"], d["b3"]), d["wd"].float(), *f32(d["sd"], d["bd"])) if "dual" in case.forms else None
    assert plain.cmid == c and plain.cout3 == co
    n, t, h, w = case.dims
    fails = []
    for form in case.forms:
        for sliced in (False, True):
            tag = "bneck_tail %s %s %s %s" % (case.name, form, "slices" if sliced else "dense", dtype)
            xa = cl(d["x"], dtype, **(dict(ld=c + 16, coff=8, seed=5) if sliced else {}))
            assert plain.applies(xa, (0, 1, 1))
            odims = (n, t // 2 if form == "pool" else t, h, w)
            out = wide_out(odims, co, 16, dtype) if sliced else None
            if form == "dual":
                x2a = cl(d["x2"], dtype, **(dict(ld=64 + 24, coff=16, seed=7) if sliced else {}))
                got = dual(xa, x2=x2a, out=out)
            else:
                ra = cl(d["res"], dtype, **(dict(ld=co + 24, coff=16, seed=6) if sliced else {}))
                got = plain(xa, residual=ra, pool_t2=form == "pool", out=out)
            assert got.dims == odims and (got.ld > co) == sliced and (xa.ld > c) == sliced
            same(nc(got), refs[form][1]["y"], tag, fails)
            if sliced:
                sentinel_intact(got, tag, fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", R.BNECK_TAIL64_CASES, ids=[c.name for c in R.BNECK_TAIL64_CASES])
def test_bneck_tail_64_equals_the_two_stage_chain(case, dtype):
    """engine.BneckTail, 64 mid channels: conv2 1x3x3 -> 16 bits (in registers) -> conv3 + residual | + the downsample branch on x2 | + residual and the
    temporal pair max (even t). Tiles crossing rows, frames and clips, a ragged last tile, frames smaller than a tile, one wide frame. Every form runs on dense
    buffers and with x, residual / x2 as channel slices of wider buffers whose other channels hold non-zero integers (ldx, ldr, ld2 > channels) and `out` a
    wider buffer (ldy > cout3) whose other channels hold a sentinel that must survive."""
    run_bneck_tail(case, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", R.BNECK_TAIL128_CASES, ids=[c.name for c in R.BNECK_TAIL128_CASES])
def test_bneck_tail_128_equals_the_two_stage_chain(case, dtype):
    """engine.BneckTail, 128 mid channels (conv_bneck_tail128_kernel: chunk-major stage A, conv3 weights streamed): the plain block, dense and on slices."""
    run_bneck_tail(case, dtype)


# ---- 4. the unet++ tail -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", R.UPP_TAIL_CASES, ids=[c.name for c in R.UPP_TAIL_CASES])
def test_unetpp_tail_equals_the_three_stage_chain(case, dtype):
    """tedspad_unetpp_tail_fwd through the C ABI, the weight image packed by the production packer UnetPlusPlus._pack_tail on a stand-in that has the three
    attributes it reads. Output sizes: one 16 x 16 patch; ragged patches on both axes; 3 x 48 x 80; 2 x 2; and 6 x 138 x 170 = 594 patches, more than twice the
    device's compute units, so that workgroups walk two and three patches: the head runs one patch behind inside the loop and the third patch lands in an X buffer
    the first one used (asserted on the device's count). ldx = 64 and a 64-channel
    slice of an 80-channel buffer. The output is fp32 and exact; one sample's worth of sentinel floats behind y must survive."""
    from ted_spad_amd import _lib, engine as E
    from ted_spad_amd.unetpp import UnetPlusPlus
    d = case.tensors()
    telling(d, ("s1", "b1"), ("s2", "b2"), (None, "bias"))
    ref = case.reference(d, dtype)
    R.fused_conditions(ref, dtype, "unetpp_tail " + case.name, case.mix)
    n, h, w = case.n, case.h, case.w
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    print("unetpp_tail %s: %d patches on %d compute units" % (case.name, case.npatch, ncu))
    if case.walk:
        assert case.npatch > 2 * ncu, "the walk case no longer has more than twice as many patches as compute units: %d <= 2 * %d" % (case.npatch, ncu)
    ns = types.SimpleNamespace
    conv = lambda wt: [ns(weight=wt[:, :, 0].float())]
    stand_in = ns(decoder=ns(blocks={"x_0_3": ns(conv1=conv(d["w1"]), conv2=conv(d["w2"]))}), segmentation_head=conv(d["w3"]), compute_dtype=dtype)
    wimg = UnetPlusPlus._pack_tail(stand_in, torch.device("cuda"))
    vec = {k: d[k].float().cuda().contiguous() for k in ("s1", "b1", "s2", "b2")}
    bias = torch.zeros(4, device="cuda")
    bias[:3] = d["bias"].float().cuda()
    want = ref[2]["y"][:, :, 0]                                            # (n, 3, h, w)
    fails = []
    for sliced in (False, True):
        tag = "unetpp_tail %s %s %s" % (case.name, "slice of 80" if sliced else "ldx 64", dtype)
        xa = cl(d["x"], dtype, **(dict(ld=80, coff=8, seed=5) if sliced else {}))
        assert xa.ld == (80 if sliced else 64)
        ybuf = torch.full(((n + 1) * 3 * h * w,), SENTINEL, dtype=torch.float32, device="cuda")
        _lib.check(_lib.lib().tedspad_unetpp_tail_fwd(xa.ptr, xa.ld, ybuf.data_ptr(), n, h, w, wimg.data_ptr(), vec["s1"].data_ptr(), vec["b1"].data_ptr(),
                                                      vec["s2"].data_ptr(), vec["b2"].data_ptr(), bias.data_ptr(), E.DTYPES[dtype][1], E._stream_ptr()),
                   "tedspad_unetpp_tail_fwd")
        host = ybuf.cpu()
        if not bool((host[n * 3 * h * w:] == SENTINEL).all()):
            fails.append(tag + ": the sentinel floats behind y were overwritten")
        got = host[:n * 3 * h * w].view(n, 3, h, w).double()
        same(got.unsqueeze(2), want.unsqueeze(2), tag, fails)
    assert not fails, "\n".join(fails)


# ---- 5. the persistent stem ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", R.STEM_CASES, ids=["x".join(map(str, c)) for c in R.STEM_CASES])
def test_stem_pt_equals_conv_pair_max_and_pool(case, dtype):
    """engine.StemPT on integer clips (an odd frame count; two channels): `conv` under variants 0 and 2 against the reference conv + the max over frame pairs;
    `conv_pool` under variants 2 and 6 and `conv_pool_clip` (w % 4 == 0) against that followed by the (1, 3, 3) / (1, 2, 2) max pool -- not against the same
    kernel's unpooled output; the clips are zero on part of the frame, so that the pooled output too is a quarter zeros and a lost ReLU shows; `conv_pool_clip` also on a non-contiguous T-slice of a longer clip whose other frames hold non-zero integers."""
    from ted_spad_amd import engine as E
    d, (conv, pair, pool) = R.stem_reference(case, dtype)
    telling(d, ("s", "b"))
    R.fused_conditions([conv, pair, pool], dtype, "stem_pt " + "x".join(map(str, case)))
    n, c, t, h, w = case
    st = E.StemPT(d["w"].float(), *f32(d["s"], d["b"]), stride=(2, 2, 2), pads=(2, 3, 3), dtype=dtype, device="cuda")
    clip = d["clip"].float().cuda()
    assert st.applies(clip)
    fails = []
    tag = "stem_pt %s %s " % ("x".join(map(str, case)), dtype)
    for v in (0, 2):
        same(nc(st.conv(st.layout(clip), variant=v)), pair["y"], tag + "conv variant %d" % v, fails)
    for v in (2, 6):
        same(nc(st.conv_pool(st.layout(clip), variant=v)), pool["y"], tag + "conv_pool variant %d" % v, fails)
    if w % 4 == 0:
        assert st.direct_applies(clip)
        same(nc(st.conv_pool_clip(clip)), pool["y"], tag + "conv_pool_clip", fails)
        big = torch.full((n, c, t + 8, h, w), 3.0, device="cuda")
        big[:, :, 4:4 + t] = clip
        view = big[:, :, 4:4 + t]
        assert not view.is_contiguous() and st.direct_applies(view)
        same(nc(st.conv_pool_clip(view)), pool["y"], tag + "conv_pool_clip on a T-slice", fails)
    assert not fails, "\n".join(fails)


# ---- 6. the folded two-frame temporal conv --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", R.TPAIR_CASES, ids=["x".join(map(str, c)) for c in R.TPAIR_CASES])
def test_tpair_conv_equals_the_temporal_conv(case, dtype, monkeypatch):
    """engine.TPairConv under forced tiles 25 and 26 (both MFMA shapes of the ping-pong kernel) and the tuner's own pick."""
    from ted_spad_amd import engine as E
    d, ref = R.tpair_reference(case, dtype)
    telling(d, ("s", "b"))
    R.fused_conditions(ref, dtype, "tpair " + "x".join(map(str, case)))
    tp = E.TPairConv(d["w"].float(), *f32(d["s"], d["b"]), dtype=dtype, device="cuda")
    xa = cl(d["x"], dtype)
    assert tp.applies(xa, (1, 0, 0))
    fails = []
    for cfg in (25, 26, None):
        monkeypatch.setattr(E, "FORCE_TILE_CFG", cfg)
        same(nc(tp(xa)), ref[0]["y"], "tpair %s %s tile %s" % ("x".join(map(str, case)), dtype, cfg), fails)
    assert not fails, "\n".join(fails)


# ---- 7, 8. two convolutions summed before the one store -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", R.DUAL_CASES, ids=["%s_ld%d" % ("x".join(map(str, c[0])), c[2]) for c in R.DUAL_CASES])
def test_call_dual_equals_the_sum_of_two_convs(case, dtype):
    """PackedConv.call_dual (tedspad_conv_pw_dual_fwd); x2 dense (ld2 = 64) or the last 64 channels of a 128-channel buffer."""
    from ted_spad_amd import engine as E
    dims, cout, ld2 = case
    d, ref = R.dual_reference(case, dtype)
    telling(d, ("s1", "b1"), ("s2", "b2"))
    R.fused_conditions(ref, dtype, "call_dual %s" % (case,))
    pc1 = E.PackedConv(d["w1"].float(), *f32(d["s1"], d["b1"]), dtype=dtype, device="cuda")
    pc2 = E.PackedConv(d["w2"].float(), *f32(d["s2"], d["b2"]), dtype=dtype, device="cuda")
    xa = cl(d["x"], dtype)
    x2a = cl(d["x2"], dtype, **(dict(ld=ld2, coff=ld2 - 64, seed=5) if ld2 > 64 else {}))
    assert pc1.dual_supported(pc2, xa, x2a) and x2a.ld == ld2
    fails = []
    same(nc(pc1.call_dual(xa, pc2, x2a, relu=True)), ref[0]["y"], "call_dual %s %s" % (case, dtype), fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", R.DUAL_P8_CASES, ids=["%s_s%d" % ("x".join(map(str, c[0])), c[4]) for c in R.DUAL_P8_CASES])
def test_call_dual_p8_equals_the_sum_of_two_convs(case, dtype):
    """PackedConv.call_dual_p8 (tedspad_conv_p8_dual_fwd) on odd and even source grids. The scales are folded into the 16-bit weights: a power of two times a
    small integer is exact (asserted in the reference), so the comparison is still torch.equal."""
    from ted_spad_amd import engine as E
    dims, c1, c2, cout, stride = case
    d, ref = R.dual_p8_reference(case, dtype)
    telling(d, ("s1", "b1"), ("s2", "b2"))
    R.fused_conditions(ref, dtype, "call_dual_p8 %s" % (case,))
    pc = E.PackedConv.fused_pair(d["w1"].float(), *f32(d["s1"], d["b1"]), d["w2"].float(), *f32(d["s2"], d["b2"]), dtype=dtype, device="cuda")
    xa, x2a = cl(d["x"], dtype), cl(d["x2"], dtype)
    assert pc.dual_p8_supported(xa, x2a, (stride, stride))
    fails = []
    same(nc(pc.call_dual_p8(xa, x2a, (stride, stride), relu=True)), ref[0]["y"], "call_dual_p8 %s %s" % (case, dtype), fails)
    assert not fails, "\n".join(fails)


# ---- 9. pointwise conv + temporal pair max --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", R.POOL_T2_CASES, ids=["x".join(map(str, c[0])) for c in R.POOL_T2_CASES])
def test_call_pool_t2_equals_conv_then_pair_max(case, dtype):
    """PackedConv.call_pool_t2 (tedspad_conv_pool_t2_fwd) against the reference conv + residual + ReLU + max over frame pairs, not against the two launches:
    an odd frame count with a ragged channel tile (cout 72), and frames of exactly two 128-pixel tiles with a residual."""
    from ted_spad_amd import engine as E
    dims, cin, cout, use_res = case
    d, ref = R.pool_t2_reference(case, dtype)
    telling(d, ("s", "b"))
    R.fused_conditions(ref, dtype, "call_pool_t2 %s" % (case,))
    pc = E.PackedConv(d["w"].float(), *f32(d["s"], d["b"]), dtype=dtype, device="cuda")
    xa = cl(d["x"], dtype)
    ra = cl(d["res"], dtype) if use_res else None
    assert pc.pool_t2_supported(xa)
    got = pc.call_pool_t2(xa, residual=ra, relu=True)
    assert got.dims == (dims[0], dims[1] // 2, dims[2], dims[3])
    fails = []
    same(nc(got), ref[1]["y"], "call_pool_t2 %s %s" % (case, dtype), fails)
    assert not fails, "\n".join(fails)
