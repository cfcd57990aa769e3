"""-m gpu: the plain forward convolution (tedspad_conv_fwd_ex through PackedConv.__call__ and PackedConv.gather) under EVERY tile configuration, against the float64
reference of tests/kernel_refs.py on SMALL-INTEGER inputs, in f16 and bf16.

Integer activations and weights, per-channel power-of-two scales and non-zero integer shifts keep every product and every partial sum a multiple of the row's step
below 2^24 steps (kernel_refs.fused_conditions checks that on the reference before anything is launched; test_kernel_refs.py checks the whole table on the CPU), so
neither a tile's K order, nor split-K, nor the head / tail split of cout = 128 k + r, nor the MFMA shape can change a bit: every live tile that takes a row must equal
kernel_refs.chain_ref64 (one stage, rounded once) under torch.equal. And a tile takes a row exactly where kernel_refs.fwd_accepts, the launcher's acceptance rule
restated from the code, says so: a TedSpadHipError refusal (TEDSPAD_EINVAL / TEDSPAD_EUNSUPPORTED before any launch) anywhere else fails, as does a launch where
the rule refuses -- a later change of a predicate can neither silently empty a row nor silently widen a tile's domain.

The sigmoid epilogue (__expf) is not exact by nature and stays with the tolerance tests of test_hip_ops.py; the folded two-frame GEMM of engine.TPairConv is held to
its exact reference under tiles 25 and 26 in test_hip_fused_exact.py."""
import pytest
import torch

import kernel_refs as R

pytestmark = pytest.mark.gpu
D = torch.float64
DTYPES = ("f16", "bf16")
SENTINEL = 12288.0             # exact in f16 and bf16
cl, nc, same = R.cl, R.nc, R.same


def where(got, want):
    """For R.same: the first differing element of (n, c, t, h, w) tensors named as sample / frame / pixel / channel, and the output channels that differ."""
    bad = (got != want) & ~(torch.isnan(got) & torch.isnan(want))
    n, c, t, h, w = (int(i) for i in bad.nonzero()[0])
    chans = bad.any(0).flatten(1).any(1).nonzero().flatten().tolist()
    return " -- sample %d frame %d pixel (%d, %d) channel %d; %d output channels differ: %s%s" % (
        n, t, h, w, c, len(chans), chans[:16], " ..." if len(chans) > 16 else "")


def under_every_tile(call, accepts, tag, fails):
    """call(cfg) under every forced tile configuration; ran <=> accepts(cfg), a mismatch either way is appended to `fails`. Returns the configurations that ran.
    Only a refusal before any launch counts as one: any other error (a failed launch) is raised at once."""
    from ted_spad_amd import _lib, engine as E
    ran = []
    try:
        for cfg in range(1, _lib.lib().tedspad_conv_num_tile_cfgs() + 1):
            E.FORCE_TILE_CFG = cfg
            try:
                call(cfg)
                took = True
            except _lib.TedSpadHipError as e:
                if "failed (-1)" not in str(e) and "failed (-3)" not in str(e):
                    raise
                took = False
            if took:
                ran.append(cfg)
            if took != bool(accepts(cfg)):
                fails.append("%s cfg %d: %s, but the launcher's rule as restated by kernel_refs says it %s" % (
                    tag, cfg, "ran" if took else "was refused", "refuses: %s" % (accepts(cfg, why=True),) if took else "accepts"))
    finally:
        E.FORCE_TILE_CFG = None
    return ran


def rule(conv, extras=(), n=None):
    def accepts(cfg, why=False):
        bad = R.fwd_refusals(cfg, conv, extras, n)
        return bad if why else not bad
    return accepts


def packed(fc, d, dtype):
    """The row's PackedConv, its input Act maker and its (pads, pads_back) in kernel form; the geometry the predicate works on is checked against the object's own."""
    from ted_spad_amd import engine as E
    c = fc.conv
    pc = E.PackedConv(d["w"].float(), d["s"].float(), d["b"].float(), stride=c.stride, dtype=dtype, device="cuda", pair_w=c.pair_w)
    g = R.FwdGeo(c)
    assert (pc.cin, pc.k, pc.stride, pc.kpad, pc.cout) == (g.cin, g.k, g.stride, g.kpad, g.cout), (c.name, pc.cin, pc.k, pc.stride, pc.kpad, pc.cout)
    if c.pair_w is not None:
        pads, pads_back = (c.pf[0], c.pf[1], pc.pair_pw), (c.pb[0], c.pb[1], pc.k[2] - 1 - pc.pair_pw)
        assert pads == g.pf
    else:
        pads, pads_back = c.pf, c.pb
    return pc, pads, pads_back


def act_x(fc, x, dtype, **kw):
    from ted_spad_amd import engine as E
    c = fc.conv
    if c.pair_w is not None:
        return E.clip_to_act(x.float().cuda(), cpad=4, dtype=dtype)          # (n, t, h, w / 2, 8): pixel pairs of 4 channels
    if c.cin % 8:
        x = torch.nn.functional.pad(x, (0, 0, 0, 0, 0, 0, 0, 8 - c.cin % 8))       # the kernel form's zero channels
    return cl(x, dtype, **kw)


def reference(fc, dtype):
    """The row's tensors and its reference, the input conditions asserted before anything is launched."""
    d, ref = R.fwd_reference(fc, dtype)
    assert R.bn_is_telling(d["s"], d["b"])
    R.fused_conditions(ref, dtype, "fwd " + fc.name)
    return d, ref[0]["y"]


def test_the_case_table_counts_the_library_s_tile_configurations():
    from ted_spad_amd import _lib
    assert _lib.lib().tedspad_conv_num_tile_cfgs() == R.NUM_TILE_CFGS


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fc", R.FWD_CASES, ids=[c.name for c in R.FWD_CASES])
def test_forward_conv_equals_float64_reference_on_every_tile(fc, dtype):
    """PackedConv.__call__ with pads, pads_back, residual, relu=True under every forced tile configuration and once through the tuner's own path: the output equals
    chain_ref64's single stage bit for bit, and ran <=> fwd_accepts for every id. The failures of all tiles are collected before the assertion."""
    d, y_ref = reference(fc, dtype)
    pc, pads, pads_back = packed(fc, d, dtype)
    xa = act_x(fc, d["x"], dtype)
    ra = cl(d["res"], dtype) if fc.residual else None
    fails = []
    tag = "fwd %s %s" % (fc.name, dtype)

    def call(cfg):
        y = pc(xa, pads=pads, pads_back=pads_back, residual=ra, relu=True)
        same(nc(y), y_ref, "%s cfg %s" % (tag, cfg), fails, detail=where)

    ran = under_every_tile(call, rule(fc.conv), tag, fails)
    call("none (heuristic / tuner)")
    print(tag, "configurations run:", ran, "-- head on the tile, tail on its 64-wide sibling:", [c for c in ran if R.fwd_is_split(c, fc.conv)])
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fc", R.FWD_SLICE_ROWS, ids=[c.name for c in R.FWD_SLICE_ROWS])
def test_forward_conv_on_channel_slices_of_wider_buffers(fc, dtype):
    """x read from the channel slice [coff, coff + cin) of a wider buffer whose other channels hold non-zero integers, the residual from a slice with its own row
    stride, the output written into a slice of a wider buffer pre-filled with a sentinel: under every accepting tile the slice equals the reference and every
    neighbouring channel still holds the sentinel. The offsets are multiples of 8 channels (16 bytes)."""
    from ted_spad_amd import engine as E
    d, y_ref = reference(fc, dtype)
    c = fc.conv
    pc, pads, pads_back = packed(fc, d, dtype)
    xa = act_x(fc, d["x"], dtype, ld=c.cin + 24, coff=16, seed=7)
    ra = cl(d["res"], dtype, ld=pc.cout + 16, coff=8, seed=8) if fc.residual else None
    assert xa.ld > xa.c and xa.coff % 8 == 0 and (ra is None or (ra.ld > ra.c and ra.ld != xa.ld))
    n = c.dims[0]
    fails = []
    tag = "fwd slices %s %s" % (fc.name, dtype)

    def call(cfg):
        buf = torch.full((n,) + tuple(c.out) + (pc.cout + 40,), SENTINEL, dtype=R.TDT[dtype], device="cuda")
        y = pc(xa, pads=pads, pads_back=pads_back, residual=ra, relu=True, out=E.Act(buf, pc.cout, 24))
        same(nc(y), y_ref, "%s cfg %s" % (tag, cfg), fails, detail=where)
        host = buf.double().cpu()
        rest = torch.cat([host[..., :24], host[..., 24 + pc.cout:]], dim=-1)
        if not bool((rest == SENTINEL).all()):
            fails.append("%s cfg %s: %d elements of the output buffer's other channels were overwritten" % (tag, cfg, int((rest != SENTINEL).sum())))

    ran = under_every_tile(call, rule(c), tag, fails)
    call("none (heuristic / tuner)")
    print(tag, "configurations run:", ran)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fc", R.FWD_STEM_ROWS, ids=[c.name for c in R.FWD_STEM_ROWS])
def test_batch_statistics_on_the_stem_rows_equal_float64_reference(fc, dtype):
    """`stats` over all rows and in groups of one sample each (the stem halo tiles need groups of whole samples, the generic tiles >= 256 rows per group) under every
    tile that takes the row with the extra, stem tiles and generic ones: the sums of z and z^2 equal conv_stats_ref64 bit for bit, the padding columns stay zero, and
    the y beside them is the row's reference."""
    d, y_ref = reference(fc, dtype)
    c = fc.conv
    n = c.dims[0]
    _, sg_ref, _ = R.fwd_stats_reference(fc, d)
    st_ref = sg_ref.sum(0)
    rows = c.out[0] * c.out[1] * c.out[2]
    assert rows >= 256
    pc, pads, pads_back = packed(fc, d, dtype)
    xa = act_x(fc, d["x"], dtype)
    fails = []
    tag = "fwd stats %s %s" % (fc.name, dtype)

    def whole(cfg):
        st = torch.zeros((2, pc.cpad), device="cuda")
        y = pc(xa, pads=pads, pads_back=pads_back, relu=True, stats=st)
        same(st.double().cpu()[:, :c.cout], st_ref, "%s cfg %s stats" % (tag, cfg), fails)
        same(st.cpu()[:, pc.cout:], torch.zeros(2, pc.cpad - pc.cout), "%s cfg %s stats padding" % (tag, cfg), fails)
        same(nc(y), y_ref, "%s cfg %s y beside stats" % (tag, cfg), fails, detail=where)

    def grouped(cfg):
        sg = torch.zeros((n, 2, pc.cpad), device="cuda")
        pc(xa, pads=pads, pads_back=pads_back, relu=True, stats=sg)
        same(sg.double().cpu()[..., :c.cout], sg_ref, "%s cfg %s statistics per sample" % (tag, cfg), fails)

    ran = under_every_tile(whole, rule(c, ("stats",)), tag, fails)
    ran_g = under_every_tile(grouped, rule(c, (("stats_rows", rows),)), tag + " grouped", fails)
    print(tag, "configurations run:", ran, "grouped:", ran_g)
    assert set(R.STEM_TILES) <= set(ran) and set(R.STEM_TILES) <= set(ran_g)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("row", R.GATHER_FWD_CASES, ids=["%dx%d_%d" % (r[0][2], r[0][3], r[2]) for r in R.GATHER_FWD_CASES])
def test_gathered_concatenation_equals_float64_reference(row, dtype):
    """PackedConv.gather: source 0 at half resolution through the x2 nearest map, the skips channel slices of wider buffers, against conv_fwd_ref64 on the concatenation
    built in float64. Tiles 32, 33, 38 and 40 (the last with cin >= 128 and 32 < cout <= 64 or cout = 128 only) take gathered sources, every other id refuses."""
    from ted_spad_amd import engine as E
    dims, chans, cout = row
    conv = R.gather_conv_case(row)
    name = conv.name
    d, ref = R.gather_fwd_reference(row, dtype)
    assert R.bn_is_telling(d["s"], d["b"])
    R.fused_conditions(ref, dtype, "fwd " + name)
    srcs = [(cl(v, dtype, ld=v.shape[1] + 16 * i, coff=8 * i, seed=9 + i) if i else cl(v, dtype), i == 0) for i, v in enumerate(d["srcs"])]
    assert all(a.ld > a.c for a, up in srcs if not up)
    pc = E.PackedConv(d["w"].float(), d["s"].float(), d["b"].float(), dtype=dtype, device="cuda")
    fails = []
    tag = "fwd %s %s" % (name, dtype)

    def call(cfg):
        same(nc(pc.gather(srcs, pads=(0, 1, 1))), ref[0]["y"], "%s cfg %s" % (tag, cfg), fails, detail=where)

    ran = under_every_tile(call, rule(conv, ("gathered",)), tag, fails)
    call("none (heuristic)")
    print(tag, "configurations run:", ran)
    assert 5 not in ran and set(ran) <= {32, 33, 38, 40} and len(ran) >= 3
    assert not fails, "\n".join(fails)
