"""-m gpu: the conv training code -- the weight gradient (csrc/conv_wgrad.hip, every launch form), the data gradient (train_engine.DgradPlan) and the training
extras of the conv epilogue (mask, y32, stats, stats_rows, nosat) under every tile configuration -- against the float64 references of tests/kernel_refs.py
on SMALL-INTEGER inputs, in f16 and bf16.

Every product and every partial sum is then an integer below 2^24 (kernel_refs.exact_in_fp32 checks that on the reference before anything is compared; the same
gate runs over every case table on the CPU in test_kernel_refs.py), so neither the order of the float atomics, nor a tile's K order, nor the pixel splits, nor
the MFMA shape can change a bit: every comparison here is torch.equal, with the reference rounded once where the output is 16-bit. There is no tolerance to
tune; a dropped, duplicated or misplaced term fails. The norm tests of test_hip_train_ops.py keep covering realistic magnitudes."""
import ctypes as C

import pytest
import torch

import kernel_refs as R

pytestmark = pytest.mark.gpu
D = torch.float64
DTYPES = ("f16", "bf16")
SENTINEL = 12345.0
GUARD = 64                     # floats in front of and behind the accumulator (256 bytes: keeps its alignment)


cl, nc = R.cl, R.nc           # (n, c, t, h, w) float64 <-> channels-last Act, with channel slices of wider buffers: shared with the other exact-arithmetic files
same = R.same                  # torch.equal, with the count and the first differing index on a mismatch


def make_layer(case, w, dtype):
    from ted_spad_amd import train_engine as TE
    wp = torch.nn.Parameter(w.float().cuda())
    return wp, TE.ConvLayer(wp, None, case.stride, case.pf, pads_back=case.pb, pair_w=case.pair_w, dtype=dtype)


def act_x(case, x, dtype, **kw):
    from ted_spad_amd import engine as E
    if case.pair_w is not None:
        return E.clip_to_act(x.float().cuda(), cpad=4, dtype=dtype)          # (n, t, h, w / 2, 8): pixel pairs of 4 channels
    return cl(x, dtype, **kw)


def assert_form(case, layer, xa, dya):
    """The launcher's predicates, from the code's formulas on the code's own geometry: a later change of the heuristics cannot silently empty a case."""
    pc = layer.geom_conv()
    pk, _ = layer._pads_k(pc)
    assert pc.kpad == (pc.K + 63) // 64 * 64 and pc.cpad == (pc.cout + 127) // 128 * 128
    form, splits = R.wgrad_form(pc.cin, pc.cout, pc.k, pc.stride, pk, xa.dims[1:], dya.dims[1:], xa.dims[0])
    assert form == case.form, (case.name, form, splits)
    if case.multi_split:
        assert splits >= 3
    return form, splits


# ---- weight gradient ------------------------------------------------------------------------------------------------------------------------------------
def wgrad_through_layer(case, dtype):
    from ted_spad_amd import train_engine as TE
    x, w, dy = case.tensors()
    want = R.conv_wgrad_ref64(x, dy, w.shape, case.stride, case.pf, case.pb)
    assert R.exact_in_fp32(R.conv_wgrad_ref64(x.abs(), dy.abs(), w.shape, case.stride, case.pf, case.pb))
    wp, layer = make_layer(case, w, dtype)
    xa, dya = act_x(case, x, dtype), cl(dy, dtype)
    form = assert_form(case, layer, xa, dya)
    TE.ARENA.reset(xa.buf.device)
    layer.wgrad(xa, dya)
    layer.flush_grad()
    print("wgrad", case.name, dtype, "form", form)
    same(wp.grad.double().cpu(), want, "wgrad %s %s" % (case.name, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", R.WGRAD_CASES, ids=[c.name for c in R.WGRAD_CASES])
def test_wgrad_equals_float64_reference(case, dtype):
    """ConvLayer.wgrad + flush_grad on every launch form: narrow <1,4>, wide <2,4>, 2x2 <2,2>, three-tile (one split and several, M ending inside a
    64-pixel step), patch with loader waves (one split and several, frames as independent images), and the generic gather on temporal, strided,
    TF-SAME and pixel-pair stem geometries."""
    wgrad_through_layer(case, dtype)


DET_CASES = ["narrow_64_40", "2x2_192_128", "three_c128_w20_h30", "patch_w63_h9", "k333_s2_tfsame"]


@pytest.mark.parametrize("dtype", DTYPES)
def test_wgrad_deterministic_mode_gives_the_same_bits(dtype, deterministic):
    """With the flush gates on (one workgroup at a time) every kernel family still equals the reference; the fixture checks that no workgroup gave up."""
    for name in DET_CASES:
        wgrad_through_layer(R.case_by_name(R.WGRAD_CASES, name), dtype)


DIRECT = [("narrow_64_40", "slice"), ("narrow_40_64", "slice"), ("s2_15", "slice"), ("three_c128_w20_h30", "slice"), ("patch_w30_h9", "slice"),
          ("wide_256_128", "twice"), ("three_c64_w65_h3", "twice"), ("patch_w63_h5", "twice")]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,mode", DIRECT, ids=["%s-%s" % d for d in DIRECT])
def test_wgrad_direct_slices_accumulation_and_padding(name, mode, dtype):
    """tedspad_conv_wgrad called directly. 'slice': x and dy are channel slices of wider buffers (ldx > cin, ldy > cout) whose other channels are non-zero.
    'twice': two calls into the same accumulator give the sum of the two references.
    Around the [cout_pad][kpad] accumulator lie sentinel floats that must stay untouched. Inside it [:cout, :K] is compared; the padding is asserted as
    far as the code visibly promises it: rows >= cout are never written by any of the three kernels (their flushes are guarded by co < Cout) -- they are
    preset to -0.0 here, which even an atomic add of +0.0 would turn into +0.0 -- and columns K .. kpad are either never written (three-tile / patch:
    k < 9 cin by construction) or receive products with the zero page (generic: the K-padding entries of the gather table), so they stay 0
    (narrow_40_64 has such columns: K = 40, kpad = 64)."""
    from ted_spad_amd import _lib, engine as E
    case = R.case_by_name(R.WGRAD_CASES, name)
    x, w, dy = case.tensors()
    sets = [(x, dy)]
    if mode == "twice":
        x2, _, dy2 = case.tensors(seed=12)
        sets.append((x2, dy2))
    want = sum(R.conv_wgrad_ref64(a, b, w.shape, case.stride, case.pf, case.pb) for a, b in sets)
    assert R.exact_in_fp32(sum(R.conv_wgrad_ref64(a.abs(), b.abs(), w.shape, case.stride, case.pf, case.pb) for a, b in sets))
    _, layer = make_layer(case, w, dtype)
    pc = layer.geom_conv()
    pk, _ = layer._pads_k(pc)
    buf = torch.full((GUARD + pc.cpad * pc.kpad + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    acc = buf[GUARD:GUARD + pc.cpad * pc.kpad].view(pc.cpad, pc.kpad)
    acc.zero_()
    acc[pc.cout:].fill_(-0.0)
    for a, b in sets:
        kw = dict(ld=case.cin + 16, coff=8, seed=5) if mode == "slice" else {}
        kwy = dict(ld=case.cout + 24, coff=16, seed=6) if mode == "slice" else {}
        xa, dya = cl(a, dtype, **kw), cl(b, dtype, **kwy)
        assert_form(case, layer, xa, dya)
        n, t, h, wd = xa.dims
        d = pc._desc(n, t, h, wd, xa.ld, pk, dya.dims[1:], dya.ld, 0, False)
        assert (d.ldx > d.cin and d.ldy > d.cout) == (mode == "slice")
        _lib.check(_lib.lib().tedspad_conv_wgrad(C.byref(d), xa.ptr, dya.ptr, pc._ktab(d).data_ptr(), acc.data_ptr(), E._stream_ptr()), "tedspad_conv_wgrad")
    torch.cuda.synchronize()
    host = buf.cpu()
    assert bool((host[:GUARD] == SENTINEL).all()) and bool((host[-GUARD:] == SENTINEL).all()), "sentinels around the accumulator were overwritten"
    hacc = host[GUARD:-GUARD].view(pc.cpad, pc.kpad)
    if pc.cout < pc.cpad:
        bits = hacc[pc.cout:].contiguous().view(torch.int32)
        assert bool((bits == -2 ** 31).all()), "padding rows >= cout were written: %d elements" % int((bits != -2 ** 31).sum())
    assert bool((hacc[:pc.cout, pc.K:] == 0).all()), "padding columns K .. kpad are not zero"
    co, ci, kt, kh, kw_ = w.shape
    got = hacc[:co, :pc.K].reshape(co, pc.k[0], pc.k[1], pc.k[2], pc.cin).permute(0, 4, 1, 2, 3)[:, :ci]
    same(got.double(), want, "direct wgrad %s %s %s" % (name, mode, dtype))


# ---- data gradient --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", R.DGRAD_CASES, ids=[c.name for c in R.DGRAD_CASES])
def test_dgrad_equals_float64_reference(case, dtype):
    """ConvLayer.dgrad (nosat, one dense sub-convolution per parity class writing in place): plain, with a mask drawn from {-1, -0.0, +0.0, 1}, and -- stride 1
    -- with a residual and a power-of-two per-channel scale folded into the weights. Input positions the forward conv never read must be exact zeros; the
    stem's d(clip) is checked in its (n, t, h, w, 4) view with channel 3 exactly zero."""
    x, w, dy = case.tensors()
    n, t, h, wd = case.dims
    _, layer = make_layer(case, w, dtype)
    pair = case.pair_w is not None
    x_dims = (t, h, wd // 2) if pair else (t, h, wd)
    dya = cl(dy, dtype)
    cm = 4 if pair else case.cin
    mask = R.signed_zero_mask(11, case.name + "mask", (n, cm, t, h, wd))
    res = R.small_ints(11, case.name + "res", tuple(x.shape), lo=-8, hi=8, density=1.0)
    scale = torch.tensor([1.0, 2.0, 4.0, 8.0], dtype=D)[torch.arange(case.cout) % 4]          # powers of two: the scaled weights stay exact in 16 bits
    unread = R.conv_dgrad_ref64(torch.ones_like(dy), torch.ones_like(w), x.shape, case.stride, case.pf, case.pb) == 0
    assert R.exact_in_fp32(R.conv_dgrad_ref64(dy.abs(), w.abs(), x.shape, case.stride, case.pf, case.pb, scale=scale) + res.abs())

    def to_act(m):           # a tensor shaped like the input -> the Act the kernel indexes like its output
        if not pair:
            return cl(m, dtype)
        from ted_spad_amd import engine as E
        v = m.permute(0, 2, 3, 4, 1).contiguous().reshape(n, t, h, wd // 2, 8)
        return E.Act(v.to(R.TDT[dtype]).cuda(), 8)

    def from_act(a, what):
        if not pair:
            return nc(a)
        v = a.buf.double().cpu().reshape(n, t, h, wd, 4)
        assert float(v[..., 3].abs().max()) == 0.0, "%s: channel 3 of d(clip) is not zero" % what
        return v[..., :3].permute(0, 4, 1, 2, 3)

    runs = [("plain", {}, {}), ("mask", dict(mask=to_act(mask)), dict(mask=mask[:, :case.cin]))]
    if case.stride == (1, 1, 1):
        runs.append(("residual+scale+mask", dict(scale=scale.float().cuda(), residual=to_act(res), mask=to_act(mask)), dict(scale=scale, residual=res, mask=mask)))
    for what, kw, rkw in runs:
        tag = "dgrad %s %s %s" % (case.name, what, dtype)
        got = from_act(layer.dgrad(dya, x_dims, **kw), tag)
        want = R.round_once(R.conv_dgrad_ref64(dy, w, x.shape, case.stride, case.pf, case.pb, **rkw), dtype)
        same(got, want, tag)
        if case.stride != (1, 1, 1):
            assert float(got[unread].abs().max() if bool(unread.any()) else 0.0) == 0.0, tag + ": a never-read input position is not zero"
    plans = [p[1] for p in layer._dgrad.values()]
    assert plans
    if bool(unread.any()):       # never-read positions exist -> the plan zeroes the output first
        assert all(p.need_zero for p in plans)


# ---- epilogue extras under every tile configuration ----------------------------------------------------------------------------------------------------
def for_each_cfg(fn):
    """fn(cfg) under every forced tile configuration."""
    from ted_spad_amd import _lib, engine as E
    try:
        for cfg in range(1, _lib.lib().tedspad_conv_num_tile_cfgs() + 1):
            E.FORCE_TILE_CFG = cfg
            fn(cfg)
    finally:
        E.FORCE_TILE_CFG = None


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case,must", R.EPILOGUE_CASES, ids=[c.name for c, _ in R.EPILOGUE_CASES])
def test_epilogue_extras_equal_float64_reference_on_every_tile(case, must, dtype):
    """PackedConv.__call__ with integer weights, an integer bias as shift and scale = 1, under every tile configuration that accepts the call (a refusal,
    TedSpadHipError, skips that call as in test_every_tile_configuration_gives_the_same_result): (a) y with residual + mask (+ ReLU), (b) y32, (c) stats over
    all rows, (d) stats in three groups whose boundaries fall inside tiles (groups of two samples; the three-sample case: of one sample), the groups summing
    to (c) exactly. A configuration that accepts an extra and ignores it fails here."""
    from ted_spad_amd import _lib, engine as E
    x, w, bias, res, mask = R.epilogue_tensors(case)
    G = R.EPILOGUE_GROUPS
    y_ref, z_ref = R.conv_fwd_ref64(x, w, case.stride, case.pf, case.pb, shift=bias, residual=res, mask=mask, relu=True)
    _, zabs = R.conv_fwd_ref64(x.abs(), w.abs(), case.stride, case.pf, case.pb, shift=bias.abs())
    sabs = R.conv_stats_ref64(z_ref.abs(), 1)
    assert R.exact_in_fp32(zabs + res.abs(), sabs[0, 0], sabs[0, 1], stats_z=zabs)
    y_ref, zy_ref = R.round_once(y_ref, dtype), R.round_once(z_ref, dtype)
    st_ref, sg_ref = R.conv_stats_ref64(z_ref, 1)[0], R.conv_stats_ref64(z_ref, G)
    assert torch.equal(sg_ref.sum(0), st_ref)
    pc = E.PackedConv(w.float(), None, bias.float(), dtype=dtype, device="cuda")
    xa, ra, ma = cl(x, dtype), cl(res, dtype), cl(mask, dtype)
    co = case.cout
    ran, fails = {}, []

    def one(cfg):
        done = []
        tag = "%s %s cfg %d " % (case.name, dtype, cfg)

        def a():
            y = pc(xa, pads=case.pf, residual=ra, mask=ma, relu=True)
            return same(nc(y), y_ref, tag + "(a) y with residual + mask", fails)

        def b():
            z = pc(xa, pads=case.pf, relu=False, y32=True)
            return same(z.double().cpu().permute(0, 4, 1, 2, 3), z_ref, tag + "(b) y32", fails)

        def c():
            st = torch.zeros((2, pc.cpad), device="cuda")
            y = pc(xa, pads=case.pf, relu=False, stats=st)
            ok = same(st.double().cpu()[:, :co], st_ref, tag + "(c) stats", fails) & same(nc(y), zy_ref, tag + "(c) y beside stats", fails)
            return ok & same(st.cpu()[:, pc.cout:], torch.zeros(2, pc.cpad - pc.cout), tag + "(c) stats padding", fails)

        def d():
            sg = torch.zeros((G, 2, pc.cpad), device="cuda")
            pc(xa, pads=case.pf, relu=False, stats=sg)
            sgc = sg.double().cpu()[..., :co]
            return same(sgc, sg_ref, tag + "(d) grouped stats", fails) & same(sgc.sum(0), st_ref, tag + "(d) groups sum to the whole", fails)

        for what, fn in (("a", a), ("b", b), ("c", c), ("d", d)):
            try:
                fn()
            except _lib.TedSpadHipError:
                continue                                   # the configuration refuses this geometry or this extra
            done.append(what)
        if done:
            ran[cfg] = "".join(done)

    for_each_cfg(one)
    print(case.name, dtype, "configurations run (a: residual + mask, b: y32, c: stats, d: grouped stats):", ran)
    for cfg in must:
        assert ran.get(cfg) == "abcd", "configuration %d did not take all four calls: %s" % (cfg, ran)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("dtype", DTYPES)
def test_nosat_stores_inf_and_saturating_stores_65504(dtype):
    """One output channel whose z is exactly 2^17 everywhere: with nosat = 1 (the training path) the f16 store is inf, with nosat = 0 it is 65504; y32 holds
    131072 both ways and the neighbouring channels are unchanged. bf16 holds 2^17 and is never clamped: 131072 both ways. Under every tile configuration
    that takes the call."""
    from ted_spad_amd import _lib, engine as E
    case = R.ConvCase("nosat", (2, 1, 9, 10), 64, 64, (1, 3, 3))
    x, w, _ = case.tensors(seed=19, density=0.5)
    x[:, 0] = 128.0
    hot = 5
    w[hot] = 0.0
    w[hot, 0, 0, 1, 1] = 1024.0
    _, z_ref = R.conv_fwd_ref64(x, w, case.stride, case.pf, case.pb)
    _, zabs = R.conv_fwd_ref64(x.abs(), w.abs(), case.stride, case.pf, case.pb)
    assert R.exact_in_fp32(zabs) and bool((z_ref[:, hot] == 2.0 ** 17).all())
    want = {1: R.round_once(z_ref, dtype)}
    want[0] = want[1].clamp(-65504.0, 65504.0) if dtype == "f16" else want[1]
    assert float(want[1][:, hot].min()) == (float("inf") if dtype == "f16" else 2.0 ** 17) and float(want[0][:, hot].max()) == (65504.0 if dtype == "f16" else 2.0 ** 17)
    others = [c for c in range(case.cout) if c != hot]
    assert bool(torch.isfinite(want[1][:, others]).all()) and float(want[1][:, others].abs().max()) < 65504.0
    pc = E.PackedConv(w.float(), None, None, dtype=dtype, device="cuda")
    xa = cl(x, dtype)
    ran, fails = {}, []

    def one(cfg):
        done = []
        for nosat in (1, 0):
            pc.nosat = bool(nosat)
            for y32 in (False, True):
                tag = "nosat %s cfg %d nosat=%d %s" % (dtype, cfg, nosat, "y32" if y32 else "y")
                try:
                    out = pc(xa, pads=case.pf, relu=False, y32=y32)
                except _lib.TedSpadHipError:
                    continue
                if y32:
                    same(out.double().cpu().permute(0, 4, 1, 2, 3), z_ref, tag, fails)
                else:
                    same(nc(out), want[nosat], tag, fails)
                done.append((nosat, y32))
        if done:
            ran[cfg] = done

    for_each_cfg(one)
    print("nosat", dtype, "configurations run:", sorted(ran))
    assert len(ran.get(5, [])) == 4, ran
    assert not fails, "\n".join(fails)
