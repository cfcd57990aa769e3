"""-m gpu: the weight images, folded BatchNorm vectors and gradient unpack of csrc/pack.hip (and tedspad_bn_fold of train_ops.hip) against host references,
bit for bit. Every convolution reads what these kernels write -- inference and training, forward and data gradient -- so a defect here makes every network
slightly wrong in the same way on both sides of each comparison the rest of the suite makes.

  images:    tedspad_pack_conv_weights and tedspad_pack_multi == kernel_refs.pack_image_ref (one fp32 multiply by the scale, one round-to-nearest-even, f16
             saturated) on weights that hold ties, f16 subnormals, -0.0 and values above 65504; every branch of the multi-job launch's plan (kernel_refs.PACK_CASES,
             the path of each row asserted through pk_plan_ref); destinations prefilled with 0x7E7E between guards: the padding must come back +0, the guards untouched
  find_job:  tables of 1 .. 4097 jobs around the boundaries of the 64-ary search, a 256-workgroup job first, in the middle and last
  fold:      scale == float32(fold_ref64) bit for bit, shift within the fp32 rounding of a value a few double ulps from the reference; second output pair, NULL outputs
  unpack:    tedspad_wgrad_unpack_multi == kernel_refs.wgrad_unpack_ref on exact values
  refusals:  TEDSPAD_EINVAL and an untouched destination"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import kernel_refs as R
from ted_spad_amd.synth import synth_tensor

pytestmark = pytest.mark.gpu
SEED = 3                 # tests/test_kernel_refs.py checks the rounding ingredients of the weights of this seed (PACK_SEED)
GUARD = 64               # elements in front of and behind everything a kernel writes (a multiple of 16 bytes: the images keep their alignment)
EINVAL = -1
NAN_BITS = 0x7FC00000


def _api():
    from ted_spad_amd import _lib, engine as E
    return _lib, _lib.lib(), E


class Slots:
    """One device buffer that holds every output of a launch, each between guards, all prefilled with a sentinel; `expected` is its host image."""

    def __init__(self, sizes, np_dtype, torch_dtype, fill):
        self.off, total = [], GUARD
        for n in sizes:
            self.off.append(total)
            total += n + GUARD
        self.sizes, self.item = list(sizes), np.dtype(np_dtype).itemsize
        self.expected = np.full(total, fill, dtype=np_dtype)
        self.buf = torch.from_numpy(self.expected.copy()).cuda()
        assert self.buf.dtype == torch_dtype and self.buf.data_ptr() % 16 == 0

    def ptr(self, i):
        return self.buf.data_ptr() + self.off[i] * self.item

    def want(self, i, values):
        values = np.asarray(values).reshape(-1)
        assert values.size == self.sizes[i]
        self.expected[self.off[i]:self.off[i] + values.size] = values

    def got(self, i):
        return self.buf[self.off[i]:self.off[i] + self.sizes[i]].cpu().numpy()

    def bits_equal(self):
        torch.cuda.synchronize()
        return np.array_equal(self.buf.cpu().numpy().view(np.uint8), self.expected.view(np.uint8))

    def first_bad_slot(self):
        g = self.buf.cpu().numpy()
        for i, (o, n) in enumerate(zip(self.off, self.sizes)):
            if not np.array_equal(g[o:o + n].view(np.uint8), self.expected[o:o + n].view(np.uint8)):
                bad = np.nonzero(g[o:o + n] != self.expected[o:o + n])[0]
                return "slot %d differs in %d of %d elements, first at %s" % (i, bad.size, n, bad[:1])
            if not np.array_equal(g[o - GUARD:o].view(np.uint8), self.expected[o - GUARD:o].view(np.uint8)):
                return "the guard in front of slot %d was written" % i
        return "the last guard was written"


def _i16_slots(sizes):
    return Slots(sizes, np.int16, torch.int16, R.SENTINEL16)


class Image:
    def __init__(self, name, w, scale, args, ref):
        self.name, self.w, self.scale, self.args, self.ref = name, w, scale, args, ref

    def job(self, _lib, out_ptr, dtype_code):
        a = self.args
        j = _lib.PackJob(w=self.w.data_ptr(), scale=self.scale.data_ptr() if self.scale is not None else None, out=out_ptr, co=a["co"], ci=a["ci"], kt=a["kt"],
                         kh=a["kh"], kw=a["kw"], cink=a["cink"], kwk=a["kwk"], pair_shift=a["pair_shift"], mode=a["mode"], rows=a["rows"], rows_pad=a["rows_pad"],
                         kpad=a["kpad"], dtype=dtype_code, block0=-1, nblocks=-1)
        for i, g in enumerate(a["geo"]):
            j.geo[i] = g
        return j

    def blocks(self):
        a = self.args
        return R.pk_plan_ref(a["mode"], a["pair_shift"], a["kw"], a["kwk"], a["ci"], a["kt"] * a["kh"] * a["kw"], a["rows_pad"], (a["co"] + 7) // 8 * 8).blocks(a["rows_pad"], a["kpad"])


@functools.lru_cache(maxsize=None)
def _images(dtype):
    """Every image of kernel_refs.PACK_CASES in one dtype, with and without the per-co scale: the forward image and the data-gradient image of every parity class of a
    real train_engine.DgradPlan (its _pack_args, its padding as tedspad_conv_cout_pad / tedspad_conv_kpad give it), each with its reference bits. Computed once."""
    _lib, L, E = _api()
    from ted_spad_amd import train_engine as TE
    out = []
    for case in R.PACK_CASES:
        w, s = R.pack_weights(case.shape, SEED)
        wd, sd = torch.from_numpy(w).cuda(), torch.from_numpy(s).cuda()
        fwd = E.PackedConv(wd, None, None, stride=case.stride, dtype=dtype, pair_w=case.pair_w)
        plan = TE.DgradPlan(wd, None, case.stride_k, case.pads_k, case.in_dims, case.out_dims, dtype, pair_w=case.pair_w)
        assert [pc._pack_args["geo"] for _, pc, _, _ in plan.subs] == case.classes(), case.name
        for pc in [fwd] + [pc for _, pc, _, _ in plan.subs]:
            a = dict(pc._pack_args, rows_pad=pc.cpad, kpad=pc.kpad)
            mode = a["mode"]
            ra = case.pack_args(mode, a["geo"] if mode else None)                      # the geometry the CPU checks of the references and of the plan used
            assert all(a[k] == ra[k] for k in ("cink", "kwk", "pair_shift", "rows", "rows_pad", "kpad")), (case.name, a, ra)
            q = case.plan(mode, a["geo"])
            assert (q.tiled, q.per_tile, q.tiled and q.tiles > R.PK_MAX_BLOCKS) == (case.dgrad if mode else case.fwd), case.name
            for scale, scale_d in ((None, None), (s, sd)):
                ref = R.pack_image_ref(w, scale, dtype=dtype, **ra)
                out.append(Image("%s/%s%s%s" % (case.name, "dgrad" if mode else "fwd", a["geo"][:6] if mode else "", "/scaled" if scale is not None else ""), wd, scale_d, a, ref))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dtype", R.BOTH)
def test_pack_conv_weights_equals_the_reference_image(dtype):
    """tedspad_pack_conv_weights (pack_body: the gather every other pack in the suite is compared with), every image of the case table."""
    _lib, L, E = _api()
    imgs = _images(dtype)
    dst = _i16_slots([im.ref.size for im in imgs])
    for i, im in enumerate(imgs):
        a = im.args
        dst.want(i, im.ref)
        geo = (C.c_int32 * 9)(*a["geo"]) if a["mode"] else None
        rc = L.tedspad_pack_conv_weights(im.w.data_ptr(), im.scale.data_ptr() if im.scale is not None else None, dst.ptr(i), a["co"], a["ci"], a["kt"], a["kh"], a["kw"],
                                         a["cink"], a["kwk"], a["pair_shift"], a["mode"], a["rows"], a["rows_pad"], a["kpad"], geo, E.DTYPES[dtype][1], E._stream_ptr())
        assert rc == 0, im.name
    if not dst.bits_equal():
        bad = dst.first_bad_slot()
        raise AssertionError("%s: %s" % (imgs[int(bad.split()[1])].name if bad.startswith("slot") else "", bad))


@pytest.mark.parametrize("dtype", R.BOTH)
def test_pack_multi_equals_the_reference_image(dtype):
    """tedspad_pack_multi with one table that holds every image of the case table: the LDS-tiled forward and data-gradient paths (one and several rows per tile, 8 / 16 / 32
    channels per tile, short last co tiles, the stride loop of jobs with more tiles than workgroups, the tiled path's own zero fill) and pack_body inside the same launch.
    The workgroups the library plans per job are those of pk_plan_ref."""
    _lib, L, E = _api()
    imgs = _images(dtype)
    dst = _i16_slots([im.ref.size for im in imgs])
    jobs = (_lib.PackJob * len(imgs))(*[im.job(_lib, dst.ptr(i), E.DTYPES[dtype][1]) for i, im in enumerate(imgs)])
    for i, im in enumerate(imgs):
        dst.want(i, im.ref)
    tab = torch.empty(C.sizeof(jobs), dtype=torch.uint8, device="cuda")
    assert L.tedspad_pack_multi(C.cast(jobs, C.c_void_p), len(imgs), tab.data_ptr(), 1, E._stream_ptr()) == 0
    b0 = 0
    for j, im in zip(jobs, imgs):
        assert (j.block0, j.nblocks) == (b0, im.blocks()), im.name
        b0 += j.nblocks
    if not dst.bits_equal():
        bad = dst.first_bad_slot()
        raise AssertionError("%s: %s" % (imgs[int(bad.split()[1])].name if bad.startswith("slot") else "", bad))


def _big_positions(n):
    return sorted({0, n // 2, n - 1})


@pytest.mark.parametrize("dtype", R.BOTH)
@pytest.mark.parametrize("njobs", R.FIND_JOB_SIZES)
def test_find_job_maps_every_workgroup_to_its_job(njobs, dtype):
    """Tables of 1 .. 4097 jobs (one, two and three rounds of the 64-ary search): one-workgroup jobs with distinct (8, 8, 1, 1, 1) weights and 8 x 64 images, and the
    256-workgroup forward image of the largest case first, in the middle and last, so that a job's first workgroup is not its index. Every image and every guard
    between them is checked."""
    _lib, L, E = _api()
    code = E.DTYPES[dtype][1]
    big = next(im for im in _images(dtype) if im.name == R.PACK_BIG + "/fwd/scaled")
    assert big.blocks() == R.PK_MAX_BLOCKS
    pos = _big_positions(njobs)
    ws = synth_tensor(SEED, "small_w%d" % njobs, (njobs, 8, 8), -1, 1).numpy().astype(np.float32)
    small_ref = R.pack_image_ref(ws.reshape(njobs * 8, 8, 1, 1, 1), None, cink=8, kwk=1, pair_shift=-1, mode=0, rows=njobs * 8, rows_pad=njobs * 8, kpad=64, geo=None,
                                 dtype=dtype).reshape(njobs, 8 * 64)
    wd = torch.from_numpy(ws).cuda()
    dst = _i16_slots([big.ref.size if i in pos else 8 * 64 for i in range(njobs)])
    jobs = (_lib.PackJob * njobs)()
    want_b0, b0 = [], 0
    for i in range(njobs):
        want_b0.append(b0)
        if i in pos:
            jobs[i] = big.job(_lib, dst.ptr(i), code)
            dst.want(i, big.ref)
            b0 += R.PK_MAX_BLOCKS
        else:
            jobs[i] = _lib.PackJob(w=wd.data_ptr() + i * 8 * 8 * 4, scale=None, out=dst.ptr(i), co=8, ci=8, kt=1, kh=1, kw=1, cink=8, kwk=1, pair_shift=-1, mode=0, rows=8,
                                   rows_pad=8, kpad=64, dtype=code, block0=-1, nblocks=-1)
            dst.want(i, small_ref[i])
            b0 += 1
    tab = torch.empty(C.sizeof(jobs), dtype=torch.uint8, device="cuda")
    assert L.tedspad_pack_multi(C.cast(jobs, C.c_void_p), njobs, tab.data_ptr(), 1, E._stream_ptr()) == 0
    assert [j.block0 for j in jobs] == want_b0 and all(j.nblocks == (R.PK_MAX_BLOCKS if i in pos else 1) for i, j in enumerate(jobs))
    assert dst.bits_equal(), dst.first_bad_slot()


UNPACK_BIG = (128, 456, 1, 3, 3)           # 525 312 elements: the 256 workgroups of a job, each thread a little more than 8 elements


def _unpack_job(_lib, dw, grad_ptr, rs, shape, cink, kpad, acc):
    co, ci, kt, kh, kw = shape
    return _lib.WgradUnpackJob(dw=dw.data_ptr(), grad=grad_ptr, row_scale=rs.data_ptr() if rs is not None else None, co=co, ci=ci, kt=kt, kh=kh, kw=kw, cink=cink, kpad=kpad,
                               accumulate=int(acc), block0=-1, nblocks=-1)


def _accumulator(seed, name, shape, cink, kpad, extra_rows=8):
    """A packed fp32 accumulator of small integers [co + extra_rows][kpad]; the K padding, the rows above co and the kernel-form channels above ci hold 12345."""
    co, ci, kt, kh, kw = shape
    taps = kt * kh * kw
    dw = np.full((co + extra_rows, kpad), 12345.0, dtype=np.float32)
    v = np.full((co, taps, cink), 12345.0, dtype=np.float32)
    v[:, :, :ci] = R.nonzero_ints(seed, name, (co, taps, ci)).numpy()
    dw[:co, :taps * cink] = v.reshape(co, taps * cink)
    return dw


def _run_unpack(jobs_spec):
    """jobs_spec: [(shape, cink, kpad, dw numpy, row_scale numpy or None, grad0 numpy or None)] -> launches them as one table and checks every gradient and guard."""
    _lib, L, E = _api()
    n = len(jobs_spec)
    dst = Slots([int(np.prod(s[0])) for s in jobs_spec], np.float32, torch.float32, -777.0)
    keep, jobs = [], (_lib.WgradUnpackJob * n)()
    want_b0, b0 = [], 0
    for i, (shape, cink, kpad, dw, rs, g0) in enumerate(jobs_spec):
        dwd = dw if isinstance(dw, torch.Tensor) else torch.from_numpy(dw).cuda()
        rsd = None if rs is None else torch.from_numpy(rs.astype(np.float32)).cuda()
        keep += [dwd, rsd]
        if g0 is not None:
            dst.buf[dst.off[i]:dst.off[i] + dst.sizes[i]] = torch.from_numpy(g0.astype(np.float32).reshape(-1)).cuda()
        jobs[i] = _unpack_job(_lib, dwd, dst.ptr(i), rsd, shape, cink, kpad, g0 is not None)
        ref = R.wgrad_unpack_ref(dwd.cpu().numpy(), shape[0], shape[1], shape[2:], cink, kpad, rs, g0)
        assert float(np.abs(ref).max()) < 2 ** 24 and np.array_equal(ref.astype(np.float32).astype(np.float64), ref)            # exact, fused or not
        dst.want(i, ref.astype(np.float32))
        want_b0.append(b0)
        b0 += max(1, min(256, (int(np.prod(shape)) + 2047) // 2048))
    tab = torch.empty(C.sizeof(jobs), dtype=torch.uint8, device="cuda")
    assert L.tedspad_wgrad_unpack_multi(C.cast(jobs, C.c_void_p), n, tab.data_ptr(), 1, E._stream_ptr()) == 0
    assert [j.block0 for j in jobs] == want_b0
    assert dst.bits_equal(), dst.first_bad_slot()
    return jobs


def test_find_job_of_the_gradient_unpack():
    """tedspad_wgrad_unpack_multi instantiates the search for its own job struct: a table of 65 jobs (two rounds), 256-workgroup jobs first, in the middle and last."""
    n = 65
    pos = _big_positions(n)
    K = 9 * UNPACK_BIG[1]
    kbig = (K + 63) // 64 * 64 + 64
    big_dw = torch.from_numpy(_accumulator(SEED, "ubig", UNPACK_BIG, UNPACK_BIG[1], kbig)).cuda()
    spec = []
    for i in range(n):
        if i in pos:
            spec.append((UNPACK_BIG, UNPACK_BIG[1], kbig, big_dw, np.full(UNPACK_BIG[0], 2.0 ** (i % 3)), None))
        else:
            spec.append(((8, 8, 1, 1, 1), 8, 64, _accumulator(SEED + i, "usmall", (8, 8, 1, 1, 1), 8, 64), None, None))
    jobs = _run_unpack(spec)
    assert all(j.nblocks == (256 if i in pos else 1) for i, j in enumerate(jobs))


def test_wgrad_unpack_multi_equals_the_numpy_reference():
    """Several jobs in one table: write and accumulate, a row scale, kernel-form channels above ci (cink = 8, ci = 3: the accumulator's unused channels hold a sentinel that
    must not leak), and a gradient of more than 256 x 2048 elements (the grid-stride loop). kpad > K everywhere; small-integer accumulators, power-of-two scales and
    integer prior gradients: exact whether or not the multiply is fused into the add."""
    spec = []
    for i, (shape, cink, acc, scaled) in enumerate([((24, 16, 1, 3, 3), 16, False, False), ((96, 40, 1, 3, 3), 40, True, True), ((16, 3, 1, 3, 3), 8, False, True),
                                                    ((512, 512, 1, 3, 3), 512, True, False)]):
        K = 9 * cink
        kpad = (K + 63) // 64 * 64
        kpad += 64 if kpad == K else 0
        assert kpad > K
        rs = R.pow2_scales(shape[0], exps=(-1, 2, 0)).numpy().astype(np.float64).reshape(-1) if scaled else None
        g0 = R.small_ints(SEED + i, "g0", shape, -50, 50, density=1.0).numpy() if acc else None
        spec.append((shape, cink, kpad, _accumulator(SEED + i, "acc", shape, cink, kpad), rs, g0))
    jobs = _run_unpack(spec)
    assert jobs[3].nblocks == 256 and 512 * 512 * 9 > 256 * 2048 and jobs[2].cink > jobs[2].ci


# ---- fold -----------------------------------------------------------------------------------------------------------------------------------------------
def _check_fold(scale_dst, shift_dst, shift_checks):
    """scale slots: bit for bit (guards and zero padding included). shift slots: everything outside the listed value ranges bit for bit, the values within
    their bound. shift_checks: [(slot, ref64 values, bound)]."""
    assert scale_dst.bits_equal(), "scale: " + scale_dst.first_bad_slot()
    got = shift_dst.buf.cpu().numpy()
    exp = shift_dst.expected.copy()
    worst = 0.0
    for slot, ref, bound in shift_checks:
        o = shift_dst.off[slot]
        g = got[o:o + len(ref)].astype(np.float64)
        assert bool(np.isfinite(g).all())
        err = np.abs(g - ref)
        worst = max(worst, float((err / bound).max()) if bool((bound > 0).all()) else 0.0)
        assert bool((err <= bound).all()), "shift slot %d: |shift - ref64| up to %.3g of its bound" % (slot, float((err / np.maximum(bound, 1e-300)).max()))
        exp[o:o + len(ref)] = got[o:o + len(ref)]                                      # checked: take them out of the bit comparison
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), "shift: padding or a guard"
    print("shift: worst |shift - ref64| / bound = %.3f" % worst)


def _nan_slots(sizes):
    s = Slots(sizes, np.float32, torch.float32, np.float32(np.nan))
    assert bool((s.expected.view(np.uint32) == NAN_BITS).all())
    return s


FOLD_ROWS = [(Cn, bias, eps) for Cn in R.FOLD_C for bias in (False, True) for eps in (1e-5, 1e-3)]


def test_bn_fold_equals_the_float64_reference():
    """tedspad_bn_fold: scale is one IEEE division, square root and addition in double, rounded once: == float32(fold_ref64), bit for bit (the library is built
    without fast-math and nothing in that expression can be contracted). shift may be contracted to FMAs: within kernel_refs.fold_shift_bound of the reference."""
    _lib, L, E = _api()
    sc_dst, sh_dst = _nan_slots([r[0] for r in FOLD_ROWS]), _nan_slots([r[0] for r in FOLD_ROWS])
    checks, keep = [], []
    for i, (Cn, bias, eps) in enumerate(FOLD_ROWS):
        g, be, m, v, cb = R.fold_inputs(Cn, SEED + i)
        cb = cb if bias else None
        dev = [None if t is None else torch.from_numpy(t).cuda() for t in (g, be, m, v, cb)]
        keep.append(dev)
        rc = L.tedspad_bn_fold(*(None if t is None else t.data_ptr() for t in dev), C.c_double(eps), Cn, sc_dst.ptr(i), sh_dst.ptr(i), E._stream_ptr())
        assert rc == 0
        sc, sh = R.fold_ref64(g, be, m, v, eps, cb)
        sc_dst.want(i, sc.astype(np.float32))
        checks.append((i, sh, R.fold_shift_bound(sh, be, m, sc, cb)))
    _check_fold(sc_dst, sh_dst, checks)


def test_fold_multi_equals_the_float64_reference():
    """tedspad_fold_multi, one table: every row of tedspad_bn_fold's test written zero-padded beyond C over NaN-prefilled vectors, with a second output pair of another
    length; per C also a job with scale NULL / shift2 NULL, one with shift NULL, gamma NULL with and without a bias, and a job that uses the second pair only."""
    _lib, L, E = _api()
    specs = []             # (C, seed, BatchNorm?, bias?, eps, n, n2, scale?, shift?, scale2?, shift2?)
    for i, (Cn, bias, eps) in enumerate(FOLD_ROWS):
        specs.append((Cn, SEED + i, True, bias, eps, Cn + 37, Cn, True, True, True, True))
    for Cn in R.FOLD_C:
        specs.append((Cn, SEED + Cn, True, True, 1e-5, Cn + 3, Cn + 9, False, True, True, False))
        specs.append((Cn, SEED + Cn, True, False, 1e-5, Cn + 5, 0, True, False, False, False))
        specs.append((Cn, SEED + Cn, False, True, 0.0, Cn + 1, 0, True, True, False, False))
        specs.append((Cn, SEED + Cn, False, False, 0.0, Cn + 2, Cn, True, True, True, True))
        specs.append((Cn, SEED + Cn, True, False, 1e-3, 0, Cn + 4, False, False, True, True))
    sizes_sc, sizes_sh = [], []
    for (Cn, seed, bn, bias, eps, n, n2, o1, o2, o3, o4) in specs:
        sizes_sc += [n if o1 else 0, n2 if o3 else 0]
        sizes_sh += [n if o2 else 0, n2 if o4 else 0]
    sc_dst, sh_dst = _nan_slots(sizes_sc), _nan_slots(sizes_sh)
    jobs = (_lib.FoldJob * len(specs))()
    checks, keep = [], []
    for i, (Cn, seed, bn, bias, eps, n, n2, o1, o2, o3, o4) in enumerate(specs):
        g, be, m, v, cb = R.fold_inputs(Cn, seed)
        cb = cb if bias else None
        if not bn:
            g = be = m = v = None
        dev = [None if t is None else torch.from_numpy(t).cuda() for t in (g, be, m, v, cb)]
        keep.append(dev)
        p = [None if t is None else t.data_ptr() for t in dev]
        jobs[i] = _lib.FoldJob(gamma=p[0], beta=p[1], mean=p[2], var=p[3], conv_bias=p[4], scale=sc_dst.ptr(2 * i) if o1 else None, shift=sh_dst.ptr(2 * i) if o2 else None,
                               scale2=sc_dst.ptr(2 * i + 1) if o3 else None, shift2=sh_dst.ptr(2 * i + 1) if o4 else None, eps=eps, C=Cn, n=n, n2=n2, reserved=0)
        sc, sh = R.fold_ref64(g, be, m, v, eps, cb, n=Cn)
        bound = R.fold_shift_bound(sh, be, m, sc, cb) if bn else np.zeros(Cn)             # no BatchNorm: the bias itself
        for slot, length, on_sc, on_sh in ((2 * i, n, o1, o2), (2 * i + 1, n2, o3, o4)):
            pad = np.zeros(max(length - Cn, 0), dtype=np.float32)
            if on_sc:
                sc_dst.want(slot, np.concatenate([sc.astype(np.float32), pad]))
            if on_sh:
                sh_dst.want(slot, np.concatenate([sh.astype(np.float32), pad]))
                checks.append((slot, sh, bound))
    tab = torch.empty(C.sizeof(jobs), dtype=torch.uint8, device="cuda")
    assert L.tedspad_fold_multi(C.cast(jobs, C.c_void_p), len(specs), tab.data_ptr(), 1, E._stream_ptr()) == 0
    _check_fold(sc_dst, sh_dst, checks)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_nothing_is_written():
    _lib, L, E = _api()
    st = E._stream_ptr()
    w = torch.from_numpy(R.pack_weights((16, 16, 1, 3, 3), SEED)[0]).cuda()
    dst = _i16_slots([128 * 192] * 3)
    geo = (C.c_int32 * 9)(1, 3, 3, 0, 0, 0, 1, 1, 1)

    def pack(kpad=192, cink=16, mode=0, g=None, out=0):
        return L.tedspad_pack_conv_weights(w.data_ptr(), None, dst.ptr(out), 16, 16, 1, 3, 3, cink, 3, -1, mode, 16, 128, kpad, g, _lib.F16, st)
    assert pack(kpad=136) == EINVAL                            # K = 144 forward
    assert pack(kpad=136, mode=1, g=geo) == EINVAL             # Et*Eh*Ew*co8 = 144 data gradient
    assert pack(cink=20) == EINVAL
    assert pack(mode=1, g=None) == EINVAL
    good = dict(w=w.data_ptr(), scale=None, co=16, ci=16, kt=1, kh=3, kw=3, cink=16, kwk=3, pair_shift=-1, mode=0, rows=16, rows_pad=128, kpad=192, dtype=_lib.F16,
                block0=0, nblocks=0)
    jobs = (_lib.PackJob * 3)(*[_lib.PackJob(out=dst.ptr(i), **dict(good, kpad=136 if i == 1 else 192)) for i in range(3)])
    tab = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    assert L.tedspad_pack_multi(C.cast(jobs, C.c_void_p), 3, tab.data_ptr(), 1, st) == EINVAL
    assert dst.bits_equal(), dst.first_bad_slot()

    fdst = _nan_slots([40] * 6)
    vec = [torch.from_numpy(t).cuda() for t in R.fold_inputs(32, SEED)]

    def fold_jobs(bad):
        js = (_lib.FoldJob * 3)()
        for i in range(3):
            n, n2 = bad if i == 1 else (40, 40)
            js[i] = _lib.FoldJob(gamma=vec[0].data_ptr(), beta=vec[1].data_ptr(), mean=vec[2].data_ptr(), var=vec[3].data_ptr(), conv_bias=None, scale=fdst.ptr(2 * i),
                                 shift=fdst.ptr(2 * i + 1), scale2=fdst.ptr(2 * i), shift2=fdst.ptr(2 * i + 1), eps=1e-5, C=32, n=n, n2=n2, reserved=0)
        return js
    for bad in ((31, 40), (40, 8), (0, 0)):                    # 0 < n < C, 0 < n2 < C, no output at all
        js = fold_jobs(bad)
        assert L.tedspad_fold_multi(C.cast(js, C.c_void_p), 3, tab.data_ptr(), 1, st) == EINVAL
    assert fdst.bits_equal(), fdst.first_bad_slot()

    gdst = Slots([16 * 16 * 9] * 3, np.float32, torch.float32, -777.0)
    dw = torch.from_numpy(_accumulator(SEED, "rdw", (16, 16, 1, 3, 3), 16, 192)).cuda()
    for bad in (dict(cink=8), dict(kpad=136)):                 # cink < ci; K = 144 > kpad
        js = (_lib.WgradUnpackJob * 3)()
        for i in range(3):
            a = dict(dict(cink=16, kpad=192), **(bad if i == 1 else {}))
            js[i] = _unpack_job(_lib, dw, gdst.ptr(i), None, (16, 16, 1, 3, 3), a["cink"], a["kpad"], False)
        assert L.tedspad_wgrad_unpack_multi(C.cast(js, C.c_void_p), 3, tab.data_ptr(), 1, st) == EINVAL
    assert gdst.bits_equal(), gdst.first_bad_slot()
