"""-m gpu: the non-local attention kernels (csrc/nonlocal.hip: the fused forward, its LSE form, the three backward launches) through the C ABI at every
remainder their code branches on, on inputs whose right answer is known bit for bit (tests/nl_exact.py; tests/test_nl_exact_host.py holds the
construction itself to its claims on the CPU).

What "bit for bit" means here: every result is compared as the VALUE its 16 bits hold against the closed form rounded once, element by element. A NaN
differs from everything; the two zeros compare equal, because which of them a sum of exact zeros ends on depends on the order of the terms (a tile whose mass
alpha = 0 wipes leaves -0 where it was negative), and the order is the one thing the construction leaves open. `fwd` against `fwd_lse`, and an item alone
against the same item in a batch, are compared as raw bits.

Two properties of the hardware are assumed, as tests/test_hip_nl_bwd.py's one-key and equal-logits tests already do: exp2(0) == 1 in v_exp_f32, and an fp32
division of an integer by a power of two is exact."""
import ctypes as C

import pytest
import torch

import nl_exact as X
import nl_grad_ref
import nl_ref
from test_hip_nl import SENTINEL, fwd_bound
from test_hip_nl_bwd import LSE_GUARD, dg_bound, lse_bound, run
from ted_spad_amd.synth import synth_tensor

pytestmark = pytest.mark.gpu
GRADS = ("dtheta", "dphi", "dg")
# every operand on a stride of its own (all multiples of 8): phi | g in one buffer with 16 unused channels between the slices and 16 behind them,
# dphi | dg likewise with 32 and 24
own_strides = lambda d: dict(theta=d + 8, dt=d + 24, t=d + 16, dtheta=d + 40, pg=(2 * d + 32, d + 16), dpg=(2 * d + 56, d + 32))


def differences(shape, key, got, want):
    """None, or one line: the shape, the tensor, how many elements differ and the first of them as (item, row, channel) with both values."""
    got = got.reshape(want.shape)
    bad = got != want                                        # float64 values of 16-bit numbers: NaN != anything, -0 == +0
    if not bool(bad.any()):
        return None
    b, r, c = (int(v) for v in torch.nonzero(bad)[0])
    return "(q, k) = %s %s: %d of %d elements differ, first at (item %d, row %d, channel %d): got %r, want %r" % (
        shape, key, int(bad.sum()), bad.numel(), b, r, c, float(got[b, r, c]), float(want[b, r, c]))


def want64(e, key, dtype):
    return e[key].float().to(X.STORAGE[dtype]).double()      # one rounding


def exact_failures(shape, r, e, dtype, keys):
    out = []
    for key in keys:
        out.append(differences(shape, key, r[key + "64"], want64(e, key, dtype)))
    if "t" in keys:
        if not torch.equal(r["t"], r["t0"]):
            out.append("(q, k) = %s: fwd and fwd_lse differ in %d elements" % (shape, int((r["t"] != r["t0"]).sum())))
        err, bound = (r["lse"] - e["lse"]).abs(), lse_bound(e["lse"])
        if not bool((err <= bound).all()):                   # a NaN fails this too
            b, i = (int(v) for v in torch.nonzero(~(err <= bound))[0])
            out.append("(q, k) = %s lse: %d rows past the bound, first at (item %d, row %d): got %r, want %r" % (
                shape, int((~(err <= bound)).sum()), b, i, float(r["lse"][b, i]), float(e["lse"][b, i])))
    return [s for s in out if s]


def run_exact(q, k, d, dtype, **kw):
    c, e = X.case(q, k, d)
    return run(c["theta"], c["phi"], c["g"], c["dt"], dtype, False, scale=c["scale"], **kw), c, e


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("d", X.WIDTHS)
def test_every_tile_edge_bit_for_bit(d, dtype):
    """The sweep: forward, LSE forward and the backward from the kernel's own T and lse, as the training path runs them."""
    fails = []
    for q, k in X.SHAPES:
        try:
            r, c, e = run_exact(q, k, d, dtype)
        except AssertionError as ex:                         # a guard or a padding was written: report it with the rest
            fails.append("(q, k) = %s: %s" % ((q, k), ex))
            continue
        fails += exact_failures((q, k), r, e, dtype, ("t",) + GRADS)
    assert not fails, "%d findings:\n%s" % (len(fails), "\n".join(fails))


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("d", X.WIDTHS)
def test_backward_from_a_host_tape(d, dtype):
    """The backward alone: T (exact) and lse (float64 rounded to fp32) come from the host, so a forward kernel that is wrong cannot hide or cause a difference."""
    fails = []
    for q, k in X.HOST_TAPE_SHAPES:
        c, e = X.case(q, k, d)
        try:
            r = run_exact(q, k, d, dtype, tape=(X.bits(e["t"], dtype), X.lse_fp32(c)))[0]
        except AssertionError as ex:
            fails.append("(q, k) = %s: %s" % ((q, k), ex))
            continue
        fails += exact_failures((q, k), r, e, dtype, GRADS)
    assert not fails, "%d findings:\n%s" % (len(fails), "\n".join(fails))


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("d", X.WIDTHS)
def test_every_operand_on_its_own_stride(d, dtype):
    """Every operand on another padded stride, phi | g and dphi | dg as slices of shared buffers, and a quiet NaN in every input's padding, guard rows and
    unused channels: anything read from there reaches a result as NaN (0 x NaN is NaN in the MFMA). The same bits must come out, the outputs' padding
    and guards stay untouched (run() asserts that), and item 1 alone gives the bits it has in the batch."""
    fails = []
    for q, k in X.STRIDE_SHAPES:
        c, e = X.case(q, k, d)
        try:
            r = run_exact(q, k, d, dtype, ld=own_strides(d), poison=True)[0]
            alone = run(c["theta"][1:], c["phi"][1:], c["g"][1:], c["dt"][1:], dtype, False, scale=c["scale"], ld=own_strides(d), poison=True)
        except AssertionError as ex:
            fails.append("(q, k) = %s: %s" % ((q, k), ex))
            continue
        fails += exact_failures((q, k), r, e, dtype, ("t",) + GRADS)
        for key, rows in (("t", q), ("dtheta", q), ("dphi", k), ("dg", k)):
            if not torch.equal(alone[key], r[key][rows:]):
                fails.append("(q, k) = %s %s: item 1 alone differs from item 1 in the batch in %d elements" % ((q, k), key, int((alone[key] != r[key][rows:]).sum())))
        if not torch.equal(alone["lse"][0], r["lse"][1]):
            fails.append("(q, k) = %s lse: item 1 alone differs from item 1 in the batch" % ((q, k),))
    assert not fails, "%d findings:\n%s" % (len(fails), "\n".join(fails))


# ---- general values on the same edges: fractional rescaling on remainder tiles, at the bounds the stored shapes are held to -----------------

def general_case(q, k, d, dtype, n=X.N_ITEMS):
    """The recipe of test_hip_nl.case / test_hip_nl_bwd.upstream at an arbitrary (q, k): theta, phi on the 2^-4 grid in [-2, 2], g and dT uniform in
    [-1, 1) rounded to the storage type."""
    tdt = X.STORAGE[dtype]
    tag = "nl_edge/%d/%d/%d/" % (q, k, d)
    grid = lambda name, rows: torch.floor(synth_tensor(7, tag + name, (n, rows, d)) * 65.0 - 32.0) / 16.0
    unif = lambda name, rows: synth_tensor(7, tag + name, (n, rows, d), -1.0, 1.0).to(tdt).float()
    return grid("theta", q), grid("phi", k), unif("g", k), unif("dt", q)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("d", X.WIDTHS)
def test_general_values_within_the_derived_bounds(d, dtype):
    fails, worst = [], dict(t=0.0, lse=0.0, dg=0.0)
    for q, k in X.SHAPES:
        theta, phi, g, dt = general_case(q, k, d, dtype)
        scale = float(d) ** -0.5
        try:
            r = run(theta, phi, g, dt, dtype, False)
        except AssertionError as ex:
            fails.append("(q, k) = %s: %s" % ((q, k), ex))
            continue
        ref = nl_grad_ref.attention_grads(theta, phi, g, dt, scale)
        assert torch.equal(r["t"], r["t0"])
        for key, got, want, bound in (("t", r["t64"], nl_ref.attention(theta, phi, g, scale), fwd_bound(g, dtype).expand(-1, q, -1)),
                                      ("lse", r["lse"], ref["lse"], lse_bound(ref["lse"])),
                                      ("dg", r["dg64"], ref["dg"], dg_bound(ref, dt, dtype))):
            err = (got - want).abs()
            ratio = float((err / bound.clamp_min(1e-30)).max())
            worst[key] = max(worst[key], ratio)
            if not bool((err <= bound).all()):
                fails.append("(q, k) = %s %s: |err| up to %.3f of its bound at %d elements" % ((q, k), key, ratio, int((~(err <= bound)).sum())))
        for key in GRADS:
            if not bool(torch.isfinite(r[key + "64"]).all()):
                fails.append("(q, k) = %s %s: not finite" % ((q, k), key))
    print("d = %d %s over %d shapes: worst |err| / bound: forward %.3f, lse %.3f, dg %.3f" % (d, dtype, len(X.SHAPES), worst["t"], worst["lse"], worst["dg"]))
    assert not fails, "%d findings:\n%s" % (len(fails), "\n".join(fails))


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------

FWD = ("theta", "ld_theta", "phi", "ld_phi", "g", "ld_g", "out", "ld_out", "n", "q", "k", "d", "scale", "dtype", "stream")
FWD_LSE = FWD[:8] + ("lse",) + FWD[8:]
BWD = ("theta", "ld_theta", "phi", "ld_phi", "g", "ld_g", "t", "ld_t", "dt", "ld_dt", "lse", "dtheta", "ld_dtheta", "dphi", "ld_dphi", "dg", "ld_dg",
       "workspace", "n", "q", "k", "d", "scale", "dtype", "stream")
BWD_PTRS = ("theta", "phi", "g", "t", "dt", "dtheta", "dphi", "dg")        # the order of the entry's `argument %d`


def test_bad_arguments_are_refused_and_nothing_is_written():
    """Every TS_REQUIRE of nl_forward, tedspad_nl_attention_fwd_lse, tedspad_nl_attention_bwd and _bwd_workspace but the 2^31 size limits. Every operand sits
    in the middle of an allocation of 64 + n max(q, k) + 64 rows of 2 d + 64 channels, so that a launch wrongly let through -- with a negative count, a short
    or odd stride, a pointer off by an element, an output on top of an input -- would stay inside memory this test owns."""
    from ted_spad_amd import _lib
    from ted_spad_amd.engine import _stream_ptr
    lib, sp = _lib.lib(), _stream_ptr()
    n, q, k, d = 2, 5, 3, 256
    slack, width = 64, 2 * d + 64
    rows = 2 * slack + n * max(q, k)
    ins = {key: torch.zeros((rows, width), dtype=torch.int16, device="cuda") for key in ("theta", "phi", "g", "t", "dt")}
    outs = {key: torch.full((rows, width), SENTINEL, dtype=torch.int16, device="cuda") for key in ("out", "dtheta", "dphi", "dg")}
    flt = {key: torch.full((4 * slack,), LSE_GUARD, dtype=torch.float32, device="cuda") for key in ("lse", "workspace")}
    ptr = {key: t.data_ptr() + slack * width * 2 for key, t in list(ins.items()) + list(outs.items())}
    ptr.update({key: t.data_ptr() + slack * 4 for key, t in flt.items()})
    base = dict(ptr, n=n, q=q, k=k, d=d, scale=2.0 ** -4, dtype=_lib.F16, stream=sp)
    base.update({"ld_" + key: d + 8 for key in ("theta", "phi", "g", "out", "t", "dt", "dtheta", "dphi", "dg")})
    entries = {"tedspad_nl_attention_fwd": FWD, "tedspad_nl_attention_fwd_lse": FWD_LSE, "tedspad_nl_attention_bwd": BWD}

    def call(entry, **change):
        a = dict(base, **change)
        return getattr(lib, entry)(*[C.c_float(a[key]) if key == "scale" else a[key] for key in entries[entry]])

    def untouched():
        ok = all(bool((t == SENTINEL).all()) for t in outs.values()) and all(bool((t == LSE_GUARD).all()) for t in flt.values())
        return ok and all(not bool(t.any()) for t in ins.values())

    # the harness itself: the unchanged arguments are accepted and do write
    for entry in ("tedspad_nl_attention_fwd", "tedspad_nl_attention_fwd_lse", "tedspad_nl_attention_bwd"):
        _lib.check(call(entry), entry)
    torch.cuda.synchronize()
    assert not untouched()
    for t in outs.values():
        t.fill_(SENTINEL)
    for t in flt.values():
        t.fill_(LSE_GUARD)
    assert untouched()

    cases = []                                               # (entry, changed arguments, the text of the check that must refuse them)
    bad, dtype_msg, rows_msg = ": bad arguments (n=", ": f16 / bf16 storage only (dtype=", ": rows must hold d channels, 16-byte aligned"
    for entry, names in entries.items():
        bwd = entry.endswith("_bwd")
        pointers = [key for key in names if key in ptr]
        for key in pointers:
            null_msg = entry + (": lse must be an fp32 (n, q) buffer" if key == "lse" and not bwd else bad)
            cases.append((entry, {key: None}, null_msg))
        for key in ("n", "q", "k"):
            for v in (0, -1):
                cases.append((entry, {key: v}, entry + bad))
        for v in (_lib.F32, -1, 7):
            cases.append((entry, {"dtype": v}, entry + dtype_msg + "%d)" % v))
        cases.append((entry, {"d": 128}, entry + ": no kernel for d = 128"))
        for key in [key for key in names if key.startswith("ld_")]:
            which = " (argument %d: ld " % BWD_PTRS.index(key[3:]) if bwd else ""
            for v in (d - 8, d + 4):
                cases.append((entry, {key: v}, entry + rows_msg + (", an item below 2^31 elements" + which + "%d)" % v if bwd else "")))
        for key in pointers:
            if key in ("lse", "workspace"):
                off_msg = entry + (": lse and the workspace are fp32 buffers" if bwd else ": lse must be an fp32 (n, q) buffer")
            else:
                off_msg = entry + rows_msg + (", an item below 2^31 elements (argument %d: ld " % BWD_PTRS.index(key) if bwd else "")
            cases.append((entry, {key: ptr[key] + 2}, off_msg))
        for v in (float("inf"), float("-inf"), float("nan")):
            cases.append((entry, {"scale": v}, entry + ": too large (n=%d q=%d k=%d) or a non-finite scale" % (n, q, k)))
        if not bwd:
            for key in ("theta", "phi", "g"):
                cases.append((entry, {"out": ptr[key]}, entry + ": out must not alias an input"))
        else:
            for o in (5, 6, 7):
                for i in range(8):
                    if i != o:                               # the entry reports the first pair in its own order: outputs 5, 6, 7 against arguments 0 .. 7
                        pair = (o, i) if i < 5 else (min(o, i), max(o, i))
                        cases.append((entry, {BWD_PTRS[o]: ptr[BWD_PTRS[i]]}, entry + ": an output must not alias another argument (%d, %d)" % pair))
    fails = []
    for entry, change, text in cases:
        try:
            _lib.check(call(entry, **change), entry)
            fails.append("%s%r: accepted" % (entry, change))
        except _lib.TedSpadHipError as ex:
            if text not in str(ex):
                fails.append("%s%r: refused with %r, not by the check %r" % (entry, change, str(ex), text))
        torch.cuda.synchronize()
        if not untouched():
            fails.append("%s%r: something was written" % (entry, change))
            break                                            # nothing after this could be told apart
    nbytes = C.c_int64(-7)
    for args in ((n, q, None), (0, q, C.byref(nbytes)), (n, 0, C.byref(nbytes)), (-1, q, C.byref(nbytes)), (n, -1, C.byref(nbytes))):
        rc = lib.tedspad_nl_attention_bwd_workspace(*args)
        msg = (lib.tedspad_last_error() or b"").decode()
        if rc == 0 or "tedspad_nl_attention_bwd_workspace: bad arguments (n=" not in msg or nbytes.value != -7:
            fails.append("workspace%r: rc %d, %r, bytes %d" % (args[:2], rc, msg, nbytes.value))
    print("%d refusals checked" % (len(cases) + 5))
    assert len(cases) > 120 and not fails, "\n".join(fails)
