"""-m gpu: the inference half of csrc/pool_layout.hip through the C ABI -- the three kernels tedspad_maxpool_fwd chooses between (LDS frame band, column walk,
generic packed), the two clip-to-channels-last kernels, channels-last to NCHW and the stride-1 average pool -- against the float64 references and case tables of
tests/kernel_refs.py (INFER_POOL_CASES, LAYOUT_CASES; tests/test_kernel_refs.py proves on the CPU which form and which solver branch every row reaches), in f16
and bf16. Inputs are channel slices of wider buffers whose other channels would win any maximum, outputs slices of sentinel-filled buffers; everything but the
average pool is compared as values with torch.equal."""
import ctypes as Ct
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:         # (run as a script: the child process of the walk-form test)
    sys.path.insert(0, ROOT)

import kernel_refs as R  # noqa: E402
from test_hip_train_kernels import DTS, In, L, Out, S, code, ok, pool_desc, within  # noqa: E402

pytestmark = pytest.mark.gpu
D = torch.float64
IDS = [c.name for c in R.INFER_POOL_CASES]
LDS_ROWS = [c for c in R.INFER_POOL_CASES if c.form == "lds"]
KNOB = "TEDSPAD_POOL_NO_LDS"


def run_pool(case, dt, x, pad_zero, idx=False):
    """One launch on `x` (n, t, h, w, c) float64: the input at channel offset 8 of a buffer c + 16 wide, the output at offset 16 of one c + 24 wide (as
    test_hip_train_kernels.run_maxpool). Returns the output as float64 and as its 16 bits."""
    nout = case.n * case.out[0] * case.out[1] * case.out[2]
    xi, y = In(x, case.c + 16, 8, R.TDT[dt]), Out(nout, case.c, case.c + 24, 16, R.TDT[dt])
    d = pool_desc(case.n, case.thw, case.c, xi.ld, y.ld, case.k, case.s, case.pf, case.out, dt)
    d.pad_zero = int(pad_zero)
    assert R.maxpool_form(d, idx=idx, no_lds=KNOB in os.environ)[0] == ("idx" if idx else case.form if KNOB not in os.environ or case.form == "generic" else "walk")
    if idx:
        ix = Out(nout, case.c, case.c, 0, torch.uint8, fill=200)
        ok(L().tedspad_maxpool_fwd_idx(Ct.byref(d), xi.ptr, y.ptr, ix.ptr, S()))
        assert ix.intact()
    else:
        ok(L().tedspad_maxpool_fwd(Ct.byref(d), xi.ptr, y.ptr, S()))
    assert y.intact(), "%s %s pad_zero=%d: wrote outside its channel slice" % (case.name, dt, pad_zero)
    shape = (case.n,) + case.out + (case.c,)
    return y.get().view(shape), y.raw().contiguous().view(torch.int16).numpy().reshape(shape)


_refs, _bits = {}, {}


def pool_ref(case, pad_zero, special=False):
    key = (case.name, bool(pad_zero), special)
    if key not in _refs:
        if (case.name, special) not in _refs:
            _refs[(case.name, special)] = R.special_values(case.x()) if special else case.x()
        _refs[key] = R.maxpool_infer_ref(_refs[(case.name, special)], case.k, case.s, case.pf, case.out, pad_zero)
    return _refs[(case.name, special)], _refs[key]


def pool_bits(case, dt, pad_zero):
    """The inference launch's output on the row's own input, checked against the reference; kept for the cross-form comparisons."""
    key = (case.name, dt, bool(pad_zero))
    if key not in _bits:
        x, ref = pool_ref(case, pad_zero)
        got, bits = run_pool(case, dt, x, pad_zero)
        assert R.first_mismatch(got, ref) == "", "%s %s pad_zero=%d (%s)" % (case.name, dt, pad_zero, R.maxpool_form(case.desc()))
        _bits[key] = bits
    return _bits[key]


@pytest.mark.parametrize("case", R.INFER_POOL_CASES, ids=IDS)
@pytest.mark.parametrize("dt", DTS)
def test_infer_pool_values_and_the_idx_kernel(dt, case):
    """Every row under the form it names (asserted from the descriptor actually passed), zero and skipped padding; then the training forward (fp32
    compare-and-select, with indices) on the same buffers: the same bits."""
    assert KNOB not in os.environ
    for pz in (0, 1):
        pool_bits(case, dt, pz)
    x, _ = pool_ref(case, 0)
    _, bits = run_pool(case, dt, x, 0, idx=True)
    assert bits.tobytes() == pool_bits(case, dt, 0).tobytes(), "the idx kernel disagrees with the %s form" % case.form


def special_check(case, dt, pz, got):
    _, ref = pool_ref(case, pz, special=True)
    what = "%s %s pad_zero=%d" % (case.name, dt, pz)
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), "%s: NaN outputs %d, reference %d" % (what, int(torch.isnan(got).sum()), int(torch.isnan(ref).sum()))
    assert R.first_mismatch(got, ref) == "", what
    for v in (float("inf"), float("-inf")):
        assert torch.equal(got == v, ref == v), what


@pytest.mark.parametrize("name", R.INFER_POOL_SPECIAL)
@pytest.mark.parametrize("dt", DTS)
def test_infer_pool_special_values(dt, name):
    """The contract of the three forms is numpy's fmax over the taps inside the input: +-inf come out unchanged, a NaN beside numbers is dropped, a window
    of NaNs alone gives NaN -- 0 where zero padding reaches it --, a window of -inf alone -inf (0 likewise). test_kernel_refs.py asserts that the planted
    values produce each of these classes on each row."""
    case = R.case_by_name(R.INFER_POOL_CASES, name)
    for pz in (0, 1):
        x, _ = pool_ref(case, pz, special=True)
        special_check(case, dt, pz, run_pool(case, dt, x, pz)[0])


def child_outputs():
    """Every LDS row under whatever form this process launches, as bits; the LDS special-value row as well."""
    out = {}
    for case in LDS_ROWS:
        for dt in DTS:
            for pz in (0, 1):
                out["%s_%s_%d" % (case.name, dt, pz)] = pool_bits(case, dt, pz)
    for name in R.INFER_POOL_SPECIAL:
        case = R.case_by_name(R.INFER_POOL_CASES, name)
        if case.form == "lds":
            for dt in DTS:
                for pz in (0, 1):
                    x, _ = pool_ref(case, pz, special=True)
                    got, bits = run_pool(case, dt, x, pz)
                    special_check(case, dt, pz, got)
                    out["special_%s_%s_%d" % (name, dt, pz)] = bits
    return out


def test_lds_rows_under_the_walk_form_bit_identical(tmp_path):
    """'Maxima are exact: bit-identical to the kernels above': TEDSPAD_POOL_NO_LDS=1 (read once per process, so one fresh child for the whole table) sends
    every LDS row through the column walk -- with seglen 1 to 4 and rows the walk's own table does not have. The child checks its outputs against the
    reference too; the bits must be this process's."""
    assert KNOB not in os.environ
    path = str(tmp_path / "walk.npz")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env={**os.environ, KNOB: "1"}, timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    walk, here = dict(np.load(path)), child_outputs()
    assert sorted(walk) == sorted(here) and len(here) >= 4 * len(LDS_ROWS) + 4
    for k in here:
        assert here[k].tobytes() == walk[k].tobytes(), k


# ---- the layouts at the module boundary ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.LAYOUT_CASES, ids=[c.name for c in R.LAYOUT_CASES])
@pytest.mark.parametrize("dt", DTS)
def test_clip_to_channels_last(dt, case):
    """fp32 (n, c, t, h, w) views of a larger non-zero clip -> 16-bit (n, t, h, w, cpad): one round-to-nearest-even per element, pad channels 0, nothing
    written behind the output. The view's strides and alignment are the ones the CPU test derived the row's form from."""
    big = R.synth_tensor(74, "lay_" + case.name, case.storage(), -1, 1).float().cuda()
    v = case.view(big)
    c, w, strides, pm = case.geometry()
    assert tuple(v.stride()) == strides and v.data_ptr() % 16 == pm and R.clip_layout_form(c, w, case.cpad, strides, pm) == case.form
    n, _, t, h, _ = v.shape
    y = Out(n * t * h * w, case.cpad, case.cpad, 0, R.TDT[dt])
    ok(L().tedspad_clip_to_channels_last(v.data_ptr(), y.ptr, n, c, t, h, w, *strides, case.cpad, code(dt), S()))
    ref = R.round_once(R.clip_layout_ref(v.cpu(), case.cpad), dt)
    got = y.get().view(n, t, h, w, case.cpad)
    assert y.intact(), "wrote behind the output"
    assert float(got[..., c:].abs().max() if c < case.cpad else 0.0) == 0.0, "pad channels"
    assert R.first_mismatch(got, ref) == "", case.name


@pytest.mark.parametrize("dt", DTS)
def test_channels_last_to_nchw(dt):
    n, t, h, w = 2, 2, 3, 5
    for c in (1, 3, 8, 24):
        x = R.synth_tensor(75, "nchw%d" % c, (n, t, h, w, c), -2, 2).to(R.TDT[dt]).to(D)
        xi = In(x, c + 5, 3, R.TDT[dt])                      # the gap holds 1000
        y = Out(n * c, t * h * w, t * h * w, 0, torch.float32)
        ok(L().tedspad_channels_last_to_nchw(xi.ptr, y.ptr, n, c, t, h, w, xi.ld, code(dt), S()))
        assert y.intact() and torch.equal(y.get().view(n, c, t, h, w), x.permute(0, 4, 1, 2, 3)), c


@pytest.mark.parametrize("dt", DTS)
def test_avgpool3d_s1_fwd_2x7x7(dt):
    """InceptionI3d's own kernel on the map equal to it and on larger ones; dyadic inputs: the fp32 sum of the 98 taps is exact, the one multiply by
    fl(1 / 98) remains -- the bound this kernel already has."""
    kt, kh, kw = 2, 7, 7
    for t, h, w in ((2, 7, 7), (3, 8, 9), (4, 7, 10)):
        for c in (8, 1024):
            x = R.dyadic(76, "a277_%d" % c, (2, t, h, w, c))
            xi = In(x, c + 8, 8, R.TDT[dt])
            to, ho, wo = t - kt + 1, h - kh + 1, w - kw + 1
            y = Out(2 * c, to * ho * wo, to * ho * wo, 0, torch.float32)
            ok(L().tedspad_avgpool3d_s1_fwd(xi.ptr, y.ptr, 2, t, h, w, c, xi.ld, kt, kh, kw, code(dt), S()))
            ref = torch.nn.functional.avg_pool3d(x.permute(0, 4, 1, 2, 3), (kt, kh, kw), 1)
            assert y.intact()
            within(y.get().view(2, c, to, ho, wo), ref, 2.0 ** -23 * ref.abs(), "avgpool3d (2, 7, 7) on %s c=%d" % ((t, h, w), c))


if __name__ == "__main__":          # the child of test_lds_rows_under_the_walk_form_bit_identical
    assert os.environ.get(KNOB) == "1"
    np.savez(sys.argv[1], **child_outputs())
