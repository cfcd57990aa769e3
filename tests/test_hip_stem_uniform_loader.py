"""-m gpu: the fp32-clip stem's loader waves with one (frame, half) per WAVE (csrc/conv_stem_pt.hip, UNI: scalar plane guards, buffer loads) against
(a) the per-lane task deal (variant bit 3 of tedspad_stem_pt_pool_clip_fwd), bit for bit, and (b) the float64 stem reference of tests/kernel_refs.py on integer
clips, bit for bit -- at the smallest shapes that reach every guard of the loader: rows above and below the frame, column quads past the right edge, a ragged
second patch row, an odd height, both temporal paddings, clips of one and two channels, strided clips, and values that saturate the 16-bit type.

The entry is called with the test's own y and side buffers, both followed by a sentinel region that must come back untouched."""
import ctypes as C
import functools

import pytest
import torch

import kernel_refs as R

pytestmark = pytest.mark.gpu
DTYPES = ("f16", "bf16")
PER_LANE = 8                   # variant bit 3
SENTINEL = 12288.0             # exact in f16 and bf16
TAIL = 4096                    # sentinel elements behind y / bytes behind side
# n, c, t, h, w
CASES = [(2, 3, 4, 20, 24),    # one column strip, a ragged second patch row (ho = 10), column quads past the right edge, halo rows above and below the frame
         (2, 3, 8, 36, 72),    # three patch columns (the pooled seam) and two frame pairs: the front and the back temporal padding
         (2, 3, 4, 21, 24),    # odd height
         (2, 1, 4, 20, 24),    # the channel guard
         (2, 2, 4, 20, 24)]
IDS = ["x".join(map(str, c)) for c in CASES]


@functools.lru_cache(maxsize=None)
def reference(case, dtype):
    """kernel_refs.stem_reference with the conditions of an exact comparison asserted: all of kernel_refs.fused_conditions on the conv and the pair max; on the
    pooled tensor exact fp32 sums and no saturation as well, but for its liveness this file's own bound: at most half zeros and some (a pooled tensor of five
    columns moves in steps of a fifth, and the clip's dark part leaves it one zero column). Shared, never modified."""
    d, (conv, pair, pool) = R.stem_reference(case, dtype)
    assert R.bn_is_telling(d["s"], d["b"])
    R.fused_conditions([conv, pair], dtype, "stem uniform loader " + "x".join(map(str, case)))
    assert R.exact_in_fp32_steps(pool["abs"], pool["step"]) and float(pool["y"].abs().max()) < 65504.0
    zeros = float((pool["y"] == 0).double().mean())
    assert 0.1 <= zeros <= 0.5, "the pooled reference is %.0f %% zeros" % (100 * zeros)
    return d, pool["y"]


def stem_of(d, dtype):
    from ted_spad_amd import engine as E
    return E.StemPT(d["w"].float(), d["s"].float(), d["b"].float(), stride=(2, 2, 2), pads=(2, 3, 3), dtype=dtype, device="cuda")


def run(st, x, variant, fails, what):
    """tedspad_stem_pt_pool_clip_fwd into y and side buffers of the test's own, each with a sentinel tail: (n, 64, tp, hp, wp) float64 cpu."""
    from ted_spad_amd import _lib, engine as E
    assert st.direct_applies(x)
    n, c, t, h, w = x.shape
    tp = st.frame_pairs(t)
    ho, wo = (h + 1) // 2, w // 2
    hp, wp = (ho - 3) // 2 + 1, (wo - 3) // 2 + 1
    ny = n * tp * hp * wp * 64
    nside = _lib.lib().tedspad_stem_pt_side_bytes(n, tp, h, w)
    assert nside > 0 and nside % 2 == 0
    y = torch.full((ny + TAIL,), SENTINEL, dtype=st.torch_dtype, device="cuda")
    side = torch.full((nside + TAIL,), 0xA5, dtype=torch.uint8, device="cuda")
    sn, sc, s_t, sh, sw = x.stride()
    E.check(_lib.lib().tedspad_stem_pt_pool_clip_fwd(x.data_ptr(), n, c, t, h, w, sn, sc, s_t, sh, sw, st.pad_t, st.stride_t, tp, st.wimg16.data_ptr(),
                                                     st.scale.data_ptr(), st.shift.data_ptr(), y.data_ptr(), side.data_ptr(), hp, wp, 64, st.nwg, variant,
                                                     st.dtype_code, E._stream_ptr()), "tedspad_stem_pt_pool_clip_fwd")
    torch.cuda.synchronize()
    if not bool((y[ny:] == SENTINEL).all()):
        fails.append(what + ": the sentinel behind y was overwritten")
    if not bool((side[nside:] == 0xA5).all()):
        fails.append(what + ": the sentinel behind side was overwritten")
    return y[:ny].view(n, tp, hp, wp, 64).double().cpu().permute(0, 4, 1, 2, 3)


def both(st, x, what, fails, want=None):
    """The two task deals on x: equal to each other, and to `want` where there is an exact reference."""
    uni = run(st, x, 0, fails, what + " uniform")
    lane = run(st, x, PER_LANE, fails, what + " per-lane")
    R.same(uni, lane, what + ": uniform against per-lane", fails)
    if want is not None:
        R.same(uni, want, what + ": uniform against the reference", fails)
        R.same(lane, want, what + ": per-lane against the reference", fails)
    return uni


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_uniform_loader_equals_per_lane_loader_and_reference(case, dtype):
    d, want = reference(case, dtype)
    fails = []
    both(stem_of(d, dtype), d["clip"].float().cuda(), "stem %s %s" % ("x".join(map(str, case)), dtype), fails, want)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("dtype", DTYPES)
def test_uniform_loader_on_strided_clips(dtype):
    """A non-contiguous T-slice of a longer clip, inside a batch whose stride is larger than a sample (a spare channel): every other element holds a non-zero
    integer, so a plane or a row fetched from the wrong place shows."""
    case = CASES[0]
    n, c, t, h, w = case
    d, want = reference(case, dtype)
    big = torch.full((n, c + 1, t + 8, h, w), 3.0, device="cuda")
    big[:, :c, 4:4 + t] = d["clip"].float().cuda()
    view = big[:, :c, 4:4 + t]
    assert not view.is_contiguous() and view.stride(0) > c * view.stride(1) and view.stride(1) > t * view.stride(2)
    fails = []
    both(stem_of(d, dtype), view, "stem on a strided view %s" % dtype, fails, want)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("dtype", DTYPES)
def test_uniform_loader_saturates_like_per_lane_loader(dtype):
    """Entries of +-1e6 (one in 16, every frame edge and the interior alike): beyond f16, so the loader's conversion saturates; the two deals must agree bit for bit,
    and the result is finite."""
    case = CASES[0]
    d, _ = reference(case, dtype)
    clip = d["clip"].float().clone()
    g = torch.Generator().manual_seed(7)
    hit = torch.rand(clip.shape, generator=g) < 1.0 / 16
    sign = torch.where(torch.rand(clip.shape, generator=g) < 0.5, -1.0, 1.0)
    clip = torch.where(hit, sign * 1e6, clip)
    clip[0, 0, 0, 0, 0], clip[-1, -1, -1, -1, -1] = 1e6, -1e6
    fails = []
    out = both(stem_of(d, dtype), clip.cuda(), "stem on +-1e6 %s" % dtype, fails)
    assert bool(torch.isfinite(out).all()) and float((out == 0).double().mean()) <= 0.5
    assert not fails, "\n".join(fails)
