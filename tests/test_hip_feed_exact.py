"""-m gpu: the frame-feed kernels (csrc/feed.hip) per element against the float64 host references of tests/feed_refs.py -- no kernel is compared with another.
Exact elements (uint8 / integer frames, divisor 256, dyadic weights; identity at divisor 255) must EQUAL the reference, in fp32 and after its one rounding to
f16 / bf16 (ties to even); the other elements must lie within k * 2^-24 relative of it, k = ytaps + xtaps + 4, and a 16-bit value between the roundings of the
two ends. tests/test_feed_refs.py holds the conditions of both and shows that each mistake of feed_refs.WRONG fails this file's comparison (feed_refs.verdict).
Every output is written into the middle of a sentinel-filled buffer: the guards stay, nothing inside keeps the fill.

What no earlier test reached, and the case (feed_refs.CASES / PIL_CASES) that now does:
  t_clip 8 and 6, their tp_n + 1 quads and pair skips   up2_wide, down4, b5, b_up (8: two pairs); up4, corners, tail_s*, b7, b9 (6: one pair);
                                                           ident255, down2 keep 16
  first < 0 in the record entries (zero frames in front)  ident255, up2_wide, down2, down4, tail_s*, b7, b_up
  an output width above 256 (second trip of `ox += 256`)  up2_wide (260 columns), pil_wide (264)
  C = 2 / C = 4 (fp32 forms); C = 4 refused elsewhere     down2, b5 / c4_up2, c4_b; test_records_and_activations_refuse_four_channels
  divisor 256 and 200, float frames                        every exact row (256); b9, b_up (200); every case runs uint8 and float frames
  the u8_px shortcut for 255, all 256 byte values          ident255
  uint8 buffers 1, 2, 3 bytes past a dword, ending inside  tail_s0 .. tail_s3 (1485 bytes; the bottom-right crop of the last frame ends the buffer);
  a dword                                                  rows at every alignment: up4 (21-byte rows), x0 * C = 1, 2, 3 mod 4: ident255, up2_wide, corners
  the 16-bit rounding, ties to even                        every exact row against kernel_refs.round_once (17 .. 22 % f16 ties on the x2 rows)
  the Pillow forms off the Shanghai loader's box           pil_wide, pil_c1, pil_sq
  T * oh >= 2^31 in tedspad_frames_crop_resize             test_crop_resize_refuses_a_grid_past_2_31

Measured on an MI355X (worst |got - ref| / (ref * 2^-24) over the bounded elements of the fp32 form, uint8 and float frames alike, beside the derived k; a 16-bit
entry has no error of its own to measure, its figure is the share of elements off the reference's own rounding, i.e. inside the interval but not at its centre):
  fp32 form, worst error / k:  down2 (ring) 2.52 / 14, down4 (ring) 2.64 / 22, c4_b 2.39 / 14, b5 2.61 / 14, b7 2.72 / 18, b9 3.30 / 22, b_up 2.99 / 10;
                               0 on every exact element (equality is asserted there)
  records      f16 0.024 %, bf16 0.005 %      ten-crop     f16 0.024 %, bf16 0.009 %
  activations  cpad 4: f16 0.016 %, bf16 0.005 %; cpad 8: f16 0.008 %, bf16 0.002 %      (the worst case each; the cap on the interval's width is 2 %)
  Nothing failed: the kernels and preprocess.py needed no fix beyond the grid check of tedspad_frames_crop_resize."""
import ctypes
import math

import numpy as np
import pytest
import torch

import feed_refs as R
import kernel_refs as K

pytestmark = pytest.mark.gpu

D = torch.float64
GUARD = 64                                                   # elements either side of an output: 16-byte multiples in every output type
SENTINEL = R.SENTINEL16
_STEMS = {}


def _stem(dtype):
    from ted_spad_amd import engine as E
    if dtype not in _STEMS:
        _STEMS[dtype] = E.StemPT(torch.zeros(64, 3, 5, 7, 7), None, None, dtype=dtype, device="cuda")
    return _STEMS[dtype]


def _gpu_frames(c, kind):
    """uint8: buf[s:s+n].view(T,H,W,C) of a buffer of s + n bytes; float: the same integer values as fp32."""
    fr = c.frames()
    if kind == "f32":
        return torch.from_numpy(fr.astype(np.float32)).cuda()
    s, n = getattr(c, "shift", 0), fr.size
    buf = torch.empty(s + n, dtype=torch.uint8, device="cuda")
    buf[s:].copy_(torch.from_numpy(fr.reshape(-1)))
    v = buf[s:s + n].view(fr.shape)
    assert v.data_ptr() % 4 == s and v.is_contiguous()
    return v


def _guarded(shape, tdt):
    n = math.prod(shape)
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=tdt, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(shape)


def _intact(buf, view, what):
    n = view.numel()
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all()), "%s: wrote outside its output" % what
    assert not bool((view == SENTINEL).any()), "%s: an element inside kept the fill" % what


def _fp32_both_ways(fn, T, C, oh, ow, what):
    """The fp32 forms: (T,C,oh,ow) into a guarded buffer, and a (C,T,oh,ow) clip through a strided view of a larger sentinel-filled tensor. Returns both as
    (T,C,oh,ow) float64 on the host."""
    buf, view = _guarded((T, C, oh, ow), torch.float32)
    fn(view, "tchw")
    _intact(buf, view, what)
    big = torch.full((C + 1, T + 2, oh + 1, ow + 3), SENTINEL, dtype=torch.float32, device="cuda")
    clip = big[:C, 1:T + 1, :oh, 2:ow + 2]
    fn(clip, "cthw")
    torch.cuda.synchronize()
    assert not bool((clip == SENTINEL).any()), "%s: an element of the strided view kept the fill" % what
    rest = big.clone()
    rest[:C, 1:T + 1, :oh, 2:ow + 2] = SENTINEL
    assert bool((rest == SENTINEL).all()), "%s: wrote outside the strided view" % what
    return view.cpu().to(D), clip.permute(1, 0, 2, 3).cpu().to(D)


def _run(c, entry, dtype, frames):
    """One launch of `entry` into guarded storage; the result as float64 on the host, in the layout of feed_refs.ends (a list: the fp32 form writes twice)."""
    from ted_spad_amd import engine as E, preprocess
    n_clips, first, clip_step, frame_step, t_clip = c.samp_of(entry)
    what = "%s %s %s" % (c.name, entry, dtype)
    if entry == "fp32":
        T, C = c.thwc[0], c.C
        return list(_fp32_both_ways(lambda out, layout: preprocess.crop_resize(frames, c.box, c.out, flip=c.flip, out=out, layout=layout, divisor=c.divisor),
                                    T, C, c.out[0], c.out[1], what))
    oh, ow = c.out
    if entry in ("rec", "ten"):
        stem = _stem(dtype)
        assert stem.frame_pairs(t_clip) == R.frame_pairs(t_clip) and stem.pad_t == R.STEM_PAD_T
        shape = ((10 if entry == "ten" else 1) * n_clips, R.frame_pairs(t_clip), oh, 2, ow // 2, 24)
        buf, view = _guarded(shape, stem.torch_dtype)
        if entry == "rec":
            preprocess.crop_resize_records(frames, c.box, c.out, stem, n_clips, first=first, clip_step=clip_step, frame_step=frame_step, t_clip=t_clip, flip=c.flip,
                                           out=view, divisor=c.divisor)
        else:
            preprocess.ten_crop_records(frames, c.box[2:], c.out, stem, n_clips, first=first, clip_step=clip_step, frame_step=frame_step, t_clip=t_clip, out=view,
                                        divisor=c.divisor)
    else:
        cpad = int(entry[3])
        buf, view = _guarded((n_clips * t_clip, 1, oh, ow // 2 if cpad == 4 else ow, 8), E.DTYPES[dtype][0])
        act = preprocess.crop_resize_act(frames, c.box, c.out, n_clips, first=first, clip_step=clip_step, frame_step=frame_step, t_clip=t_clip, cpad=cpad,
                                         dtype=dtype, flip=c.flip, divisor=c.divisor, out=view)
        assert act.buf is view and act.cpad == cpad
    torch.cuda.synchronize()
    _intact(buf, view, what)
    return [view.cpu().to(D)]


_RUNS = [(c, e) for c in R.CASES for e in c.entries]


@pytest.mark.parametrize("c,entry", _RUNS, ids=["%s-%s" % (c.name, e) for c, e in _RUNS])
def test_antialiased_entries_against_the_host_reference(c, entry):
    """Every antialiased entry on every row of the table, uint8 and float frames, f16 and bf16: feed_refs.verdict per element."""
    fails = []
    for kind in ("u8", "f32"):
        frames = _gpu_frames(c, kind)
        for dtype in ((None,) if entry == "fp32" else ("f16", "bf16")):
            for got in _run(c, entry, dtype, frames):
                msg = R.verdict(c, entry, dtype, got)
                if entry == "fp32":
                    print("\n%s fp32 %s: worst %.2f units of 2^-24, k = %d" % (c.name, kind, R.worst_units(c, entry, got), R.bound_k(c.box, c.out)))
                else:
                    centre = R.round16(R.ends(c, entry)[0], dtype)
                    print("\n%s %s %s %s: %.5f of %d elements off the reference's own rounding" % (c.name, entry, dtype, kind, float((got != centre).double().mean()),
                                                                                                 got.numel()))
                if msg:
                    fails.append(kind + " " + msg)
    assert not fails, "\n".join(fails)


def test_the_librarys_weight_table_has_the_references_bits():
    """preprocess.aa_table_host against feed_refs.aa_table (torch's rule restated in fp32) for every size pair of the table: first index, count, weight bits."""
    from ted_spad_amd import preprocess
    pairs = {(c.box[2], c.out[0]) for c in R.CASES} | {(c.box[3], c.out[1]) for c in R.CASES} | {(864, 224), (1536, 224), (9, 27), (3, 5)}
    for n_in, n_out in sorted(pairs):
        tab = preprocess.aa_table_host(n_in, n_out)
        first, count, w = R.aa_table(n_in, n_out)
        assert tab.shape == (n_out, 2 + R.aa_taps(n_in, n_out)), (n_in, n_out)
        assert np.array_equal(tab[:, 0], first) and np.array_equal(tab[:, 1], count) and np.array_equal(tab[:, 2:], w.view(np.int32)), (n_in, n_out)


# ---- the Pillow forms ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.PIL_CASES, ids=[c.name for c in R.PIL_CASES])
def test_pillow_forms_equal_pillow(c):
    """crop_resize_pil (both output layouts) and crop_resize_act(resample="pil") at cpad 4 / 8 in f16 / bf16: torch.equal to Pillow's own resize of the cropped
    array / 255, and to its one rounding in the case's clip sampling."""
    from ted_spad_amd import engine as E, preprocess
    frames = _gpu_frames(c, "u8")
    T, C = c.thwc[0], c.thwc[3]
    oh, ow = c.out
    ref = R.pil_ref(c)
    for got in _fp32_both_ways(lambda out, layout: preprocess.crop_resize_pil(frames, c.box, c.out, out=out, layout=layout), T, C, oh, ow, c.name):
        assert K.first_mismatch(got, ref) == "", c.name
    n_clips, first, clip_step, frame_step, t_clip = c.samp
    for cpad in (4, 8):
        for dtype in ("f16", "bf16"):
            want = K.round_once(R.pil_ref(c, cpad), dtype)
            buf, view = _guarded(tuple(want.shape), E.DTYPES[dtype][0])
            preprocess.crop_resize_act(frames, c.box, c.out, n_clips, first=first, clip_step=clip_step, frame_step=frame_step, t_clip=t_clip, cpad=cpad, dtype=dtype,
                                       resample="pil", out=view)
            torch.cuda.synchronize()
            _intact(buf, view, "%s act%d %s" % (c.name, cpad, dtype))
            assert K.first_mismatch(view.cpu().to(D), want) == "", (c.name, cpad, dtype)
            assert bool((want != 0).any()) and bool((want.reshape(-1, cpad)[:, C:] == 0).all())


# ---- refusals: the host rejects the call before any launch -------------------------------------------------------------------------------------------------------
def _refused(fn, buf, entry):
    from ted_spad_amd import _lib
    from ted_spad_amd._lib import TedSpadHipError
    with pytest.raises(TedSpadHipError):
        fn()
    torch.cuda.synchronize()
    assert entry + b":" in _lib.lib().tedspad_last_error(), _lib.lib().tedspad_last_error()
    assert bool((buf == SENTINEL).all()), "%s launched" % entry.decode()


def test_records_and_activations_refuse_four_channels():
    """C = 4 is the fp32 forms' alone (cmax 4 against 3); the output keeps its fill and tedspad_last_error names the entry."""
    from ted_spad_amd import preprocess
    v = torch.zeros((6, 12, 16, 4), dtype=torch.uint8, device="cuda")
    stem = _stem("f16")
    buf, view = _guarded((1, 1, 8, 2, 4, 24), stem.torch_dtype)
    _refused(lambda: preprocess.crop_resize_records(v, (0, 0, 8, 8), (8, 8), stem, 1, t_clip=6, out=view), buf, b"tedspad_frames_crop_resize_tp")
    buf, view = _guarded((10, 1, 8, 2, 4, 24), stem.torch_dtype)
    _refused(lambda: preprocess.ten_crop_records(v, (8, 8), (8, 8), stem, 1, t_clip=6, out=view), buf, b"tedspad_frames_ten_crop_tp")
    for cpad in (4, 8):
        buf, view = _guarded((6, 1, 8, 8 // 2 if cpad == 4 else 8, 8), torch.float16)
        _refused(lambda: preprocess.crop_resize_act(v, (0, 0, 8, 8), (8, 8), 1, t_clip=6, cpad=cpad, dtype="f16", out=view), buf, b"tedspad_frames_crop_resize_act")
        _refused(lambda: preprocess.crop_resize_act(v, (0, 0, 8, 8), (8, 8), 1, t_clip=6, cpad=cpad, dtype="f16", resample="pil", out=view), buf,
                 b"tedspad_frames_crop_resize_pil_act")


def test_activations_refuse_frames_in_front_of_the_video():
    """first < 0: the record entries give zero frames (the table's first_lt0 rows), the activation entries refuse."""
    from ted_spad_amd import preprocess
    v = torch.zeros((6, 12, 16, 3), dtype=torch.uint8, device="cuda")
    buf, view = _guarded((6, 1, 8, 8, 8), torch.float16)
    _refused(lambda: preprocess.crop_resize_act(v, (0, 0, 8, 8), (8, 8), 1, first=-1, t_clip=6, cpad=8, dtype="f16", out=view), buf, b"tedspad_frames_crop_resize_act")
    _refused(lambda: preprocess.crop_resize_act(v, (0, 0, 8, 8), (8, 8), 1, first=-1, t_clip=6, cpad=8, dtype="f16", resample="pil", out=view), buf,
             b"tedspad_frames_crop_resize_pil_act")


def test_crop_resize_refuses_a_grid_past_2_31():
    """T * oh >= 2^31 does not fit the grid's 32-bit block index: both fp32 forms refuse before any launch (the C entries by themselves: T is only a number
    here, no frame is read), the output keeps its fill and tedspad_last_error names the entry."""
    from ted_spad_amd import _lib, preprocess
    L = _lib.lib()
    v = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device="cuda")
    T, oh, ow = 70_000_000, 32, 8
    assert T * oh >= 2 ** 31 and T < 2 ** 31
    buf, view = _guarded((2, 3, oh, ow), torch.float32)
    ytab, xtab = preprocess._table(8, oh, v.device), preprocess._table(8, ow, v.device)
    rc = L.tedspad_frames_crop_resize(v.data_ptr(), 0, T, 8, 8, 3, 0, 0, 8, 8, oh, ow, ytab.data_ptr(), xtab.data_ptr(), ctypes.c_float(255.0), 0, view.data_ptr(),
                                      3 * oh * ow, oh * ow, ow, 1, None)
    assert rc == -1 and b"tedspad_frames_crop_resize:" in L.tedspad_last_error() and b"do not fit" in L.tedspad_last_error(), L.tedspad_last_error()
    (ytab, ky), (xtab, kx) = preprocess._pil_table(8, oh, v.device), preprocess._pil_table(8, ow, v.device)
    rc = L.tedspad_frames_crop_resize_pil(v.data_ptr(), T, 8, 8, 3, 0, 0, 8, 8, oh, ow, ytab.data_ptr(), ky, xtab.data_ptr(), kx, view.data_ptr(),
                                          3 * oh * ow, oh * ow, ow, 1, None)
    assert rc == -1 and b"tedspad_frames_crop_resize_pil:" in L.tedspad_last_error()
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())
