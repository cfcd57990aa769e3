"""-m gpu: torchvision's ten_crop from decoded frames in one launch (tedspad_frames_ten_crop_tp, preprocess.ten_crop_records) against the ten
tedspad_frames_crop_resize_tp launches over preprocess.ten_crop_boxes it replaces (that kernel is pinned to torch's antialiased interpolate by
tests/test_hip_feed.py), and the `crops=10` form of the two extraction drivers against the fp32-clip paths. Every comparison but the oracle's is on the raw bits."""
import ctypes

import pytest
import torch

from ted_spad_amd.synth import synth_state_dict, synth_tensor

pytestmark = pytest.mark.gpu


def _frames(t, h, w, name):
    return (synth_tensor(0, name, (t, h, w, 3)) * 256).floor().clamp(0, 255)      # integer-valued 0..255, fp32


def _bits(t):
    return t.view(torch.int16)


# (t, first, h, w, ch, cw, oh, ow, n_clips)
CASES = [
    (70, 0, 120, 160, 96, 128, 112, 112, 3),     # overlapping corner crops, aligned origins, the last clip runs past the end
    (41, 0, 97, 131, 77, 104, 64, 96, 2),        # 393-byte rows, right origin 81 B, centre origin 42 B (27 / 2 -> 14, half to even), different scales
    (16, 0, 120, 160, 48, 64, 64, 64, 1),        # disjoint corner crops with a gap between them; up-sampling, three taps
    (16, 0, 64, 96, 64, 96, 32, 48, 1),          # the crop is the frame: the five boxes coincide, only the mirrors differ
    (32, 1, 120, 160, 96, 128, 64, 64, 2),       # clip 0's last frame is the video's last: the bottom-right crop ends at the buffer's last byte; clip 1 is all zero frames
    (16, 0, 241, 321, 192, 256, 224, 224, 1),    # odd source size at the production output size
    (18, 0, 1080, 1920, 864, 1536, 224, 224, 1), # the LDS budget of the full-width row buffers
]

_STEMS, _SOURCES = {}, {}


def _stem(dtype):
    from ted_spad_amd import engine as E
    if dtype not in _STEMS:
        _STEMS[dtype] = E.StemPT(synth_tensor(3, "stemw", (64, 3, 5, 7, 7), -0.1, 0.1), torch.ones(64), torch.zeros(64), dtype=dtype, device="cuda")
    return _STEMS[dtype]


def _ten_launches(frames, h, w, ch, cw, out_hw, stem, n_clips, first, divisor=255.0):
    """The launches the fused kernel replaces: one crop_resize_records per (box, flip) of ten_crop_boxes, interleaved crop-minor."""
    from ted_spad_amd import preprocess
    per = [preprocess.crop_resize_records(frames, b[:4], out_hw, stem, n_clips, first=first, flip=b[4], divisor=divisor) for b in preprocess.ten_crop_boxes(h, w, ch, cw)]
    return torch.stack(per, dim=1).reshape((10 * n_clips,) + tuple(per[0].shape[1:]))


def _check_case(case, dtype, kinds=("u8", "f32"), divisor=255.0):
    from ted_spad_amd import preprocess
    t, first, h, w, ch, cw, oh, ow, n_clips = case
    if case not in _SOURCES:                                      # built once, shared by the storage types
        _SOURCES[case] = _frames(t, h, w, "ten%dx%d_%d" % (h, w, t))
    v = _SOURCES[case]
    stem = _stem(dtype)
    for kind in kinds:
        frames = v.to(torch.uint8).cuda() if kind == "u8" else v.cuda()
        got = preprocess.ten_crop_records(frames, (ch, cw), (oh, ow), stem, n_clips, first=first, divisor=divisor)
        want = _ten_launches(frames, h, w, ch, cw, (oh, ow), stem, n_clips, first, divisor)
        centre = preprocess.crop_resize_records(frames, preprocess.center_crop_box(h, w, ch, cw), (oh, ow), stem, n_clips, first=first, divisor=divisor)
        torch.cuda.synchronize()
        assert got.shape == want.shape == (10 * n_clips, stem.frame_pairs(16), oh, 2, ow // 2, 24) and got.dtype == want.dtype
        for k in range(10):                                       # per crop, so that a failure names it
            assert torch.equal(_bits(got[k::10]), _bits(want[k::10])), (kind, "crop %d" % k)
        assert torch.equal(_bits(got[4::10]), _bits(centre)), kind   # crop 4 is today's centre crop
        assert bool(_bits(want).any())                            # (not a comparison of zeros)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("case", CASES)
def test_ten_crop_records_equal_the_ten_launches_bit_for_bit(case, dtype):
    """uint8 and float frames, f16 and bf16 records; [4::10] is crop_resize_records on center_crop_box without a flip."""
    _check_case(case, dtype)


def test_ten_crop_records_with_another_divisor():
    """divisor 128 with uint8 frames: the workgroup's value table instead of the /255 arithmetic."""
    _check_case(CASES[1], "f16", kinds=("u8",), divisor=128.0)


def test_ten_crop_records_of_one_channel_frames_equal_those_of_zero_padded_channels():
    """C = 1: the `c < C` branches. A zero channel resamples to +0, which is what the kernel writes for c >= C: the records of (T,H,W,1) frames have the bits
    of the records of the 3-channel frames whose channels 1 and 2 are zero; uint8 and float frames (W - cw is odd: two centre column origins)."""
    from ted_spad_amd import preprocess
    v1 = (synth_tensor(0, "ten_c1", (20, 50, 70, 1)) * 256).floor().clamp(0, 255)
    v3 = torch.cat([v1, torch.zeros(20, 50, 70, 2)], dim=3)
    stem = _stem("f16")
    for cast in (lambda x: x.to(torch.uint8).cuda(), lambda x: x.cuda()):
        got = preprocess.ten_crop_records(cast(v1), (40, 57), (32, 48), stem, 1)
        want = preprocess.ten_crop_records(cast(v3), (40, 57), (32, 48), stem, 1)
        torch.cuda.synchronize()
        assert torch.equal(_bits(got), _bits(want))
        assert bool(_bits(want).any())


def test_ten_crop_records_fill_out():
    from ted_spad_amd import preprocess
    t, first, h, w, ch, cw, oh, ow, n_clips = CASES[1]
    stem = _stem("f16")
    frames = _frames(t, h, w, "ten_out").to(torch.uint8).cuda()
    out = torch.full((10 * n_clips, stem.frame_pairs(16), oh, 2, ow // 2, 24), 7.0, dtype=stem.torch_dtype, device="cuda")
    got = preprocess.ten_crop_records(frames, (ch, cw), (oh, ow), stem, n_clips, out=out)
    want = _ten_launches(frames, h, w, ch, cw, (oh, ow), stem, n_clips, 0)
    torch.cuda.synchronize()
    assert got is out and torch.equal(_bits(out), _bits(want))    # every record is written: nothing of the fill is left


# ---- features -------------------------------------------------------------------------------------------------------------------------------------------------

def _load(m):
    m.load_state_dict(synth_state_dict(m.state_dict(), 0), strict=True)
    return m.cuda().eval()


def _ten_crop_clips(frames, t_clip_idx, boxes, out_hw, layout):
    """fp32 clips of one clip time, one per (box, flip): (10, 3, 16, oh, ow) for 'cthw', (10, 16, 3, oh, ow) for 'tchw'; frames past the end stay zero."""
    from ted_spad_amd import preprocess
    shape = (10, 3, 16) + out_hw if layout == "cthw" else (10, 16, 3) + out_hw
    clips = torch.zeros(shape, device="cuda")
    sel = frames[t_clip_idx[0]:t_clip_idx[-1] + 1:2].contiguous()
    for k, b in enumerate(boxes):
        dst = clips[k, :, :len(t_clip_idx)] if layout == "cthw" else clips[k, :len(t_clip_idx)]
        preprocess.crop_resize(sel, b[:4], out_hw, flip=b[4], out=dst, layout=layout)
    return clips


def test_ten_crop_features_equal_the_fp32_clip_path_and_meet_the_gate(monkeypatch):
    """extract_video_features_uint8(crops=10) == extract_features on fp32 clips filled by crop_resize per (box, flip), bit for bit (tuner off: same tiles);
    [:, 4] is the crops=1 result; crop 6 of clip 0 (the flipped frame's bottom-left) within the 1e-3 gate of the CPU oracle on the flipped, cropped source;
    the block goes through MGFN's loader."""
    from oracle import i3res50_ref, preprocess_ref
    from ted_spad_amd import engine as E, extraction, mgfn_feed, preprocess
    from ted_spad_amd.model_loaders import load_ft_model
    monkeypatch.setattr(E, "AUTOTUNE", False)
    ft = load_ft_model("largei3d", num_classes=102)
    sd = synth_state_dict(ft.state_dict(), 0)
    ft.load_state_dict(sd)
    ft = ft.cuda().eval()
    t, h, w = 80, 120, 160
    v = _frames(t, h, w, "ten_e2e")
    frames = v.to(torch.uint8).cuda()
    got = extraction.extract_video_features_uint8(ft, frames, out_hw=(112, 112), batch=20, crops=10)
    assert got.shape == (3, 10, 2048) and got.dtype == torch.float32
    boxes = preprocess.ten_crop_boxes(h, w, 96, 128)
    clips = torch.cat([_ten_crop_clips(frames, [32 * i + 2 * f for f in range(16) if 32 * i + 2 * f < t], boxes, (112, 112), "cthw") for i in range(3)])
    with torch.no_grad():
        want = torch.cat([ft.i3d.extract_features(clips[i:i + 20]).flatten(1) for i in (0, 20)])      # the driver's forwards: 2 clip times, then 1
    one = extraction.extract_video_features_uint8(ft, frames, out_hw=(112, 112), batch=2)
    torch.cuda.synchronize()
    assert torch.equal(got.view(30, 2048), want)
    assert torch.equal(got[:, 4], one)
    # crops 6 and 7 of clip 0 -- in torchvision's order the horizontally flipped frame's top-right and bottom-left -- through the oracle's own resize of the
    # flipped, cropped source (cropping factor 1: its centre crop takes everything), one oracle forward for both
    with torch.no_grad():
        fl = v[0:32:2].flip(2)                                                            # (16, H, W, 3), mirrored
        ref_clips = [preprocess_ref.val_augmentations(s.unsqueeze(0).contiguous(), 1.0, False, 112, 112)[0].permute(1, 0, 2, 3)
                     for s in (fl[:, :96, w - 128:], fl[:, h - 96:, :128])]
        ref = i3res50_ref.extract_features(torch.stack(ref_clips), {k[4:]: x for k, x in sd.items() if k.startswith("i3d.")}).flatten(1)
    for k, r in zip((6, 7), ref):
        rel = float((got[0, k].cpu().double() - r.double()).norm() / r.double().norm())
        print("crop %d of clip 0 against the CPU oracle: rel-L2 %.3e" % (k, rel))
        assert rel < 1e-3, (k, rel)
    item = mgfn_feed.getitem(got, test_mode=True)
    assert item.shape == (3, 10, 2049)


def test_ten_crop_anonymised_features(monkeypatch):
    """extract_anonymized_video_features_uint8(crops=10), unet++ -> I3Res50: [:, 4] is the crops=1 rows; a corner crop (3, bottom-right) and a mirrored crop
    (5, the flipped frame's top-left) equal extract_anonymized_clip_features on the fp32 clips of that box and flip. The second clip holds 4 real frames."""
    from ted_spad_amd import engine as E, extraction, preprocess
    from ted_spad_amd.model_loaders import load_fa_model, load_ft_model
    monkeypatch.setattr(E, "AUTOTUNE", False)
    ft, fa = _load(load_ft_model("largei3d", num_classes=102)), _load(load_fa_model())
    t, h, w = 40, 120, 160
    frames = _frames(t, h, w, "ten_anon").to(torch.uint8).cuda()
    got = extraction.extract_anonymized_video_features_uint8(ft, fa, frames, out_hw=(112, 112), batch=2, fa_batch=2, crops=10)
    one = extraction.extract_anonymized_video_features_uint8(ft, fa, frames, out_hw=(112, 112), batch=2, fa_batch=2)
    assert got.shape == (2, 10, 2048) and one.shape == (2, 2048)
    boxes = preprocess.ten_crop_boxes(h, w, 96, 128)
    clips = torch.stack([_ten_crop_clips(frames, [32 * i + 2 * f for f in range(16) if 32 * i + 2 * f < t], boxes, (112, 112), "tchw") for i in range(2)])  # (2, 10, 16, 3, ..)
    torch.cuda.synchronize()
    assert torch.equal(got[:, 4], one)
    for k in (3, 5):
        want = extraction.extract_anonymized_clip_features(ft, fa, clips[:, k].contiguous(), batch=2, fa_batch=2)
        torch.cuda.synchronize()
        assert torch.equal(got[:, k], want), k
    assert not torch.equal(got[:, 5], got[:, 1])                  # the mirror is another clip, not the same rows


# ---- argument errors ------------------------------------------------------------------------------------------------------------------------------------------

def test_the_entry_refuses_bad_arguments_and_launches_nothing():
    from ted_spad_amd import _lib, preprocess
    from ted_spad_amd._lib import TedSpadHipError
    stem = _stem("f16")
    v = torch.zeros((20, 32, 32, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(TedSpadHipError):
        preprocess.ten_crop_records(v, (32, 40), (16, 16), stem, 1)                # wider than the frame
    with pytest.raises(TedSpadHipError):
        preprocess.ten_crop_records(v, (24, 24), (16, 15), stem, 1)                # odd output width: records hold pixel pairs
    with pytest.raises(ValueError):
        preprocess.ten_crop_records(v, (24, 24), (16, 16), stem, 1, out=torch.zeros((10, 4, 16, 2, 8, 24), device="cuda"))      # fp32 out
    with pytest.raises(TedSpadHipError):
        preprocess.ten_crop_records(v.cpu(), (24, 24), (16, 16), stem, 1)
    # the C entry by itself: the records keep their fill, i.e. nothing ran
    L = _lib.lib()
    rec = torch.full((10, 4, 16, 2, 8, 24), 7.0, dtype=torch.float16, device="cuda")
    ytab, xtab = preprocess._table(24, 16, v.device), preprocess._table(40, 16, v.device)

    def call(cw, xc, ow, xtab, dst):
        return L.tedspad_frames_ten_crop_tp(v.data_ptr(), 0, 20, 32, 32, 3, 1, 0, 32, 2, 16, 24, cw, 4, xc, 16, ow, ytab.data_ptr(), xtab.data_ptr(),
                                            ctypes.c_float(255.0), dst, stem.pad_t, stem.stride_t, 4, stem.dtype_code, None)
    assert call(40, 0, 16, xtab, rec.data_ptr()) == -1 and b"larger than" in L.tedspad_last_error()
    assert call(24, 4, 15, preprocess._table(24, 15, v.device), rec.data_ptr()) == -1 and b"even" in L.tedspad_last_error()
    assert call(24, 9, 16, preprocess._table(24, 16, v.device), rec.data_ptr()) == -1 and b"outside" in L.tedspad_last_error()      # centre origin off the frame
    assert call(24, 4, 16, preprocess._table(24, 16, v.device), rec.data_ptr() + 2) == -1 and b"16-byte aligned" in L.tedspad_last_error()
    torch.cuda.synchronize()
    assert bool((rec == 7.0).all())
