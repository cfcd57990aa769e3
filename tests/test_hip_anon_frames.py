"""-m gpu: decoded frames -> the anonymizer's 16-bit input activation in one launch (tedspad_frames_crop_resize_act / _pil_act, preprocess.crop_resize_act),
the anonymizers' forward from that activation (forward_act) and extraction.extract_anonymized_video_features_uint8, each against the chain of pre-existing
calls it replaces. Every comparison is on the raw bits."""
import pytest
import torch

from ted_spad_amd.synth import synth_state_dict, synth_tensor

pytestmark = pytest.mark.gpu

T_CLIP = 16


def _frames(t, h, w, c, name):
    return (synth_tensor(0, name, (t, h, w, c)) * 256).floor().clamp(0, 255)          # integer-valued 0..255, fp32


def _bits(t):
    return t.view(torch.int16)


def _source(i, f, first, clip_step, frame_step):
    return first + i * clip_step + f * frame_step


_FP32 = {}


def _fp32_frames(key, frames, box, out_hw, n_clips, first, clip_step, frame_step, flip, divisor, resample="aa"):
    """The pre-existing path's fp32 frames (n_clips * 16, C, oh, ow): crop_resize / crop_resize_pil of the frames that exist, zeros for those past the end.
    Built once per input and shared by the storage types and layouts compared against it."""
    from ted_spad_amd import preprocess
    if key not in _FP32:
        t, c = frames.shape[0], frames.shape[3]
        x = torch.zeros((n_clips * T_CLIP, c, out_hw[0], out_hw[1]), device="cuda")
        for i in range(n_clips):
            idx = [_source(i, f, first, clip_step, frame_step) for f in range(T_CLIP)]
            live = [s for s in idx if s < t]
            if not live:
                continue
            sel = frames[torch.tensor(live, device="cuda")].contiguous()
            dst = x[i * T_CLIP:i * T_CLIP + len(live)]
            if resample == "aa":
                preprocess.crop_resize(sel, box, out_hw, flip=flip, out=dst, divisor=divisor)
            else:
                preprocess.crop_resize_pil(sel, box, out_hw, out=dst)
        _FP32[key] = x
    return _FP32[key]


def _check_act(act, want_x, cpad, dtype, c, dead_frames):
    from ted_spad_amd import engine as E
    want = E.clip_to_act(want_x.unsqueeze(2), cpad=cpad, dtype=dtype)
    torch.cuda.synchronize()
    n, _, oh, ow = want_x.shape
    assert act.dims == want.dims == (n, 1, oh, ow // 2 if cpad == 4 else ow)
    assert act.buf.dtype == want.buf.dtype and act.c == 8 and act.cpad == cpad
    assert torch.equal(_bits(act.buf), _bits(want.buf))
    px = _bits(act.buf).reshape(n, oh, ow, cpad)
    assert not px[..., c:].any()                                 # the padded channel(s)
    for f in dead_frames:
        assert not px[f].any()                                   # a frame past the end of the video is an all-zero block


AA_CASES = [(70, 120, 160, 112, 112, False), (41, 96, 130, 64, 96, True), (16, 241, 321, 224, 224, False), (5, 33, 47, 48, 64, False)]


@pytest.mark.parametrize("cpad", [4, 8])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("case", AA_CASES)
def test_act_from_frames_equals_crop_resize_then_clip_to_act(case, dtype, cpad):
    """HybridValPipe's sampling (a clip per 32 frames, every 2nd frame): uint8 and float frames, divisor 255 and 200, an odd source width with a crop whose
    rows start off a 4-byte boundary, a last clip with missing frames, a flip, up-sampling with three taps."""
    from ted_spad_amd import preprocess
    t, h, w, oh, ow, flip = case
    v = _frames(t, h, w, 3, "act%d" % t)
    box = preprocess.center_crop_box(h, w, int(h * 0.8), int(w * 0.8))
    n_clips = -(-t // 32)
    dead = [i * T_CLIP + f for i in range(n_clips) for f in range(T_CLIP) if _source(i, f, 0, 32, 2) >= t]
    assert dead
    for kind, frames in (("u8", v.to(torch.uint8).cuda()), ("f32", v.cuda())):
        for divisor in (255.0, 200.0):
            want_x = _fp32_frames((case, kind, divisor), frames, box, (oh, ow), n_clips, 0, 32, 2, flip, divisor)
            act = preprocess.crop_resize_act(frames, box, (oh, ow), n_clips, cpad=cpad, dtype=dtype, flip=flip, divisor=divisor)
            _check_act(act, want_x, cpad, dtype, 3, dead)


@pytest.mark.parametrize("cpad", [4, 8])
@pytest.mark.parametrize("sampling", [(3, 8, 1, 4, 3), (7, 32, 2, 2, 3), (30, 32, 2, 2, 3), (0, 20, 3, 3, 1), (2, 5, 2, 6, 1)])
def test_act_sampling_first_overlap_and_single_channel(sampling, cpad):
    """A non-zero `first`, a clip_step shorter than a clip (overlapping clips), a clip that lies wholly past the end, one-channel frames; `out=` is filled."""
    from ted_spad_amd import engine as E, preprocess
    first, clip_step, frame_step, n_clips, c = sampling
    t, h, w, oh, ow = 41, 50, 70, 32, 48
    v = _frames(t, h, w, c, "samp%d" % c)
    box = (3, 5, 40, 57)                                         # x0 * c off a 4-byte boundary for c = 1 and 3
    dead = [i * T_CLIP + f for i in range(n_clips) for f in range(T_CLIP) if _source(i, f, first, clip_step, frame_step) >= t]
    assert dead
    for kind, frames in (("u8", v.to(torch.uint8).cuda()), ("f32", v.cuda())):
        want_x = _fp32_frames((sampling, kind), frames, box, (oh, ow), n_clips, first, clip_step, frame_step, False, 255.0)
        out = torch.full((n_clips * T_CLIP, 1, oh, ow // 2 if cpad == 4 else ow, 8), 7.0, dtype=E.DTYPES["f16"][0], device="cuda")
        act = preprocess.crop_resize_act(frames, box, (oh, ow), n_clips, first=first, clip_step=clip_step, frame_step=frame_step, cpad=cpad, dtype="f16", out=out)
        assert act.buf is out
        _check_act(act, want_x, cpad, "f16", c, dead)


@pytest.mark.parametrize("cpad,dtype", [(4, "f16"), (8, "bf16"), (4, "bf16"), (8, "f16")])
@pytest.mark.parametrize("case", [(40, 97, 131, 64, 64), (33, 224, 224, 224, 224)])
def test_pil_act_equals_crop_resize_pil_then_clip_to_act(case, cpad, dtype):
    """The Shanghai loader's frames (first = 1, every 2nd frame, 32 source frames per clip) through Pillow's resample; the last clip runs past the end."""
    import numpy as np
    from ted_spad_amd import preprocess
    t, h, w, oh, ow = case
    rng = np.random.default_rng(h * 10007 + w)
    fr = rng.integers(0, 256, (t, h, w, 3), dtype=np.uint8)
    fr[1] = (np.add.outer(np.arange(h), np.arange(w))[..., None] * np.array([1, 2, 3])) % 256          # smooth ramps: the rounding ties
    frames = torch.from_numpy(fr).cuda()
    side, _ = preprocess.shanghai_crop_size(h, w, 3)
    box = preprocess.center_crop_box(h, w, side, side)
    n_clips = 2
    dead = [i * T_CLIP + f for i in range(n_clips) for f in range(T_CLIP) if _source(i, f, 1, 32, 2) >= t]
    assert dead
    want_x = _fp32_frames((case, "pil"), frames, box, (oh, ow), n_clips, 1, 32, 2, False, 255.0, resample="pil")
    act = preprocess.crop_resize_act(frames, box, (oh, ow), n_clips, first=1, clip_step=32, frame_step=2, cpad=cpad, dtype=dtype, resample="pil")
    _check_act(act, want_x, cpad, dtype, 3, dead)


# ---- forward_act ------------------------------------------------------------------------------------------------------------------------------------------

def _load(m):
    m.load_state_dict(synth_state_dict(m.state_dict(), 0), strict=True)
    return m.cuda().eval()


@pytest.fixture(scope="module")
def unetpp():
    from ted_spad_amd.model_loaders import load_fa_model
    return _load(load_fa_model())


@pytest.fixture(scope="module")
def unet():
    from ted_spad_amd.model_loaders import load_fa_model
    return _load(load_fa_model(arch="unet"))


@pytest.fixture(scope="module")
def wrapper():
    from ted_spad_amd.model_loaders import load_ft_model
    return _load(load_ft_model("largei3d", num_classes=102))


@pytest.mark.parametrize("gather", [True, False])
def test_unetpp_forward_act_equals_forward(unetpp, gather, monkeypatch):
    from ted_spad_amd import engine as E
    monkeypatch.setattr(E, "AUTOTUNE", False)
    monkeypatch.setattr(E, "GATHER_CAT", gather)
    x = synth_tensor(0, "fwd_act", (3, 3, 64, 96)).cuda()
    with torch.no_grad():
        want = unetpp(x)
        got = unetpp.forward_act(E.clip_to_act(x.unsqueeze(2), cpad=4, dtype=unetpp.compute_dtype))
    torch.cuda.synchronize()
    assert got.shape == want.shape == (3, 3, 64, 96) and got.dtype == torch.float32
    assert torch.equal(got, want)


def test_unet_forward_act_equals_forward(unet, monkeypatch):
    from ted_spad_amd import engine as E
    monkeypatch.setattr(E, "AUTOTUNE", False)
    x = synth_tensor(0, "fwd_act", (3, 3, 64, 96)).cuda()
    with torch.no_grad():
        want = unet(x)
        got = unet.forward_act(E.clip_to_act(x.unsqueeze(2), cpad=8, dtype=unet.compute_dtype))
    torch.cuda.synchronize()
    assert got.shape == want.shape == (3, 3, 64, 96) and got.dtype == torch.float32
    assert torch.equal(got, want)


def test_forward_act_rejections(unetpp, unet, monkeypatch):
    from ted_spad_amd import engine as E
    monkeypatch.setattr(E, "AUTOTUNE", False)
    x = torch.zeros((1, 3, 32, 32), device="cuda")
    for net, cpad, other in ((unetpp, 4, 8), (unet, 8, 4)):
        good = E.clip_to_act(x.unsqueeze(2), cpad=cpad, dtype=net.compute_dtype)
        with pytest.raises(ValueError):
            net.forward_act(E.clip_to_act(x.unsqueeze(2), cpad=cpad, dtype="bf16" if net.compute_dtype == "f16" else "f16"))      # the other storage type
        with pytest.raises(ValueError):
            net.forward_act(E.clip_to_act(x.unsqueeze(2), cpad=other, dtype=net.compute_dtype))      # the other network's padded-channel count
        with pytest.raises(TypeError):
            net.forward_act(x)                                                               # a tensor is forward's argument
        net.train()
        try:
            with pytest.raises(RuntimeError):
                net.forward_act(good)
        finally:
            net.eval()
    bad = E.clip_to_act(torch.zeros((1, 3, 1, 40, 64), device="cuda"), cpad=4, dtype=unetpp.compute_dtype)
    with pytest.raises(RuntimeError, match="Wrong input shape height=40, width=64. Expected image height and width divisible by 16."):
        unetpp.forward_act(bad)


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------------------

def _e2e_frames():
    return _frames(80, 120, 160, 3, "anon_e2e").to(torch.uint8).cuda()


@pytest.mark.parametrize("layout", ["reference", "permute"])
def test_anonymised_features_from_uint8_frames_equal_the_fp32_clip_path(wrapper, unetpp, layout, monkeypatch):
    """extract_anonymized_video_features_uint8 == val_augmentations per clip into (n, 16, 3, h, w) with zeros past the end -> extract_anonymized_clip_features,
    bit for bit (tuner off: same tiles). Clip 2 holds 8 real and 8 zero frames; the zero frames go through fa, whose output for a black frame is not black."""
    from ted_spad_amd import engine as E, extraction, preprocess
    monkeypatch.setattr(E, "AUTOTUNE", False)
    frames = _e2e_frames()
    t = frames.shape[0]
    got = extraction.extract_anonymized_video_features_uint8(wrapper, unetpp, frames, out_hw=(112, 112), batch=2, fa_batch=2, layout=layout)
    assert got.shape == (3, 2048) and got.dtype == torch.float32
    clips = torch.zeros((3, 16, 3, 112, 112), device="cuda")
    for i in range(3):
        idx = [32 * i + 2 * f for f in range(16) if 32 * i + 2 * f < t]
        aug = preprocess.val_augmentations(frames[idx[0]:idx[-1] + 1:2].unsqueeze(0).contiguous(), reso_h=112, reso_w=112)      # (1, T', 3, 112, 112)
        clips[i, :len(idx)] = aug[0]
    assert len(idx) == 8
    want = extraction.extract_anonymized_clip_features(wrapper, unetpp, clips, batch=2, fa_batch=2, layout=layout)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    # what the row would be had the 8 frames past the end skipped fa (zeros behind it instead of fa(black))
    with torch.no_grad():
        fr = torch.zeros((16, 3, 112, 112), device="cuda")
        fr[:8] = unetpp(clips[2, :8])
        x = fr.reshape(1, 3, 16, 112, 112) if layout == "reference" else fr.reshape(1, 16, 3, 112, 112).permute(0, 2, 1, 3, 4)
        skipped = wrapper.i3d.extract_features(x).flatten(1)
    torch.cuda.synchronize()
    assert not torch.equal(got[2:3], skipped)
    assert float((got[2:3] - skipped).abs().max()) > 0 and bool(got[2].abs().sum() > 0)


def test_anonymised_features_pil_path_with_unet(wrapper, unet, monkeypatch):
    """The Shanghai loader's path (Pillow resample, frames 1, 3, 5, ...; whole clips only) with the UNet anonymizer."""
    from ted_spad_amd import engine as E, extraction, preprocess
    monkeypatch.setattr(E, "AUTOTUNE", False)
    frames = _e2e_frames()
    got = extraction.extract_anonymized_video_features_uint8(wrapper, unet, frames, out_hw=(112, 112), first=1, clip_step=32, batch=2, fa_batch=1, resample="pil")
    assert got.shape == (2, 2048)                                # frames 1 .. 31 and 33 .. 63; the third clip would need frame 95
    clips = torch.stack([preprocess.shanghai_augmentation(frames[1 + 32 * i:32 + 32 * i:2], reso_h=112, reso_w=112) for i in range(2)])      # (2, 16, 3, 112, 112)
    want = extraction.extract_anonymized_clip_features(wrapper, unet, clips, batch=2, fa_batch=1)
    torch.cuda.synchronize()
    assert torch.equal(got, want)


def test_anonymised_features_with_inception_i3d(unet, monkeypatch):
    """The other encoder the scripts accept (arch 'i3d': 1024 features), at the 224 x 224 its pooling needs."""
    from ted_spad_amd import engine as E, extraction, preprocess
    from ted_spad_amd.model_loaders import load_ft_model
    monkeypatch.setattr(E, "AUTOTUNE", False)
    ft = _load(load_ft_model("i3d", num_classes=102))
    frames = _frames(40, 120, 160, 3, "anon_i3d").to(torch.uint8).cuda()
    got = extraction.extract_anonymized_video_features_uint8(ft, unet, frames, batch=2, fa_batch=1)
    assert got.shape == (2, 1024)
    clips = torch.zeros((2, 16, 3, 224, 224), device="cuda")
    clips[0] = preprocess.val_augmentations(frames[0:32:2].unsqueeze(0).contiguous())[0]
    clips[1, :4] = preprocess.val_augmentations(frames[32:40:2].unsqueeze(0).contiguous())[0]
    want = extraction.extract_anonymized_clip_features(ft, unet, clips, batch=2, fa_batch=1)
    torch.cuda.synchronize()
    assert torch.equal(got, want)


# ---- argument errors --------------------------------------------------------------------------------------------------------------------------------------

def test_crop_resize_act_rejects_bad_arguments():
    from ted_spad_amd import _lib, preprocess
    from ted_spad_amd._lib import TedSpadHipError
    v = torch.zeros((20, 32, 32, 3), dtype=torch.uint8, device="cuda")
    for resample in ("aa", "pil"):
        with pytest.raises(TedSpadHipError):
            preprocess.crop_resize_act(v, (0, 0, 40, 32), (16, 16), 1, resample=resample)                # box outside the frame
        with pytest.raises(ValueError):
            preprocess.crop_resize_act(v, (0, 0, 32, 32), (16, 15), 1, cpad=4, resample=resample)       # odd width: cpad 4 holds pixel pairs
        preprocess.crop_resize_act(v, (0, 0, 32, 32), (16, 15), 1, cpad=8, resample=resample)           # cpad 8 takes it
        with pytest.raises(ValueError):
            preprocess.crop_resize_act(v, (0, 0, 32, 32), (16, 16), 1, resample=resample, out=torch.zeros((16, 1, 16, 8, 8), device="cuda"))        # fp32 out
        with pytest.raises(ValueError):
            preprocess.crop_resize_act(v, (0, 0, 32, 32), (16, 16), 1, resample=resample, out=torch.zeros((16, 1, 16, 16, 8), dtype=torch.float16, device="cuda"))
        with pytest.raises(TedSpadHipError):
            preprocess.crop_resize_act(v.cpu(), (0, 0, 32, 32), (16, 16), 1, resample=resample)          # no CPU path
    with pytest.raises(ValueError):
        preprocess.crop_resize_act(v.float(), (0, 0, 32, 32), (16, 16), 1, resample="pil")               # PIL images are 8-bit
    with pytest.raises(ValueError):
        preprocess.crop_resize_act(v, (0, 0, 32, 32), (16, 16), 1, cpad=6)
    # the C entry refuses the same by itself: an odd width for pixel pairs, a misaligned activation
    L, out = _lib.lib(), torch.zeros(16 * 16 * 16 * 4 + 8, dtype=torch.float16, device="cuda")
    ytab, xtab = preprocess._table(32, 16, v.device), preprocess._table(32, 15, v.device)
    import ctypes
    assert L.tedspad_frames_crop_resize_act(v.data_ptr(), 0, 20, 32, 32, 3, 1, 0, 32, 2, 16, 0, 0, 32, 32, 16, 15, ytab.data_ptr(), xtab.data_ptr(),
                                            ctypes.c_float(255.0), 0, out.data_ptr(), 4, 0, None) != 0
    assert b"even" in L.tedspad_last_error()
    xtab = preprocess._table(32, 16, v.device)
    assert L.tedspad_frames_crop_resize_act(v.data_ptr(), 0, 20, 32, 32, 3, 1, 0, 32, 2, 16, 0, 0, 32, 32, 16, 16, ytab.data_ptr(), xtab.data_ptr(),
                                            ctypes.c_float(255.0), 0, out.data_ptr() + 2, 4, 0, None) != 0
    assert b"16-byte aligned" in L.tedspad_last_error()


def test_extract_anonymized_video_rejects_bad_arguments(wrapper, unetpp):
    from ted_spad_amd import extraction
    from ted_spad_amd._lib import TedSpadHipError
    frames = torch.zeros((32, 24, 32, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(TypeError):
        extraction.extract_anonymized_video_features_uint8(wrapper, torch.nn.Identity(), frames, out_hw=(16, 16))       # an anonymizer without forward_act
    with pytest.raises(TedSpadHipError):
        extraction.extract_anonymized_video_features_uint8(wrapper, unetpp, frames.cpu(), out_hw=(16, 16))
    with pytest.raises(ValueError):
        extraction.extract_anonymized_video_features_uint8(wrapper, unetpp, frames, out_hw=(16, 16), out=torch.zeros((1, 1024), device="cuda"))
    with pytest.raises(ValueError):
        extraction.extract_anonymized_video_features_uint8(wrapper, unetpp, frames, out_hw=(16, 16), layout="transpose")
