"""GPU: tedspad_clip_augment (csrc/augment.hip, ted_spad_amd/augment.py) against Pillow itself (tests/augment_ref.py). Everything is BIT-equal
(torch.equal): the reference chain runs on 8-bit PIL images, so there is no tolerance anywhere in this file."""
import json
import os
import types

import numpy as np
import pytest
import torch

import augment_ref
from conftest import GOLDEN_DIR
from ted_spad_amd import augment as A
from ted_spad_amd import preprocess as PP
from ted_spad_amd._lib import TedSpadHipError

pytestmark = pytest.mark.gpu

R = A.frame_record


def random_video(t, h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(t, h, w, 3)).astype(np.uint8)


def ramp_video(t, h, w, seed):
    """smooth ramps: resample sums that land on rounding ties, slowly varying colours"""
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    fr = [np.stack([(xx * 2 + k + seed) % 256, (yy * 3 + xx + 2 * k) % 256, ((xx + yy) // 2 + 128 * k) % 256], axis=-1) for k in range(t)]
    return np.stack(fr).astype(np.uint8)


def check(videos, records, reso):
    """one launch == Pillow, record by record; returns the device result"""
    dev = [torch.from_numpy(v).cuda() for v in videos]
    got = A.augment_batch(dev, records, reso=reso)
    ref = augment_ref.apply_records(videos, records, reso)
    assert got.shape == ref.shape and got.dtype == torch.float32
    got = got.cpu()
    for b in range(ref.shape[0]):
        for k in range(ref.shape[1]):
            assert torch.equal(got[b, k], ref[b, k]), "record (%d, %d): %r, %d bytes differ" % (
                b, k, records[b][k], int((got[b, k] != ref[b, k]).sum()))
    return got


def op_records(box):
    """each op alone, the factors at which a fused multiply-add would change bytes (0.93, 1.1), and whole chains"""
    e2 = [(3, 5, 9, 6), (20, 17, 12, 30)]
    recs = [R(0, box)]
    recs += [R(0, box, contrast=f) for f in (0.93, 1.1)] + [R(1, box, contrast=f, contrast_late=True) for f in (0.93, 1.1)]
    recs += [R(0, box, saturation=f) for f in (0.93, 1.1)] + [R(1, box, brightness=f) for f in (0.9, 1.1)]
    recs += [R(0, box, hue=f) for f in (-0.05, 0.031)]
    recs += [R(1, box, gray=True), R(1, box, gray=True, gamma=0.85), R(0, box, gray=True, gamma=1.15)]
    recs += [R(0, box, reverse=True), R(1, box, hflip=True), R(1, box, reverse=True, hflip=True, saturation=1.1)]
    recs += [R(0, box, contrast=1.1, hue=0.04, brightness=1.1), R(0, box, contrast=1.1, contrast_late=True, hue=0.04, brightness=1.1)]      # 17, 18
    recs += [R(1, box, contrast=0.93, hue=-0.03, saturation=0.93, brightness=0.9, gray=True, gamma=0.85, hflip=True, erase=e2),
             R(1, box, contrast=1.1, contrast_late=True, hue=0.05, saturation=1.1, brightness=1.1, gray=True, gamma=1.15, hflip=True, erase=e2),
             R(0, box, contrast=1.1, hue=0.05, saturation=1.1, brightness=1.1, hflip=True, erase=e2, reverse=True),
             R(0, box, contrast=0.93, contrast_late=True, hue=-0.05, saturation=0.93, brightness=0.9, erase=e2)]
    return recs


@pytest.mark.parametrize("make", [random_video, ramp_video], ids=["random", "ramp"])
@pytest.mark.parametrize("h,w,reso", [(97, 131, 28), (240, 320, 112), (240, 320, 224)])
def test_each_op_and_full_chain(make, h, w, reso):
    video = make(2, h, w, 5)
    box = (h // 13, w // 11, int(h * 0.73), int(w * 0.73))
    recs = op_records(box)
    got = check([video], [recs], (reso, reso))
    assert not torch.equal(got[0, 17], got[0, 18])          # contrast before hue / after brightness: two different results, each matched above


@pytest.mark.parametrize("factor", [-0.05, -0.0123, 0.0, 0.031, 0.05])
def test_hue_over_every_colour(factor):
    """512 frames of 128 x 256 hold all 2^24 colours; the box is the whole frame and the output has its size, so the resample is the identity."""
    c = np.arange(1 << 24, dtype=np.uint32)
    frames = np.stack([c >> 16, (c >> 8) & 255, c & 255], axis=-1).astype(np.uint8).reshape(512, 128, 256, 3)
    dev = torch.from_numpy(frames).cuda()
    recs = [[R(k, (0, 0, 128, 256), hue=factor) for k in range(512)]]
    got = A.augment_batch([dev], recs, reso=(128, 256))
    from PIL import Image
    ref = np.array(augment_ref.adjust_hue(Image.fromarray(frames.reshape(512 * 128, 256, 3), "RGB"), factor), dtype=np.uint8)
    ref = torch.from_numpy(ref.reshape(512, 128, 256, 3)).permute(0, 3, 1, 2).contiguous()
    value = (torch.arange(256, dtype=torch.float32) / 255).cuda()          # to_tensor's 256 possible values, divided on the CPU
    assert torch.equal(got[0], value[ref.cuda().long()])
    if factor == 0.0:
        plain = A.augment_batch([dev], [[R(k, (0, 0, 128, 256)) for k in range(512)]], reso=(128, 256))
        assert torch.equal(plain[0], value[dev.permute(0, 3, 1, 2).long()])          # identity resample
        assert not torch.equal(plain, got)          # (the HSV round trip itself is lossy)


def test_contrast_mean_at_a_tie_and_on_a_constant_frame():
    tie = np.full((1, 28, 28, 3), 10, np.uint8)
    tie[0, 14:] = 11                                # luma 10 on one half, 11 on the other: mean 10.5 -> int(mean + 0.5) = 11
    const = np.full((1, 28, 28, 3), 77, np.uint8)
    box = (0, 0, 28, 28)
    recs = [[R(0, box, contrast=f, contrast_late=late, video=v) for v in (0, 1) for f in (0.93, 1.1, 0.5) for late in (False, True)]]
    got = check([tie, const], recs, (28, 28))
    d = 11 + np.float32(0.5) * np.float32(10 - 11)
    assert int(got[0, 4, 0, 0, 0] * 255 + 0.5) == int(d)          # blend(11, 10, 0.5) truncates 10.5


def test_boxes_overflowing_and_degenerate():
    video = random_video(1, 97, 131, 2)
    boxes = [(10, 60, 50, 100), (60, 10, 70, 50), (50, 70, 80, 90), (96, 130, 30, 30), (0, 0, 97, 131), (0, 0, 98, 132),
             (40, 20, 1, 60), (40, 20, 60, 1), (96, 130, 1, 1), (5, 5, 28, 28)]
    recs = [[R(0, b) for b in boxes] + [R(0, b, contrast=1.1, hue=0.031, hflip=True) for b in boxes[:3]]]
    check([video], recs, (28, 28))


def test_erase_boxes():
    video = ramp_video(1, 60, 80, 1)
    box = (2, 3, 50, 70)
    cases = [[(0, 0, 5, 6)], [(25, 20, 10, 30)], [(20, 25, 30, 10)], [(27, 0, 4, 28)], [(0, 27, 28, 4)], [(27, 27, 19, 19)],
             [(3, 3, 10, 10), (8, 8, 10, 10)], [(5, 1, 6, 9), (5, 1, 6, 9)], [(0, 0, 40, 40)], [(4, 4, 0, 5), (4, 4, 5, 0)]]
    recs = [[R(0, box, erase=e) for e in cases] + [R(0, box, hflip=True, erase=e) for e in cases]]
    got = check([video], recs, (28, 28))
    assert not torch.equal(got[0, 0].flip(-1), got[0, len(cases)])          # erase comes after the flip: the box does not move with it


def test_ragged_batch_into_a_strided_out():
    """two videos of different resolution in one launch, three 16-frame clips each written where AnonymizerTrainStep wants them, `out` a strided
    view: nothing outside the frames is touched"""
    p = types.SimpleNamespace(num_frames=16, fix_skip=2, reso_h=28, reso_w=28, min_crop_factor_training=0.6, weak_aug=False, no_ar_distortion=False,
                              aspect_ratio_aug=False, temporal_loss="trip", temporal_align=False, temporal_distance=None)
    videos = [augment_ref.synthetic_video(40, 97, 131, 11), augment_ref.synthetic_video(64, 240, 320, 12)]
    records = []
    for v, video in enumerate(videos):
        lists, clips = A.sample_contrastive(np.random.RandomState(100 + v), p, *video.shape[:3])
        row = [dict(r, video=v) for clip in clips for r in clip]
        assert len(row) == 48
        records.append(row)
    base = torch.full((2, 50, 3, 30, 33), -7.0, dtype=torch.float32, device="cuda")
    out = base[:, 1:49, :, 1:29, 2:30]
    ret = A.augment_batch([torch.from_numpy(v).cuda() for v in videos], records, out=out, reso=(28, 28))
    assert ret is out
    ref = augment_ref.apply_records(videos, records, (28, 28))
    assert torch.equal(out.cpu(), ref)
    mask = torch.ones_like(base, dtype=torch.bool)
    mask[:, 1:49, :, 1:29, 2:30] = False
    assert bool((base[mask] == -7.0).all())


def test_all_ops_off_equals_crop_resize_pil():
    video = torch.from_numpy(random_video(4, 240, 320, 9)).cuda()
    for box, reso in (((12, 40, 180, 240), (112, 112)), ((0, 0, 240, 320), (224, 224)), ((30, 20, 144, 192), (28, 40))):
        want = PP.crop_resize_pil(video, box, reso)
        got = A.augment_batch([video], [[R(k, box) for k in range(4)]], reso=reso)
        assert torch.equal(got[0], want)


@pytest.mark.parametrize("name", ["weak_trip", "strong_trip", "strong_single", "frame_wise", "no_ar_distortion", "aspect_ratio_aug", "short_video"])
def test_fixture_clips(name):
    """the clips the reference's loaders returned (tests/golden/make_aug_golden.py), from the same seed; twice gives the same bits"""
    with open(os.path.join(GOLDEN_DIR, "aug_golden_meta.json")) as f:
        meta = json.load(f)
    case = [c for c in meta["cases"] if c["name"] == name][0]
    clips = torch.from_numpy(np.load(os.path.join(GOLDEN_DIR, "aug_golden.npz"))[name + "_clips"])
    params = types.SimpleNamespace(**case["params"])
    t, h, w, _ = case["video"]
    rs = np.random.RandomState(case["seed"])
    if case["loader"] == "contrastive":
        records = A.sample_contrastive(rs, params, t, h, w, frame_wise_aug=case["frame_wise_aug"])[1]
    else:
        records = [A.sample_single(rs, params, t, h, w, frame_wise_aug=case["frame_wise_aug"])[1]]
    video = torch.from_numpy(augment_ref.synthetic_video(*case["video"])).cuda()
    reso = tuple(meta["reso"])
    got = A.augment_batch([video], records, reso=reso)
    again = A.augment_batch([video], records, reso=reso)
    assert torch.equal(got.cpu(), clips.to(torch.float32).div(255))
    assert torch.equal(got, again)


def test_bad_arguments_raise():
    video = torch.from_numpy(random_video(2, 60, 80, 0)).cuda()
    ok = [[R(0, (0, 0, 40, 40))]]
    with pytest.raises(ValueError):
        A.augment_batch([video], [[R(0, (-1, 0, 40, 40))]], reso=(28, 28))
    with pytest.raises(ValueError):
        A.augment_batch([video], [[R(0, (0, -2, 40, 40))]], reso=(28, 28))
    with pytest.raises(ValueError):
        A.augment_batch([video.float()], ok, reso=(28, 28))
    with pytest.raises(ValueError):
        A.augment_batch([video], ok, out=torch.empty((1, 1, 3, 28, 27), device="cuda"), reso=(28, 28))
    with pytest.raises(ValueError):
        A.augment_batch([video], ok, out=torch.empty((1, 1, 3, 28, 28), device="cuda", dtype=torch.float16), reso=(28, 28))
    with pytest.raises(ValueError):
        A.augment_batch([video], [[R(2, (0, 0, 40, 40))]], reso=(28, 28))          # frame outside the video
    with pytest.raises(TedSpadHipError, match="no CPU path"):
        A.augment_batch([video.cpu()], ok, reso=(28, 28))
    with pytest.raises(TedSpadHipError, match="LDS"):
        A.augment_batch([video], ok, reso=(225, 224))
    with pytest.raises(TedSpadHipError, match="start inside"):
        A.augment_batch([video], [[R(0, (60, 0, 10, 10))]], reso=(28, 28))          # origin below the frame
    A.augment_batch([video], ok, reso=(28, 28))          # and the good call still runs
