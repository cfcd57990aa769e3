"""GPU: tedspad_image_augment (csrc/augment_image.hip, ted_spad_amd/vispr_augment.py) against torch's own CPU arithmetic (tests/vispr_ref.py).

* The resize is `torch.equal` at dyadic scales, where every weight, product and sum is exact in fp32 in any order. At general scales torch's own last bit
  depends on the order and fusing of its sums, so a byte may differ by one ONLY where torch's fp32 value before rounding lies within 2^-10 of k + 0.5
  (two fp32 orderings differ by < 5e-5); the share of such pixels, computed from the reference alone, must stay under 1 %.
* A difference in one resized byte moves the contrast mean and with it every pixel, so the colour chain is checked bit for bit against the DEVICE's own
  resized bytes: every record runs twice, once with every op off and once in full, and full == vispr_ref.colour_chain(resized bytes) / 255."""
import json
import os
import types

import numpy as np
import pytest
import torch

import vispr_ref
from conftest import GOLDEN_DIR
from ted_spad_amd import vispr_augment as VA
from ted_spad_amd._lib import TedSpadHipError

pytestmark = pytest.mark.gpu

R = VA.image_record


def random_image(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(3, h, w)).astype(np.uint8)


def ramp_image(h, w, seed):
    """smooth ramps: resample sums that land on rounding ties, slowly varying colours"""
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return np.stack([(xx * 2 + seed) % 256, (yy * 3 + xx) % 256, ((xx + yy) // 2 + 128) % 256]).astype(np.uint8)


def to_bytes(x):
    """fp32 views -> the bytes they are / 255 of (checked: the division gives the same floats back)"""
    x = x.cpu()
    b = (x * 255).round().to(torch.uint8)
    assert torch.equal(b / 255.0, x)
    return b


def launch(images, recs, reso):
    """one launch of a flat list of records -> (len(recs), 3, oh, ow) bytes"""
    dev = [torch.from_numpy(i).cuda() for i in images]
    return to_bytes(VA.augment_images(dev, [recs], reso=reso)[0])


def plain(rec):
    return R(rec["image"], rec["box"])


def check_two_step(images, recs, reso):
    """every record with all ops off and in full, in ONE launch; the full result must be the reference's colour chain of the device's resized bytes"""
    got = launch(images, [plain(r) for r in recs] + list(recs), reso)
    n = len(recs)
    for k, r in enumerate(recs):
        want = vispr_ref.colour_chain(got[k], r)
        assert torch.equal(got[n + k], want), "record %d: %r, %d bytes differ" % (k, r, int((got[n + k] != want).sum()))
    return got[:n], got[n:]


def check_resize(img, box, reso, exact):
    """the resize alone against torch: equal (exact scales), or equal except by one at torch's own near-ties (general scales)"""
    got = launch([img], [R(0, box)], reso)[0]
    cropped = vispr_ref.crop(torch.from_numpy(img), *box)
    ref_f = vispr_ref.resize_float(cropped, reso)
    ref = torch.round(ref_f).to(torch.uint8)
    if exact:
        assert torch.equal(got, ref), "box %r: %d bytes differ" % (box, int((got != ref).sum()))
        return
    near = ((ref_f - torch.floor(ref_f)) - 0.5).abs() < 2.0 ** -10
    share = float(near.float().mean())
    diff = (got.int() - ref.int()).abs()
    print("box %r -> %r: %d bytes differ, near-tie share %.4f" % (box, reso, int((diff != 0).sum()), share))
    assert share < 0.01
    assert int(diff[~near].max()) == 0, "%d bytes differ away from a tie" % int((diff[~near] != 0).sum())
    assert int(diff.max()) <= 1


# ---- resize alone -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("make", [random_image, ramp_image], ids=["random", "ramp"])
def test_resize_exact_scales(make):
    """boxes of 1x, 2x, 4x and 1/2x the output at odd offsets; the last box of each list overflows right and bottom"""
    small, large = make(97, 131, 3), make(240, 320, 4)
    for box in [(3, 5, 28, 28), (7, 9, 56, 56), (11, 13, 14, 14), (60, 90, 56, 56)]:
        check_resize(small, box, (28, 28), True)
    for box in [(13, 17, 28, 28), (1, 3, 56, 56), (5, 7, 112, 112), (15, 19, 14, 14), (200, 290, 112, 112)]:
        check_resize(large, box, (28, 28), True)
    for box in [(9, 11, 224, 224), (101, 201, 224, 224)]:
        check_resize(large, box, (112, 112), True)


@pytest.mark.parametrize("h,w,reso", [(97, 131, 28), (181, 233, 224), (240, 320, 224), (300, 451, 224), (1100, 1500, 224)])
def test_resize_general_scales(h, w, reso):
    check_resize(random_image(h, w, h + w), (0, 0, h, w), (reso, reso), False)


def test_resize_general_scale_with_offset_and_overflow():
    img = random_image(181, 233, 8)
    check_resize(img, (17, 31, 150, 180), (28, 28), False)
    check_resize(img, (90, 100, 130, 170), (28, 28), False)


# ---- colour chain -------------------------------------------------------------------------------------------------------------------

def op_records(box):
    """each op alone at the factors where a fused multiply-add would change bytes (0.93, 1.1; brightness 0.9), both contrast positions, whole chains"""
    e1, e2 = [(3, 5, 9, 6)], [(20, 17, 12, 30)]
    recs = [R(0, box, contrast=f) for f in (0.93, 1.1)] + [R(1, box, contrast=f, contrast_late=True) for f in (0.93, 1.1)]
    recs += [R(0, box, saturation=f) for f in (0.93, 1.1)] + [R(1, box, brightness=f) for f in (0.9, 1.1)]
    recs += [R(0, box, hue=f) for f in (-0.05, 0.031)]
    recs += [R(1, box, gray=True), R(1, box, gray=True, gamma=0.85), R(0, box, gray=True, gamma=1.15), R(1, box, hflip=True)]
    recs += [R(0, box, contrast=1.1, hue=0.04, brightness=1.1), R(0, box, contrast=1.1, contrast_late=True, hue=0.04, brightness=1.1)]      # 14, 15
    recs += [R(1, box, contrast=0.93, hue=-0.03, saturation=0.93, brightness=0.9, gray=True, gamma=0.85, hflip=True, erase=e1),
             R(1, box, contrast=1.1, contrast_late=True, hue=0.05, saturation=1.1, brightness=1.1, gray=True, gamma=1.15, hflip=True, erase=e2),
             R(0, box, contrast=1.1, hue=0.05, saturation=1.1, brightness=1.1, hflip=True, erase=e2),
             R(0, box, contrast=0.93, contrast_late=True, hue=-0.05, saturation=0.93, brightness=0.9, erase=e1)]
    return recs


@pytest.mark.parametrize("make", [random_image, ramp_image], ids=["random", "ramp"])
@pytest.mark.parametrize("h,w,reso", [(97, 131, 28), (240, 320, 112)])
def test_each_op_and_full_chain(make, h, w, reso):
    images = [make(h, w, 5), make(h, w, 6)]
    box = (h // 13, w // 11, int(h * 0.73), int(w * 0.73))
    _, full = check_two_step(images, op_records(box), (reso, reso))
    assert not torch.equal(full[14], full[15])          # contrast before hue / after brightness: two different results, each matched above


@pytest.mark.parametrize("factor", [-0.05, -0.0123, 0.0, 0.031, 0.05])
def test_hue_over_every_colour(factor):
    """512 images of 128 x 256 hold all 2^24 colours; the box is the whole image and the output has its size, so the resample is the identity"""
    c = np.arange(1 << 24, dtype=np.uint32).reshape(512, 1, 128, 256)
    images = torch.from_numpy(np.concatenate([c >> 16, (c >> 8) & 255, c & 255], axis=1).astype(np.uint8))          # (512, 3, 128, 256)
    dev = images.cuda()
    got = VA.augment_images(list(dev), [[R(k, (0, 0, 128, 256), hue=factor) for k in range(512)]], reso=(128, 256))[0]
    flat = images.permute(1, 0, 2, 3).reshape(3, 512 * 128, 256)
    ref = vispr_ref.adjust_hue(flat, factor).reshape(3, 512, 128, 256).permute(1, 0, 2, 3).contiguous()
    value = (torch.arange(256, dtype=torch.float32) / 255.0).cuda()          # the 256 possible values, divided on the CPU
    assert torch.equal(got, value[ref.cuda().long()])
    if factor == 0.0:
        same = VA.augment_images(list(dev), [[R(k, (0, 0, 128, 256)) for k in range(512)]], reso=(128, 256))[0]
        assert torch.equal(same, value[dev.long()])          # identity resample


def test_contrast_on_a_half_half_and_a_constant_image():
    half = np.full((3, 28, 28), 10, np.uint8)
    half[:, 14:] = 11                                # gray 9 / 10 halves: the mean is k + 0.5
    const = np.full((3, 28, 28), 77, np.uint8)
    box = (0, 0, 28, 28)
    recs = [R(i, box, contrast=f, contrast_late=late) for i in (0, 1) for f in (0.5, 0.93, 1.1) for late in (False, True)]
    resized, full = check_two_step([half, const], recs, (28, 28))
    assert torch.equal(resized[0], torch.from_numpy(half)) and torch.equal(resized[6], torch.from_numpy(const))
    g = int(vispr_ref._gray(torch.from_numpy(const))[0, 0, 0])
    want = int(np.float32(0.5) * np.float32(77) + np.float32(0.5) * np.float32(g))          # _blend with the mean of a constant gray image
    assert int(full[6, 0, 0, 0]) == want


def test_gray_and_gamma():
    img = ramp_image(60, 80, 2)
    img[:] = img[0]                                  # a gray image: every byte value goes through the table
    box = (0, 0, 60, 80)
    recs = [R(0, box, gray=True), R(0, box, gray=True, gamma=0.85), R(0, box, gray=True, gamma=1.15), R(0, box, gray=True, gamma=1.0)]
    _, full = check_two_step([img], recs, (28, 28))
    assert not torch.equal(full[1], full[2])


def test_erase_boxes():
    img = ramp_image(60, 80, 1)
    box = (2, 3, 50, 70)
    cases = [(0, 0, 5, 6), (25, 20, 10, 30), (20, 25, 30, 10), (27, 0, 4, 28), (0, 27, 28, 4), (27, 27, 19, 19), (0, 0, 40, 40), (4, 4, 0, 5),
             (4, 4, 5, 0), (30, 3, 5, 5), (3, 30, 5, 5)]
    recs = [R(0, box, erase=[e]) for e in cases] + [R(0, box, hflip=True, erase=[e]) for e in cases]
    _, full = check_two_step([img], recs, (28, 28))
    assert not torch.equal(full[0].flip(-1), full[len(cases)])          # erase comes after the flip: the box does not move with it
    assert int(full[6].max()) == 0 and torch.equal(full[7], full[8])          # the whole image erased; empty boxes erase nothing


# ---- batches ------------------------------------------------------------------------------------------------------------------------

def test_ragged_ssl_batch_into_a_strided_out():
    """two source images of different size, two views each (the second may overflow its image), written into a strided view of a larger buffer"""
    from ted_spad_amd.train_step import AnonymizerTrainStep
    images = [vispr_ref.synthetic_image(97, 131, 11), vispr_ref.synthetic_image(240, 320, 12)]
    per_image = [VA.sample_vispr_ssl(np.random.RandomState(100 + n), *img.shape[1:], (28, 28), image=n) for n, img in enumerate(images)]
    records = [[per_image[n][v] for n in range(2)] for v in range(2)]
    dev = [torch.from_numpy(i).cuda() for i in images]
    base = torch.full((3, 4, 3, 30, 33), -7.0, dtype=torch.float32, device="cuda")
    out = base[:2, 1:3, :, 1:29, 2:30]
    ret = VA.augment_images(dev, records, out=out, reso=(28, 28))
    assert ret is out
    first = out.clone()
    mask = torch.ones_like(base, dtype=torch.bool)
    mask[:2, 1:3, :, 1:29, 2:30] = False
    assert bool((base[mask] == -7.0).all())
    VA.augment_images(dev, records, out=out, reso=(28, 28))
    assert torch.equal(out, first)
    flat = [r for row in records for r in row]
    _, full = check_two_step(images, flat, (28, 28))
    assert torch.equal(to_bytes(out).reshape(4, 3, 28, 28), full)
    views = AnonymizerTrainStep._views(types.SimpleNamespace(fb=object()), [out[0], out[1]])
    assert len(views) == 2 and views[0].shape == views[1].shape == (2, 3, 28, 28) and views[0].dtype == torch.float32


@pytest.mark.parametrize("name", [c["name"] for c in json.load(open(os.path.join(GOLDEN_DIR, "vispr_aug_golden_meta.json")))["cases"]])
def test_fixture_cases(name):
    """the records the samplers give for the fixture's seeds (tests/test_vispr_augment_host.py ties them to the reference's calls and bytes), on the device"""
    with open(os.path.join(GOLDEN_DIR, "vispr_aug_golden_meta.json")) as f:
        meta = json.load(f)
    case = [c for c in meta["cases"] if c["name"] == name][0]
    h, w, _ = case["image"]
    reso = tuple(meta["reso"])
    if case["split"] != "train":
        recs = [VA.center_record(h, w)] * (2 if case["loader"] == "ssl" else 1)
    elif case["loader"] == "ssl":
        recs = VA.sample_vispr_ssl(np.random.RandomState(case["seed"]), h, w, reso)
    else:
        recs = [VA.sample_vispr(np.random.RandomState(case["seed"]), h, w, reso)]
    img = vispr_ref.synthetic_image(*case["image"])
    resized, full = check_two_step([img], recs, reso)
    # the fixture's own bytes: equal wherever the resize had no near-tie to decide (then the whole chain is the reference's)
    views = torch.from_numpy(np.load(os.path.join(GOLDEN_DIR, "vispr_aug_golden.npz"))[name + "_views"])
    for k, r in enumerate(recs):
        if torch.equal(resized[k], vispr_ref.resized_crop(torch.from_numpy(img), *r["box"], reso)):
            assert torch.equal(full[k], views[k])


def test_bad_arguments_and_limits_raise():
    img = torch.from_numpy(random_image(60, 80, 0)).cuda()
    ok = [[R(0, (0, 0, 40, 40))]]
    for rec in (R(0, (-1, 0, 40, 40)), R(0, (0, -2, 40, 40)), R(0, (0, 0, 0, 40)), R(0, (60, 0, 10, 10)), R(0, (0, 0, 40, 40), hue=0.6),
                R(0, (0, 0, 40, 40), gamma=0.9), R(0, (0, 0, 40, 40), erase=[(1, 1, 2, 2), (3, 3, 2, 2)])):
        with pytest.raises(ValueError):
            VA.augment_images([img], [[rec]], reso=(28, 28))
    with pytest.raises(ValueError):
        VA.augment_images([img.float()], ok, reso=(28, 28))
    with pytest.raises(ValueError):
        VA.augment_images([img.permute(1, 2, 0).contiguous()], ok, reso=(28, 28))
    with pytest.raises(ValueError):
        VA.augment_images([img], ok, out=torch.empty((1, 1, 3, 28, 27), device="cuda"), reso=(28, 28))
    with pytest.raises(ValueError):
        VA.augment_images([img], ok, out=torch.empty((1, 1, 3, 28, 28), device="cuda", dtype=torch.float16), reso=(28, 28))
    with pytest.raises(TedSpadHipError, match="no CPU path"):
        VA.augment_images([img.cpu()], ok, reso=(28, 28))
    with pytest.raises(TedSpadHipError, match="LDS"):
        VA.augment_images([img], ok, reso=(225, 224))
    with pytest.raises(TedSpadHipError, match="crop boxes up to 4096 x 4096"):
        VA.augment_images([img], [[R(0, (0, 0, 4097, 40))]], reso=(28, 28))
    with pytest.raises(TedSpadHipError, match="crop boxes up to 4096 x 4096"):
        VA.augment_images([img], [[R(0, (0, 0, 40, 5000))]], reso=(28, 28))
    big = VA.augment_images([img], [[R(0, (0, 0, 4096, 4096))]], reso=(28, 28))          # at the limit: runs (all but a corner is zero fill)
    assert bool(torch.isfinite(big).all())
    good = VA.augment_images([img], ok, reso=(28, 28))          # and the good call still runs
    assert bool(torch.isfinite(good).all())
    check_resize(img.cpu().numpy(), (0, 0, 40, 40), (28, 28), False)
