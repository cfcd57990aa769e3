"""CPU: the host half of ted_spad_amd.vispr_augment against the fixture the reference's VISPR loaders produced (tests/golden/make_vispr_aug_golden.py):
the samplers reproduce the logged calls from the same seed, tests/vispr_ref.py applied to their records reproduces the returned bytes, and the argument
checks that need no device raise."""
import json
import os

import numpy as np
import pytest
import torch

import vispr_ref
from conftest import GOLDEN_DIR
from ted_spad_amd import vispr_augment as VA
from ted_spad_amd._lib import TedSpadHipError

with open(os.path.join(GOLDEN_DIR, "vispr_aug_golden_meta.json")) as _f:
    META = json.load(_f)
RESO = tuple(META["reso"])
NAMES = [c["name"] for c in META["cases"]]


def case_records(case):
    """the records the build's samplers give for a fixture case, from the case's seed"""
    h, w, _ = case["image"]
    if case["split"] != "train":
        return [VA.center_record(h, w)] * (2 if case["loader"] == "ssl" else 1)
    rs = np.random.RandomState(case["seed"])
    return VA.sample_vispr_ssl(rs, h, w, RESO) if case["loader"] == "ssl" else [VA.sample_vispr(rs, h, w, RESO)]


def calls_of(rec, train):
    """the functional calls the loader makes for a record, as vispr_ref logs them"""
    top, left, ch, cw = rec["box"]
    if not train:
        return [["center_crop", {"size": ch}], ["resize", {"size": list(RESO)}]]
    calls = [["resized_crop", {"top": top, "left": left, "height": ch, "width": cw, "size": list(RESO)}]]
    contrast = [["adjust_contrast", {"factor": rec["contrast"]}]] if rec["contrast"] is not None else []
    if not rec["contrast_late"]:
        calls += contrast
    for name in ("hue", "saturation", "brightness"):
        if rec[name] is not None:
            calls.append(["adjust_" + name, {"factor": rec[name]}])
    if rec["contrast_late"]:
        calls += contrast
    if rec["gray"]:
        calls.append(["rgb_to_grayscale", {"num_output_channels": 3}])
        if rec["gamma"] is not None:
            calls.append(["adjust_gamma", {"gamma": rec["gamma"], "gain": 1.0}])
    if rec["hflip"]:
        calls.append(["hflip", {}])
    for (i, j, h, w) in rec["erase"]:
        calls.append(["erase", {"i": i, "j": j, "h": h, "w": w, "v": 0.0}])
    return calls


@pytest.mark.parametrize("name", NAMES)
def test_samplers_give_the_logged_calls(name):
    case = [c for c in META["cases"] if c["name"] == name][0]
    recs = case_records(case)
    want = [c for r in recs for c in calls_of(r, case["split"] == "train")]
    assert want == case["calls"]


@pytest.mark.parametrize("name", NAMES)
def test_reference_on_the_records_gives_the_fixture_bytes(name):
    case = [c for c in META["cases"] if c["name"] == name][0]
    views = np.load(os.path.join(GOLDEN_DIR, "vispr_aug_golden.npz"))[name + "_views"]
    img = torch.from_numpy(vispr_ref.synthetic_image(*case["image"]))
    recs = case_records(case)
    assert len(recs) == len(views)
    for r, want in zip(recs, views):
        assert np.array_equal(vispr_ref.apply_record_bytes(img, r, RESO).numpy(), want)


def test_fixture_covers_every_op():
    covered = set(f for c in META["cases"] for f in c["covers"])
    assert covered >= {"contrast_first", "contrast_late", "adjust_hue", "adjust_saturation", "adjust_brightness", "rgb_to_grayscale", "adjust_gamma",
                       "hflip", "erase", "overflow"}


def test_sampler_draw_order_and_unused_draws():
    """size-(2,) draws of which index 0 is used, random_color_dropped drawn although unused, rand(8) last: the generator ends where the reference's does"""
    rs, ref = np.random.RandomState(7), np.random.RandomState(7)
    rec = VA.sample_vispr(rs, 97, 131, (28, 28))
    x_erase, y_erase = ref.randint(0, 28, size=(2,)), ref.randint(0, 28, size=(2,))
    cf = ref.uniform(0.6, 1, size=(2,))
    x0, y0 = ref.randint(0, 131 - 131 * cf[0] + 1), ref.randint(0, 97 - 97 * cf[0] + 1)
    for lo, hi in ((0.9, 1.1), (-0.05, 0.05), (0.9, 1.1), (0.9, 1.1), (0.85, 1.15)):
        ref.uniform(lo, hi, size=(2,))
    ref.randint(9, 19, size=(2,)), ref.randint(9, 19, size=(2,)), ref.randint(0, 3, (2,))
    ref.rand(8)
    assert rec["box"] == (y0, x0, int(97 * cf[0]), int(131 * cf[0]))
    assert rs.rand() == ref.rand()
    # the SSL loader: both views share the origin, each crops with its own factor
    v0, v1 = VA.sample_vispr_ssl(np.random.RandomState(7), 97, 131, (28, 28))
    assert v0["box"] == rec["box"] and v1["box"][:2] == rec["box"][:2] and v1["box"][2:] == (int(97 * cf[1]), int(131 * cf[1]))


def test_erase_row_is_x_erase_and_shares_the_flip_draw():
    for seed in range(200):
        rec = VA.sample_vispr(np.random.RandomState(seed), 240, 320, (28, 28))
        assert not (rec["hflip"] and rec["erase"])
        if rec["erase"]:
            ref = np.random.RandomState(seed)
            x_erase, y_erase = ref.randint(0, 28, size=(2,)), ref.randint(0, 28, size=(2,))
            assert rec["erase"][0][:2] == (x_erase[0], y_erase[0])          # x_erase goes to erase's i: the ROW
            return
    raise AssertionError("no seed with an erase box")


@pytest.mark.parametrize("h,w,box", [(97, 131, (0, 17, 97, 97)), (96, 131, (0, 18, 96, 96)), (131, 96, (18, 0, 96, 96)), (131, 97, (17, 0, 97, 97)),
                                     (100, 105, (0, 2, 100, 100)), (100, 103, (0, 2, 100, 100)), (100, 101, (0, 0, 100, 100)), (64, 64, (0, 0, 64, 64))])
def test_center_record_origins(h, w, box):
    """int(round(margin / 2.0)) with Python's round: 17.0 -> 17, 17.5 -> 18, 2.5 -> 2, 1.5 -> 2, 0.5 -> 0"""
    rec = VA.center_record(h, w)
    assert rec["box"] == box
    img = torch.from_numpy(vispr_ref.synthetic_image(h, w, 3))
    side = min(h, w)
    assert torch.equal(vispr_ref.center_crop(img, side), vispr_ref.crop(img, *rec["box"]))
    assert all(rec[k] is None for k in ("contrast", "hue", "saturation", "brightness", "gamma")) and not rec["gray"] and not rec["hflip"]


def test_gamma_table_is_torchs_own_pow():
    g = torch.arange(256, dtype=torch.uint8).view(1, 16, 16).expand(3, 16, 16)
    for gamma in (0.85, 1.0, 1.15):
        assert np.array_equal(VA.gamma_lut(gamma), vispr_ref.adjust_gamma(g, gamma)[0].reshape(-1).numpy())


def test_bad_arguments_raise_without_a_device():
    img = torch.zeros((3, 60, 80), dtype=torch.uint8)
    R = VA.image_record
    strides = (3 * 28 * 28, 3 * 28 * 28, 28 * 28, 28, 1)
    bad = [R(0, (-1, 0, 40, 40)), R(0, (0, -2, 40, 40)), R(0, (0, 0, 0, 40)), R(0, (0, 0, 40, 0)), R(0, (60, 0, 10, 10)), R(0, (0, 80, 10, 10)),
           R(0, (0, 0, 40, 40), hue=0.51), R(0, (0, 0, 40, 40), hue=-0.6), R(0, (0, 0, 40, 40), gamma=0.9),
           R(0, (0, 0, 40, 40), erase=[(1, 1, 2, 2), (3, 3, 2, 2)]), R(0, (0, 0, 40, 40), erase=[(-1, 1, 2, 2)]), R(1, (0, 0, 40, 40))]
    for rec in bad:
        with pytest.raises(ValueError):
            VA.build_table([img], [[rec]], strides, (28, 28))
    ok = [[R(0, (0, 0, 40, 40))]]
    for wrong in (img.float(), img.permute(1, 2, 0).contiguous(), img[:, :, ::2], img[0], torch.zeros((1, 60, 80), dtype=torch.uint8)):
        with pytest.raises(ValueError):
            VA.augment_images([wrong], ok, reso=(28, 28))
    with pytest.raises(ValueError):
        VA.augment_images([], ok, reso=(28, 28))
    with pytest.raises(TedSpadHipError, match="no CPU path"):
        VA.augment_images([img], ok, reso=(28, 28))
