"""CPU: the host half of the device augmentation (ted_spad_amd/augment.py) against the fixture the reference's two training loaders wrote
(tests/golden/make_aug_golden.py -> aug_golden.npz / aug_golden_meta.json): `sample_*` draws the reference's frame lists and parameters from the
same seed, those records run through Pillow (tests/augment_ref.py) give the reference's clips byte for byte with the reference's call sequence, and
the small host rules (hue offset wrap, gamma table, resample tables, record layout) hold."""
import ctypes
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


@pytest.fixture(scope="module")
def aug_golden():
    with open(os.path.join(GOLDEN_DIR, "aug_golden_meta.json")) as f:
        meta = json.load(f)
    return meta, dict(np.load(os.path.join(GOLDEN_DIR, "aug_golden.npz")))


def sample_case(case):
    """(frame lists (clips, n), records[clip][frame]) of a fixture case from ted_spad_amd.augment alone."""
    params = types.SimpleNamespace(**case["params"])
    t, h, w, _ = case["video"]
    rs = np.random.RandomState(case["seed"])
    if case["loader"] == "contrastive":
        res = A.sample_contrastive(rs, params, t, h, w, frame_wise_aug=case["frame_wise_aug"])
        assert res is not None
        return np.stack([np.asarray(l) for l in res[0]]), res[1]
    res = A.sample_single(rs, params, t, h, w, frame_wise_aug=case["frame_wise_aug"])
    assert res is not None
    return np.asarray(res[0])[None], [res[1]]


CASES = ["weak_trip", "strong_trip", "strong_single", "frame_wise", "no_ar_distortion", "aspect_ratio_aug", "short_video"]


def reference_call_order(case, records):
    """The reference interleaves clip 1 and clip 2 frame by frame when they share their frames (temporal_align, ucf101_dl.py:515-526)."""
    aligned = case["loader"] == "contrastive" and (case["params"]["temporal_align"] or case["params"]["temporal_loss"] == "trip")
    if not aligned:
        return [(c, k) for c in range(len(records)) for k in range(len(records[c]))]
    order = [(c, k) for k in range(len(records[0])) for c in (0, 1)]
    return order + [(c, k) for c in range(2, len(records)) for k in range(len(records[c]))]


@pytest.mark.parametrize("name", CASES)
def test_sampling_and_pillow_chain_reproduce_the_reference(aug_golden, name):
    meta, arrays = aug_golden
    case = [c for c in meta["cases"] if c["name"] == name][0]
    frames, records = sample_case(case)
    assert np.array_equal(frames, arrays[name + "_frames"])
    clips = arrays[name + "_clips"]
    assert clips.shape[:2] == (len(records), len(records[0]))
    video = augment_ref.synthetic_video(*case["video"])
    reso = tuple(meta["reso"])
    got = torch.empty(clips.shape, dtype=torch.float32)
    augment_ref.CALLS = []
    try:
        for c, k in reference_call_order(case, records):
            rec = records[c][k]
            assert rec["frame"] == frames[c, k]
            got[c, k] = augment_ref.apply_record(video[rec["frame"]], rec, reso)
    finally:
        calls, augment_ref.CALLS = augment_ref.CALLS, None
    # every call the reference made, with its arguments, in its order (floats survive JSON exactly)
    assert json.loads(json.dumps([[n, kw] for n, kw in calls])) == case["calls"]
    assert torch.equal(got, torch.from_numpy(clips).to(torch.float32).div(255))


def test_fixture_covers_every_op(aug_golden):
    meta, _ = aug_golden
    covered = set().union(*[set(c["covers"]) for c in meta["cases"]])
    assert covered >= {"contrast_first", "contrast_late", "adjust_hue", "adjust_saturation", "adjust_brightness", "to_grayscale", "adjust_gamma",
                       "hflip", "erase", "overflow"}
    short = [c for c in meta["cases"] if c["name"] == "short_video"][0]
    assert short["video"][0] < short["params"]["fix_skip"] * short["params"]["num_frames"]          # the skip was halved


def test_sampling_gives_up_where_the_reference_does():
    p = types.SimpleNamespace(num_frames=16, fix_skip=2, reso_h=28, reso_w=28, min_crop_factor_training=0.6, weak_aug=False, no_ar_distortion=False,
                              aspect_ratio_aug=False, temporal_loss="trip", temporal_align=False, temporal_distance=None)
    assert A.sample_contrastive(np.random.RandomState(0), p, 16, 240, 320) is None       # randint(0, 0)
    assert A.sample_single(np.random.RandomState(0), p, 16, 240, 320) is None
    p.temporal_loss, p.temporal_align = None, True
    assert A.sample_contrastive(np.random.RandomState(0), p, 60, 240, 320) is None       # frames_full2 is never defined (:463)
    p.reso_h = 2                                                                        # empty erase-size range
    p.temporal_align = False
    assert A.sample_contrastive(np.random.RandomState(0), p, 60, 240, 320) is None


def test_hue_offset_wraps_for_negative_factors():
    assert A.hue_offset(0.05) == 12 and A.hue_offset(0.031) == 7 and A.hue_offset(0.0) == 0
    assert A.hue_offset(-0.05) == 256 - 12 and A.hue_offset(-0.0123) == 256 - 3 and A.hue_offset(-0.001) == 0
    assert A.hue_offset(-0.5) == 256 - 127 and A.hue_offset(0.5) == 127
    for f in (-0.05, -0.0123, 0.0, 0.031, 0.05):
        assert A.hue_offset(f) == augment_ref.hue_offset(f)


def test_gamma_table_equals_the_shims():
    for g in (0.85, 1.0, 1.15, 0.9371):
        assert A.gamma_lut(g).tolist() == augment_ref.gamma_table(g, 1)
        assert A.gamma_lut(g).dtype == np.uint8


def test_fast_table_equals_pil_table():
    for i, o in [(144, 28), (239, 112), (240, 112), (320, 224), (97, 28), (131, 28), (28, 28), (1, 28), (3, 7), (192, 224), (143, 224)]:
        a, ka = PP.pil_table(i, o)
        b, kb = A.pil_table_fast(i, o)
        assert ka == kb and np.array_equal(a, b), (i, o)


def test_record_layout_matches_the_header():
    """RECORD is tedspad_augment_record: same field names in the header's order, 112 bytes (csrc/augment.hip static_asserts the size)."""
    import re
    from conftest import ROOT
    hdr = open(os.path.join(ROOT, "include", "tedspad_hip.h")).read()
    body = re.search(r"typedef struct tedspad_augment_record \{(.*?)\} tedspad_augment_record;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        for piece in decl.split(","):
            ids = re.findall(r"[A-Za-z_][A-Za-z0-9_]*", re.sub(r"\[\d+\]", "", piece))
            if ids:
                names.append(ids[-1])
    assert names == list(A.RECORD.names) and A.RECORD.itemsize == 112
    flags = dict(re.findall(r"TEDSPAD_AUG_([A-Z_]+) = (\d+)", hdr))
    assert {k: int(v) for k, v in flags.items()} == {"CONTRAST_FIRST": A.CONTRAST_FIRST, "HUE": A.HUE, "SATURATION": A.SATURATION,
                                                     "BRIGHTNESS": A.BRIGHTNESS, "CONTRAST_LATE": A.CONTRAST_LATE, "GRAY": A.GRAY,
                                                     "GAMMA": A.GAMMA, "HFLIP": A.HFLIP, "REVERSE": A.REVERSE}


def test_entry_refuses_bad_tables_on_the_host():
    """No GPU: tedspad_clip_augment checks the blob before it touches the device."""
    from ted_spad_amd import _lib
    L = _lib.lib()
    assert L.tedspad_clip_augment(None, None, 0, 0, 0, 0, 0, 0, None, 0, 28, 28, 0, 0, 0, None) != 0
    assert b"tedspad_clip_augment" in L.tedspad_last_error()
    buf = (ctypes.c_uint64 * 64)()
    assert L.tedspad_clip_augment(buf, buf, 112, 1, 112, 0, 112, 0, buf, 10, 225, 224, 1, 1, 1, None) == -3          # TEDSPAD_EUNSUPPORTED
    assert b"LDS" in L.tedspad_last_error()
    assert L.tedspad_clip_augment(buf, buf, 112, 1, 112, 0, 112, 0, buf, 10, 28, 28, 1, 1, 1, None) == -1            # record 0 has no source
    assert b"record 0" in L.tedspad_last_error()
