"""CPU: the host half of the validation clips (ted_spad_amd/val_clips.py) against the fixture the reference's two validation loaders wrote
(tests/golden/make_val_clip_golden.py -> val_clip_golden.npz / val_clip_golden_meta.json): `sample_val_*` gives the reference's frame lists and its
Nones, those records run through Pillow (tests/val_clips_ref.py) give the reference's clips byte for byte with the reference's call sequence, and the
crop rule (torchvision's center_crop with its padding branch, the single loader's swapped height / width) holds."""
import ctypes
import json
import os
import types

import numpy as np
import pytest
import torch

import augment_ref
import val_clips_ref
from conftest import GOLDEN_DIR
from ted_spad_amd import preprocess as PP
from ted_spad_amd import val_clips as V


@pytest.fixture(scope="module")
def val_golden():
    with open(os.path.join(GOLDEN_DIR, "val_clip_golden_meta.json")) as f:
        meta = json.load(f)
    return meta, dict(np.load(os.path.join(GOLDEN_DIR, "val_clip_golden.npz")))


def sample(loader, params, frame_count, h, w, mode, hflip, cf, seed):
    """(frame lists, records[clip][frame]) from ted_spad_amd.val_clips alone, or None."""
    p = types.SimpleNamespace(**params)
    if loader == "contrastive":
        return V.sample_val_contrastive(np.random.RandomState(seed), p, frame_count, h, w, mode, hflip=hflip, cropping_factor=cf)
    res = V.sample_val_single(p, frame_count, h, w, mode, hflip=hflip, cropping_factor=cf)
    return None if res is None else ([res[0]], [res[1]])


CASES = ["single_landscape", "single_portrait", "contrastive_trip", "temporal_distance", "no_ar_distortion", "factor_1", "factor_1p2", "hflip",
         "short_20", "clamped_19"]


def reference_call_order(case, records):
    """The contrastive loader interleaves clip 1 and clip 2 frame by frame when they share their frames (temporal_align, ucf101_dl.py:800-810)."""
    aligned = case["loader"] == "contrastive" and (case["params"]["temporal_align"] or case["params"]["temporal_loss"] == "trip")
    if not aligned:
        return [(c, k) for c in range(len(records)) for k in range(len(records[c]))]
    order = [(c, k) for k in range(len(records[0])) for c in (0, 1)]
    return order + [(c, k) for c in range(2, len(records)) for k in range(len(records[c]))]


def test_fixture_has_every_case(val_golden):
    meta, _ = val_golden
    assert [c["name"] for c in meta["cases"]] == CASES
    assert len(meta["sweep"]) == 2 * 6 * 5


@pytest.mark.parametrize("name", CASES)
def test_sampling_and_pillow_chain_reproduce_the_reference(val_golden, name):
    meta, arrays = val_golden
    case = [c for c in meta["cases"] if c["name"] == name][0]
    t, h, w, _ = case["video"]
    cf = case["cropping_factor"]
    res = sample(case["loader"], case["params"], t, h, w, case["mode"], case["hflip"], cf, case["seed"])
    assert res is not None
    lists, records = res
    assert np.array_equal(np.stack([np.asarray(l) for l in lists]), arrays[name + "_frames"])
    clips = arrays[name + "_clips"]
    assert clips.shape[:2] == (len(records), len(records[0]))
    reso = V.val_reso(types.SimpleNamespace(**case["params"]), cf)
    assert list(reso) == case["reso"] and clips.shape[3:] == reso
    video = augment_ref.synthetic_video(*case["video"])
    got = torch.empty(clips.shape, dtype=torch.float32)
    augment_ref.CALLS = []
    try:
        for c, k in reference_call_order(case, records):
            rec = records[c][k]
            assert rec["reverse"] and rec["hflip"] == (case["hflip"] != 0) and not rec["erase"] and rec["contrast"] is None
            got[c, k] = val_clips_ref.apply_val_record(video[rec["frame"]], rec, reso, center=cf <= 1)
    finally:
        calls, augment_ref.CALLS = augment_ref.CALLS, None
    # every call the reference made, with its arguments, in its order
    assert json.loads(json.dumps([[n, kw] for n, kw in calls])) == case["calls"]
    assert torch.equal(got, torch.from_numpy(clips).to(torch.float32).div(255))


def test_records_follow_the_pixels_not_the_lists(val_golden):
    """With a temporal distance and temporal_align (forced by 'trip') list 2 is reassigned to list 1; without 'trip' the loader returns the distant list
    for clip 2 and builds the clip from it. The records name the frames the clips are made of."""
    meta, arrays = val_golden
    case = [c for c in meta["cases"] if c["name"] == "temporal_distance"][0]
    t, h, w, _ = case["video"]
    lists, records = sample("contrastive", case["params"], t, h, w, case["mode"], 0, 0.8, 0)
    assert [r["frame"] for r in records[1]] == list(lists[1]) and list(lists[1]) != list(lists[0])
    lists, records = sample("contrastive", dict(case["params"], temporal_loss="trip"), t, h, w, case["mode"], 0, 0.8, 0)
    assert len(lists) == 3 and list(lists[1]) == list(lists[0]) and [r["frame"] for r in records[1]] == list(lists[0])
    assert [r["frame"] for r in records[2]] == list(arrays["temporal_distance_frames"][1])          # start3 = start2: nothing is drawn
    lists, records = sample("contrastive", dict(case["params"], temporal_align=True), t, h, w, case["mode"], 0, 0.8, 0)
    assert list(lists[1]) != list(lists[0]) and [r["frame"] for r in records[1]] == list(lists[0])   # list 2 says one thing, clip 2 holds another


def test_sweep_of_modes_and_frame_counts(val_golden):
    meta, _ = val_golden
    seen = set()
    for s in meta["sweep"]:
        res = sample(s["loader"], s["params"], s["frame_count"], 24, 34, s["mode"], 0, 0.8, s["seed"])
        key = (s["loader"], s["frame_count"], s["mode"])
        if s["frames"] is None:
            assert res is None, key
        else:
            assert res is not None and [[int(v) for v in l] for l in res[0]] == s["frames"], key
        seen.add((s["loader"], s["frame_count"], s["frames"] is None))
    got = {(s["loader"], s["frame_count"], s["mode"]): s["frames"] for s in meta["sweep"]}
    assert [got[("single", 41, m)][0][0] for m in range(5)] == [0, 0, 0, 0, 4]           # 41 frames: only mode 4 falls back to `mode`
    assert [got[("single", 20, m)][0][:2] for m in range(5)] == [[m, m + 1] for m in range(5)]       # 20 frames: halved skip, start = mode
    assert got[("single", 19, 4)] is None and got[("contrastive", 19, 4)][0][-2:] == [18, 18]        # only the contrastive loader clamps
    assert got[("single", 17, 4)] is None and got[("contrastive", 17, 4)] is None                    # and only the last index


def test_sampling_gives_up_where_the_reference_does():
    p = types.SimpleNamespace(num_frames=16, fix_skip=2, reso_h=28, reso_w=28, num_modes=5, no_ar_distortion=False, temporal_loss=None,
                              temporal_align=True, temporal_distance=None)
    assert V.sample_val_contrastive(np.random.RandomState(0), p, 60, 240, 320, 0) is None      # frames_full2 is never defined (:789)
    p.temporal_align = False
    assert V.sample_val_contrastive(np.random.RandomState(0), p, 60, 240, 320, 0) is not None
    assert V.sample_val_contrastive(np.random.RandomState(0), p, 60, 240, 320, 5) is None      # mode outside num_modes
    assert V.sample_val_single(p, 60, 240, 320, 5) is None
    assert V.sample_val_contrastive(np.random.RandomState(0), p, 20, 240, 320, 2) is None      # clip 2's start has no fallback: -3
    p.temporal_distance = 8
    assert V.sample_val_contrastive(np.random.RandomState(0), p, 60, 240, 320, 0) is None      # left_over2 < 0
    rs = np.random.RandomState(0)
    before = rs.get_state()[1].copy()
    assert V.sample_val_contrastive(rs, p, 90, 240, 320, 0) is not None
    assert np.array_equal(rs.get_state()[1], before)                                           # nothing is drawn with a temporal distance


def test_center_crop_box_padded():
    p = types.SimpleNamespace(no_ar_distortion=False)
    assert V.val_box(p, 240, 320, 0.8, "single") == (-8, 64, 256, 192)
    assert V.val_box(p, 24, 34, 0.8, "single") == (-1, 8, 27, 19)
    assert V.val_box(p, 34, 24, 0.8, "single") == (8, -1, 19, 27)
    assert V.val_box(p, 240, 320, 0.8, "contrastive") == (24, 32, 192, 256)
    assert V.val_box(p, 240, 320, 1.2, "single") == (0, 0, 240, 320) == V.val_box(p, 240, 320, 1.2, "contrastive")
    assert V.val_box(p, 240, 320, 1, "single") == (-40, 40, 320, 240)
    q = types.SimpleNamespace(no_ar_distortion=True)
    assert V.val_box(q, 240, 320, 0.8, "single") == V.val_box(q, 240, 320, 0.8, "contrastive") == (24, 64, 192, 192)
    assert V.center_crop_box_padded(5, 5, 8, 9) == (-1, -2, 8, 9)                       # padded on all four sides: (3 // 2, 4 // 2) in front
    assert V.center_crop_box_padded(5, 5, 6, 6) == (0, 0, 6, 6)                         # an odd excess goes behind
    with pytest.raises(ValueError):
        V.val_box(p, 240, 320, 0.8, "train")


def test_center_crop_box_padded_equals_center_crop_box_inside_the_frame():
    for h in range(1, 14):
        for w in (1, 2, 7, 12, 13):
            for ch in range(1, h + 1):
                for cw in range(1, w + 1):
                    assert V.center_crop_box_padded(h, w, ch, cw) == PP.center_crop_box(h, w, ch, cw)
    with pytest.raises(ValueError):
        PP.center_crop_box(240, 320, 256, 192)                                          # stays as it is


def test_center_crop_box_padded_is_what_pillow_crops():
    """the box against the shim's center_crop (ImageOps.expand + crop) on an image whose pixels name their coordinates"""
    from PIL import Image
    for (h, w, ch, cw) in [(24, 34, 27, 19), (34, 24, 19, 27), (5, 5, 8, 9), (5, 6, 6, 7), (9, 7, 4, 12), (9, 7, 9, 7), (9, 7, 3, 2)]:
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        img = Image.fromarray(np.stack([yy + 1, xx + 1, yy * 0 + 200], axis=-1).astype(np.uint8), "RGB")
        a = np.array(val_clips_ref.center_crop(img, (ch, cw)))
        b = np.array(val_clips_ref.padded_crop(img, V.center_crop_box_padded(h, w, ch, cw)))
        assert a.shape == (ch, cw, 3) and np.array_equal(a, b), (h, w, ch, cw)


def test_val_reso():
    p = types.SimpleNamespace(reso_h=224, reso_w=224)
    assert V.val_reso(p, 1) == (280, 280) == V.val_reso(p, 1.0)
    assert V.val_reso(p, 0.8) == (224, 224) == V.val_reso(p, 1.2) == V.val_reso(p, 0.999)
    assert V.val_reso(types.SimpleNamespace(reso_h=28, reso_w=28), 1) == (35, 35)


def test_record_layout_matches_the_header():
    """RECORD is tedspad_val_record: same field names in the header's order, 64 bytes (csrc/val_clips.hip static_asserts the size)."""
    import re
    from conftest import ROOT
    hdr = open(os.path.join(ROOT, "include", "tedspad_hip.h")).read()
    body = re.search(r"typedef struct tedspad_val_record \{(.*?)\} tedspad_val_record;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        for piece in decl.split(","):
            ids = re.findall(r"[A-Za-z_][A-Za-z0-9_]*", piece)
            if ids:
                names.append(ids[-1])
    assert names == list(V.RECORD.names) and V.RECORD.itemsize == 64


def test_band_height_follows_the_lds_budget():
    from ted_spad_amd import _lib
    L = _lib.lib()
    budget, cap = L.tedspad_val_clips_lds_bytes(), L.tedspad_val_clips_band_max()
    R = V.frame_record
    assert V.band_height([[R(0, (0, 0, 24, 34))]], (1, 2)) == 1
    assert V.band_height([[R(0, (0, 0, 24, 34))]], (cap, 28)) == cap == V.band_height([[R(0, (0, 0, 24, 34))]], (cap + 1, 28))
    assert V.band_height([[R(0, (24, 32, 192, 256))]], (224, 224), cpad=4) < cap             # the packed rows count: 16 x 1792 + the temporary rows
    recs = [[R(0, (0, 0, 200, 9))]]
    b = V.band_height(recs, (7, 64))                                                    # 200 -> 7 rows: 59 taps a row
    tab, _ = V.pil_table_fast(200, 7)
    rows = lambda band: max(tab[min(i + band, 7) - 1, 0] + tab[min(i + band, 7) - 1, 1] - tab[i, 0] for i in range(0, 7, band))
    assert 1 <= b < 7 and 3 * rows(b) * 64 <= budget < 3 * rows(b + 1) * 64


def test_entry_refuses_bad_tables_on_the_host():
    """No GPU: both entries check the blob before they touch the device."""
    from ted_spad_amd import _lib
    L = _lib.lib()
    assert L.tedspad_val_clips(None, None, 0, 0, 0, 0, None, 0, 28, 28, 1, 0, 0, 0, None) != 0
    assert b"tedspad_val_clips" in L.tedspad_last_error()
    buf = (ctypes.c_uint64 * 64)()
    assert L.tedspad_val_clips(buf, buf, 64, 1, 64, 0, buf, 10, 28, 28, 1, 1, 1, 1, None) == -1            # record 0 has no source
    assert b"record 0" in L.tedspad_last_error()
    assert L.tedspad_val_clips(buf, buf, 64, 1, 64, 0, buf, 10, 28, 28, 17, 1, 1, 1, None) == -1           # band above the maximum
    assert L.tedspad_val_clips_act(buf, buf, 64, 1, 64, 0, buf, 10, 1, 28, 27, 1, 4, 0, None) == -1        # odd width with pixel pairs
    assert b"even" in L.tedspad_last_error()
    # one real record whose single output row needs more temporary rows than the budget holds: refused, not clamped
    rec = np.zeros(1, dtype=V.RECORD)
    tab_y, ky = V.pil_table_fast(4000, 1)
    tab_x, kx = V.pil_table_fast(8, 8)
    rec[0]["src"], rec[0]["H"], rec[0]["W"], rec[0]["ch"], rec[0]["cw"] = 64, 4000, 8, 4000, 8
    rec[0]["ytab"], rec[0]["ytaps"], rec[0]["xtab"], rec[0]["xtaps"] = 0, ky, tab_y.size, kx
    tables = np.concatenate([tab_y.reshape(-1), tab_x.reshape(-1)]).astype(np.int32)
    blob = np.concatenate([rec.view(np.uint8).reshape(-1), tables.view(np.uint8)])
    assert 3 * 4000 * 8 > L.tedspad_val_clips_lds_bytes()
    assert L.tedspad_val_clips(blob.ctypes.data, buf, blob.nbytes, 1, 64, tables.size, buf, 1000, 1, 8, 1, 64, 8, 1, None) == -3      # TEDSPAD_EUNSUPPORTED
    assert b"LDS" in L.tedspad_last_error()
