"""Training clips on the device: the build's counterpart of the two training loaders of aux_code/ucf101_dl.py (`contrastive_train_dataloader`
:324-642, `single_train_dataloader` :23-195). The reference turns every frame of a batch into a PIL image on the host (resized_crop, the colour
chain, hflip, to_tensor, two erased boxes); here decoded uint8 frames stay in HBM and ONE launch (tedspad_clip_augment, csrc/augment.hip) writes the
fp32 `(B, n, 3, h, w)` batch `AnonymizerTrainStep` / `PrivacyTrainStep` take, bit-identical to the Pillow chain.

Two halves:

* `sample_contrastive` / `sample_single` draw a clip's frame lists and augmentation parameters from a `numpy.random.RandomState` in exactly the
  order, and with exactly the calls, of the two `build_clip` bodies (same seed -> same frames and parameters as the reference), and return them as
  per-frame records (plain dicts, `frame_record`).
* `augment_batch` turns records into the kernel's record table and launches.

torchvision is not installed here. What its functional calls do with a PIL image is restated from its published 0.15.2 `_functional_pil.py` (the
same standing as `preprocess.center_crop_box`): which Pillow call each one makes, and `adjust_hue`'s `uint8(hue_factor * 255)` offset. The arithmetic
itself is Pillow's, which IS installed and pins the kernel bit for bit (tests/augment_ref.py, tests/test_hip_augment.py).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._lib import check
from .engine import _stream_ptr, require_cuda
from .preprocess import PIL_PRECISION_BITS

CONTRAST_FIRST, HUE, SATURATION, BRIGHTNESS, CONTRAST_LATE, GRAY, GAMMA, HFLIP, REVERSE = 1, 2, 4, 8, 16, 32, 64, 128, 256   # TEDSPAD_AUG_*

# tedspad_augment_record (include/tedspad_hip.h)
RECORD = np.dtype([("src", "<u8"), ("dst", "<i8"), ("H", "<i4"), ("W", "<i4"), ("top", "<i4"), ("left", "<i4"), ("ch", "<i4"), ("cw", "<i4"),
                   ("ytab", "<i4"), ("xtab", "<i4"), ("ytaps", "<i4"), ("xtaps", "<i4"), ("flags", "<i4"), ("gamma_lut", "<i4"),
                   ("contrast", "<f4"), ("saturation", "<f4"), ("brightness", "<f4"), ("hue_off", "<i4"), ("erase", "<i4", (8,))])
assert RECORD.itemsize == 112

LDS_FRAME_BYTES = 3 * 224 * 224          # the largest resized frame a workgroup holds (csrc/augment.hip)


# ---- parameters -------------------------------------------------------------------------------------------------------------------

def hue_offset(hue_factor) -> int:
    """adjust_hue's `np.uint8(hue_factor * 255)`: truncation towards zero, wrapped modulo 256 (the reference environment's numpy 1.x wraps a negative
    value; numpy 2 raises instead, so the wrap is written out)."""
    return int(float(hue_factor) * 255) % 256


def gamma_lut(gamma, gain=1.0) -> np.ndarray:
    """adjust_gamma's 256-entry `point` table, in Python doubles as torchvision builds it; clipped to a byte as Pillow stores an 8-bit lookup table."""
    return np.array([min(max(int((255 + 1 - 1e-3) * gain * pow(e / 255.0, float(gamma))), 0), 255) for e in range(256)], dtype=np.uint8)


def frame_record(frame, box, video=0, contrast=None, contrast_late=False, hue=None, saturation=None, brightness=None, gray=False, gamma=None,
                 hflip=False, reverse=False, erase=()):
    """One output frame: source `frame` of `video`, crop `box` = (top, left, height, width) (may overflow right / bottom), the ops that apply
    (None / False: skipped) in the reference's fixed order, and up to two erase boxes (i = row, j = column, h, w)."""
    return {"video": int(video), "frame": int(frame), "box": tuple(int(v) for v in box), "contrast": None if contrast is None else float(contrast),
            "contrast_late": bool(contrast_late), "hue": None if hue is None else float(hue),
            "saturation": None if saturation is None else float(saturation), "brightness": None if brightness is None else float(brightness),
            "gray": bool(gray), "gamma": None if gamma is None else float(gamma), "hflip": bool(hflip), "reverse": bool(reverse),
            "erase": [tuple(int(v) for v in e) for e in erase]}


def _box(params, h, w, cf, x0, y0):
    """resized_crop's (top, left, height, width) as augmentation / weak_augmentation pass them (:601-604)."""
    if params.no_ar_distortion:
        m = min(h, w)
        return (y0, x0, int(m * cf), int(m * cf))
    return (y0, x0, int(h * cf), int(w * cf))


def _strong(params, h, w, frame, r, x_erase, y_erase, cf, x0, y0, contrast, hue, saturation, brightness, gamma, es1, es2, reverse):
    """`augmentation` (:596-630 / :149-183): which op runs is decided by the row `r` of random_array. `x_erase` is passed as erase's ROW."""
    er = []
    if r[7] < 0.4:
        er.append((x_erase[0], y_erase[0], es1[0], es2[0]))
    if r[8] < 0.4:
        er.append((x_erase[1], y_erase[1], es1[1], es2[1]))
    first, late = r[0] < 0.125 / 2, (r[0] > 0.125 / 2 and r[0] < 0.25 / 2)
    gray = r[4] > 0.9
    return frame_record(frame, _box(params, h, w, cf, x0, y0), contrast=contrast if (first or late) else None, contrast_late=late,
                        hue=hue if r[1] < 0.3 / 2 else None, saturation=saturation if r[2] < 0.3 / 2 else None,
                        brightness=brightness if r[3] < 0.3 / 2 else None, gray=gray, gamma=gamma if (gray and r[5] > 0.25) else None,
                        hflip=r[6] > 0.5, reverse=reverse, erase=er)


def _frames(start, skip, n):
    return start + np.asarray([int(int(skip) * f) for f in range(n)])


def _check_frames(fr, frame_count):
    """decord's get_batch raises for an index outside the video (the reference's except then returns None)."""
    if np.any(np.asarray(fr) < 0) or np.any(np.asarray(fr) >= frame_count):
        raise IndexError("frame index outside the video")


def _colour_draws(rs, params, h, w, rows, framewise, erase_size=19):
    shape = (rows,) if rows else (2,)
    eshape = (rows, 2) if rows else (2,)
    contrast = rs.uniform(0.9, 1.1, size=shape)
    hue = rs.uniform(-0.05, 0.05, size=shape)
    saturation = rs.uniform(0.9, 1.1, size=shape)
    brightness = rs.uniform(0.9, 1.1, size=shape)
    gamma = rs.uniform(0.85, 1.15, size=shape)
    if framewise:
        es1 = rs.randint(int(erase_size / 2), erase_size, size=eshape)
        es2 = rs.randint(int(erase_size / 2), erase_size, size=eshape)
    else:
        es1 = rs.randint(int((h / 6) * (params.reso_h / 224)), int((h / 3) * (params.reso_h / 224)), size=eshape)
        es2 = rs.randint(int((w / 6) * (params.reso_h / 224)), int((w / 3) * (params.reso_h / 224)), size=eshape)
    rs.randint(0, 3, shape[0])          # random_color_dropped: drawn, never used
    return contrast, hue, saturation, brightness, gamma, es1, es2


def _origin(rs, params, h, w, cf):
    """x0, y0 (:481-489): drawn for cropping_factor1[0] (or [1] for y0 with aspect_ratio_aug), used by every clip."""
    if not params.no_ar_distortion:
        x0 = rs.randint(0, (w - w * cf[0]) + 1)
        if params.aspect_ratio_aug:
            y0 = rs.randint(0, (h - h * cf[1]) + 1)
        else:
            y0 = rs.randint(0, (h - h * cf[0]) + 1)
    else:
        m = min(h, w)
        x0 = rs.randint(0, (w - m * cf[0]) + 1)
        y0 = rs.randint(0, (h - m * cf[0]) + 1)
    return x0, y0


def sample_contrastive(rs, params, frame_count, h, w, frame_wise_aug=False):
    """`contrastive_train_dataloader.build_clip` (:386-593) without the pixels: `rs` is a numpy.random.RandomState standing where the reference uses
    the global numpy generator. Returns (frame_lists, records): the 2 (3 with temporal_loss 'trip') frame-index arrays and, per clip, one record per
    frame; or None where the reference's try / except gives up on the video."""
    try:
        n = params.num_frames
        trip = params.temporal_loss == 'trip'
        skip = params.fix_skip
        left_over = frame_count - params.fix_skip * n
        temporal_align = params.temporal_align
        frames2 = None
        if params.temporal_distance:
            left_over2 = left_over - skip * n - params.temporal_distance
            if left_over2 > 0:
                start = rs.randint(0, int(left_over2))
            else:
                skip /= 2
                left_over = frame_count - skip * n
                left_over2 = left_over - skip * n - params.temporal_distance
                start = rs.randint(0, int(left_over2))
            start2 = start + skip * (n - 1) + params.temporal_distance
            frames2 = _frames(start2, skip, n)
        else:
            if left_over > 0:
                start = rs.randint(0, int(left_over))
            else:
                skip /= 2
                left_over = frame_count - skip * n
                start = rs.randint(0, int(max(0, left_over)))
            if trip:
                temporal_align = True
            if not temporal_align:
                start2 = rs.randint(0, int(left_over))
                frames2 = _frames(start2, skip, n)
        frames1 = _frames(start, skip, n)
        if frames1[-1] >= frame_count:
            frames1[-1] = int(frame_count - 1)
        if not temporal_align:
            if frames2[-1] >= frame_count:
                frames2[-1] = int(frame_count - 1)
        if trip:
            temporal_align = True
            frames2 = frames1
            if params.temporal_distance:
                start3 = start2
            else:
                start3 = rs.randint(0, int(left_over))
            frames3 = _frames(start3, skip, n)
            if frames3[-1] >= frame_count:
                frames3[-1] = int(frame_count - 1)
        else:
            frames3 = None
        if frames2 is None:
            raise NameError("frames_full2")          # (:463: temporal_align without 'trip' or a temporal distance never defines it)
        _check_frames(frames1, frame_count)
        if not temporal_align:
            _check_frames(frames2, frame_count)
        if trip:
            _check_frames(frames3, frame_count)

        r = rs.rand(3, 10)
        x_erase = rs.randint(0, params.reso_w, size=(3, 2))
        y_erase = rs.randint(0, params.reso_h, size=(3, 2))
        cf = rs.uniform(params.min_crop_factor_training, 1, size=(3,))
        x0, y0 = _origin(rs, params, h, w, cf)
        col = _colour_draws(rs, params, h, w, 3, False)

        def rec(k, frame):
            if params.weak_aug:
                return frame_record(frame, _box(params, h, w, cf[k], x0, y0))
            c, hu, s, b, g, es1, es2 = col
            return _strong(params, h, w, frame, r[k], x_erase[k], y_erase[k], cf[k], x0, y0, c[k], hu[k], s[k], b[k], g[k], es1[k], es2[k], False)

        clip1, clip2, clip3 = [], [], []
        for f in frames1:
            if frame_wise_aug:
                col = _colour_draws(rs, params, h, w, 3, True)
            clip1.append(rec(0, f))
            if temporal_align:
                clip2.append(rec(1, f))
        if not temporal_align:
            clip2 = [rec(1, f) for f in frames2]
        if trip:
            clip3 = [rec(2, f) for f in frames3]
            return [frames1, frames2, frames3], [clip1, clip2, clip3]
        return [frames1, frames2], [clip1, clip2]
    except Exception:
        return None


def sample_single(rs, params, frame_count, h, w, frame_wise_aug=False):
    """`single_train_dataloader.build_clip` (:65-146): one clip; the frames' channels are reversed (:124). Returns (frame_list, records) or None."""
    try:
        n = params.num_frames
        skip = params.fix_skip
        left_over = frame_count - params.fix_skip * n
        if left_over > 0:
            start = rs.randint(0, int(left_over))
        else:
            skip /= 2
            left_over = frame_count - skip * n
            start = rs.randint(0, int(left_over))
        frames = _frames(start, skip, n)
        if frames[-1] >= frame_count:
            frames[-1] = int(frame_count - 1)
        _check_frames(frames, frame_count)
        r = rs.rand(2, 10)
        x_erase = rs.randint(0, params.reso_w, size=(2,))
        y_erase = rs.randint(0, params.reso_h, size=(2,))
        cf = rs.uniform(params.min_crop_factor_training, 1, size=(2,))
        x0, y0 = _origin(rs, params, h, w, cf)
        col = _colour_draws(rs, params, h, w, 0, False)
        clip = []
        for f in frames:
            if frame_wise_aug:
                col = _colour_draws(rs, params, h, w, 0, True)
            if params.weak_aug:
                rec = frame_record(f, _box(params, h, w, cf[0], x0, y0), reverse=True)
            else:
                c, hu, s, b, g, es1, es2 = col
                rec = _strong(params, h, w, f, r[0], x_erase, y_erase, cf[0], x0, y0, c[0], hu[0], s[0], b[0], g[0], es1, es2, True)
            clip.append(rec)
        return frames, clip
    except Exception:
        return None


# ---- Pillow's resample tables -------------------------------------------------------------------------------------------------------

_PIL_TABLES = {}


def pil_table_fast(in_size: int, out_size: int):
    """`preprocess.pil_table` (libImaging/Resample.c precompute_coeffs + normalize_coeffs_8bpc, BILINEAR), cached per (in, out) and built with numpy
    over whole rows; the weight sum runs over the taps in order like the C loop, so the coefficients are the same integers."""
    key = (int(in_size), int(out_size))
    t = _PIL_TABLES.get(key)
    if t is not None:
        return t
    in_size, out_size = key
    scale = float(in_size) / float(out_size)
    filterscale = scale if scale >= 1.0 else 1.0
    support = 1.0 * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    x = np.arange(ksize, dtype=np.float64)[None, :]
    a = np.abs((x + xmin[:, None] - center[:, None] + 0.5) * ss)
    k = np.where(a < 1.0, 1.0 - a, 0.0)
    k[x >= xmax[:, None]] = 0.0
    ww = np.zeros(out_size, dtype=np.float64)
    for j in range(ksize):               # the C loop's order of additions
        ww = ww + k[:, j]
    k = np.where(ww[:, None] != 0.0, k / np.where(ww == 0.0, 1.0, ww)[:, None], k)
    v = k * (1 << PIL_PRECISION_BITS)
    kk = np.where(k < 0, -0.5 + v, 0.5 + v).astype(np.int64)       # C's truncating (int) cast
    kk[x >= xmax[:, None]] = 0
    tab = np.zeros((out_size, 2 + ksize), dtype=np.int32)
    tab[:, 0], tab[:, 1] = xmin, xmax
    tab[:, 2:] = kk
    t = (tab, ksize)
    _PIL_TABLES[key] = t
    return t


# ---- the launch --------------------------------------------------------------------------------------------------------------------

_KEEP = []           # the last launch's host blob: alive until the next one (the upload is asynchronous on the stream)


def build_table(videos, records, out, reso):
    """records[b][k] -> (blob uint8 array {records | tables | gamma tables}, nrec, tables_off, table_words, luts_off, nluts)."""
    oh, ow = int(reso[0]), int(reso[1])
    flat = [(b, k, r) for b, row in enumerate(records) for k, r in enumerate(row)]
    rec = np.zeros(len(flat), dtype=RECORD)
    tabs, tab_off, words = [], {}, 0
    luts, lut_idx = [], {}

    def table(in_size, out_size):
        nonlocal words
        key = (in_size, out_size)
        e = tab_off.get(key)
        if e is None:
            tab, ks = pil_table_fast(in_size, out_size)
            e = (words, ks)
            tab_off[key] = e
            tabs.append(tab.reshape(-1))
            words += tab.size
        return e

    sb, sk = out.stride(0), out.stride(1)
    for i, (b, k, r) in enumerate(flat):
        v = videos[r["video"]]
        t, h, w, _ = v.shape
        if not 0 <= r["frame"] < t:
            raise ValueError("augment_batch: record (%d, %d): frame %d outside the video's %d frames" % (b, k, r["frame"], t))
        top, left, ch, cw = r["box"]
        if top < 0 or left < 0:
            raise ValueError("augment_batch: record (%d, %d): negative crop origin (%d, %d)" % (b, k, top, left))
        if ch < 1 or cw < 1:
            raise ValueError("augment_batch: record (%d, %d): empty crop %d x %d" % (b, k, ch, cw))
        e = rec[i]
        e["src"] = v.data_ptr() + r["frame"] * h * w * 3
        e["dst"] = b * sb + k * sk
        e["H"], e["W"], e["top"], e["left"], e["ch"], e["cw"] = h, w, top, left, ch, cw
        (e["ytab"], e["ytaps"]), (e["xtab"], e["xtaps"]) = table(ch, oh), table(cw, ow)
        flags = 0
        if r.get("contrast") is not None:
            flags |= CONTRAST_LATE if r.get("contrast_late") else CONTRAST_FIRST
            e["contrast"] = r["contrast"]
        if r.get("hue") is not None:
            if not -0.5 <= r["hue"] <= 0.5:
                raise ValueError("augment_batch: hue_factor (%r) is not in [-0.5, 0.5]" % (r["hue"],))
            flags |= HUE
            e["hue_off"] = hue_offset(r["hue"])
        if r.get("saturation") is not None:
            flags |= SATURATION
            e["saturation"] = r["saturation"]
        if r.get("brightness") is not None:
            flags |= BRIGHTNESS
            e["brightness"] = r["brightness"]
        if r.get("gray"):
            flags |= GRAY
            if r.get("gamma") is not None:
                flags |= GAMMA
                g = r["gamma"]
                if g not in lut_idx:
                    lut_idx[g] = len(luts)
                    luts.append(gamma_lut(g))
                e["gamma_lut"] = lut_idx[g]
        elif r.get("gamma") is not None:
            raise ValueError("augment_batch: gamma applies only to a grayscale frame (ucf101_dl.py:616-619)")
        if r.get("hflip"):
            flags |= HFLIP
        if r.get("reverse"):
            flags |= REVERSE
        e["flags"] = flags
        er = list(r.get("erase", ()))
        if len(er) > 2:
            raise ValueError("augment_batch: at most two erase boxes per frame")
        for q, (ei, ej, eh, ew) in enumerate(er):
            if ei < 0 or ej < 0:
                raise ValueError("augment_batch: negative erase origin")
            e["erase"][4 * q:4 * q + 4] = (ei, ej, eh, ew)
    tables = np.concatenate(tabs).astype(np.int32)
    lut_bytes = np.concatenate(luts) if luts else np.zeros(0, np.uint8)
    blob = np.concatenate([rec.view(np.uint8).reshape(-1), tables.view(np.uint8), lut_bytes])
    tables_off = rec.nbytes
    return blob, len(flat), tables_off, tables.size, tables_off + tables.nbytes, len(luts)


def augment_batch(videos, records, out: torch.Tensor = None, reso=(224, 224)) -> torch.Tensor:
    """videos: list of contiguous (T, H, W, 3) uint8 CUDA tensors (decoded frames; sizes may differ). records[b][k]: the record (`frame_record`,
    `sample_*`) of output frame k of batch item b; rec["video"] indexes `videos`. Returns / fills the fp32 (B, n, 3, h, w) batch (`out` may be any
    view with those sizes whose strides are non-negative: only the elements of the B * n frames are written). One table upload and one launch on
    the current stream."""
    if not videos or not records or not records[0]:
        raise ValueError("augment_batch: no videos / records")
    for v in videos:
        require_cuda(v, "augment_batch")
        if v.dim() != 4 or v.shape[3] != 3 or v.dtype != torch.uint8 or not v.is_contiguous():
            raise ValueError("augment_batch: videos must be contiguous (T,H,W,3) uint8 tensors (PIL images are 8-bit)")
    oh, ow = int(reso[0]), int(reso[1])
    if oh < 1 or ow < 1:
        raise ValueError("augment_batch: bad resolution %r" % (reso,))
    B, n = len(records), len(records[0])
    if any(len(row) != n for row in records):
        raise ValueError("augment_batch: every batch item needs the same number of frames")
    shape = (B, n, 3, oh, ow)
    dev = videos[0].device
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    if tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != dev or any(s < 0 for s in out.stride()):
        raise ValueError("augment_batch: out must be fp32 %s on %s" % (shape, dev))
    blob, nrec, tables_off, table_words, luts_off, nluts = build_table(videos, records, out, (oh, ow))
    blob_dev = torch.empty(blob.nbytes, dtype=torch.uint8, device=dev)
    s = out.stride()
    span = 1 + sum((d - 1) * st for d, st in zip(shape, s))
    _KEEP[:] = [blob]
    check(_lib.lib().tedspad_clip_augment(blob.ctypes.data, blob_dev.data_ptr(), blob.nbytes, nrec, tables_off, table_words, luts_off, nluts,
                                          out.data_ptr(), span, oh, ow, s[2], s[3], s[4], _stream_ptr()), "tedspad_clip_augment")
    return out
