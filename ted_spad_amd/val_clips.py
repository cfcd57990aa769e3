"""Validation clips on the device: the build's counterpart of the two validation loaders of aux_code/ucf101_dl.py (`single_val_dataloader` :199-320,
`contrastive_val_dataloader` :646-896), whose batches decide which checkpoint is kept. The reference runs center_crop -> resize -> hflip -> to_tensor on a
PIL image per frame, `num_modes` times over the test list in every validation epoch; here decoded uint8 frames stay in HBM and ONE launch
(tedspad_val_clips / tedspad_val_clips_act, csrc/val_clips.hip) writes either the fp32 `(B, n, 3, h, w)` batch `ActionValidator.evaluate` takes or, with an
anonymizer in front, the 16-bit activation its first conv reads (`ActionValidator.evaluate_frames`), bit-identical to the Pillow chain.

Two halves, as in `augment`:

* `sample_val_single` / `sample_val_contrastive` restate the two `build_clip` bodies statement for statement -- the `np.linspace(0, F - 10, num_modes)[mode]`
  starts, the halved (float) skip, `start < 0 -> mode`, the last-index clamp only the contrastive loader has, the `temporal_distance` branch, the third
  clip's random start -- and return per-frame `augment.frame_record` dicts. `val_box` is the crop both `augmentation` bodies take, the single loader's swapped
  height / width read (:284) included; `center_crop_box_padded` is torchvision 0.15.2's `center_crop` with its zero-padding branch.
* `val_clips` / `val_clips_act` turn records into the kernel's record table and launch.

`threeCrop` is not offered: no script passes it; `five_crop` is called with the size of the image it is given (:307, :883), so the "three crops" are three
copies of one picture; with `no_ar_distortion` that size differs from the image's and five_crop raises; and the single loader appends the 3-tuples
`augmentation` then returns to the clip, which `collate_fn_val` cannot stack.

torchvision is not installed here; what `center_crop` / `resize` do with a PIL image is restated from its published 0.15.2 `functional.py` (the standing of
`preprocess.center_crop_box`). The arithmetic is Pillow's, which is installed and pins the kernel bit for bit (tests/val_clips_ref.py).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._lib import check
from .augment import HFLIP, REVERSE, _check_frames, _frames, frame_record, pil_table_fast
from .engine import DTYPES, Act, _stream_ptr, require_cuda

# tedspad_val_record (include/tedspad_hip.h)
RECORD = np.dtype([("src", "<u8"), ("dst", "<i8"), ("H", "<i4"), ("W", "<i4"), ("top", "<i4"), ("left", "<i4"), ("ch", "<i4"), ("cw", "<i4"),
                   ("ytab", "<i4"), ("xtab", "<i4"), ("ytaps", "<i4"), ("xtaps", "<i4"), ("flags", "<i4"), ("reserved", "<i4")])
assert RECORD.itemsize == 64


# ---- the crop ---------------------------------------------------------------------------------------------------------------------------

def center_crop_box_padded(h: int, w: int, ch: int, cw: int):
    """torchvision 0.15.2 `center_crop` of an (h, w) image to (ch, cw), as the (top, left, ch, cw) box in the coordinates of the UNPADDED frame: where the
    crop is larger than the image it first pads with zeros, padding_ltrb = [(cw-w)//2, (ch-h)//2, (cw-w+1)//2, (ch-h+1)//2] on the sides concerned, then takes
    crop_top = int(round((H' - ch) / 2.0)) of the padded size (Python round: half to even), the same for crop_left. top / left are negative where it padded;
    pixels outside the frame are zero. Equals `preprocess.center_crop_box` wherever that does not raise."""
    h, w, ch, cw = int(h), int(w), int(ch), int(cw)
    pad_l = (cw - w) // 2 if cw > w else 0
    pad_t = (ch - h) // 2 if ch > h else 0
    pad_r = (cw - w + 1) // 2 if cw > w else 0
    pad_b = (ch - h + 1) // 2 if ch > h else 0
    hp, wp = h + pad_t + pad_b, w + pad_l + pad_r
    return int(round((hp - ch) / 2.0)) - pad_t, int(round((wp - cw) / 2.0)) - pad_l, ch, cw


def val_box(params, h: int, w: int, cropping_factor=0.8, loader: str = "contrastive"):
    """The box `augmentation` (:297-304 / :873-880) crops from an (h, w) frame. loader 'single' reads `ori_reso_w, ori_reso_h = frames.shape[1:3]` (:284), so
    its crop is int(w * factor) rows by int(h * factor) columns: (-8, 64, 256, 192) for 240 x 320 at 0.8; 'contrastive' reads them straight (:797).
    cropping_factor > 1: no crop."""
    if loader not in ("single", "contrastive"):
        raise ValueError("val_box: loader must be 'single' or 'contrastive', got %r" % (loader,))
    if cropping_factor > 1:
        return (0, 0, int(h), int(w))
    ori_h, ori_w = (w, h) if loader == "single" else (h, w)
    if params.no_ar_distortion:
        m = min(ori_h, ori_w)
        ch = cw = int(m * cropping_factor)
    else:
        ch, cw = int(ori_h * cropping_factor), int(ori_w * cropping_factor)
    return center_crop_box_padded(h, w, ch, cw)


def val_reso(params, cropping_factor=0.8):
    """(output_reso_h, output_reso_w) of both loaders' __init__ (:228-233): the 1 / 0.8 larger output exactly when the factor == 1."""
    if cropping_factor == 1:
        return int(params.reso_h / 0.8), int(params.reso_w / 0.8)
    return int(params.reso_h), int(params.reso_w)


# ---- frame sampling ---------------------------------------------------------------------------------------------------------------------

def _records(frames, box, hflip):
    return [frame_record(int(f), box, hflip=hflip != 0, reverse=True) for f in frames]


def sample_val_single(params, frame_count, h, w, mode, hflip=0, cropping_factor=0.8):
    """`single_val_dataloader.build_clip` (:253-294) without the pixels: (frame_list, records), or None where the reference's except returns None (an
    index outside the video: decord raises)."""
    try:
        N, n = frame_count, params.num_frames
        skip = params.fix_skip
        if skip * n > N:
            skip /= 2
        left_over = skip * n
        F = N - left_over
        start = 0 + int(np.linspace(0, F - 10, params.num_modes)[mode])
        if start < 0:
            start = mode
        frames = _frames(start, skip, n)
        _check_frames(frames, frame_count)
        return frames, _records(frames, val_box(params, h, w, cropping_factor, "single"), hflip)
    except Exception:
        return None


def sample_val_contrastive(rs, params, frame_count, h, w, mode, hflip=0, cropping_factor=0.8):
    """`contrastive_val_dataloader.build_clip` + `process_data` (:689-870) without the pixels: (frame_lists, records) of 2 clips (3 with temporal_loss
    'trip') in the order process_data extends them, or None where the reference gives up. `rs` is a numpy.random.RandomState standing where the reference uses
    the global generator: the third clip's start is its only draw, and nothing is drawn with a temporal distance. The frame LISTS are the reference's, the
    RECORDS are the frames its clips are really made of: with temporal_align clip 2 is built from clip 1's frames whatever list 2 says."""
    try:
        N, n = frame_count, params.num_frames
        trip = params.temporal_loss == 'trip'
        skip = params.fix_skip
        if skip * n > N:
            skip /= 2
        temporal_align = params.temporal_align
        if trip:
            temporal_align = True
        frames2 = None
        if params.temporal_distance:
            left_over = N - n * skip
            left_over2 = left_over - skip * n - params.temporal_distance
            if left_over2 < 0:
                return None
            start = 0 + int(np.linspace(0, left_over2 - 1, params.num_modes)[mode])
            start2 = start + (n - 1) * skip + params.temporal_distance
            frames2 = _frames(start2, skip, n)
        else:
            left_over = skip * n
            F = N - left_over
            start = 0 + int(np.linspace(0, F - 10, params.num_modes)[mode])
            if start < 0:
                start = mode
            if not temporal_align:
                start2 = 0 + int(np.linspace(0, F - 10, params.num_modes)[mode])          # (no fallback for this one)
                frames2 = _frames(start2, skip, n)
        frames1 = _frames(start, skip, n)
        if frames1[-1] >= frame_count:
            frames1[-1] = int(frame_count - 1)
        if not temporal_align:
            if frames2[-1] >= frame_count:
                frames2[-1] = int(frame_count - 1)
        if trip:
            frames2 = frames1
            if params.temporal_distance:
                start3 = start2
            else:
                start3 = rs.randint(0, int(left_over))
            frames3 = _frames(start3, skip, n)
            if frames3[-1] >= frame_count:
                frames3[-1] = int(frame_count - 1)
        if frames2 is None:
            raise NameError("frames_full2")          # (:789: temporal_align without 'trip' or a temporal distance never defines it)
        _check_frames(frames1, frame_count)
        if not temporal_align:
            _check_frames(frames2, frame_count)
        if trip:
            _check_frames(frames3, frame_count)
        box = val_box(params, h, w, cropping_factor, "contrastive")
        lists = [frames1, frames2] + ([frames3] if trip else [])
        pixels = [frames1, frames1 if temporal_align else frames2] + ([frames3] if trip else [])
        return lists, [_records(f, box, hflip) for f in pixels]
    except Exception:
        return None


# ---- the launch -------------------------------------------------------------------------------------------------------------------------

_KEEP = []           # the last launch's host blob: alive until the next one (the upload is asynchronous on the stream)
_BANDS = {}          # (crop heights, oh, ow, cpad) -> band: a validation pass asks for the same few boxes batch after batch


def band_height(records, reso, cpad: int = 0) -> int:
    """Output rows per workgroup for these records: the largest band (at most tedspad_val_clips_band_max()) whose temporary rows -- three planes of `ow`
    bytes per row the band's vertical taps reach, over the worst record and band -- and, in the activation form (cpad 4 / 8), whose packed output rows fit the
    kernel's LDS budget. 1 where even one row does not fit: the entry then refuses."""
    oh, ow = int(reso[0]), int(reso[1])
    key = (frozenset(r["box"][2] for row in records for r in row), oh, ow, cpad)
    band = _BANDS.get(key)
    if band is not None:
        return band
    lib = _lib.lib()
    budget, band = lib.tedspad_val_clips_lds_bytes(), min(lib.tedspad_val_clips_band_max(), oh)
    spans = []
    for ch in key[0]:
        tab, _ = pil_table_fast(ch, oh)
        spans.append((tab[:, 0].astype(np.int64), tab[:, 0].astype(np.int64) + tab[:, 1]))
    while band > 1:
        first = np.arange(0, oh, band)
        last = np.minimum(first + band, oh) - 1
        trows = max(int((hi[last] - lo[first]).max()) for lo, hi in spans)
        if band * ow * cpad * 2 + 3 * trows * ow <= budget:
            break
        band -= 1
    _BANDS[key] = band
    return band


def _build_table(who, videos, records, reso, dst):
    """records[b][k] -> (blob uint8 array {records | tables}, nrec, tables_off, table_words); dst(b, k): the record's output offset."""
    oh, ow = reso
    tabs, tab_off, words = [], {}, 0

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

    vinfo = [(v.data_ptr(),) + tuple(v.shape[:3]) for v in videos]
    rows = []
    for b, row in enumerate(records):
        for k, r in enumerate(row):
            ptr, t, h, w = vinfo[r["video"]]
            frame = r["frame"]
            if not 0 <= frame < t:
                raise ValueError("%s: record (%d, %d): frame %d outside the video's %d frames" % (who, b, k, frame, t))
            top, left, ch, cw = r["box"]
            if ch < 1 or cw < 1:
                raise ValueError("%s: record (%d, %d): empty crop %d x %d" % (who, b, k, ch, cw))
            if (r.get("contrast") is not None or r.get("hue") is not None or r.get("saturation") is not None or r.get("brightness") is not None or
                    r.get("gamma") is not None or r.get("gray") or r.get("erase")):
                raise ValueError("%s: record (%d, %d): the validation loaders have no colour ops and no erase (augment.augment_batch has)" % (who, b, k))
            (ytab, ytaps), (xtab, xtaps) = table(ch, oh), table(cw, ow)
            rows.append((ptr + frame * h * w * 3, dst(b, k), h, w, top, left, ch, cw, ytab, xtab, ytaps, xtaps,
                         (HFLIP if r.get("hflip") else 0) | (REVERSE if r.get("reverse") else 0), 0))
    rec = np.array(rows, dtype=RECORD)
    tables = np.concatenate(tabs).astype(np.int32)
    blob = np.concatenate([rec.view(np.uint8).reshape(-1), tables.view(np.uint8)])
    return blob, len(rows), rec.nbytes, tables.size


def _check_inputs(who, videos, records, reso):
    if not videos or not records or not records[0]:
        raise ValueError("%s: no videos / records" % who)
    for v in videos:
        require_cuda(v, who)
        if v.dim() != 4 or v.shape[3] != 3 or v.dtype != torch.uint8 or not v.is_contiguous():
            raise ValueError("%s: videos must be contiguous (T,H,W,3) uint8 tensors (PIL images are 8-bit)" % who)
    oh, ow = int(reso[0]), int(reso[1])
    if oh < 1 or ow < 1:
        raise ValueError("%s: bad resolution %r" % (who, reso))
    n = len(records[0])
    if any(len(row) != n for row in records):
        raise ValueError("%s: every batch item needs the same number of frames" % who)
    return oh, ow, len(records), n


def val_clips(videos, records, reso, out: torch.Tensor = None) -> torch.Tensor:
    """videos: list of contiguous (T, H, W, 3) uint8 CUDA tensors (decoded frames; sizes may differ). records[b][k]: the record (`sample_val_*`,
    `augment.frame_record`; box origins may be negative) of output frame k of batch item b; rec["video"] indexes `videos`. Returns / fills the fp32
    (B, n, 3, oh, ow) batch `ActionValidator.evaluate` takes (`out`: any view of those sizes with non-negative strides; only the B * n frames are
    written). One table upload and one launch on the current stream."""
    who = "val_clips"
    oh, ow, B, n = _check_inputs(who, videos, records, reso)
    shape = (B, n, 3, oh, ow)
    dev = videos[0].device
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    if tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != dev or any(s < 0 for s in out.stride()):
        raise ValueError("%s: out must be fp32 %s on %s" % (who, shape, dev))
    s = out.stride()
    blob, nrec, tables_off, table_words = _build_table(who, videos, records, (oh, ow), lambda b, k: b * s[0] + k * s[1])
    blob_dev = torch.empty(blob.nbytes, dtype=torch.uint8, device=dev)
    span = 1 + sum((d - 1) * st for d, st in zip(shape, s))
    _KEEP[:] = [blob]
    check(_lib.lib().tedspad_val_clips(blob.ctypes.data, blob_dev.data_ptr(), blob.nbytes, nrec, tables_off, table_words, out.data_ptr(), span, oh, ow,
                                       band_height(records, (oh, ow)), s[2], s[3], s[4], _stream_ptr()), "tedspad_val_clips")
    return out


def val_clips_act(videos, records, reso, cpad: int, dtype: str, out: torch.Tensor = None) -> Act:
    """The same frames as the input activation of the anonymizer for the pseudo-images the validation loops hand it: bit-identical to
    `engine.clip_to_act(AnonymizerTrainStep._feed(val_clips(...))[0].unsqueeze(2), cpad, dtype)` -- (B*n, 1, oh, ow/2, 8) for cpad 4, (B*n, 1, oh, ow, 8) for
    cpad 8 -- without the fp32 batch or its permuted copy ever being written. `out`: a contiguous 16-bit tensor of that shape to fill."""
    who = "val_clips_act"
    oh, ow, B, n = _check_inputs(who, videos, records, reso)
    if cpad not in (4, 8):
        raise ValueError("%s: cpad must be 4 (pixel pairs) or 8" % who)
    if cpad == 4 and ow % 2:
        raise ValueError("%s: cpad=4 packs pixel pairs, the output width %d must be even" % (who, ow))
    tdt, code = DTYPES[dtype]
    dev = videos[0].device
    shape = (B * n, 1, oh, ow // 2 if cpad == 4 else ow, 8)
    if out is None:
        out = torch.empty(shape, dtype=tdt, device=dev)
    if tuple(out.shape) != shape or out.dtype != tdt or out.device != dev or not out.is_contiguous():
        raise ValueError("%s: out must be a contiguous %s tensor of %s on %s" % (who, shape, tdt, dev))
    blob, nrec, tables_off, table_words = _build_table(who, videos, records, (oh, ow), lambda b, k: 0)
    blob_dev = torch.empty(blob.nbytes, dtype=torch.uint8, device=dev)
    _KEEP[:] = [blob]
    check(_lib.lib().tedspad_val_clips_act(blob.ctypes.data, blob_dev.data_ptr(), blob.nbytes, nrec, tables_off, table_words, out.data_ptr(),
                                           out.numel() * 2, n, oh, ow, band_height(records, (oh, ow), cpad), cpad, code, _stream_ptr()),
          "tedspad_val_clips_act")
    return Act(out, 8, 0, cpad)
