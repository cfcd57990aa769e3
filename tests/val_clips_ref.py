"""Pillow reference for the validation clips (helper, not a test): `augment_ref` plus the three `torchvision.transforms.functional` calls the two
validation loaders of `aux_code/ucf101_dl.py` make on PIL images (:297-320 / :873-896) that the training shim lacks, each mapped to the Pillow call
torchvision 0.15.2's PIL path makes (restated from its published `functional.py` / `_functional_pil.py`, the standing of `augment_ref`); the arithmetic is
Pillow's own, called here:

    center_crop   where the crop is larger than the image: ImageOps.expand(border=(l, t, r, b), fill=0) with padding_ltrb = [(cw-w)//2, (ch-h)//2,
                  (cw-w+1)//2, (ch-h+1)//2]; then img.crop at int(round((H' - ch) / 2.0)), int(round((W' - cw) / 2.0))
    resize        img.resize((w, h), BILINEAR)          (antialias has no meaning for a PIL image)
    five_crop     only so that the reference module imports and a stray call is seen in the log

Everything of `augment_ref` is re-exported, so this module is the `functional` shim `tests/golden/make_val_clip_golden.py` hands to the reference's
loader code; calls are appended to `augment_ref.CALLS` like the others. `apply_val_record` runs one record of `ted_spad_amd.val_clips` through them.
"""
import numpy as np
from PIL import Image, ImageOps

import augment_ref
from augment_ref import *  # noqa: F401,F403  (the shim: to_pil_image, hflip, to_tensor, synthetic_video, ...)
from augment_ref import _log, hflip, to_tensor


def center_crop(img, output_size):
    ch, cw = int(output_size[0]), int(output_size[1])
    _log("center_crop", output_size=[ch, cw])
    w, h = img.size
    if cw > w or ch > h:
        ltrb = ((cw - w) // 2 if cw > w else 0, (ch - h) // 2 if ch > h else 0, (cw - w + 1) // 2 if cw > w else 0, (ch - h + 1) // 2 if ch > h else 0)
        img = ImageOps.expand(img, border=ltrb, fill=0)
        w, h = img.size
        if cw == w and ch == h:
            return img
    top, left = int(round((h - ch) / 2.0)), int(round((w - cw) / 2.0))
    return img.crop((left, top, left + cw, top + ch))


def resize(img, size, antialias=True):
    _log("resize", size=[int(size[0]), int(size[1])])
    return img.resize((int(size[1]), int(size[0])), Image.BILINEAR)


def five_crop(img, size):
    _log("five_crop", size=[int(size[0]), int(size[1])])
    raise NotImplementedError("threeCrop is not offered (ted_spad_amd/val_clips.py)")


def padded_crop(img, box):
    """A (top, left, ch, cw) box that may leave the image on any side: zero borders (ImageOps.expand) where it does, then crop."""
    top, left, ch, cw = (int(v) for v in box)
    w, h = img.size
    ltrb = (max(0, -left), max(0, -top), max(0, left + cw - w), max(0, top + ch - h))
    if any(ltrb):
        img = ImageOps.expand(img, border=ltrb, fill=0)
    left, top = left + ltrb[0], top + ltrb[1]
    return img.crop((left, top, left + cw, top + ch))


def apply_val_record(frame_hwc, rec, reso, center=False):
    """frame_hwc: (H, W, 3) uint8 array; rec: a record of ted_spad_amd.val_clips.sample_val_* / augment.frame_record; reso: (oh, ow). Returns the fp32
    (3, oh, ow) tensor the loaders' `augmentation` returns. center=True takes the crop through `center_crop` itself, as the loaders do for
    cropping_factor <= 1 (the call is logged), and requires the record's box to be the one that call takes; otherwise the box is cropped as it stands."""
    a = np.asarray(frame_hwc)
    if rec.get("reverse"):
        a = a[:, :, ::-1]
    img = Image.fromarray(np.ascontiguousarray(a), "RGB")
    top, left, ch, cw = rec["box"]
    want = padded_crop(img, rec["box"])
    if center:
        img = center_crop(img, (ch, cw))
        assert img.size == want.size and img.tobytes() == want.tobytes(), "the record's box %r is not center_crop's" % (rec["box"],)
    else:
        img = want
    img = resize(img, reso)
    if rec.get("hflip"):
        img = hflip(img)
    return to_tensor(img)


def apply_val_records(videos, records, reso):
    """videos: list of (T, H, W, 3) uint8 arrays; records[b][k] with rec["video"] / rec["frame"]. -> fp32 (B, n, 3, oh, ow)."""
    import torch
    out = torch.empty((len(records), len(records[0]), 3, reso[0], reso[1]), dtype=torch.float32)
    for b, row in enumerate(records):
        for k, rec in enumerate(row):
            out[b, k] = apply_val_record(videos[rec["video"]][rec["frame"]], rec, reso)
    return out
