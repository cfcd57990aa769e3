"""Pillow reference for the training-clip augmentation (helper, not a test): the `torchvision.transforms.functional` calls that
`aux_code/ucf101_dl.py`'s two training loaders make on PIL images (augmentation :596-630 / :149-183, weak_augmentation :632-642), each mapped to the
Pillow call torchvision's PIL path makes. torchvision is not installed: the mapping is restated from its published 0.15.2 `_functional_pil.py` /
`functional.py` (the same standing as `preprocess.center_crop_box`); the ARITHMETIC is Pillow's own, called here, never restated:

    resized_crop      img.crop((left, top, left + w, top + h)).resize((ow, oh), BILINEAR)
    adjust_brightness / _saturation (Color) / _contrast      ImageEnhance.*(img).enhance(factor)
    adjust_hue        convert("HSV"), h += uint8(factor * 255) modulo 256, merge, convert("RGB")
    to_grayscale(3)   convert("L") stacked three times
    adjust_gamma      point(table * 3), table[e] = int((255 + 1 - 1e-3) * gain * pow(e / 255., gamma))
    hflip             transpose(FLIP_LEFT_RIGHT)
    to_tensor         uint8 (H, W, C) -> float32 (C, H, W) / 255
    erase             img[..., i:i+h, j:j+w] = v on a copy

The module doubles as the `functional` shim `tests/golden/make_aug_golden.py` hands to the reference's loader code (every call is appended to `CALLS`
when logging is on), and `apply_record` runs one of `ted_spad_amd.augment`'s per-frame records through the same functions, in the reference's order.
"""
import numpy as np
import torch
from PIL import Image, ImageEnhance

CALLS = None            # a list while make_aug_golden.py records; None otherwise


def _log(name, **kw):
    if CALLS is not None:
        CALLS.append((name, kw))


def synthetic_video(t, h, w, seed):
    """(t, h, w, 3) uint8 frames from integer arithmetic alone (reproduces anywhere): moving ramps, a coarse checker and hashed noise."""
    tt, yy, xx = np.meshgrid(np.arange(t, dtype=np.int64), np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), indexing="ij")
    n = (xx * 73856093) ^ (yy * 19349663) ^ (tt * 83492791) ^ (int(seed) * 2654435761)
    n = ((n & 0xFFFFFFFF) * 1103515245 + 12345) >> 16
    r = (xx * 3 + yy + tt * 5 + seed * 17 + (n & 31)) % 256
    g = ((xx * xx) // 97 + yy * 2 + tt * 11 + seed * 29 + ((n >> 5) & 15)) % 256
    b = ((yy * 255) // max(h - 1, 1) + 96 * (((xx // 16) + (yy // 16) + tt) & 1) + ((n >> 9) & 63)) % 256
    return np.stack([r, g, b], axis=-1).astype(np.uint8)


def hue_offset(hue_factor):
    """uint8(hue_factor * 255) as the reference environment's numpy 1.x computes it: truncation towards zero, then modulo 256."""
    return int(float(hue_factor) * 255) % 256


def gamma_table(gamma, gain=1):
    return [int((255 + 1 - 1e-3) * gain * pow(ele / 255.0, gamma)) for ele in range(256)]


# ---- the functional shim ------------------------------------------------------------------------------------------------------------

def to_pil_image(pic):
    """ToPILImage for a (C, H, W) uint8 tensor / array."""
    a = pic.numpy() if isinstance(pic, torch.Tensor) else np.asarray(pic)
    assert a.dtype == np.uint8 and a.ndim == 3 and a.shape[0] == 3
    return Image.fromarray(np.ascontiguousarray(a.transpose(1, 2, 0)), "RGB")


def resized_crop(img, top, left, height, width, size, antialias=True):
    _log("resized_crop", top=int(top), left=int(left), height=int(height), width=int(width), size=[int(size[0]), int(size[1])])
    top, left, height, width = int(top), int(left), int(height), int(width)
    return img.crop((left, top, left + width, top + height)).resize((int(size[1]), int(size[0])), Image.BILINEAR)


def adjust_contrast(img, contrast_factor):
    _log("adjust_contrast", factor=float(contrast_factor))
    return ImageEnhance.Contrast(img).enhance(float(contrast_factor))


def adjust_saturation(img, saturation_factor):
    _log("adjust_saturation", factor=float(saturation_factor))
    return ImageEnhance.Color(img).enhance(float(saturation_factor))


def adjust_brightness(img, brightness_factor):
    _log("adjust_brightness", factor=float(brightness_factor))
    return ImageEnhance.Brightness(img).enhance(float(brightness_factor))


def adjust_hue(img, hue_factor):
    _log("adjust_hue", factor=float(hue_factor))
    if not -0.5 <= hue_factor <= 0.5:
        raise ValueError("hue_factor (%r) is not in [-0.5, 0.5]" % (hue_factor,))
    h, s, v = img.convert("HSV").split()
    np_h = (np.array(h, dtype=np.uint8).astype(np.int64) + hue_offset(hue_factor)) % 256
    h = Image.fromarray(np_h.astype(np.uint8), "L")
    return Image.merge("HSV", (h, s, v)).convert("RGB")


def to_grayscale(img, num_output_channels=1):
    _log("to_grayscale", num_output_channels=int(num_output_channels))
    assert num_output_channels == 3
    l = np.array(img.convert("L"), dtype=np.uint8)
    return Image.fromarray(np.dstack([l, l, l]), "RGB")


def adjust_gamma(img, gamma, gain=1):
    _log("adjust_gamma", gamma=float(gamma), gain=float(gain))
    return img.point(gamma_table(float(gamma), gain) * 3)


def hflip(img):
    _log("hflip")
    return img.transpose(Image.FLIP_LEFT_RIGHT)


def to_tensor(img):
    _log("to_tensor")
    a = np.array(img, dtype=np.uint8)
    return torch.from_numpy(a).permute(2, 0, 1).contiguous().to(torch.float32).div(255)


def erase(img, i, j, h, w, v=0, inplace=False):
    _log("erase", i=int(i), j=int(j), h=int(h), w=int(w), v=float(v))
    img = img.clone()
    img[..., int(i):int(i) + int(h), int(j):int(j) + int(w)] = v
    return img


# ---- one per-frame record of ted_spad_amd.augment through the chain above -------------------------------------------------------------

def apply_record(frame_hwc, rec, reso):
    """frame_hwc: (H, W, 3) uint8 array; rec: a record of ted_spad_amd.augment.sample_* / frame_record; reso: (oh, ow). Returns the fp32 (3, oh, ow)
    tensor the reference's augmentation / weak_augmentation returns for those parameters."""
    a = np.asarray(frame_hwc)
    if rec.get("reverse"):
        a = a[:, :, ::-1]
    img = Image.fromarray(np.ascontiguousarray(a), "RGB")
    top, left, ch, cw = rec["box"]
    img = resized_crop(img, top, left, ch, cw, reso)
    if rec.get("contrast") is not None and not rec.get("contrast_late"):
        img = adjust_contrast(img, rec["contrast"])
    if rec.get("hue") is not None:
        img = adjust_hue(img, rec["hue"])
    if rec.get("saturation") is not None:
        img = adjust_saturation(img, rec["saturation"])
    if rec.get("brightness") is not None:
        img = adjust_brightness(img, rec["brightness"])
    if rec.get("contrast") is not None and rec.get("contrast_late"):
        img = adjust_contrast(img, rec["contrast"])
    if rec.get("gray"):
        img = to_grayscale(img, 3)
        if rec.get("gamma") is not None:
            img = adjust_gamma(img, rec["gamma"], 1)
    if rec.get("hflip"):
        img = hflip(img)
    x = to_tensor(img)
    for (i, j, h, w) in rec.get("erase", ()):
        x = erase(x, i, j, h, w, 0)
    return x


def apply_records(videos, records, reso):
    """videos: list of (T, H, W, 3) uint8 arrays; records: records[b][k] with rec["video"] / rec["frame"]. -> fp32 (B, n, 3, oh, ow)."""
    out = torch.empty((len(records), len(records[0]), 3, reso[0], reso[1]), dtype=torch.float32)
    for b, row in enumerate(records):
        for k, rec in enumerate(row):
            out[b, k] = apply_record(videos[rec["video"]][rec["frame"]], rec, reso)
    return out
