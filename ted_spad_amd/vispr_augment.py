"""VISPR views on the device: the build's counterpart of the augmentation of aux_code/vispr_dl.py (`vispr_dataset.augmentation` :71-129,
`vispr_ssl_dataset.augmentation` :186-251). The reference runs torchvision's float-tensor ops on the host for every image of every iteration; here the
decoded uint8 `(3, H, W)` images stay in HBM and ONE launch (tedspad_image_augment, csrc/augment_image.hip) writes the fp32 `(V, N, 3, h, w)` views:
`out[0]` is what `PrivacyTrainStep.step / evaluate` take, `out[0], out[1]` the `inputs_vispr` of `AnonymizerTrainStep.step_fa / step_ft`.

Two halves, as in `augment.py`:

* `sample_vispr` / `sample_vispr_ssl` draw one image's parameters from a `numpy.random.RandomState` in exactly the order, and with exactly the calls, of
  the two `augmentation` bodies (same seed -> same parameters as the reference) and return records (plain dicts, `image_record`); `center_record` is
  their non-train branch.
* `augment_images` turns records into the kernel's record table and launches.

`read_image` returns a uint8 tensor, so the reference's calls take torchvision's TENSOR path: an fp32 antialiased resize rounded once, fp32 blends
truncated to a byte, an fp32 HSV round trip. torchvision is not installed here; what its 0.15.2 `_functional_tensor.py` does is restated in
tests/vispr_ref.py with torch CPU ops, and torch itself pins the arithmetic (tests/test_hip_vispr_augment.py).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._lib import check
from .augment import BRIGHTNESS, CONTRAST_FIRST, CONTRAST_LATE, GAMMA, GRAY, HFLIP, HUE, SATURATION
from .engine import _stream_ptr, require_cuda
from .preprocess import aa_table_host

# tedspad_image_record (include/tedspad_hip.h)
RECORD = np.dtype([("src", "<u8"), ("dst", "<i8"), ("tmp", "<i8"), ("H", "<i4"), ("W", "<i4"), ("top", "<i4"), ("left", "<i4"), ("ch", "<i4"),
                   ("cw", "<i4"), ("ytab", "<i4"), ("xtab", "<i4"), ("ytaps", "<i4"), ("xtaps", "<i4"), ("flags", "<i4"), ("gamma_lut", "<i4"),
                   ("contrast", "<f4"), ("contrast_1m", "<f4"), ("saturation", "<f4"), ("saturation_1m", "<f4"), ("brightness", "<f4"),
                   ("brightness_1m", "<f4"), ("hue", "<f4"), ("erase", "<i4", (4,)), ("reserved", "<i4")])
assert RECORD.itemsize == 120

ERASE_SIZE = 19          # vispr_dl.py:35


# ---- parameters -------------------------------------------------------------------------------------------------------------------

def gamma_lut(gamma, gain=1) -> np.ndarray:
    """adjust_gamma's tensor path for each of the 256 bytes, computed with torch's own CPU ops (so the table is whatever the host's `pow` gives):
    byte / 255 -> (gain * x ** gamma).clamp(0, 1) -> * (255 + 1.0 - 1e-3) -> uint8."""
    x = torch.arange(256, dtype=torch.uint8).to(torch.float32) / 255.0
    return (gain * x ** float(gamma)).clamp(0, 1).mul(255 + 1.0 - 1e-3).to(torch.uint8).numpy()


def image_record(image, box, contrast=None, contrast_late=False, hue=None, saturation=None, brightness=None, gray=False, gamma=None, hflip=False,
                 erase=()):
    """One output view: source image `image`, crop `box` = (top, left, height, width) (may overflow right / bottom), the ops that apply (None / False:
    skipped) in the reference's fixed order, and at most one erase box (i = row, j = column, h, w)."""
    return {"image": int(image), "box": tuple(int(v) for v in box), "contrast": None if contrast is None else float(contrast),
            "contrast_late": bool(contrast_late), "hue": None if hue is None else float(hue),
            "saturation": None if saturation is None else float(saturation), "brightness": None if brightness is None else float(brightness),
            "gray": bool(gray), "gamma": None if gamma is None else float(gamma), "hflip": bool(hflip),
            "erase": [tuple(int(v) for v in e) for e in erase]}


def _draws(rs, h, w, reso, count):
    """the draws in front of the per-view loop (:76-89 / :192-205). x0, y0 come from cropping_factor1[0] whichever view uses them."""
    x_erase = rs.randint(0, reso[0], size=(count,))
    y_erase = rs.randint(0, reso[1], size=(count,))
    cf = rs.uniform(0.6, 1, size=(count,))
    x0 = rs.randint(0, w - w * cf[0] + 1)
    y0 = rs.randint(0, h - h * cf[0] + 1)
    contrast = rs.uniform(0.9, 1.1, size=(count,))
    hue = rs.uniform(-0.05, 0.05, size=(count,))
    saturation = rs.uniform(0.9, 1.1, size=(count,))
    brightness = rs.uniform(0.9, 1.1, size=(count,))
    gamma = rs.uniform(0.85, 1.15, size=(count,))
    es1 = rs.randint(int(ERASE_SIZE / 2), ERASE_SIZE, size=(count,))
    es2 = rs.randint(int(ERASE_SIZE / 2), ERASE_SIZE, size=(count,))
    rs.randint(0, 3, (count,))          # random_color_dropped: drawn, never used
    return x_erase, y_erase, cf, x0, y0, contrast, hue, saturation, brightness, gamma, es1, es2


def _view(d, i, r, h, w, image):
    """one pass of the op list (:95-120 / :213-238) for view i: which op runs is decided by `r` = rand(8). `x_erase` is passed as erase's ROW, and the
    erase shares r[6] with the flip (below 0.25 / above 0.5), so a view is never flipped and erased."""
    x_erase, y_erase, cf, x0, y0, contrast, hue, saturation, brightness, gamma, es1, es2 = d
    first, late = r[0] < 0.125 / 2, (r[0] > 0.125 / 2 and r[0] < 0.25 / 2)
    gray = r[4] > 0.9
    return image_record(image, (y0, x0, int(h * cf[i]), int(w * cf[i])), contrast=contrast[i] if (first or late) else None, contrast_late=late,
                        hue=hue[i] if r[1] < 0.3 / 2 else None, saturation=saturation[i] if r[2] < 0.3 / 2 else None,
                        brightness=brightness[i] if r[3] < 0.3 / 2 else None, gray=gray, gamma=gamma[i] if (gray and r[5] > 0.25) else None,
                        hflip=r[6] > 0.5, erase=[(x_erase[i], y_erase[i], es1[i], es2[i])] if r[6] < 0.5 / 2 else [])


def sample_vispr(rs, h, w, reso=(224, 224), image=0):
    """`vispr_dataset.augmentation`, train split (:73-120), without the pixels: `rs` is a numpy.random.RandomState standing where the reference uses the
    global numpy generator; `reso` = (params.reso_h, params.reso_w). Every draw has size (2,) and index 0 is used. Returns one record."""
    d = _draws(rs, h, w, reso, 2)
    return _view(d, 0, rs.rand(8), h, w, image)


def sample_vispr_ssl(rs, h, w, reso=(224, 224), image=0, augmentation_count=2):
    """`vispr_ssl_dataset.augmentation`, train split (:188-240): `augmentation_count` views of one image. The origin x0, y0 is drawn for
    cropping_factor1[0] and shared, but view i crops with cropping_factor1[i], so a later view can overflow the image (zero fill). One rand(8) per
    view, drawn inside the loop. Returns the list of records."""
    d = _draws(rs, h, w, reso, augmentation_count)
    return [_view(d, i, rs.rand(8), h, w, image) for i in range(augmentation_count)]


def center_record(h, w, image=0):
    """the non-train branch (:122-127 / :242-249): center_crop(min(h, w)) with torchvision's int(round((h - side) / 2.0)) origin (Python's round: half
    to even), then the resize."""
    side = min(h, w)
    return image_record(image, (int(round((h - side) / 2.0)), int(round((w - side) / 2.0)), side, side))


# ---- the launch --------------------------------------------------------------------------------------------------------------------

_AA_TABLES = {}
_KEEP = []           # the last launch's host blob: alive until the next one (the upload is asynchronous on the stream)


def _aa_table(in_size, out_size):
    key = (int(in_size), int(out_size))
    t = _AA_TABLES.get(key)
    if t is None:
        t = aa_table_host(*key)
        _AA_TABLES[key] = t
    return t


def _f32(v):
    return float(np.float32(v))


def build_table(images, records, out_strides, reso):
    """records[v][n] -> (blob uint8 array {records | tables | gamma tables}, nrec, tables_off, table_words, luts_off, nluts, scratch_elems). Every
    record is checked before a table is built (ValueError)."""
    oh, ow = int(reso[0]), int(reso[1])
    flat = [(v, n, r) for v, row in enumerate(records) for n, r in enumerate(row)]
    for v, n, r in flat:
        who = "augment_images: record (%d, %d)" % (v, n)
        if not 0 <= r["image"] < len(images):
            raise ValueError("%s: image %d of %d" % (who, r["image"], len(images)))
        _, h, w = images[r["image"]].shape
        top, left, ch, cw = r["box"]
        if top < 0 or left < 0:
            raise ValueError("%s: negative crop origin (%d, %d)" % (who, top, left))
        if ch < 1 or cw < 1:
            raise ValueError("%s: empty crop %d x %d" % (who, ch, cw))
        if top >= h or left >= w:
            raise ValueError("%s: crop origin (%d, %d) outside the %d x %d image" % (who, top, left, h, w))
        if r.get("hue") is not None and not -0.5 <= r["hue"] <= 0.5:
            raise ValueError("augment_images: hue_factor (%r) is not in [-0.5, 0.5]" % (r["hue"],))
        if r.get("gamma") is not None and not r.get("gray"):
            raise ValueError("augment_images: gamma applies only to a grayscale image (vispr_dl.py:110-113)")
        if r.get("gamma") is not None and r["gamma"] < 0:
            raise ValueError("augment_images: gamma should be a non-negative real number")
        er = list(r.get("erase", ()))
        if len(er) > 1:
            raise ValueError("augment_images: at most one erase box per view")
        if er and (er[0][0] < 0 or er[0][1] < 0):
            raise ValueError("augment_images: negative erase origin")
    rec = np.zeros(len(flat), dtype=RECORD)
    tabs, tab_off, words = [], {}, 0
    luts, lut_idx = [], {}

    def table(in_size, out_size):
        nonlocal words
        key = (in_size, out_size)
        e = tab_off.get(key)
        if e is None:
            tab = _aa_table(in_size, out_size)
            e = (words, tab.shape[1] - 2)
            tab_off[key] = e
            tabs.append(tab.reshape(-1))
            words += tab.size
        return e

    sv, sn = out_strides[0], out_strides[1]
    scratch = 0
    for i, (v, n, r) in enumerate(flat):
        img = images[r["image"]]
        _, h, w = img.shape
        top, left, ch, cw = r["box"]
        e = rec[i]
        e["src"] = img.data_ptr()
        e["dst"] = v * sv + n * sn
        e["tmp"] = scratch
        scratch += 3 * min(ch, h - top) * ow
        e["H"], e["W"], e["top"], e["left"], e["ch"], e["cw"] = h, w, top, left, ch, cw
        (e["ytab"], e["ytaps"]), (e["xtab"], e["xtaps"]) = table(ch, oh), table(cw, ow)
        flags = 0
        for name, flag in (("contrast", None), ("saturation", SATURATION), ("brightness", BRIGHTNESS)):
            f = r.get(name)
            if f is None:
                continue
            flags |= flag if flag is not None else (CONTRAST_LATE if r.get("contrast_late") else CONTRAST_FIRST)
            e[name], e[name + "_1m"] = f, 1.0 - f          # _blend: the ratio and (1.0 - ratio), each rounded to fp32 from a double
        if r.get("hue") is not None:
            flags |= HUE
            e["hue"] = r["hue"]
        if r.get("gray"):
            flags |= GRAY
            if r.get("gamma") is not None:
                flags |= GAMMA
                g = r["gamma"]
                if g not in lut_idx:
                    lut_idx[g] = len(luts)
                    luts.append(gamma_lut(g))
                e["gamma_lut"] = lut_idx[g]
        if r.get("hflip"):
            flags |= HFLIP
        e["flags"] = flags
        for (ei, ej, eh, ew) in r.get("erase", ()):
            e["erase"] = (ei, ej, eh, ew)
    tables = np.concatenate(tabs).astype(np.int32)
    lut_bytes = np.concatenate(luts) if luts else np.zeros(0, np.uint8)
    blob = np.concatenate([rec.view(np.uint8).reshape(-1), tables.view(np.uint8), lut_bytes])
    tables_off = rec.nbytes
    return blob, len(flat), tables_off, tables.size, tables_off + tables.nbytes, len(luts), scratch


def augment_images(images, records, out: torch.Tensor = None, reso=(224, 224)) -> torch.Tensor:
    """images: list of contiguous (3, H, W) uint8 CUDA tensors (what `torchvision.io.read_image` returns, a gray image repeated to three channels;
    sizes may differ). records[v][n]: the record (`image_record`, `sample_vispr*`, `center_record`) of view v of batch item n; rec["image"] indexes
    `images`, and two records may name the same image. Returns / fills the fp32 (V, N, 3, h, w) views (`out` may be any view with those sizes whose
    strides are non-negative: only the elements of the V * N images are written). One table upload and one launch on the current stream; the
    width-pass intermediate of the resize lives in a scratch buffer allocated here. Limits (the C entry refuses beyond them): outputs up to 224 x 224,
    sources up to 16384 x 16384, crop boxes up to 4096 x 4096."""
    if not images or not records or not records[0]:
        raise ValueError("augment_images: no images / records")
    for im in images:
        if not isinstance(im, torch.Tensor) or im.dim() != 3 or im.shape[0] != 3 or im.dtype != torch.uint8 or not im.is_contiguous():
            raise ValueError("augment_images: images must be contiguous (3,H,W) uint8 tensors (read_image's layout)")
    for im in images:
        require_cuda(im, "augment_images")
    oh, ow = int(reso[0]), int(reso[1])
    if oh < 1 or ow < 1:
        raise ValueError("augment_images: bad resolution %r" % (reso,))
    V, N = len(records), len(records[0])
    if any(len(row) != N for row in records):
        raise ValueError("augment_images: every view needs the same number of images")
    shape = (V, N, 3, oh, ow)
    dev = images[0].device
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    if tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != dev or any(s < 0 for s in out.stride()):
        raise ValueError("augment_images: out must be fp32 %s on %s" % (shape, dev))
    s = out.stride()
    blob, nrec, tables_off, table_words, luts_off, nluts, scratch_elems = build_table(images, records, s, (oh, ow))
    blob_dev = torch.empty(blob.nbytes, dtype=torch.uint8, device=dev)
    scratch = torch.empty(scratch_elems, dtype=torch.float32, device=dev)
    span = 1 + sum((d - 1) * st for d, st in zip(shape, s))
    _KEEP[:] = [blob]
    check(_lib.lib().tedspad_image_augment(blob.ctypes.data, blob_dev.data_ptr(), blob.nbytes, nrec, tables_off, table_words, luts_off, nluts,
                                           scratch.data_ptr(), scratch_elems, out.data_ptr(), span, oh, ow, s[2], s[3], s[4], _stream_ptr()),
          "tedspad_image_augment")
    return out
