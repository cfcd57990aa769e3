"""torch-CPU reference for the VISPR image augmentation (helper, not a test): the `torchvision.transforms.functional` calls that
`aux_code/vispr_dl.py`'s `vispr_dataset.augmentation` (:71-129) and `vispr_ssl_dataset.augmentation` (:186-251) make on the uint8 TENSOR that
`torchvision.io.read_image` returns, so every call takes torchvision's tensor path. torchvision is not installed: what each call does is RESTATED
from its published 0.15.2 `_functional_tensor.py` / `functional.py` with torch CPU ops only (the same standing as `tests/augment_ref.py`, which
restates the PIL path); the ARITHMETIC is torch's own, called here, never restated:

    crop              img[..., top:bottom, left:right], zero-padded right of / below the image
    resize            F.interpolate(x.float(), size, mode="bilinear", align_corners=False, antialias=True) -> round -> uint8
    resized_crop      crop, then resize;   center_crop: top = int(round((h - side) / 2.0)), same for left
    _blend            (ratio * img1 + (1.0 - ratio) * img2).clamp(0, 255).to(uint8)
    rgb_to_grayscale  (0.2989 * r + 0.587 * g + 0.114 * b).to(uint8), expanded to three channels
    adjust_brightness _blend(img, zeros, f);  adjust_saturation _blend(img, gray(img), f)
    adjust_contrast   _blend(img, mean(gray(img).float()), f)
    adjust_hue        img / 255 -> _rgb2hsv -> (h + f) % 1.0 -> _hsv2rgb -> * (255 + 1.0 - 1e-3) -> uint8
    adjust_gamma      img / 255 -> (gain * x ** gamma).clamp(0, 1) -> * (255 + 1.0 - 1e-3) -> uint8
    hflip             img.flip(-1);   erase: img[..., i:i+h, j:j+w] = v on a copy

The module doubles as the `functional` shim `tests/golden/make_vispr_aug_golden.py` hands to the reference's loader code (every call is appended to
`CALLS` while logging is on), and `apply_record` / `colour_chain` run one of `ted_spad_amd.vispr_augment`'s records through the same functions in the
reference's order.
"""
import numpy as np
import torch
import torch.nn.functional as F

CALLS = None            # a list while make_vispr_aug_golden.py records; None otherwise


def _log(name, **kw):
    if CALLS is not None:
        CALLS.append((name, kw))


def synthetic_image(h, w, seed):
    """(3, h, w) uint8 image from integer arithmetic alone (reproduces anywhere): ramps, a coarse checker and hashed noise."""
    yy, xx = np.meshgrid(np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), indexing="ij")
    n = (xx * 73856093) ^ (yy * 19349663) ^ (int(seed) * 2654435761)
    n = ((n & 0xFFFFFFFF) * 1103515245 + 12345) >> 16
    r = (xx * 3 + yy + seed * 17 + (n & 31)) % 256
    g = ((xx * xx) // 97 + yy * 2 + seed * 29 + ((n >> 5) & 15)) % 256
    b = ((yy * 255) // max(h - 1, 1) + 96 * (((xx // 16) + (yy // 16)) & 1) + ((n >> 9) & 63)) % 256
    return np.stack([r, g, b], axis=0).astype(np.uint8)


def _u8(img):
    img = torch.as_tensor(img)
    assert img.dtype == torch.uint8 and img.dim() == 3 and img.shape[0] == 3
    return img


# ---- the functional shim ------------------------------------------------------------------------------------------------------------

def crop(img, top, left, height, width):
    img = _u8(img)
    top, left, height, width = int(top), int(left), int(height), int(width)
    assert top >= 0 and left >= 0
    h, w = img.shape[-2:]
    bottom, right = top + height, left + width
    part = img[..., top:min(bottom, h), left:min(right, w)]
    if bottom > h or right > w:
        part = F.pad(part, [0, width - part.shape[-1], 0, height - part.shape[-2]], value=0)
    return part


def _resize(img, size):
    return torch.round(resize_float(img, size)).to(torch.uint8)


def resize(img, size, antialias=True):
    _log("resize", size=[int(size[0]), int(size[1])])
    assert antialias
    return _resize(img, size)


def resize_float(img, size):
    """the fp32 image `resize` rounds: what the near-tie rule of the tests is computed from"""
    return F.interpolate(_u8(img).unsqueeze(0).to(torch.float32), size=[int(size[0]), int(size[1])], mode="bilinear", align_corners=False,
                         antialias=True).squeeze(0)


def resized_crop(img, top, left, height, width, size, antialias=True):
    _log("resized_crop", top=int(top), left=int(left), height=int(height), width=int(width), size=[int(size[0]), int(size[1])])
    assert antialias
    return _resize(crop(img, top, left, height, width), size)


def center_crop(img, output_size):
    side = int(output_size)
    _log("center_crop", size=side)
    h, w = _u8(img).shape[-2:]
    assert side <= h and side <= w
    return crop(img, int(round((h - side) / 2.0)), int(round((w - side) / 2.0)), side, side)


def _blend(img1, img2, ratio):
    ratio = float(ratio)
    return (ratio * img1 + (1.0 - ratio) * img2).clamp(0, 255).to(img1.dtype)


def rgb_to_grayscale(img, num_output_channels=1):
    _log("rgb_to_grayscale", num_output_channels=int(num_output_channels))
    return _gray(_u8(img), num_output_channels)


def _gray(img, num_output_channels=1):
    r, g, b = img.unbind(dim=-3)
    l_img = (0.2989 * r + 0.587 * g + 0.114 * b).to(img.dtype).unsqueeze(dim=-3)
    return l_img.expand(img.shape) if num_output_channels == 3 else l_img


def adjust_brightness(img, brightness_factor):
    _log("adjust_brightness", factor=float(brightness_factor))
    img = _u8(img)
    return _blend(img, torch.zeros_like(img), brightness_factor)


def adjust_contrast(img, contrast_factor):
    _log("adjust_contrast", factor=float(contrast_factor))
    img = _u8(img)
    mean = torch.mean(_gray(img).to(torch.float32), dim=(-3, -2, -1), keepdim=True)
    return _blend(img, mean, contrast_factor)


def adjust_saturation(img, saturation_factor):
    _log("adjust_saturation", factor=float(saturation_factor))
    img = _u8(img)
    return _blend(img, _gray(img), saturation_factor)


def _rgb2hsv(img):
    r, g, b = img.unbind(dim=-3)
    maxc = torch.max(img, dim=-3).values
    minc = torch.min(img, dim=-3).values
    eqc = maxc == minc
    cr = maxc - minc
    ones = torch.ones_like(maxc)
    s = cr / torch.where(eqc, ones, maxc)
    cr_divisor = torch.where(eqc, ones, cr)
    rc = (maxc - r) / cr_divisor
    gc = (maxc - g) / cr_divisor
    bc = (maxc - b) / cr_divisor
    hr = (maxc == r) * (bc - gc)
    hg = ((maxc == g) & (maxc != r)) * (2.0 + rc - bc)
    hb = ((maxc != g) & (maxc != r)) * (4.0 + gc - rc)
    h = hr + hg + hb
    h = torch.fmod((h / 6.0 + 1.0), 1.0)
    return torch.stack((h, s, maxc), dim=-3)


def _hsv2rgb(img):
    h, s, v = img.unbind(dim=-3)
    i = torch.floor(h * 6.0)
    f = (h * 6.0) - i
    i = i.to(dtype=torch.int32)
    p = torch.clamp((v * (1.0 - s)), 0.0, 1.0)
    q = torch.clamp((v * (1.0 - (s * f))), 0.0, 1.0)
    t = torch.clamp((v * (1.0 - (s * (1.0 - f)))), 0.0, 1.0)
    i = i % 6
    mask = i.unsqueeze(dim=-3) == torch.arange(6, device=i.device).view(-1, 1, 1)
    a1 = torch.stack((v, q, p, p, t, v), dim=-3)
    a2 = torch.stack((t, v, v, q, p, p), dim=-3)
    a3 = torch.stack((p, p, t, v, v, q), dim=-3)
    a4 = torch.stack((a1, a2, a3), dim=-4)
    return torch.einsum("...ijk, ...xijk -> ...xjk", mask.to(dtype=img.dtype), a4)


def _to_float(img):
    return img.to(torch.float32) / 255.0


def _to_u8(img):
    return img.mul(255 + 1.0 - 1e-3).to(torch.uint8)


def adjust_hue(img, hue_factor):
    _log("adjust_hue", factor=float(hue_factor))
    if not -0.5 <= hue_factor <= 0.5:
        raise ValueError("hue_factor (%r) is not in [-0.5, 0.5]." % (hue_factor,))
    x = _rgb2hsv(_to_float(_u8(img)))
    h, s, v = x.unbind(dim=-3)
    h = (h + float(hue_factor)) % 1.0
    return _to_u8(_hsv2rgb(torch.stack((h, s, v), dim=-3)))


def adjust_gamma(img, gamma, gain=1):
    _log("adjust_gamma", gamma=float(gamma), gain=float(gain))
    if gamma < 0:
        raise ValueError("Gamma should be a non-negative real number")
    return _to_u8((gain * _to_float(_u8(img)) ** float(gamma)).clamp(0, 1))


def hflip(img):
    _log("hflip")
    return _u8(img).flip(-1)


def erase(img, i, j, h, w, v=0, inplace=False):
    _log("erase", i=int(i), j=int(j), h=int(h), w=int(w), v=float(v))
    img = img.clone()
    img[..., int(i):int(i) + int(h), int(j):int(j) + int(w)] = v
    return img


# ---- one record of ted_spad_amd.vispr_augment through the chain above -----------------------------------------------------------------

def colour_chain(resized, rec):
    """everything after the resize: (3, oh, ow) uint8 -> (3, oh, ow) uint8, in the order of vispr_dl.py:100-120"""
    img = _u8(resized)
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
        img = rgb_to_grayscale(img, 3)
        if rec.get("gamma") is not None:
            img = adjust_gamma(img, rec["gamma"], 1)
    if rec.get("hflip"):
        img = hflip(img)
    for (i, j, h, w) in rec.get("erase", ()):
        img = erase(img, i, j, h, w, 0)
    return img.contiguous()


def apply_record_bytes(image_chw, rec, reso):
    top, left, ch, cw = rec["box"]
    return colour_chain(resized_crop(image_chw, top, left, ch, cw, reso), rec)


def apply_record(image_chw, rec, reso):
    """image_chw: (3, H, W) uint8; rec: a record of ted_spad_amd.vispr_augment; reso: (oh, ow). Returns the fp32 (3, oh, ow) tensor the reference's
    `augmentation` returns for those parameters (`image / 255.0`)."""
    return apply_record_bytes(image_chw, rec, reso) / 255.0
