"""Writes tests/golden/vispr_aug_golden.npz + vispr_aug_golden_meta.json: what the REFERENCE's two VISPR loaders (aux_code/vispr_dl.py
`vispr_dataset.augmentation`, `vispr_ssl_dataset.augmentation`, train and val) return for seeded runs on synthetic images.

The reference module is imported in place (tests/golden/_refimport.py's recipe, as make_aug_golden.py: nothing of it is copied) with the absent
`torchvision` replaced by a stub whose `transforms.functional` is `tests/vispr_ref` itself -- every call goes to torch CPU ops -- and logs each call
it receives. Both `augmentation` bodies run on objects made with object.__new__ (their __init__ reads the dataset's label pickles), with
`params.reso_h = params.reso_w = 28` set on the imported module at run time and `np.random.seed(seed)` in front of every call.

Stored: the call log with arguments, and the returned images as bytes (the loaders return `image / 255.0` of a uint8 tensor; the generator checks
that dividing the stored bytes by 255 gives the returned floats back bit for bit).

What this pins: the reference's GLUE -- the order of the random draws, which draw goes to which argument of which call, the op order and gating,
the size-(2,) draws of which index 0 is used, the shared origin of the SSL views. It does NOT pin torchvision (absent; its tensor path is restated
in vispr_ref.py); the arithmetic is pinned by torch, which the tests call directly.

Images are 97 x 131 and 240 x 320 at reso 28, regenerated from a seed (`vispr_ref.synthetic_image`). The seed of every train case is searched so
that, over all cases, every op, both contrast positions, the erase box and an overflowing second view occur; the meta file records which case
covers what.

Run from the repository root:  python tests/golden/make_vispr_aug_golden.py
"""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import _refimport  # noqa: E402
import vispr_ref  # noqa: E402

RESO = 28


def import_loader():
    if not _refimport.reference_available():
        raise RuntimeError("reference not present at %s" % _refimport.REFERENCE_ROOT)
    sys.dont_write_bytecode = True
    tv = types.ModuleType("torchvision")
    tr = types.ModuleType("torchvision.transforms")
    tr.functional = vispr_ref
    tv.transforms = tr
    sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tr
    if _refimport.REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, _refimport.REFERENCE_ROOT)
    import aux_code.vispr_dl as dl
    dl.params.reso_h = dl.params.reso_w = RESO
    return dl


CASES = [   # name, loader, split, image (h, w, seed)
    ("train_small_a", "vispr", "train", (97, 131, 1)),
    ("train_small_b", "vispr", "train", (97, 131, 2)),
    ("train_large_a", "vispr", "train", (240, 320, 3)),
    ("train_large_b", "vispr", "train", (240, 320, 4)),
    ("ssl_small_a", "ssl", "train", (97, 131, 5)),
    ("ssl_small_b", "ssl", "train", (97, 131, 6)),
    ("ssl_large_a", "ssl", "train", (240, 320, 7)),
    ("ssl_large_b", "ssl", "train", (240, 320, 8)),
    ("val_small", "vispr", "val", (97, 131, 9)),
    ("val_large", "vispr", "val", (240, 320, 10)),
    ("ssl_val_tall", "ssl", "val", (131, 96, 11)),
]
FEATURES = ["contrast_first", "contrast_late", "adjust_hue", "adjust_saturation", "adjust_brightness", "rgb_to_grayscale", "adjust_gamma", "hflip",
            "erase", "overflow"]
COLOUR = ("adjust_hue", "adjust_saturation", "adjust_brightness")


def run_case(dl, loader, split, image, seed):
    img = torch.from_numpy(vispr_ref.synthetic_image(*image))
    obj = object.__new__(dl.vispr_dataset if loader == "vispr" else dl.vispr_ssl_dataset)
    obj.data_split, obj.erase_size = split, 19
    vispr_ref.CALLS = []
    np.random.seed(seed)
    try:
        res = obj.augmentation(img) if loader == "vispr" else obj.augmentation([img, img])
    finally:
        calls, vispr_ref.CALLS = vispr_ref.CALLS, None
    return ([res] if loader == "vispr" else list(res)), calls


def features(calls, image):
    """contrast directly after resized_crop is ambiguous from the log alone when no other colour op ran; the r[0] thresholds decide it in the
    reference, so only a contrast with another colour op behind it (first) or in front of it (late) counts."""
    f = set()
    h, w, _ = image
    for i, (name, kw) in enumerate(calls):
        if name == "resized_crop" and (kw["top"] + kw["height"] > h or kw["left"] + kw["width"] > w):
            f.add("overflow")
        elif name == "adjust_contrast":
            if calls[i - 1][0] == "resized_crop" and i + 1 < len(calls) and calls[i + 1][0] in COLOUR:
                f.add("contrast_first")
            if calls[i - 1][0] in COLOUR:
                f.add("contrast_late")
        elif name in FEATURES:
            f.add(name)
    return f


def main():
    dl = import_loader()
    arrays, meta, missing = {}, {"reso": [RESO, RESO], "cases": []}, set(FEATURES)
    for name, loader, split, image in CASES:
        best = None
        for seed in range(1 if split == "val" else 3000):
            views, calls = run_case(dl, loader, split, image, seed)
            f = features(calls, image)
            gain = len(f & missing)
            if best is None or gain > best[0]:
                best = (gain, seed, views, calls, f)
            if gain >= min(3, len(missing)):
                break
        gain, seed, views, calls, f = best
        missing -= f
        x = torch.stack(views)                                            # (views, 3, h, w) fp32
        b = (x * 255).round().to(torch.uint8)
        assert x.dtype == torch.float32 and torch.equal(b / 255.0, x)
        arrays[name + "_views"] = b.numpy()
        meta["cases"].append({"name": name, "loader": loader, "split": split, "image": list(image), "seed": seed, "covers": sorted(f),
                              "calls": [[n, kw] for n, kw in calls]})
        print(name, "seed", seed, "covers", sorted(f))
    assert not missing, "not covered by any case: %s" % sorted(missing)
    np.savez_compressed(os.path.join(HERE, "vispr_aug_golden.npz"), **arrays)
    with open(os.path.join(HERE, "vispr_aug_golden_meta.json"), "w") as fh:
        json.dump(meta, fh, separators=(",", ":"))
    print("wrote", sum(a.nbytes for a in arrays.values()), "bytes of views")


if __name__ == "__main__":
    main()
