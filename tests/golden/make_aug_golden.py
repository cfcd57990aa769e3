"""Writes tests/golden/aug_golden.npz + aug_golden_meta.json: what the REFERENCE's two training loaders (aux_code/ucf101_dl.py
`contrastive_train_dataloader.build_clip`, `single_train_dataloader.build_clip`) produce for seeded runs on synthetic videos.

The reference module is imported in place (tests/golden/_refimport.py's recipe: nothing of it is copied) with two absent third-party imports
replaced by stubs:
  * `decord`: a VideoReader that serves `tests/augment_ref.synthetic_video` frames (and raises for an index outside the video, as decord does);
  * `torchvision.transforms`: `functional` is `tests/augment_ref` itself -- every call goes to Pillow -- and logs each call it receives.
Both `build_clip` bodies run on objects made with object.__new__ (their __init__ reads dataset lists).

Stored: the frame lists, the call log with arguments, and the returned clips as bytes (value * 255, exact: to_tensor divides a byte by 255).

What this pins: the reference's GLUE -- frame sampling, the order of the random draws, which draw goes to which argument of which call, the op
order and gating. It does NOT pin torchvision (absent; its PIL path is restated in augment_ref.py); the arithmetic is pinned by Pillow, which the
tests call directly.

Videos are 240 x 320 at reso 28 so that the erase-size ranges are non-empty and a 48-frame clip is 113 KB. The seed of every case is searched so
that, over all cases, every op, both contrast positions and a crop box that overflows the frame occur; the meta file records which case covers what.

Run from the repository root:  python tests/golden/make_aug_golden.py
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
import augment_ref  # noqa: E402

VIDEOS = {}          # path -> (t, h, w, seed)


class _VideoReader:
    def __init__(self, path, ctx=None):
        self.frames = augment_ref.synthetic_video(*VIDEOS[path])

    def __len__(self):
        return len(self.frames)

    def get_batch(self, idx):
        idx = np.asarray(idx)
        if np.any(idx < 0) or np.any(idx >= len(self.frames)):
            raise IndexError("out of bound indices")
        return torch.from_numpy(self.frames[idx.astype(np.int64)])


def import_loader():
    if not _refimport.reference_available():
        raise RuntimeError("reference not present at %s" % _refimport.REFERENCE_ROOT)
    sys.dont_write_bytecode = True
    sys.modules["decord"] = types.SimpleNamespace(VideoReader=_VideoReader, cpu=lambda *a: None, bridge=types.SimpleNamespace(set_bridge=lambda *a: None))
    tv = types.ModuleType("torchvision")
    tr = types.ModuleType("torchvision.transforms")
    tr.functional = augment_ref
    tr.ToPILImage = lambda: augment_ref.to_pil_image
    tr.ToTensor = lambda: augment_ref.to_tensor
    tv.transforms = tr
    sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tr
    if _refimport.REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, _refimport.REFERENCE_ROOT)
    import aux_code.ucf101_dl as dl
    return dl


def make_params(**kw):
    p = dict(num_frames=16, fix_skip=2, reso_h=28, reso_w=28, min_crop_factor_training=0.6, weak_aug=False, no_ar_distortion=False,
             aspect_ratio_aug=False, temporal_loss=None, temporal_align=False, temporal_distance=None)
    p.update(kw)
    return p


CASES = [   # name, loader, frame_wise_aug, params, video (t, h, w, seed)
    ("weak_trip", "contrastive", False, make_params(weak_aug=True, temporal_loss="trip"), (60, 240, 320, 1)),
    ("strong_trip", "contrastive", False, make_params(temporal_loss="trip"), (60, 240, 320, 2)),
    ("strong_single", "single", False, make_params(), (50, 240, 320, 3)),
    ("frame_wise", "contrastive", True, make_params(), (48, 240, 320, 4)),
    ("no_ar_distortion", "contrastive", False, make_params(no_ar_distortion=True), (48, 240, 320, 5)),
    ("aspect_ratio_aug", "contrastive", False, make_params(aspect_ratio_aug=True), (48, 240, 320, 6)),
    ("short_video", "contrastive", False, make_params(temporal_loss="trip"), (30, 240, 320, 7)),
]
FEATURES = ["contrast_first", "contrast_late", "adjust_hue", "adjust_saturation", "adjust_brightness", "to_grayscale", "adjust_gamma", "hflip",
            "erase", "overflow"]


def run_case(dl, loader, frame_wise, params, video, seed):
    path = "video"
    VIDEOS[path] = video
    cls = dl.contrastive_train_dataloader if loader == "contrastive" else dl.single_train_dataloader
    obj = object.__new__(cls)
    obj.params = types.SimpleNamespace(**params)
    obj.PIL, obj.TENSOR, obj.erase_size, obj.framewise_aug = augment_ref.to_pil_image, augment_ref.to_tensor, 19, frame_wise
    augment_ref.CALLS = []
    np.random.seed(seed)
    try:
        res = obj.build_clip(path)
    finally:
        calls, augment_ref.CALLS = augment_ref.CALLS, None
    if res[0] is None:
        return None
    half = len(res) // 2
    clips, lists = (res[:half], res[half:]) if loader == "contrastive" else ([res[0]], [res[1]])
    return clips, [np.asarray(l) for l in lists], calls


def features(calls, video):
    f = set()
    _, h, w, _ = video
    for name, kw in calls:
        if name == "resized_crop" and (kw["top"] + kw["height"] > h or kw["left"] + kw["width"] > w):
            f.add("overflow")
        elif name in FEATURES:
            f.add(name)
    return f


def contrast_position(calls):
    """contrast directly after resized_crop is ambiguous from the log alone when no other colour op ran; the r[0] thresholds decide it in the
    reference, so the generator searches for seeds where another op sits between (late) or follows (first)."""
    first = late = False
    for i, (name, _) in enumerate(calls):
        if name != "adjust_contrast":
            continue
        before = calls[i - 1][0]
        after = calls[i + 1][0]
        if before == "resized_crop" and after in ("adjust_hue", "adjust_saturation", "adjust_brightness"):
            first = True
        if before in ("adjust_hue", "adjust_saturation", "adjust_brightness"):
            late = True
    return first, late


def main():
    dl = import_loader()
    arrays, meta, missing = {}, {"reso": [28, 28], "cases": []}, set(FEATURES)
    for name, loader, fw, params, video in CASES:
        best = None
        for seed in range(400):
            res = run_case(dl, loader, fw, params, video, seed)
            if res is None:
                continue
            clips, lists, calls = res
            f = features(calls, video)
            first, late = contrast_position(calls)
            f |= ({"contrast_first"} if first else set()) | ({"contrast_late"} if late else set())
            gain = len(f & missing)
            if best is None or gain > best[0]:
                best = (gain, seed, clips, lists, calls, f)
            if params["weak_aug"] or gain >= min(4, len(missing)):
                break
        gain, seed, clips, lists, calls, f = best
        missing -= f
        clip = torch.stack([torch.stack(c) for c in clips])                    # (clips, n, 3, h, w)
        b = clip * 255
        assert torch.equal(b, b.round()) and float(b.min()) >= 0 and float(b.max()) <= 255
        arrays[name + "_clips"] = b.to(torch.uint8).numpy()
        arrays[name + "_frames"] = np.stack(lists).astype(np.int64)
        meta["cases"].append({"name": name, "loader": loader, "frame_wise_aug": fw, "params": params, "video": list(video), "seed": seed,
                              "covers": sorted(f), "calls": [[n, kw] for n, kw in calls]})
        print(name, "seed", seed, "covers", sorted(f))
    assert not missing, "not covered by any case: %s" % sorted(missing)
    np.savez_compressed(os.path.join(HERE, "aug_golden.npz"), **arrays)
    with open(os.path.join(HERE, "aug_golden_meta.json"), "w") as fh:
        json.dump(meta, fh, separators=(",", ":"))
    print("wrote", sum(a.nbytes for a in arrays.values()), "bytes of clips")


if __name__ == "__main__":
    main()
