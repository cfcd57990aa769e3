"""Writes tests/golden/val_clip_golden.npz + val_clip_golden_meta.json: what the REFERENCE's two validation loaders (aux_code/ucf101_dl.py
`single_val_dataloader.build_clip` :253-294, `contrastive_val_dataloader.build_clip` :718-870) produce on synthetic videos.

make_aug_golden.py's recipe: the reference module is imported in place (nothing of it is copied) with the `decord` stub of that script (a VideoReader
that serves `augment_ref.synthetic_video` frames and raises for an index outside the video) and a `torchvision.transforms` stub whose `functional` is
`tests/val_clips_ref` -- every call goes to Pillow and is logged. Both `build_clip` bodies run on objects made with object.__new__; the attributes their
__init__ would set (mode, hflip, cropping_factor, and output_reso_* by the rule of :228-233 / :674-679) are set here. The contrastive clips are kept per
clip; `process_data` (:700-711) extends them in that order.

Stored per case: the frame lists, the call log with arguments, and the returned clips as bytes (value * 255, exact: to_tensor divides a byte by 255).
`sweep` holds frame lists alone (or null where build_clip returned None) for every mode 0..4 at frame counts 17, 19, 20, 41, 48 and 60 of both loaders, on
24 x 34 videos: 20 halves the skip and takes `start < 0 -> mode`; at 41 only mode 4 falls back; at 19, mode 4, the single loader returns None (index 19)
while the contrastive loader's clamp of the last index lets it through when the third clip's random start allows; at 17, mode 4, both return None.

What this pins is the reference's GLUE: frame sampling, the swapped height / width of the single loader, which crop and output size each
cropping_factor takes, the call order. The arithmetic is Pillow's (val_clips_ref.py calls it; torchvision is absent and its PIL path restated there).

Run from the repository root:  python tests/golden/make_val_clip_golden.py
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

import augment_ref  # noqa: E402
import make_aug_golden  # noqa: E402
import val_clips_ref  # noqa: E402


def import_loader():
    dl = make_aug_golden.import_loader()
    sys.modules["torchvision.transforms"].functional = val_clips_ref          # looked up at call time (`trans.functional.center_crop`)
    return dl


def make_params(**kw):
    p = dict(num_frames=16, fix_skip=2, reso_h=28, reso_w=28, num_modes=5, no_ar_distortion=False, temporal_loss=None, temporal_align=False,
             temporal_distance=None)
    p.update(kw)
    return p


CASES = [   # name, loader, params, video (t, h, w, seed), mode, hflip, cropping_factor, numpy seed
    ("single_landscape", "single", make_params(), (60, 240, 320, 1), 2, 0, 0.8, 0),                 # padded above and below
    ("single_portrait", "single", make_params(num_frames=8), (48, 320, 240, 2), 1, 0, 0.8, 0),      # padded left and right
    ("contrastive_trip", "contrastive", make_params(temporal_loss="trip"), (60, 240, 320, 3), 3, 0, 0.8, 5),
    ("temporal_distance", "contrastive", make_params(num_frames=8, temporal_distance=8), (60, 240, 320, 4), 4, 0, 0.8, 0),
    ("no_ar_distortion", "single", make_params(num_frames=8, no_ar_distortion=True), (48, 240, 320, 5), 0, 0, 0.8, 0),
    ("factor_1", "single", make_params(num_frames=8), (48, 240, 320, 6), 2, 0, 1, 0),               # 35 x 35 output
    ("factor_1p2", "single", make_params(num_frames=8), (48, 240, 320, 7), 4, 0, 1.2, 0),           # no crop
    ("hflip", "contrastive", make_params(num_frames=8), (60, 240, 320, 8), 1, 1, 0.8, 0),
    ("short_20", "single", make_params(), (20, 240, 320, 9), 3, 0, 0.8, 0),                         # halved skip, start < 0 -> mode
    ("clamped_19", "contrastive", make_params(temporal_loss="trip"), (19, 240, 320, 10), 4, 0, 0.8, None),   # seed searched: start3 <= 4
]
SWEEP_COUNTS = [17, 19, 20, 41, 48, 60]
SWEEP_SEED = 5          # the third clip starts at frame 3: short videos get through


def make_loader(dl, loader, params, mode, hflip, cropping_factor):
    cls = dl.contrastive_val_dataloader if loader == "contrastive" else dl.single_val_dataloader
    obj = object.__new__(cls)
    obj.params = types.SimpleNamespace(**params)
    obj.total_num_modes, obj.threecrop = params["num_modes"], False
    obj.PIL, obj.TENSOR = augment_ref.to_pil_image, augment_ref.to_tensor
    obj.mode, obj.hflip, obj.cropping_factor = mode, hflip, cropping_factor
    if cropping_factor == 1:                                                    # :228-233
        obj.output_reso_h, obj.output_reso_w = int(params["reso_h"] / 0.8), int(params["reso_w"] / 0.8)
    else:
        obj.output_reso_h, obj.output_reso_w = int(params["reso_h"]), int(params["reso_w"])
    return obj


def run_case(dl, loader, params, video, mode, hflip, cropping_factor, seed):
    path = "video"
    make_aug_golden.VIDEOS[path] = video
    obj = make_loader(dl, loader, params, mode, hflip, cropping_factor)
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
    return clips, [np.asarray(l) for l in lists], calls, (obj.output_reso_h, obj.output_reso_w)


def main():
    dl = import_loader()
    arrays, meta = {}, {"cases": [], "sweep": []}
    for name, loader, params, video, mode, hflip, cf, seed in CASES:
        if seed is None:
            seed = [s for s in range(100) if run_case(dl, loader, params, video, mode, hflip, cf, s) is not None][0]
        clips, lists, calls, reso = run_case(dl, loader, params, video, mode, hflip, cf, seed)
        clip = torch.stack([torch.stack(c) for c in clips])                    # (clips, n, 3, h, w)
        b = clip * 255
        assert torch.equal(b, b.round()) and float(b.min()) >= 0 and float(b.max()) <= 255
        arrays[name + "_clips"] = b.to(torch.uint8).numpy()
        frames = np.stack(lists)
        assert np.array_equal(frames, frames.astype(np.int64))
        arrays[name + "_frames"] = frames.astype(np.int64)
        meta["cases"].append({"name": name, "loader": loader, "params": params, "video": list(video), "mode": mode, "hflip": hflip,
                              "cropping_factor": cf, "seed": seed, "reso": list(reso), "calls": [[n, kw] for n, kw in calls]})
        print(name, "seed", seed, "reso", reso, "frames", frames[:, 0].tolist(), "..", frames[:, -1].tolist())
    for loader in ("single", "contrastive"):
        params = make_params(temporal_loss="trip" if loader == "contrastive" else None)
        for count in SWEEP_COUNTS:
            for mode in range(5):
                res = run_case(dl, loader, params, (count, 24, 34, count), mode, 0, 0.8, SWEEP_SEED)
                frames = None if res is None else [[int(v) for v in l] for l in res[1]]
                meta["sweep"].append({"loader": loader, "params": params, "frame_count": count, "mode": mode, "seed": SWEEP_SEED, "frames": frames})
                print("sweep", loader, count, mode, None if frames is None else [f[0] for f in frames])
    got = {(s["loader"], s["frame_count"], s["mode"]): s["frames"] for s in meta["sweep"]}
    assert got[("single", 19, 4)] is None and got[("single", 17, 4)] is None and got[("contrastive", 17, 4)] is None
    assert got[("contrastive", 19, 4)][0][-2:] == [18, 18]          # the clamp: 4 .. 18, 18
    assert [got[("single", 41, m)][0][0] for m in range(5)] == [0, 0, 0, 0, 4]          # only mode 4 falls back
    np.savez_compressed(os.path.join(HERE, "val_clip_golden.npz"), **arrays)
    with open(os.path.join(HERE, "val_clip_golden_meta.json"), "w") as fh:
        json.dump(meta, fh, separators=(",", ":"))
    print("wrote", sum(a.nbytes for a in arrays.values()), "bytes of clips")


if __name__ == "__main__":
    main()
