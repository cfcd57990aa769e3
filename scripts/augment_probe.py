"""Training-clip augmentation on 1 MI355X against the host chain it replaces: a batch of 8 videos of 240 x 320, 3 x 16 frames each (the
contrastive loader's 'trip' batch, 384 frames), at 112 x 112 and 224 x 224. Prints one JSON line per resolution with, in ms per batch:
  weak / strong / every_op   ted_spad_amd.augment.augment_batch (table building, one upload, one launch), host clock around calls that end in a
                             synchronise; *_dev the same window by device events; *_launch the C entry alone on a table built once (upload + kernel,
                             device events): what the device spends
  weak_24_crop_resize_pil    the same weak batch as 24 preprocess.crop_resize_pil launches (one per clip; each clip's frames gathered first)
  pillow_16_threads          the reference's host chain (tests/augment_ref.py: Pillow) for the strong batch on 16 threads, frames already decoded in memory
                             (torch's own thread pool set to 1); pillow_1_thread the same on one
  sample / table             the host side per batch: sample_contrastive for 8 videos; augment.build_table alone
The strong batch draws its ops as the reference does (each colour op on ~15 % of the clips); every_op forces the whole chain on every frame."""
import argparse
import json
import os
import sys
import time
import types
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import augment_ref  # noqa: E402
from ted_spad_amd import augment as A  # noqa: E402
from ted_spad_amd import _lib  # noqa: E402
from ted_spad_amd import preprocess as PP  # noqa: E402
from ted_spad_amd.engine import _stream_ptr  # noqa: E402

torch.set_num_threads(1)

ap = argparse.ArgumentParser()
ap.add_argument("--videos", type=int, default=8)
ap.add_argument("--frames", type=int, default=48, help="frames per video")
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--res", type=int, nargs="*", default=[112, 224])
a = ap.parse_args()
assert torch.cuda.is_available(), "augment_probe needs the GPU: there is no CPU path to time"

H, W = 240, 320
videos_np = [augment_ref.synthetic_video(a.frames, H, W, 50 + v) for v in range(a.videos)]
videos = [torch.from_numpy(v).cuda() for v in videos_np]


def params(res, weak):
    return types.SimpleNamespace(num_frames=16, fix_skip=2, reso_h=res, reso_w=res, min_crop_factor_training=0.6, weak_aug=weak,
                                 no_ar_distortion=False, aspect_ratio_aug=False, temporal_loss="trip", temporal_align=False, temporal_distance=None)


def sample(res, weak, seed):
    rs, rows = np.random.RandomState(seed), []
    for v in range(a.videos):
        _, clips = A.sample_contrastive(rs, params(res, weak), a.frames, H, W)
        rows.append([dict(r, video=v) for clip in clips for r in clip])
    return rows


def timed(fn, iters=None):
    iters = iters or a.iters
    for _ in range(a.warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters, e0.elapsed_time(e1) / iters


for res in a.res:
    out = torch.empty((a.videos, 48, 3, res, res), dtype=torch.float32, device="cuda")
    weak = sample(res, True, 1)
    for row in weak:                      # crop_resize_pil takes in-frame boxes only: both weak paths crop from the frame's origin
        for r in row:
            r["box"] = (0, 0) + r["box"][2:]
    strong = sample(res, False, 2)
    every = [[dict(r, contrast=1.1, contrast_late=bool(k & 1), hue=0.04, saturation=0.93, brightness=1.1, gray=True, gamma=0.9, hflip=True,
                   erase=[(3, 5, res // 6, res // 5), (res // 2, res // 3, res // 5, res // 6)]) for k, r in enumerate(row)] for row in strong]
    line = {"res": res, "videos": a.videos, "frames": a.videos * 48}
    for name, recs in (("weak", weak), ("strong", strong), ("every_op", every)):
        line[name], line[name + "_dev"] = [round(v, 3) for v in timed(lambda: A.augment_batch(videos, recs, out=out, reso=(res, res)))]
        blob, nrec, toff, words, loff, nluts = A.build_table(videos, recs, out, (res, res))
        blob_dev = torch.empty(blob.nbytes, dtype=torch.uint8, device="cuda")
        st = out.stride()

        def launch():
            _lib.check(_lib.lib().tedspad_clip_augment(blob.ctypes.data, blob_dev.data_ptr(), blob.nbytes, nrec, toff, words, loff, nluts, out.data_ptr(),
                                                       out.numel(), res, res, st[2], st[3], st[4], _stream_ptr()), "tedspad_clip_augment")
        line[name + "_launch"] = round(timed(launch, 200)[1], 4)

    def pil24():
        for b, row in enumerate(weak):
            for c in range(3):
                idx = torch.tensor([r["frame"] for r in row[16 * c:16 * c + 16]], device="cuda")
                PP.crop_resize_pil(videos[b].index_select(0, idx), row[16 * c]["box"], (res, res), out=out[b, 16 * c:16 * c + 16])
    ref = A.augment_batch(videos, weak, reso=(res, res))
    pil24()
    assert torch.equal(ref, out), "the two weak paths disagree"
    line["weak_24_crop_resize_pil"], line["weak_24_crop_resize_pil_dev"] = [round(v, 3) for v in timed(pil24)]

    flat = [r for row in strong for r in row]
    with ThreadPoolExecutor(max_workers=a.threads) as ex:
        def host():
            return list(ex.map(lambda r: augment_ref.apply_record(videos_np[r["video"]][r["frame"]], r, (res, res)), flat))
        host()
        t0 = time.perf_counter()
        for _ in range(3):
            host()
        line["pillow_%d_threads" % a.threads] = round((time.perf_counter() - t0) * 1e3 / 3, 2)
    t0 = time.perf_counter()
    for r in flat:
        augment_ref.apply_record(videos_np[r["video"]][r["frame"]], r, (res, res))
    line["pillow_1_thread"] = round((time.perf_counter() - t0) * 1e3, 2)

    t0 = time.perf_counter()
    for i in range(20):
        sample(res, False, 100 + i)
    line["sample"] = round((time.perf_counter() - t0) * 1e3 / 20, 3)
    t0 = time.perf_counter()
    for i in range(20):
        A.build_table(videos, strong, out, (res, res))
    line["table"] = round((time.perf_counter() - t0) * 1e3 / 20, 3)
    print(json.dumps(line), flush=True)
