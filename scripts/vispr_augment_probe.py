"""VISPR view augmentation on 1 MI355X: one launch of 2 x 12 views (the two SSL views of 12 images, sources of about 1000 x 750 whose sizes differ) at
224 x 224. Prints one JSON line with, in ms per batch:
  strong / every_op / center   ted_spad_amd.vispr_augment.augment_images (table building, one upload, one launch), host clock around calls that end in a
                               synchronise; *_dev the same window by device events; *_launch the C entry alone on a table built once (upload + kernel,
                               device events): what the device spends
  *_gbs                        achieved bytes/s of the launch alone, in GB/s: the source bytes under the crop boxes read once + the fp32 views written
                               (the width-pass intermediate, which goes to scratch and comes back, is not counted)
  torch_cpu_16_threads         the reference's host chain (tests/vispr_ref.py: torch CPU ops) for the strong batch, images already decoded in memory
  sample / table               the host side per batch: sample_vispr_ssl for the 12 images; vispr_augment.build_table alone
The strong batch draws its ops as the reference does (each colour op on ~15 % of the views); every_op forces the whole chain on every view; center is the
validation branch (centre crop + resize)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vispr_ref  # noqa: E402
from ted_spad_amd import _lib  # noqa: E402
from ted_spad_amd import vispr_augment as VA  # noqa: E402
from ted_spad_amd.engine import _stream_ptr  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, default=12)
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--res", type=int, default=224)
a = ap.parse_args()
assert torch.cuda.is_available(), "vispr_augment_probe needs the GPU: there is no CPU path to time"
torch.set_num_threads(a.threads)

res = (a.res, a.res)
sizes = [(750 - 13 * (n % 4), 1000 + 17 * (n % 5)) if n % 3 else (1000 + 11 * n, 750 - 7 * n) for n in range(a.images)]
images_np = [vispr_ref.synthetic_image(h, w, 50 + n) for n, (h, w) in enumerate(sizes)]
images = [torch.from_numpy(i).cuda() for i in images_np]


def sample(seed):
    rs = np.random.RandomState(seed)
    per_image = [VA.sample_vispr_ssl(rs, h, w, res, image=n) for n, (h, w) in enumerate(sizes)]
    return [[per_image[n][v] for n in range(a.images)] for v in range(2)]


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


def traffic(recs):
    n = 0
    for row in recs:
        for r in row:
            h, w = sizes[r["image"]]
            top, left, ch, cw = r["box"]
            n += 3 * min(ch, h - top) * min(cw, w - left) + 3 * a.res * a.res * 4
    return n


out = torch.empty((2, a.images, 3, a.res, a.res), dtype=torch.float32, device="cuda")
strong = sample(2)
every = [[dict(r, contrast=1.1, contrast_late=bool(k & 1), hue=0.04, saturation=0.93, brightness=1.1, gray=True, gamma=0.9, hflip=True,
               erase=[(3, 5, a.res // 6, a.res // 5)]) for k, r in enumerate(row)] for row in strong]
center = [[VA.center_record(h, w, image=n) for n, (h, w) in enumerate(sizes)]] * 2
line = {"res": a.res, "images": a.images, "views": 2 * a.images, "sizes": sizes}
for name, recs in (("strong", strong), ("every_op", every), ("center", center)):
    line[name], line[name + "_dev"] = [round(v, 3) for v in timed(lambda: VA.augment_images(images, recs, out=out, reso=res))]
    st = out.stride()
    blob, nrec, toff, words, loff, nluts, scratch_elems = VA.build_table(images, recs, st, res)
    blob_dev = torch.empty(blob.nbytes, dtype=torch.uint8, device="cuda")
    scratch = torch.empty(scratch_elems, dtype=torch.float32, device="cuda")

    def launch():
        _lib.check(_lib.lib().tedspad_image_augment(blob.ctypes.data, blob_dev.data_ptr(), blob.nbytes, nrec, toff, words, loff, nluts, scratch.data_ptr(),
                                                    scratch_elems, out.data_ptr(), out.numel(), a.res, a.res, st[2], st[3], st[4], _stream_ptr()),
                   "tedspad_image_augment")
    ms = timed(launch, 100)[1]
    line[name + "_launch"] = round(ms, 4)
    line[name + "_gbs"] = round(traffic(recs) / (ms * 1e-3) / 1e9, 2)

flat = [r for row in strong for r in row]
cpu_images = [torch.from_numpy(i) for i in images_np]
for r in flat[:2]:
    vispr_ref.apply_record(cpu_images[r["image"]], r, res)
t0 = time.perf_counter()
for r in flat:
    vispr_ref.apply_record(cpu_images[r["image"]], r, res)
line["torch_cpu_%d_threads" % a.threads] = round((time.perf_counter() - t0) * 1e3, 2)

t0 = time.perf_counter()
for i in range(20):
    sample(100 + i)
line["sample"] = round((time.perf_counter() - t0) * 1e3 / 20, 3)
t0 = time.perf_counter()
for i in range(20):
    VA.build_table(images, strong, out.stride(), res)
line["table"] = round((time.perf_counter() - t0) * 1e3 / 20, 3)
print(json.dumps(line), flush=True)
