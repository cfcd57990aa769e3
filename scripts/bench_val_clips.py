"""One validation batch of the reference's defaults from decoded frames resident in HBM -- 8 videos of 240 x 320, temporal_loss 'trip' (48 records each:
`val_clips.sample_val_contrastive`, the contrastive loader's boxes, which both paths can express), 224 x 224 output, the unet++ anonymizer's input
(cpad 4, f16) -- two ways:

  (A) val_clips.val_clips_act: one launch writes the 16-bit activation of the pseudo-images (154 MB);
  (B) what the tree offered before it: augment.augment_batch of the same records (231 MB of fp32), AnonymizerTrainStep._feed (the permuted copy: 231 MB
      read, 231 MB written) and engine.clip_to_act (231 MB read, 154 MB written).

Timed alternately after a warm-up, `--repeats` windows each, a device synchronise at both ends of every window, at two levels: `call` is the public
launchers (the host's table building included, `--steps` calls a window); `device` replays prebuilt record tables through the C entries (`--device-steps`
launches a window, enough that the queue never runs dry), which leaves the kernels. Prints ONE JSON line: milliseconds per batch of both as median and
[min, max] over the windows, and whether the two activations are equal bit for bit.

    python scripts/bench_val_clips.py [--videos 8] [--steps 20] [--device-steps 200] [--repeats 7]"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=8)
    ap.add_argument("--frames", type=int, default=96)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--device-steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--hw", type=int, nargs=2, default=(240, 320))
    ap.add_argument("--reso", type=int, default=224)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_val_clips: needs an MI355X (no CPU path, no fallback)")
    from ted_spad_amd import _lib, augment as A, engine as E, val_clips as V
    from ted_spad_amd.engine import _stream_ptr
    from ted_spad_amd.train_step import AnonymizerTrainStep
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    h, w = args.hw
    reso = (args.reso, args.reso)
    cpad, dtype = 4, "f16"                        # UnetPlusPlus.ACT_CPAD, its default storage type
    p = types.SimpleNamespace(num_frames=16, fix_skip=2, reso_h=args.reso, reso_w=args.reso, num_modes=5, no_ar_distortion=False, temporal_loss="trip",
                              temporal_align=False, temporal_distance=None)
    g = torch.Generator(device=dev).manual_seed(0)
    videos = [torch.randint(0, 256, (args.frames, h, w, 3), dtype=torch.uint8, device=dev, generator=g) for _ in range(args.videos)]
    records = []
    for v in range(args.videos):
        _, clips = V.sample_val_contrastive(np.random.RandomState(v), p, args.frames, h, w, mode=v % 5)
        records.append([dict(r, video=v) for clip in clips for r in clip])
    B, n = len(records), len(records[0])
    x = torch.empty((B, n, 3) + reso, dtype=torch.float32, device=dev)
    act = torch.empty((B * n, 1, reso[0], reso[1] // 2, 8), dtype=torch.float16, device=dev)

    def call_a():
        return V.val_clips_act(videos, records, reso, cpad, dtype, out=act)

    def call_b():
        A.augment_batch(videos, records, out=x, reso=reso)
        return E.clip_to_act(AnonymizerTrainStep._feed(x)[0].unsqueeze(2), cpad=cpad, dtype=dtype)

    L = _lib.lib()
    band = V.band_height(records, reso, cpad)
    blob_a, nrec, toff_a, words_a = V._build_table("bench_val_clips", videos, records, reso, lambda b, k: 0)
    blob_b, _, toff_b, words_b, luts_off, nluts = A.build_table(videos, records, x, reso)
    dev_a = torch.empty(blob_a.nbytes, dtype=torch.uint8, device=dev)
    dev_b = torch.empty(blob_b.nbytes, dtype=torch.uint8, device=dev)
    s = x.stride()

    def device_a():
        _lib.check(L.tedspad_val_clips_act(blob_a.ctypes.data, dev_a.data_ptr(), blob_a.nbytes, nrec, toff_a, words_a, act.data_ptr(), act.numel() * 2, n,
                                           reso[0], reso[1], band, cpad, _lib.F16, _stream_ptr()), "tedspad_val_clips_act")

    def device_b():
        _lib.check(L.tedspad_clip_augment(blob_b.ctypes.data, dev_b.data_ptr(), blob_b.nbytes, nrec, toff_b, words_b, luts_off, nluts, x.data_ptr(),
                                          x.numel(), reso[0], reso[1], s[2], s[3], s[4], _stream_ptr()), "tedspad_clip_augment")
        E.clip_to_act(AnonymizerTrainStep._feed(x)[0].unsqueeze(2), cpad=cpad, dtype=dtype)

    def window(fn, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3

    for _ in range(3):                            # warm-up: code objects, the caching allocator's blocks for B's two temporaries
        call_a(), call_b(), device_a(), device_b()
    torch.cuda.synchronize()
    want = call_b().buf.clone()
    equal = bool(torch.equal(call_a().buf.view(torch.int16), want.view(torch.int16)))
    device_a()
    torch.cuda.synchronize()
    equal = equal and bool(torch.equal(act.view(torch.int16), want.view(torch.int16)))
    ca, cb, da, db = [], [], [], []
    for _ in range(args.repeats):                 # alternating: both see the same neighbours on the machine
        ca.append(window(call_a, args.steps))
        cb.append(window(call_b, args.steps))
        da.append(window(device_a, args.device_steps))
        db.append(window(device_b, args.device_steps))

    def ms(ts):
        return {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}

    def verdict(a, b):
        """A is faster only if its slowest window beats B's fastest"""
        return "A faster beyond the spread" if max(a) < min(b) else ("B faster beyond the spread" if max(b) < min(a) else "within the spread")

    print(json.dumps({
        "config": "%d videos of %d x %d x 3 uint8 frames in HBM, %d records each ('trip', contrastive val loader), centre crop 0.8 -> %d x %d, band of %d "
                  "rows; A = val_clips_act (cpad %d, %s), B = augment_batch + _feed + clip_to_act" % (B, h, w, n, reso[0], reso[1], band, cpad, dtype),
        "device": torch.cuda.get_device_name(dev), "windows": args.repeats, "steps_per_window": {"call": args.steps, "device": args.device_steps},
        "call_ms_per_batch": {"a_val_clips_act": ms(ca), "b_augment_feed_clip_to_act": ms(cb), "verdict": verdict(ca, cb)},
        "device_ms_per_batch": {"a_val_clips_act": ms(da), "b_augment_feed_clip_to_act": ms(db), "verdict": verdict(da, db)},
        "b_over_a_device_median": round(statistics.median(db) / statistics.median(da), 3),
        "bytes_written_mb": {"a": round(act.numel() * 2 / 1e6, 1), "b": round((2 * x.numel() * 4 + act.numel() * 2) / 1e6, 1)},
        "activations_equal_bit_for_bit": equal}))


if __name__ == "__main__":
    main()
