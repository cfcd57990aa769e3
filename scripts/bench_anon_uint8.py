"""Anonymised extraction from decoded frames resident in HBM, two ways on the same frames (bench.py's bench_e2e_uint8 input: (T, 240, 320, 3) uint8, a clip
per 32 source frames; bench_anon_extract's clip count and warm-up):

  (a) what the pre-existing functions offer: a preprocess.crop_resize launch per clip into the fp32 (n, 16, 3, 224, 224) batch, then
      extraction.extract_anonymized_clip_features (whose anonymizer forward converts that batch to its 16-bit activation again);
  (b) extraction.extract_anonymized_video_features_uint8: one preprocess.crop_resize_act launch per anonymizer batch writes that activation directly.

The two are timed alternately, `--repeats` windows of `--steps` passes each, a device synchronise at both ends of every window; the front-end launches of
each (everything in front of the anonymizer's first conv) are timed alone the same way. Prints ONE JSON line: clips/s of both as median and [min, max] over
the windows, the front-end milliseconds per pass, and whether the two feature matrices are equal bit for bit.

    python scripts/bench_anon_uint8.py [--clips 225] [--steps 5] [--repeats 5]"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=225)
    ap.add_argument("--batch", type=int, default=75)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--hw", type=int, nargs=2, default=(240, 320))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_anon_uint8: needs an MI355X (no CPU path, no fallback)")
    from ted_spad_amd import engine as E, extraction, preprocess
    from ted_spad_amd.model_loaders import load_fa_model, load_ft_model
    from ted_spad_amd.synth import synth_state_dict
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    with contextlib.redirect_stdout(io.StringIO()):
        fa, ft = load_fa_model(), load_ft_model("largei3d", num_classes=102)
    fa.load_state_dict(synth_state_dict(fa.state_dict(), 0))
    ft.load_state_dict(synth_state_dict(ft.state_dict(), 0))
    fa, ft = fa.to(dev).eval(), ft.to(dev).eval()
    n, batch = args.clips, args.batch
    h, w = args.hw
    t_src = n * 32
    g = torch.Generator(device=dev).manual_seed(0)
    frames = torch.empty((t_src, h, w, 3), dtype=torch.uint8, device=dev)
    for i in range(0, t_src, 4000):
        k = min(4000, t_src - i)
        frames[i:i + k] = torch.randint(0, 256, (k, h, w, 3), dtype=torch.uint8, device=dev, generator=g)
    box = extraction.anonymized_video_box(h, w)
    clips = torch.empty((n, 16, 3, 224, 224), dtype=torch.float32, device=dev)
    out_a = torch.empty((n, 2048), dtype=torch.float32, device=dev)
    out_b = torch.empty((n, 2048), dtype=torch.float32, device=dev)

    def front_a():          # a launch per clip into the fp32 batch ...
        for q in range(n):
            preprocess.crop_resize(frames[32 * q:32 * q + 32:2].contiguous(), box, (224, 224), out=clips[q])

    def front_a_layout():   # ... and the conversion UnetPlusPlus.forward runs over it, per anonymizer batch
        for i in range(0, n, batch):
            E.clip_to_act(clips[i:i + batch].reshape(-1, 3, 224, 224).unsqueeze(2), cpad=fa.ACT_CPAD, dtype=fa.compute_dtype)

    def front_b():
        for i in range(0, n, batch):
            preprocess.crop_resize_act(frames, box, (224, 224), min(batch, n - i), first=32 * i, cpad=fa.ACT_CPAD, dtype=fa.compute_dtype)

    def path_a():
        front_a()
        extraction.extract_anonymized_clip_features(ft, fa, clips, batch=75, fa_batch=batch, layout="reference", out=out_a, streams=2)

    def path_b():
        extraction.extract_anonymized_video_features_uint8(ft, fa, frames, batch=75, fa_batch=batch, layout="reference", out=out_b, streams=2)

    def window(fn, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps

    with torch.no_grad():
        warm = 0
        for i in range(40):                       # until the tile tuner has settled the anonymizer's and the encoder's conv geometries
            path_a()
            path_b()
            warm += 1
            if i >= 2 and not E.tuning_pending():
                break
        path_a()                                  # one pass of each on the settled tiles (a pass above may still have run a candidate) for the comparison
        path_b()
        torch.cuda.synchronize()
        equal = bool(torch.equal(out_a, out_b))
        ta, tb, fa_ms, fal_ms, fb_ms = [], [], [], [], []
        for _ in range(args.repeats):             # alternating: both see the same neighbours on the machine
            ta.append(window(path_a, args.steps))
            tb.append(window(path_b, args.steps))
            fa_ms.append(window(front_a, args.steps) * 1e3)
            fal_ms.append(window(front_a_layout, args.steps) * 1e3)
            fb_ms.append(window(front_b, args.steps) * 1e3)

    def rate(ts):
        r = sorted(n / t for t in ts)
        return {"median": round(statistics.median(r), 1), "min": round(r[0], 1), "max": round(r[-1], 1)}

    def ms(ts):
        return {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}

    ra, rb = rate(ta), rate(tb)
    print(json.dumps({
        "config": "%d x %d x 3 uint8 frames in HBM, a 16-frame clip (every 2nd frame) per 32 source frames -> /255, centre crop 0.8, antialiased resize to 224 x 224 -> "
                  "unet++ on every frame -> Q1 reshape -> largei3d extract_features; %d clips, %d per anonymizer forward, 75 per encoder forward, f16 activations, "
                  "random-init weights" % (h, w, n, batch),
        "device": torch.cuda.get_device_name(dev), "warmup_passes": warm, "steps_per_window": args.steps, "windows": args.repeats,
        "a_crop_resize_per_clip_then_fp32_clip_path_clips_per_s": ra,
        "b_extract_anonymized_video_features_uint8_clips_per_s": rb,
        "b_over_a_median": round(rb["median"] / ra["median"], 4),
        "b_not_slower_than_a_beyond_spread": bool(rb["median"] >= ra["min"]),        # b's median inside or above the range a's own windows span
        "front_end_ms_per_pass": {"a_crop_resize_per_clip": ms(fa_ms), "a_clip_to_act": ms(fal_ms), "b_crop_resize_act": ms(fb_ms)},
        "features_equal_bit_for_bit": equal}))


if __name__ == "__main__":
    main()
