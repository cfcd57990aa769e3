"""Ten-crop pre-processing from decoded frames: ONE tedspad_frames_ten_crop_tp launch against the ten tedspad_frames_crop_resize_tp launches it replaces, at
bench_e2e_uint8's shape (240 x 320 x 3 uint8 frames -> 224 x 224, 37 clip times = 370 clips per launch), timed with device events in alternating turns of one
process; then extraction.extract_video_features_uint8 with crops=10 beside crops=1, in clip-forwards per second. Prints one JSON line.

Usage: python scripts/bench_ten_crop.py [--turns 9] [--reps 5] [--clip-times 225] [--steps 3] [--no-features]"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ted_spad_amd import engine as E, extraction, preprocess      # noqa: E402


def _stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "spread_ms": round(max(ms) - min(ms), 4), "turns": len(ms)}


def bench_kernels(dev, turns, reps, n=37, hw=(240, 320), out_hw=(224, 224)):
    h, w = hw
    ch, cw = int(h * 0.8), int(w * 0.8)
    frames = torch.randint(0, 256, (n * 32, h, w, 3), dtype=torch.uint8, device=dev)
    stem = E.StemPT(torch.zeros(64, 3, 5, 7, 7), torch.ones(64), torch.zeros(64), device=dev)
    boxes = preprocess.ten_crop_boxes(h, w, ch, cw)
    rec10 = torch.empty((10 * n, stem.frame_pairs(16), out_hw[0], 2, out_hw[1] // 2, 24), dtype=stem.torch_dtype, device=dev)
    per = [torch.empty((n,) + tuple(rec10.shape[1:]), dtype=stem.torch_dtype, device=dev) for _ in boxes]

    def one():
        preprocess.ten_crop_records(frames, (ch, cw), out_hw, stem, n, out=rec10)

    def ten():
        for b, dst in zip(boxes, per):
            preprocess.crop_resize_records(frames, b[:4], out_hw, stem, n, flip=b[4], out=dst)

    for _ in range(3):                                            # warm up both
        one()
        ten()
    torch.cuda.synchronize()
    same = all(torch.equal(rec10[k::10].view(torch.int16), per[k].view(torch.int16)) for k in range(10))
    times = {"one": [], "ten": []}
    for _ in range(turns):                                        # alternating turns, `reps` calls per turn between two device events
        for name, fn in (("one", one), ("ten", ten)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / reps)
    o, t = _stats(times["one"]), _stats(times["ten"])
    out_gb = rec10.numel() * 2 / 1e9
    return {"clips_per_launch": 10 * n, "records_gb": round(out_gb, 3), "bit_identical": bool(same), "one_launch": o, "ten_launches": t,
            "ratio_ten_over_one": round(t["median_ms"] / o["median_ms"], 3),
            "gap_ms": round(t["min_ms"] - o["max_ms"], 4),       # > 0: the slowest one-launch turn is faster than the fastest ten-launch turn
            "one_launch_store_tb_per_s": round(out_gb / o["median_ms"], 3)}


def bench_features(dev, clip_times, steps, batch=375, hw=(240, 320)):
    from ted_spad_amd.model_loaders import load_ft_model
    from ted_spad_amd.synth import synth_state_dict
    with contextlib.redirect_stdout(io.StringIO()):
        ft = load_ft_model("largei3d", num_classes=102)
    ft.load_state_dict(synth_state_dict(ft.state_dict(), 0))
    ft = ft.to(dev).eval()
    res = {}
    for crops, n in ((10, clip_times), (1, 10 * clip_times)):     # the same number of clip forwards either way
        frames = torch.randint(0, 256, (n * 32, hw[0], hw[1], 3), dtype=torch.uint8, device=dev)
        out = torch.empty((n, 10, 2048) if crops == 10 else (n, 2048), dtype=torch.float32, device=dev)

        def step():
            extraction.extract_video_features_uint8(ft, frames, batch=batch, streams=2, out=out, crops=crops)
        with torch.no_grad():
            for i in range(60):
                step()
                if i >= 1 and not E.tuning_pending():
                    break
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / steps
        res["crops_%d" % crops] = {"clip_forwards_per_step": n * crops, "step_s": round(dt, 4), "clip_forwards_per_s": round(n * crops / dt, 1)}
        del frames, out
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--turns", type=int, default=9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--clip-times", type=int, default=225)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--no-features", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ten_crop: needs an MI355X (no CPU path, no CPU timing)")
    dev = torch.device("cuda:0")
    res = {"kernels": bench_kernels(dev, a.turns, a.reps)}
    if not a.no_features:
        res["features"] = bench_features(dev, a.clip_times, a.steps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
