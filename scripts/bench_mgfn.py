"""MGFN inference on one MI355X: a UCF-test-sized STAND-IN (290 videos x 10 crops, F = 2048, T_i = 8 + floor(1017 u_i) segments with
u_i = synth_tensor values; the real length mix is not available here), timed three ways in alternating turns:

  (i)   MGFN.score on the whole list (one ragged batch, csrc/mgfn.hip)
  (ii)  test.py's loop: MGFN.forward per video, batch 1
  (iii) the fp32 torch-eager restatement (tests/mgfn_restate.py) per video, batch 1: a stand-in for running the reference on this GPU

Each turn is timed with device synchronisation after a warm-up that runs each of them once on the whole list. Prints one JSON line:
per-run seconds, videos/s, segments/s, achieved FLOP/s from the shape-based FLOP count below, and its share of the 157 TF f32 matrix peak.

    python scripts/bench_mgfn.py [--videos 290] [--turns 3]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from ted_spad_amd.mgfn import MGFN  # noqa: E402
from ted_spad_amd.synth import synth_mgfn_state_dict, synth_tensor  # noqa: E402

PEAK_F32_MATRIX = 157.3e12


def flops(T, F=2048, nc=10, dims=(64, 128, 1024), depths=(3, 3, 2), types=("gb", "fb", "fb")):
    """Multiply-adds x 2 of one video's forward, by layer shapes."""
    n = nc * T
    f = 2 * n * 3 * (F + 1) * dims[0]                               # to_tokens + to_mag
    for si, (d, depth, t) in enumerate(zip(dims, depths, types)):
        per = 2 * n * 3 * d * d + 2 * n * d * 4 * d * 2              # scc + feed-forward
        if t == "gb":
            per += 2 * n * d * 3 * d + 2 * n * d * d + 4 * nc * T * T * d   # qkv, to_out, QK^T + PV
        else:
            per += 2 * n * d * d * 2 + 2 * n * d * 5                 # to_v, to_out, rel_pos
        f += depth * per
        if si + 1 < len(dims):
            f += 2 * n * d * dims[si + 1]
    return f + 4 * n * dims[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=290)
    ap.add_argument("--turns", type=int, default=3)
    a = ap.parse_args()
    import mgfn_restate
    torch.cuda.set_device(0)
    lengths = [8 + int(1017 * float(u)) for u in synth_tensor(0, "mgfn_bench_len", (a.videos,))]
    feats = [synth_tensor(0, "mgfn_bench/%d" % i, (T, 10, 2049), 0.0, 2.0, device="cuda") for i, T in enumerate(lengths)]
    m = MGFN().eval()
    m.load_state_dict(synth_mgfn_state_dict(m.state_dict(), 0))
    m = m.cuda()
    sd = {k: v.cuda() for k, v in m.state_dict().items()}
    cfg = (2048, (3, 3, 2), ("gb", "fb", "fb"), 0.1)

    def run_i(vids):
        return m.score(vids)

    def run_ii(vids):
        with torch.no_grad():
            return [m(f.permute(1, 0, 2).unsqueeze(0))[4] for f in vids]

    def run_iii(vids):
        with torch.no_grad():
            return [mgfn_restate.forward(sd, f.permute(1, 0, 2).unsqueeze(0), cfg)["crop_scores"] for f in vids]

    runs = {"i_score_ragged": run_i, "ii_forward_bs1": run_ii, "iii_torch_eager_bs1": run_iii}
    # warm-up, untimed: every run once on the whole list -- the caching allocator grows to the one-batch working set of (i), the
    # weights are packed, and MIOpen searches the eager path's convolution algorithms once per new sequence length
    for k, fn in runs.items():
        t0 = time.perf_counter()
        fn(feats)
        torch.cuda.synchronize()
        print("warm-up %s (%d distinct lengths): %.1f s" % (k, len(set(lengths)), time.perf_counter() - t0), flush=True)
    times = {k: [] for k in runs}
    for _ in range(a.turns):
        for k, fn in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(feats)
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
            del out
            print(k, "%.3f s" % times[k][-1], flush=True)
    total_flop = sum(flops(T) for T in lengths)
    segs = sum(lengths)
    res = {"videos": a.videos, "segments": segs, "tokens": 10 * segs, "tflop": total_flop / 1e12, "runs": {}}
    for k, ts in times.items():
        best, worst = min(ts), max(ts)
        res["runs"][k] = {"seconds": ts, "videos_per_s": [a.videos / worst, a.videos / best], "segments_per_s": [segs / worst, segs / best],
                          "tflop_per_s": [total_flop / worst / 1e12, total_flop / best / 1e12],
                          "f32_matrix_peak_share": [total_flop / worst / PEAK_F32_MATRIX, total_flop / best / PEAK_F32_MATRIX]}
    res["condition_slowest_i_faster_than_fastest_iii"] = max(times["i_score_ragged"]) < min(times["iii_torch_eager_bs1"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
