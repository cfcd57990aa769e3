"""The non-local blocks of I3Res50 (use_nl=True) at the cfg2 shapes -- 375 clips of (3, 16, 224, 224) per forward, f16 -- measured two ways in ONE process:

  network   clips/s of `extract_features` with use_nl=True beside use_nl=False (same weights but for the nl keys, same clips), timed alternately.
  kernel    tedspad_nl_attention_fwd per block shape -- layer2: 1568 queries x 392 keys, d = 256; layer3: 392 x 98, d = 512 -- beside the chain it fuses,
            `torch.bmm(theta, phi^T) -> softmax(scale * .) -> torch.bmm(p, g)` on the same 16-bit tensors (the measuring stick only: nothing in the package
            calls it), timed alternately. FLOP = 4 n q k d (the two products; the softmax is not counted), TFLOP/s = FLOP over the median window time.

Every window ends in a device synchronise and holds `--steps` (network) or `--kernel-steps` (kernel) calls after a warm-up that also lets the conv tile
tuner settle; `--repeats` windows of each, alternating, so both sides see the same neighbours on the machine. A is called faster only if its slowest
window beats B's fastest (the run-to-run spread this script itself reports). Prints ONE JSON line.

    python scripts/bench_nl.py [--clips 375] [--steps 3] [--kernel-steps 20] [--repeats 7]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BLOCK_SHAPES = {"layer2 (28x28x2 -> 14x14x2, d=256)": (1568, 392, 256), "layer3 (14x14x2 -> 7x7x2, d=512)": (392, 98, 512)}


def window(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def ms(ts):
    return {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}


def verdict(a, b, na, nb):
    return "%s faster beyond the spread" % na if max(a) < min(b) else ("%s faster beyond the spread" % nb if max(b) < min(a) else "within the spread")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=375)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--kernel-steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--skip-network", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_nl: needs an MI355X (no CPU path, no fallback)")
    from ted_spad_amd import _lib, engine as E
    from ted_spad_amd.engine import _stream_ptr
    from ted_spad_amd.model_loaders import wrapper_i3d
    from ted_spad_amd.synth import synth_clips, synth_state_dict, synth_tensor
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n = args.clips
    res = {"device": torch.cuda.get_device_name(dev), "clips_per_forward": n, "windows": args.repeats,
           "steps_per_window": {"network": args.steps, "kernel": args.kernel_steps}, "kernel": {}}

    # ---- the attention kernel beside the chain it fuses -------------------------------------------------------------------------------------
    L = _lib.lib()
    for name, (q, k, d) in BLOCK_SHAPES.items():
        scale = float(d) ** -0.5
        theta = (synth_tensor(1, "bench_nl/theta%d" % d, (n, q, d), -1, 1, device=dev) * 1.5).half()          # logits with a standard deviation near 1
        pg = synth_tensor(1, "bench_nl/pg%d" % d, (n, k, 2 * d), -1, 1, device=dev)
        pg[:, :, :d] *= 1.5
        pg = pg.half()                                                                                       # phi | g as the block's one GEMM writes them
        phi, g = pg[:, :, :d].contiguous(), pg[:, :, d:].contiguous()                                        # the chain gets contiguous operands
        out = torch.empty((n, q, d), dtype=torch.float16, device=dev)

        def fused():
            _lib.check(L.tedspad_nl_attention_fwd(theta.data_ptr(), d, pg.data_ptr(), 2 * d, pg.data_ptr() + 2 * d, 2 * d, out.data_ptr(), d, n, q, k, d,
                                                  C.c_float(scale), _lib.F16, _stream_ptr()), "tedspad_nl_attention_fwd")

        def chain():
            return torch.bmm(torch.softmax(torch.bmm(theta, phi.transpose(1, 2)) * scale, dim=-1), g)

        for _ in range(3):
            fused(), chain()
        torch.cuda.synchronize()
        ref = chain().float()
        diff = float((out.float() - ref).abs().max())
        tf, tc = [], []
        for _ in range(args.repeats):
            tf.append(window(fused, args.kernel_steps))
            tc.append(window(chain, args.kernel_steps))
        flop = 4.0 * n * q * k * d
        res["kernel"][name] = {"q": q, "k": k, "d": d, "gflop_per_call": round(flop / 1e9, 2), "fused_ms": ms(tf), "bmm_softmax_bmm_ms": ms(tc),
                               "fused_tflops": round(flop / statistics.median(tf) / 1e9, 1), "chain_tflops": round(flop / statistics.median(tc) / 1e9, 1),
                               "chain_over_fused_median": round(statistics.median(tc) / statistics.median(tf), 3),
                               "verdict": verdict(tf, tc, "fused", "chain"), "max_abs_diff_vs_chain": diff,
                               "score_matrix_mb_not_written": round(n * q * k * 2 / 1e6, 1)}
        del theta, pg, phi, g, out, ref

    # ---- the network with and without the blocks --------------------------------------------------------------------------------------------
    if not args.skip_network:
        nets = {}
        for use_nl in (False, True):
            w = wrapper_i3d(num_classes=102, use_nl=use_nl)
            sd = synth_state_dict(w.state_dict(), 0)
            for key in sd:                                   # a branch that enters the residual stream small, and moderate logits, as tests/nl_ref.nl_state_dict
                if key.endswith(".nl.bn.weight"):
                    sd[key] = sd[key] * 0.2
                if ".nl.theta." in key or ".nl.phi." in key:
                    sd[key] = sd[key] * 0.25
            w.load_state_dict(sd, strict=True)
            nets[use_nl] = w.cuda().eval().i3d
        x = torch.cat([synth_clips(0, min(25, n - i), (3, 16, 224, 224), device=dev, first=i) for i in range(0, n, 25)])
        run = {u: (lambda u=u: nets[u].extract_features(x)) for u in nets}
        with torch.no_grad():
            for u in nets:
                for _ in range(60):                          # warm-up: until the conv tile tuner has settled on this geometry
                    run[u]()
                    if not E.tuning_pending():
                        break
                run[u]()
            t = {False: [], True: []}
            for _ in range(args.repeats):
                for u in (True, False):
                    t[u].append(window(run[u], args.steps))
        cps = lambda ts: round(n / (statistics.median(ts) / 1e3), 1)
        res["network"] = {"use_nl_true_ms": ms(t[True]), "use_nl_false_ms": ms(t[False]), "use_nl_true_clips_per_s": cps(t[True]),
                          "use_nl_false_clips_per_s": cps(t[False]), "ms_added_by_the_five_blocks": round(statistics.median(t[True]) - statistics.median(t[False]), 3),
                          "verdict": verdict(t[False], t[True], "use_nl=False", "use_nl=True")}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
