"""The training side of the non-local attention core -- tedspad_nl_attention_fwd_lse + tedspad_nl_attention_bwd -- beside torch's autograd through
`torch.bmm(theta, phi^T) -> softmax(scale * .) -> torch.bmm(p, g)` on the same f16 tensors (the measuring stick only: nothing in the package calls it),
at the four block shapes of a training iteration: layer2 and layer3 at 224^2 and at 112^2, 24 items (cfg3's 8 x 3 clips).

Each side runs forward + backward per call. FLOP = 4 n q k d forward + 10 n q k d backward (five products: S and dP recomputed once per kernel would be
more -- the count is the chain's, so the TFLOP/s of the two sides compare). `--repeats` windows of `--steps` calls each, alternating, every window ending
in a device synchronise; reported as median [min, max] in ms. A is called faster only if its slowest window beats B's fastest. Prints ONE JSON line.
Reading it: a window is wall time, host dispatch included. Where the chain's time does not move with the shape's FLOP count (the three small shapes) its
windows are bound by the dispatch of the Python autograd chain, and the ratio there compares dispatch paths, not kernels; the device arithmetic of the
two sides is compared at layer2 @224 only.

    python scripts/bench_nl_bwd.py [--items 24] [--steps 20] [--repeats 7]"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_nl import ms, verdict, window  # noqa: E402

SHAPES = {"layer2 @224 (q 1568, k 392, d 256)": (1568, 392, 256), "layer3 @224 (q 392, k 98, d 512)": (392, 98, 512),
          "layer2 @112 (q 392, k 98, d 256)": (392, 98, 256), "layer3 @112 (q 98, k 18, d 512)": (98, 18, 512)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=24)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_nl_bwd: needs an MI355X (no CPU path, no fallback)")
    import statistics
    from ted_spad_amd import _lib
    from ted_spad_amd.engine import _stream_ptr
    from ted_spad_amd.synth import synth_tensor
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n, L = args.items, _lib.lib()
    res = {"device": torch.cuda.get_device_name(dev), "items": n, "windows": args.repeats, "steps_per_window": args.steps, "shapes": {}}
    for name, (q, k, d) in SHAPES.items():
        scale = float(d) ** -0.5
        theta = (synth_tensor(1, "bench_nl_bwd/theta%d" % q, (n, q, d), -1, 1, device=dev) * 1.5).half()      # logits with a standard deviation near 1
        pg = synth_tensor(1, "bench_nl_bwd/pg%d" % q, (n, k, 2 * d), -1, 1, device=dev)
        pg[:, :, :d] *= 1.5
        pg = pg.half()                                                                                         # phi | g as one buffer
        dt = synth_tensor(1, "bench_nl_bwd/dt%d" % q, (n, q, d), -1, 1, device=dev).half()
        out, dth, dpg = torch.empty_like(theta), torch.empty_like(theta), torch.empty_like(pg)
        lse = torch.empty((n, q), dtype=torch.float32, device=dev)
        nbytes = C.c_int64(0)
        _lib.check(L.tedspad_nl_attention_bwd_workspace(n, q, C.byref(nbytes)), "tedspad_nl_attention_bwd_workspace")
        ws = torch.empty(nbytes.value // 4, dtype=torch.float32, device=dev)
        th_c, ph_c, g_c = theta.clone().requires_grad_(), pg[:, :, :d].contiguous().requires_grad_(), pg[:, :, d:].contiguous().requires_grad_()

        def fused():
            sp = _stream_ptr()
            _lib.check(L.tedspad_nl_attention_fwd_lse(theta.data_ptr(), d, pg.data_ptr(), 2 * d, pg.data_ptr() + 2 * d, 2 * d, out.data_ptr(), d, lse.data_ptr(),
                                                      n, q, k, d, C.c_float(scale), _lib.F16, sp), "tedspad_nl_attention_fwd_lse")
            _lib.check(L.tedspad_nl_attention_bwd(theta.data_ptr(), d, pg.data_ptr(), 2 * d, pg.data_ptr() + 2 * d, 2 * d, out.data_ptr(), d, dt.data_ptr(), d,
                                                  lse.data_ptr(), dth.data_ptr(), d, dpg.data_ptr(), 2 * d, dpg.data_ptr() + 2 * d, 2 * d, ws.data_ptr(), n, q, k, d,
                                                  C.c_float(scale), _lib.F16, sp), "tedspad_nl_attention_bwd")

        def chain():
            th_c.grad = ph_c.grad = g_c.grad = None
            torch.bmm(torch.softmax(torch.bmm(th_c, ph_c.transpose(1, 2)) * scale, dim=-1), g_c).backward(dt)

        for _ in range(3):
            fused(), chain()
        torch.cuda.synchronize()
        diff = {"dtheta": float((dth.float() - th_c.grad.float()).abs().max()), "dphi": float((dpg[:, :, :d].float() - ph_c.grad.float()).abs().max()),
                "dg": float((dpg[:, :, d:].float() - g_c.grad.float()).abs().max())}
        tf, tc = [], []
        for _ in range(args.repeats):
            tf.append(window(fused, args.steps))
            tc.append(window(chain, args.steps))
        flop = 14.0 * n * q * k * d
        res["shapes"][name] = {"q": q, "k": k, "d": d, "gflop_per_call": round(flop / 1e9, 2), "fused_ms": ms(tf), "torch_autograd_chain_ms": ms(tc),
                               "fused_tflops": round(flop / statistics.median(tf) / 1e9, 1), "chain_tflops": round(flop / statistics.median(tc) / 1e9, 1),
                               "chain_over_fused_median": round(statistics.median(tc) / statistics.median(tf), 3), "verdict": verdict(tf, tc, "fused", "chain"),
                               "max_abs_diff_vs_chain": diff}
        del theta, pg, dt, out, dth, dpg, lse, ws, th_c, ph_c, g_c
    print(json.dumps(res))


if __name__ == "__main__":
    main()
