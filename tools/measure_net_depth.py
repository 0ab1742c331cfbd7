"""Launch time of the default net kernel against the depth of the tower (`Net(..., n_residual=K)`).

    python tools/measure_net_depth.py [--rounds 7] [--reps 40] [--out profiles/net_depth_measure.json]

Two shapes, the default form of each (HipNet mode "f32w"): connect four at 1 536 rows (one full round of row-Winograd
tiles on 256 compute units) and 15x15 at 7 600 boards (the 2-D Winograd form, one board per workgroup, + k_net_heads).
K in {1, 2, 5, 10, 20}: K = 5 runs the kernels compiled for it, every other K the run-time-depth ones.

Method: every (shape, K) is warmed up first; then `rounds` passes, each timing `reps` back-to-back launches of every K
between two device events, the K visited in an order that alternates direction from pass to pass (clock and
temperature drift hit every K alike).  Reported per K: the median over the passes of the mean launch time, the
min-max spread, and the flops the launch executes on the matrix pipe (`HipNet.workgroup_mfma_flops` x workgroups,
padding rows included) over the time, against the float32 matrix peak of the chip.  An affine fit t = a + b K (least
squares over the medians) with its residuals says how far "conv_in + heads fixed, trunk per layer" describes the launch.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEPTHS = (1, 2, 5, 10, 20)
SHAPES = (("connect4_1536_rows", (2, 6, 7), 7, 1536), ("15x15_7600_boards", (2, 15, 15), 225, 7600))
PEAK_F32_MFMA = 256 * 256 * 2.4e9  # 256 CUs x 256 flop / cycle (4 SIMDs x 64, v_mfma_f32_32x32x2_f32) x 2.4 GHz = 157.3 TFLOP/s (bench.py's figure)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default=os.path.join("profiles", "net_depth_measure.json"))
    args = ap.parse_args()
    from caro_ai_amd.lib.model import Net
    from caro_ai_amd.net_hip import HipNet
    dev = "cuda:0"
    result = {"depths": list(DEPTHS), "rounds": args.rounds, "reps": args.reps, "peak_f32_mfma_flops": PEAK_F32_MFMA,
              "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name, shape, A, rows in SHAPES:
        g = torch.Generator().manual_seed(rows)
        x = (torch.rand((rows,) + shape, generator=g) < 0.3).float()
        x[:, 1] *= (1 - x[:, 0])
        x = x.to(dev)
        nets = {}
        for K in DEPTHS:
            torch.manual_seed(K)
            nets[K] = HipNet(Net(shape, A, n_residual=K).eval(), dev)
            for _ in range(10):  # warm-up of this (shape, K): code object, weights into L2, the clock under load
                nets[K](x)
        torch.cuda.synchronize()
        times = {K: [] for K in DEPTHS}
        for r in range(args.rounds):
            for K in (DEPTHS if r % 2 == 0 else DEPTHS[::-1]):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                nets[K](x)
                e0.record()
                for _ in range(args.reps):
                    nets[K](x)
                e1.record()
                e1.synchronize()
                times[K].append(e0.elapsed_time(e1) * 1e3 / args.reps)  # us per launch
        tb = nets[5].L.caro_net_boards_per_workgroup(nets[5].h)
        wgs = -(-rows // tb)
        med = {K: float(np.median(times[K])) for K in DEPTHS}
        a_, b_ = np.linalg.lstsq(np.stack([np.ones(len(DEPTHS)), np.array(DEPTHS, float)], 1),
                                 np.array([med[K] for K in DEPTHS]), rcond=None)[0]
        per = {}
        for K in DEPTHS:
            flops = nets[K].workgroup_mfma_flops() * wgs
            per[str(K)] = {"us_median": med[K], "us_min": float(min(times[K])), "us_max": float(max(times[K])),
                           "mfma_flops": flops, "share_of_f32_mfma_peak": flops / (med[K] * 1e-6) / PEAK_F32_MFMA,
                           "fit_us": float(a_ + b_ * K), "residual_us": float(med[K] - (a_ + b_ * K))}
            nets[K].close()
        result["shapes"][name] = {"rows": rows, "mode": nets[5].mode, "boards_per_workgroup": tb, "workgroups": wgs,
                                  "fit": {"fixed_us": float(a_), "per_layer_us": float(b_)}, "per_depth": per}
        print("%s (%s, %d workgroups): t = %.1f + %.1f K us" % (name, nets[5].mode, wgs, a_, b_))
        for K in DEPTHS:
            p = per[str(K)]
            print("  K=%2d  %8.1f us  [%8.1f, %8.1f]  fit %+6.1f us  %.1f %% of the f32 matrix peak"
                  % (K, p["us_median"], p["us_min"], p["us_max"], p["residual_us"], 100 * p["share_of_f32_mfma_peak"]))
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
