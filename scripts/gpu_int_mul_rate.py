"""Issue rate of v_mad_u64_u32 (the Philox multiply) against v_fma_f64 and v_bitop3_b32 on the MI355X: pta_microbench kind 9, 16 independent
chains per lane and nothing else in the loop, 4 (and 8) waves per SIMD, the three instructions alternating, median of `--reps` launches.
DESIGN 4.1's instruction-count estimates weigh the integer multiply with this ratio.

    python scripts/gpu_int_mul_rate.py [--reps 7] [--iters 20000] [--out profiles/r23_int_mul_rate.json]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OPS = {"v_fma_f64": 0, "v_mad_u64_u32": 1, "v_bitop3_b32": 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20000)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    from pta_replicator_amd import _lib, device as dv
    info = dv.device_info()
    res = {"device": torch.cuda.get_device_name(0), "cu_count": info["cu_count"], "chains_per_lane": 16, "iters": args.iters, "launches": args.reps,
           "unit": "tera lane-instructions / s (median [min, max])", "waves_per_simd": {}}
    for wps in (4, 8):
        rate = {k: [] for k in OPS}
        for rep in range(args.reps):
            for name, op in OPS.items():
                r = ctypes.c_double(0.0)
                _lib.call("pta_microbench", 9, wps, args.iters, op, ctypes.byref(r))
                rate[name].append(r.value)
        row = {k: [round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)] for k, v in rate.items()}
        fma = statistics.median(rate["v_fma_f64"])
        row["relative_to_v_fma_f64"] = {k: round(statistics.median(v) / fma, 3) for k, v in rate.items()}
        res["waves_per_simd"][str(wps)] = row
    txt = json.dumps(res, indent=1)
    if args.out:
        open(args.out, "w").write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
