"""Per-item attribution of the chirp-z ladder bits 16 / 32 / 64 and of the red-noise loop addressing on the headline workload (68 x 5000,
R = 1024): ONE process, blocks of steps alternating between kernel variants (the method of scripts/gpu_hyper_throughput.py), HIP events.

    python scripts/gpu_lean_kernels_ab.py [--reps 25] [--steps 6] [--out FILE]

czt_variant 25 / synth_variant 2 are the kernels as they were before those items (bit-identical results: tests/test_gpu_czt_lean.py,
tests/test_gpu_synth_lean.py).  The comparison against the parent COMMIT in profiles/r13_lean_kernels.json is bench.py itself, run
alternately with PTA_REPLICATOR_AMD_LIB naming a build of the parent's library and without it."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG = {"default": (0, 0), "before (czt 25, synth 2)": (25, 2), "czt 25": (25, 0), "synth 2": (0, 2),
       "czt 15+16": (41, 0), "czt 15+32": (57, 0), "czt 15+64": (89, 0), "czt 15+16+32+64": (137, 0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    from bench import build_engine
    from pta_replicator_amd import device as dv
    eng, _, _ = build_engine(68, 5000, seed=20260921)
    R = 1024
    out = dv.empty((R, eng.n_toa))
    for c, s in CFG.values():
        eng.czt_variant, eng.synth_variant = c, s
        for i in range(2):
            eng.generate(R, r0=i * R, out=out)
    torch.cuda.synchronize()
    times = {k: [] for k in CFG}
    for rep in range(args.reps):
        for name, (c, s) in CFG.items():
            eng.czt_variant, eng.synth_variant = c, s
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(args.steps):
                eng.generate(R, r0=(rep * args.steps + i) * R, out=out)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.steps)
    res = {k: {"czt_variant": CFG[k][0], "synth_variant": CFG[k][1], "median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
               "max_ms": round(max(v), 4), "p25_ms": round(sorted(v)[len(v) // 4], 4), "p75_ms": round(sorted(v)[3 * len(v) // 4], 4)}
           for k, v in times.items()}
    line = {"config": "68 x 5000, R = 1024, throughput mode", "device": torch.cuda.get_device_name(0), "blocks_per_variant": args.reps,
            "steps_per_block": args.steps, "ms_per_step": res}
    txt = json.dumps(line, indent=1)
    if args.out:
        open(args.out, "w").write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
