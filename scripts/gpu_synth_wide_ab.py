"""The synthesis kernel with four adjacent TOAs per lane (synth_variant 0) against the kernel as it was (synth_variant 2) on the headline
workload (68 x 5000, R = 1024): ONE process, blocks of steps alternating between the two (the method of scripts/gpu_lean_kernels_ab.py),
HIP events.

    python scripts/gpu_synth_wide_ab.py [--reps 25] [--steps 6] [--out FILE]

synth_variant 2 is the same code in every build since round 13, so its row is the drift between processes; the per-step blocks of
profiles/r17_synth_wide.json are this script run with PTA_REPLICATOR_AMD_LIB naming builds of the library with the steps switched on one
after the other, and the comparison against the parent COMMIT is bench.py itself, run alternately with a build of the parent's library."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG = {"synth 0": 0, "synth 2": 2}


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
    for s in CFG.values():
        eng.synth_variant = s
        for i in range(2):
            eng.generate(R, r0=i * R, out=out)
    torch.cuda.synchronize()
    times = {k: [] for k in CFG}
    for rep in range(args.reps):
        for name, s in CFG.items():
            eng.synth_variant = s
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(args.steps):
                eng.generate(R, r0=(rep * args.steps + i) * R, out=out)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.steps)
    res = {k: {"synth_variant": CFG[k], "median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
           for k, v in times.items()}
    line = {"config": "68 x 5000, R = 1024, throughput mode", "device": torch.cuda.get_device_name(0), "blocks_per_variant": args.reps,
            "steps_per_block": args.steps, "ms_per_step": res}
    txt = json.dumps(line, indent=1)
    if args.out:
        open(args.out, "w").write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
