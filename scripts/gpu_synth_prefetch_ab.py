"""Per-piece attribution of the memory-operand pipelining of k_engine_synth_mfma on the headline workload (68 x 5000, R = 1024): ONE
process, blocks of steps alternating between kernel variants (the method of scripts/gpu_lean_kernels_ab.py), HIP events.

    python scripts/gpu_synth_prefetch_ab.py [--reps 25] [--steps 6] [--out FILE]

synth_variant 16 + pf + 8 w3 (pta_engine_synth): pf 4 = the epilogue's GWB operands one step ahead, 5 = all of its operands, 2 = the
rotation's first two K-steps requested before the ECORR staging, 6 / 7 = 4 / 5 with 2; w3 = compiled for 3 workgroups per CU (the
epilogue prefetch does not fit 128 VGPRs without scratch, so it exists at 3 only).  48 is the kernel without any of it (bit-identical
results: tests/test_gpu_synth_prefetch.py).  A kernel compiled for 3 per CU that needs no more than 128 VGPRs still runs at 4 (24, 26): what 3
per CU cost by themselves is variant 112, the default kernel with its LDS padded.  16 + 32 + pf = the copy of the kernel that serves
any plan (ALL = false) instead of the one compiled for a complete plan: 50 against 48 is the prologue alone, 16 against 48 the
straight-line copy alone (its GWB row addresses are computed once, not per epilogue step).  The comparison against the parent COMMIT in profiles/r16_synth_prefetch.json is bench.py
itself, run alternately with PTA_REPLICATOR_AMD_LIB naming a build of the parent's library and without it."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG = {"default (0)": 0, "the kernel as it was: no pipelining, 4 per CU, the copy for any plan (48)": 48, "no pipelining, 4 per CU (16)": 16, "rotation prologue, 4 per CU (18)": 18,
       "rotation prologue, 4 per CU, the copy for any plan (50)": 50,
       "default kernel held to 3 workgroups per CU by 12 KB of unused LDS (112)": 112, "no pipelining, 3 per CU (24)": 24, "rotation prologue, 3 per CU (26)": 26,
       "epilogue GWB operands ahead, 3 per CU (28)": 28, "epilogue all operands ahead, 3 per CU (29)": 29,
       "GWB operands ahead + rotation prologue, 3 per CU (30)": 30, "all operands ahead + rotation prologue, 3 per CU (31)": 31}


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
    res = {k: {"synth_variant": CFG[k], "median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
               "p25_ms": round(sorted(v)[len(v) // 4], 4), "p75_ms": round(sorted(v)[3 * len(v) // 4], 4)}
           for k, v in times.items()}
    line = {"config": "68 x 5000, R = 1024, throughput mode", "device": torch.cuda.get_device_name(0), "blocks_per_variant": args.reps,
            "steps_per_block": args.steps, "ms_per_step": res}
    txt = json.dumps(line, indent=1)
    if args.out:
        open(args.out, "w").write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
