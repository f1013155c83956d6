"""The ORF mix as a streaming kernel (pta_gwb_mix variant 0, k_gwb_mix_stream) against the kernel it replaces (variant 3, k_gwb_mix_small)
on the headline workload (68 x 5000, R = 1024, npts = 600): ONE process, blocks alternating between the two (the method of
scripts/gpu_lean_kernels_ab.py), HIP events.  Two things are timed, each in `--rounds` independent rounds of `--reps` blocks per variant:
the launch alone on the engine's own workspace, and the whole step with engine.mix_variant switched.

    python scripts/gpu_mix_stream_ab.py [--reps 15] [--steps 6] [--rounds 2] [--out FILE]

The rule the result is judged by: the new kernel stays only if its median is below the old one's lower quartile in every round."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG = {"stream (variant 0)": 0, "small (variant 3)": 3}


def quartiles(v):
    q = statistics.quantiles(v, n=4, method="inclusive")
    return {"median_ms": round(q[1], 5), "p25_ms": round(q[0], 5), "p75_ms": round(q[2], 5), "min_ms": round(min(v), 5), "max_ms": round(max(v), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    from bench import build_engine
    from pta_replicator_amd import _lib, device as dv
    eng, _, _ = build_engine(68, 5000, seed=20260921)
    R = 1024
    out = dv.empty((R, eng.n_toa))
    ws = eng.workspace(R)
    for v in CFG.values():
        eng.mix_variant = v
        for i in range(2):
            eng.generate(R, r0=i * R, out=out)
    torch.cuda.synchronize()
    s, P, npts = dv.stream_ptr(), eng.P, eng.plan.gw_npts

    def launch(v):
        _lib.call("pta_gwb_mix", dv.ptr(eng.d_M), P, dv.ptr(ws["G0"]), R, npts, npts, dv.ptr(ws["G"]), v, s)

    def step(v, i):
        eng.mix_variant = v
        eng.generate(R, r0=i * R, out=out)

    def block(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(args.steps):
            fn(i)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.steps

    rounds = []
    for rnd in range(args.rounds):
        kern, steps = {k: [] for k in CFG}, {k: [] for k in CFG}
        for rep in range(args.reps):
            for name, v in CFG.items():
                kern[name].append(block(lambda i: launch(v)))
        for rep in range(args.reps):
            for name, v in CFG.items():
                steps[name].append(block(lambda i: step(v, (rnd * args.reps + rep) * args.steps + i)))
        new, old = list(CFG)
        rounds.append({"launch_alone": {k: quartiles(x) for k, x in kern.items()}, "whole_step": {k: quartiles(x) for k, x in steps.items()},
                       "launch_new_median_below_old_p25": statistics.median(kern[new]) < quartiles(kern[old])["p25_ms"],
                       "step_new_median_below_old_p25": statistics.median(steps[new]) < quartiles(steps[old])["p25_ms"]})
    eng.mix_variant = 0
    line = {"config": "68 x 5000, R = 1024, npts = %d, throughput mode" % npts, "device": torch.cuda.get_device_name(0),
            "blocks_per_variant": args.reps, "per_block": args.steps, "bytes_moved": 16 * R * P * npts, "rounds": rounds}
    txt = json.dumps(line, indent=1)
    if args.out:
        open(args.out, "w").write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
