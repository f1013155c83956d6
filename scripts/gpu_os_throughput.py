"""Throughput of the per-realisation optimal statistic, headline configuration (68 pulsars x 5000 TOAs, HD GWB + RN + EFAC/EQUAD +
ECORR), R realisations per batch, timed with HIP events in ONE process:

  generate     eng.generate(R)                          (the bench.py headline path)
  generate_os  eng.generate_os(R, chunk=R)              (the same generation + pta_os_project + pta_os_pairs, statistics only)

The two alternate step by step after a warm-up, so clock drift hits both alike.  The two OS kernels are also timed on their own on
one batch of residuals, with the projection's byte count (every residual once + W once) over its time as a fraction of 8 TB/s.
The host preparation (prepare_optimal_statistic) is timed with a host clock.  Prints one JSON line; --out also writes it to a file.

    timeout -k 10 600 python scripts/gpu_os_throughput.py --steps 20 --warmup 3 --out profiles/r07_os_throughput.json
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench import build_engine  # noqa: E402
from pta_replicator_amd import device as dv  # noqa: E402


def event_ms(fn, reps=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20, help="launches per per-kernel timing")
    ap.add_argument("--components", type=int, default=14)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    R = a.batch
    eng, _, _ = build_engine(68, 5000, seed=1234)
    t0 = time.perf_counter()
    eng.prepare_optimal_statistic(components=a.components)
    torch.cuda.synchronize()
    prep_s = time.perf_counter() - t0
    out = dv.empty((R, eng.n_toa))
    r0 = 0
    for _ in range(a.warmup):
        eng.generate(R, r0=r0, out=out)
        eng.generate_os(R, r0=r0, chunk=R)
        r0 += R
    torch.cuda.synchronize()
    t_gen, t_os = [], []
    for _ in range(a.steps):
        t_gen.append(event_ms(lambda: eng.generate(R, r0=r0, out=out)))
        t_os.append(event_ms(lambda: eng.generate_os(R, r0=r0, chunk=R)))
        r0 += R

    # the two kernels on their own, on one batch of residuals
    eng.generate(R, r0=0, out=out)
    st = eng._os
    A2 = dv.empty((R, st["n_orf"]))
    rho = dv.empty((R, len(st["plan"].den)))
    eng._os_launch(out, R, A2, rho)
    Y = st["Y"]
    from pta_replicator_amd import _lib
    P, C, s = eng.P, st["C"], dv.stream_ptr()
    proj = lambda: _lib.call("pta_os_project", dv.ptr(st["Wt"]), eng.n_toa, C, dv.ptr(st["off"]), P, dv.ptr(out), out.stride(0), R,  # noqa: E731
                             dv.ptr(Y), P * C, s)
    npairs = len(st["plan"].den)

    def pairs(with_rho):
        return lambda: _lib.call("pta_os_pairs", dv.ptr(Y), P * C, P, C, R, dv.ptr(st["pa"]), dv.ptr(st["pb"]), npairs, dv.ptr(st["wt"]),
                                 st["n_orf"], dv.ptr(A2), st["n_orf"], dv.ptr(st["den"]) if with_rho else None,
                                 dv.ptr(rho) if with_rho else None, npairs if with_rho else 0, s)
    proj()
    t_proj = event_ms(proj, a.reps)
    t_pairs = event_ms(pairs(False), a.reps)
    t_pairs_rho = event_ms(pairs(True), a.reps)
    torch.cuda.synchronize()

    bytes_proj = 8.0 * (R * eng.n_toa + C * eng.n_toa + R * P * C)
    flops_useful = 2.0 * R * eng.n_toa * C
    mg, mo = float(np.median(t_gen)), float(np.median(t_os))
    res = dict(
        config="68 x 5000, HD GWB + RN(67) + EFAC/EQUAD + ECORR, throughput mode; OS: spin model, GWB auto-term, ORFs hd/monopole/dipole",
        device=torch.cuda.get_device_name(0), batch=R, steps=a.steps, warmup=a.warmup, components=a.components, columns=C,
        prepare_optimal_statistic_s=round(prep_s, 3),
        generate_ms_per_batch_median=round(mg, 4), generate_os_ms_per_batch_median=round(mo, 4),
        generate_ms_min=round(min(t_gen), 4), generate_os_ms_min=round(min(t_os), 4),
        generate_realisations_per_s=round(R / mg * 1e3, 1), generate_os_realisations_per_s=round(R / mo * 1e3, 1),
        generate_os_over_generate=round(mg / mo, 4),
        os_project_ms=round(t_proj, 4), os_project_GB=round(bytes_proj / 1e9, 4),
        os_project_TBps=round(bytes_proj / (t_proj * 1e-3) / 1e12, 3), os_project_fraction_of_8TBps=round(bytes_proj / (t_proj * 1e-3) / 8e12, 3),
        os_project_useful_TFLOPs=round(flops_useful / (t_proj * 1e-3) / 1e12, 2),
        os_pairs_ms=round(t_pairs, 4), os_pairs_with_rho_ms=round(t_pairs_rho, 4), n_pairs=npairs,
    )
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
