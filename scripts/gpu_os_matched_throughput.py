"""Throughput of the optimal statistic under per-realisation noise parameters, headline configuration (68 pulsars x 5000 TOAs, HD GWB
+ RN + EFAC/EQUAD + ECORR; K = 60 + 28 = 88 columns per pulsar), R realisations per batch with theta drawn from a prior, timed with
HIP events in ONE process:

  generate             eng.generate(R, theta=theta)
  generate_os          eng.generate_os(R, theta=theta, chunk=R)                  (the fixed-noise statistic: the parent's path)
  generate_os matched  eng.generate_os(R, theta=theta, matched=True, chunk=R)

The three alternate step by step after a warm-up, so clock drift hits all alike.  The kernels of the matched path are also timed on
their own on one batch of residuals: the pta_os_project calls (one per block of 64 rows of V), pta_os_matched_prior,
pta_os_matched_solve (with its operation count from the shapes over the measured fp64 FMA rate of pta_microbench kind 1) and
pta_os_matched_pairs with and without the per-pair output.  The host preparation is timed with a host clock.  Prints one JSON line;
--out also writes it to a file.

    timeout -k 10 900 python scripts/gpu_os_matched_throughput.py --steps 10 --warmup 2 --out profiles/r09_os_matched_throughput.json
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench import build_engine  # noqa: E402
from pta_replicator_amd import _lib, device as dv  # noqa: E402


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
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5, help="launches per per-kernel timing")
    ap.add_argument("--components", type=int, default=14)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    R = a.batch
    eng, _, _ = build_engine(68, 5000, seed=1234)
    t0 = time.perf_counter()
    eng.prepare_optimal_statistic(components=a.components)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    eng.prepare_optimal_statistic(components=a.components, matched=True)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    eng.set_hyper_prior(gwb_log10_A=(-15.0, -14.0), gwb_gamma=(3.5, 5.0), rn_log10_A=(-15.5, -13.0), rn_gamma=(2.0, 6.0))
    theta = eng.sample_theta(R)
    out = dv.empty((R, eng.n_toa))
    runs = (lambda: eng.generate(R, out=out, theta=theta), lambda: eng.generate_os(R, theta=theta, chunk=R),
            lambda: eng.generate_os(R, theta=theta, matched=True, chunk=R))
    for _ in range(a.warmup):
        for f in runs:
            f()
    torch.cuda.synchronize()
    times = [[], [], []]
    for _ in range(a.steps):
        for t, f in zip(times, runs):
            t.append(event_ms(f))

    # the kernels on their own, on one batch of residuals
    eng.generate(R, out=out, theta=theta)
    st = eng._os
    m = st["matched"]
    dev = eng._os_matched_theta(st, theta, R, "bench")
    res_out = eng._os_matched_out(st, R, True)
    eng._os_matched_launch(out, R, dev, 0, res_out)
    ws = m["ws"]
    P, C, K, K_rn, s = eng.P, st["C"], m["K"], m["K_rn"], dv.stream_ptr()
    npairs = len(st["plan"].den)
    hy = eng._hyper_tables()

    def proj(k0):
        return lambda: _lib.call("pta_os_project", ctypes.c_void_p(m["Vt"].data_ptr() + 8 * k0 * eng.n_toa), eng.n_toa, min(64, K - k0), dv.ptr(st["off"]),
                                 P, dv.ptr(out), out.stride(0), R, ctypes.c_void_p(ws["q"].data_ptr() + 8 * P * k0), P * K, s)
    prior = lambda: _lib.call("pta_os_matched_prior", R, P, K_rn, C, dv.ptr(hy["rn_f"]), dv.ptr(hy["rn_tspan"]), dv.ptr(m["rn_phi"]),  # noqa: E731
                              dv.ptr(dev["rn_log10_A"]), dv.ptr(dev["rn_gamma"]), m["T"], dv.ptr(dev["gw_log10_A"]), dv.ptr(dev["gw_gamma"]),
                              dv.ptr(m["s"]), dv.ptr(ws["b"]), s)
    solve = lambda: _lib.call("pta_os_matched_solve", dv.ptr(m["A"]), P, K, C, R, dv.ptr(ws["b"]), dv.ptr(ws["q"]), P * K, 64, dv.ptr(m["S"]),  # noqa: E731
                              dv.ptr(m["s"]), dv.ptr(ws["X"]), dv.ptr(ws["Z"]), s)

    def pairs(with_rho):
        A2, sg, rho, sp = res_out["A2"], res_out["sigma"], res_out["rho"], res_out["sigma_pair"]
        return lambda: _lib.call("pta_os_matched_pairs", dv.ptr(ws["X"]), dv.ptr(ws["Z"]), P, C, R, dv.ptr(st["pa"]), dv.ptr(st["pb"]), npairs,
                                 dv.ptr(m["G"]), dv.ptr(m["G2"]), st["n_orf"], dv.ptr(A2), st["n_orf"], dv.ptr(sg), st["n_orf"],
                                 dv.ptr(rho) if with_rho else None, dv.ptr(sp) if with_rho else None, npairs if with_rho else 0, s)
    t_proj = [event_ms(proj(k0), a.reps) for k0 in range(0, K, 64)]
    t_prior, t_solve = event_ms(prior, a.reps), event_ms(solve, a.reps)
    t_pairs, t_pairs_rho = event_ms(pairs(False), a.reps), event_ms(pairs(True), a.reps)
    torch.cuda.synchronize()
    fma = ctypes.c_double(0.0)
    _lib.call("pta_microbench", 1, 1 << 30, 2000, 0, ctypes.byref(fma))

    flop = R * P * (K ** 3 / 3.0 + K ** 2 * (1.0 + C) + C ** 2 * K)       # Cholesky K^3/3 + substitution + H_F^T H_F (half of the count of the products taken in full)
    floor_ms = flop / (fma.value * 1e12) * 1e3
    nz = C * (C + 1) // 2
    pair_bytes = 8.0 * R * npairs * 2 * (nz + C)
    med = [float(np.median(t)) for t in times]
    res = dict(
        config="68 x 5000, HD GWB + RN(67) + EFAC/EQUAD + ECORR, throughput mode, theta ~ prior (gwb_log10_A, gwb_gamma, rn_log10_A, rn_gamma); "
               "OS: spin model, GWB auto-term, ORFs hd/monopole/dipole",
        device=torch.cuda.get_device_name(0), batch=R, steps=a.steps, warmup=a.warmup, components=a.components, C=C, K=K, n_pairs=npairs,
        prepare_optimal_statistic_s=round(t1 - t0, 3), prepare_optimal_statistic_matched_s=round(t2 - t1, 3),
        generate_theta_ms_median=round(med[0], 4), generate_os_theta_ms_median=round(med[1], 4), generate_os_matched_ms_median=round(med[2], 4),
        generate_theta_ms_min=round(min(times[0]), 4), generate_os_theta_ms_min=round(min(times[1]), 4), generate_os_matched_ms_min=round(min(times[2]), 4),
        generate_theta_realisations_per_s=round(R / med[0] * 1e3, 1), generate_os_theta_realisations_per_s=round(R / med[1] * 1e3, 1),
        generate_os_matched_realisations_per_s=round(R / med[2] * 1e3, 1),
        os_project_blocks_ms=[round(t, 4) for t in t_proj], os_matched_prior_ms=round(t_prior, 4), os_matched_solve_ms=round(t_solve, 4),
        os_matched_pairs_ms=round(t_pairs, 4), os_matched_pairs_with_rho_ms=round(t_pairs_rho, 4),
        fp64_fma_tflops=round(fma.value, 2), solve_GFLOP=round(flop / 1e9, 2), solve_floor_ms=round(floor_ms, 4),
        solve_fraction_of_fma_floor=round(floor_ms / t_solve, 4), solve_lds_bytes_per_workgroup=8 * (K * (K + C) - K * (K - 1) // 2 + 2 * K),
        pairs_cache_read_GB=round(pair_bytes / 1e9, 3), pairs_cache_read_TBps=round(pair_bytes / (t_pairs * 1e-3) / 1e12, 3),
    )
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
