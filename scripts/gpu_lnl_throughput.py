"""Throughput of the marginalised log-likelihood on a theta grid, headline configuration (68 pulsars x 5000 TOAs, HD GWB + RN +
EFAC/EQUAD + ECORR; K = 60 + 28 = 88 columns per pulsar, 3 timing-model rows), R realisations against G grid points, timed with HIP
events in ONE process:

  per kernel, for G in --grids   the pta_os_project calls (one per block of 64 operator rows), pta_lnl_quad, pta_os_matched_prior,
                                 pta_lnl_factor, pta_lnl_apply, pta_lnl_reduce on one batch of residuals, and log_likelihood as a whole
  generate                       eng.generate(R, theta=theta)
  optimal_statistic matched      eng.optimal_statistic(rows, theta=theta)            (the parent's per-realisation-noise path)
  generate_lnl                   eng.generate_lnl(R, grid of the first G, theta=theta, chunk=R)

The last three alternate step by step after a warm-up, so clock drift hits all alike.  pta_lnl_apply is quoted in TFLOP/s twice: the
algorithm's count G P K^2 R (2 flops per entry of the lower triangle), and the count the matrix cores execute (the triangle in blocks
of 16 rows x 4 columns, rows padded to 16), both against the fp64 MFMA rate pta_microbench kind 0 measures in the same process;
pta_lnl_quad in TB/s over the residual bytes it must read once.  Prints one JSON line; --out also writes it to a file.

    timeout -k 10 900 python scripts/gpu_lnl_throughput.py --steps 10 --warmup 2 --out profiles/r10_lnl_throughput.json
"""
import argparse
import ctypes
import json
import os
import sys

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
    ap.add_argument("--grids", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5, help="launches per per-kernel timing")
    ap.add_argument("--components", type=int, default=14)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    R = a.batch
    eng, _, _ = build_engine(68, 5000, seed=1234)
    eng.workspace_bytes = 32 << 30          # one grid chunk at G = 1024 (4.3 MB of operators per grid point)
    eng.prepare_optimal_statistic(components=a.components, matched=True)
    eng.prepare_likelihood(components=a.components)
    eng.set_hyper_prior(gwb_log10_A=(-15.0, -14.0), gwb_gamma=(3.5, 5.0), rn_log10_A=(-15.5, -13.0), rn_gamma=(2.0, 6.0))
    theta = eng.sample_theta(R)
    rows = dv.empty((R, eng.n_toa))
    eng.generate(R, out=rows, theta=theta)
    st = eng._lnl
    P, K, Kt, C, m, K_rn = eng.P, st["K"], st["Kt"], st["C"], st["m"], st["K_rn"]
    s = dv.stream_ptr()
    hy = eng._hyper_tables()
    mfma = ctypes.c_double(0.0)
    _lib.call("pta_microbench", 0, 1 << 30, 2000, 0, ctypes.byref(mfma))
    rng = np.random.default_rng(1)
    res = dict(config="68 x 5000, HD GWB + RN(67) + EFAC/EQUAD + ECORR; likelihood: spin model, common process on 14 frequencies, grid ~ prior "
                      "(gwb_log10_A, gwb_gamma, rn_log10_A, rn_gamma)", device=torch.cuda.get_device_name(0), batch=R, steps=a.steps, warmup=a.warmup,
               reps=a.reps, K=K, C=C, timing_model_rows=m, fp64_mfma_tflops=round(mfma.value, 2), grids={})
    kt = (K + 15) // 16
    nks = (K + 3) // 4
    mfma_per_tile = sum(min(4 * (it + 1), nks) for it in range(kt) if 16 * it < K)
    grids = {}
    for G in a.grids:
        grid = {"gwb_log10_A": rng.uniform(-15.0, -14.0, G), "gwb_gamma": rng.uniform(3.5, 5.0, G), "rn_log10_A": rng.uniform(-15.5, -13.0, (G, P)),
                "rn_gamma": rng.uniform(2.0, 6.0, (G, P))}
        grids[G] = grid
        th, _ = eng._lnl_check_grid(st, grid)
        dev = eng._lnl_grid_device(st, th, G)
        Rc, Gc = eng._lnl_chunks(st, R, G, False, False)
        assert (Rc, Gc) == (R, G), (Rc, Gc)
        out = eng._lnl_out(R, G, False)
        for _ in range(a.warmup):
            out["factored"] = None
            eng._lnl_launch(rows, R, 0, dev, Rc, Gc, out)
        ws = st["ws"]

        def proj(k0):
            return lambda: _lib.call("pta_os_project", ctypes.c_void_p(st["Vt"].data_ptr() + 8 * k0 * eng.n_toa), eng.n_toa, min(64, Kt - k0), dv.ptr(st["off"]),
                                     P, dv.ptr(rows), rows.stride(0), R, ctypes.c_void_p(ws["q"].data_ptr() + 8 * P * k0), P * Kt, s)
        quad = lambda: _lib.call("pta_lnl_quad", dv.ptr(rows), rows.stride(0), R, dv.ptr(st["off"]), P, dv.ptr(st["dinv"]), dv.ptr(st["psr_ep"]),  # noqa: E731
                                 dv.ptr(st["ep_ptr"]), dv.ptr(st["ep_idx"]), dv.ptr(st["ep_g"]), dv.ptr(ws["q"]), P * Kt, 64, K, m, dv.ptr(st["Ht"]), eng.n_toa, dv.ptr(ws["r0"]), s)
        prior = lambda: _lib.call("pta_os_matched_prior", G, P, K_rn, C, dv.ptr(hy["rn_f"]), dv.ptr(hy["rn_tspan"]), dv.ptr(st["rn_phi"]),  # noqa: E731
                                  dv.ptr(dev["rn_log10_A"]), dv.ptr(dev["rn_gamma"]), st["T"], dv.ptr(dev["gw_log10_A"]), dv.ptr(dev["gw_gamma"]),
                                  dv.ptr(st["s"]), dv.ptr(ws["b"]), s)
        factor = lambda: _lib.call("pta_lnl_factor", dv.ptr(st["A"]), P, K, C, G, dv.ptr(ws["b"]), dv.ptr(ws["Lt"]), dv.ptr(ws["logdet"]), s)  # noqa: E731
        apply_ = lambda: _lib.call("pta_lnl_apply", dv.ptr(ws["Lt"]), dv.ptr(ws["logdet"]), dv.ptr(ws["b"]), P, K, C, G, dv.ptr(ws["q"]), P * Kt, 64, Kt, R,  # noqa: E731
                                   dv.ptr(ws["r0"]), dv.ptr(st["s"]), dv.ptr(st["c"]), dv.ptr(ws["lp"]), P * R, R, s)
        reduce_ = lambda: _lib.call("pta_lnl_reduce", dv.ptr(ws["lp"]), P * R, R, P, G, R, dv.ptr(out["lnl"]), R, s)  # noqa: E731
        t_proj = [event_ms(proj(k0), a.reps) for k0 in range(0, Kt, 64)]
        t_quad, t_prior, t_factor = event_ms(quad, a.reps), event_ms(prior, a.reps), event_ms(factor, a.reps)
        t_apply, t_reduce = event_ms(apply_, a.reps), event_ms(reduce_, a.reps)
        whole = [event_ms(lambda: eng.log_likelihood(rows, grid)) for _ in range(a.steps)]
        torch.cuda.synchronize()
        flop_alg = float(G) * P * K * K * R
        flop_mfma = float(G) * P * mfma_per_tile * 2048.0 * 2 * ((R + 31) // 32)
        flop_factor = float(G) * P * (K ** 3 / 3.0 + K * 16 * 16 / 3.0)        # Cholesky K^3/3 + the K/16 diagonal blocks' inverses
        t_whole = float(np.median(whole))
        res["grids"][str(G)] = dict(
            os_project_blocks_ms=[round(t, 4) for t in t_proj], lnl_quad_ms=round(t_quad, 4), os_matched_prior_ms=round(t_prior, 4),
            lnl_factor_ms=round(t_factor, 4), lnl_apply_ms=round(t_apply, 4), lnl_reduce_ms=round(t_reduce, 4),
            log_likelihood_ms_median=round(t_whole, 4), log_likelihood_ms_min=round(min(whole), 4),
            evaluations_per_s=round(R * G / t_whole * 1e3, 1), pulsar_evaluations_per_s=round(R * G * P / t_whole * 1e3, 1),
            apply_GFLOP_algorithm=round(flop_alg / 1e9, 2), apply_TFLOPs_algorithm=round(flop_alg / (t_apply * 1e-3) / 1e12, 2),
            apply_GFLOP_mfma=round(flop_mfma / 1e9, 2), apply_TFLOPs_mfma=round(flop_mfma / (t_apply * 1e-3) / 1e12, 2),
            apply_fraction_of_mfma_rate=round(flop_mfma / (t_apply * 1e-3) / 1e12 / mfma.value, 4),
            apply_operator_read_GB=round(8.0 * G * P * K * K * ((R + 127) // 128) / 1e9, 3),
            factor_GFLOP=round(flop_factor / 1e9, 2), factor_TFLOPs=round(flop_factor / (t_factor * 1e-3) / 1e12, 3),
            quad_row_GB=round(8.0 * R * eng.n_toa / 1e9, 3), quad_TBps=round(8.0 * R * eng.n_toa / (t_quad * 1e-3) / 1e12, 3),
            project_TBps=[round(8.0 * R * eng.n_toa / (t * 1e-3) / 1e12, 3) for t in t_proj])

    # generate_lnl against generate and against the matched optimal statistic, alternating
    g0 = grids[a.grids[0]]
    out_rows = dv.empty((R, eng.n_toa))
    runs = (lambda: eng.generate(R, out=out_rows, theta=theta), lambda: eng.optimal_statistic(rows, theta=theta),
            lambda: eng.generate_lnl(R, g0, theta=theta, chunk=R))
    for _ in range(a.warmup):
        for f in runs:
            f()
    torch.cuda.synchronize()
    times = [[], [], []]
    for _ in range(a.steps):
        for t, f in zip(times, runs):
            t.append(event_ms(f))
    med = [float(np.median(t)) for t in times]
    res.update(compare_grid=a.grids[0], generate_theta_ms_median=round(med[0], 4), optimal_statistic_matched_ms_median=round(med[1], 4),
               generate_lnl_ms_median=round(med[2], 4), generate_theta_ms_min=round(min(times[0]), 4),
               optimal_statistic_matched_ms_min=round(min(times[1]), 4), generate_lnl_ms_min=round(min(times[2]), 4),
               generate_theta_realisations_per_s=round(R / med[0] * 1e3, 1), generate_lnl_realisations_per_s=round(R / med[2] * 1e3, 1),
               generate_lnl_over_generate=round(med[2] / med[0], 3), likelihood_part_over_matched_os=round((med[2] - med[0]) / med[1], 3))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
