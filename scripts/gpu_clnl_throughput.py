"""Throughput of the correlated likelihood ratio on a (log10_A, gamma) grid, headline configuration (68 pulsars x 5000 TOAs, HD GWB + RN +
EFAC/EQUAD + ECORR; 14 frequencies: n = 68 * 28 = 1904 rows for "hd" and "curn"), R realisations against G grid points, timed with HIP
events in ONE process, every comparison in alternating blocks (one timing of each candidate per block; median and [min, max] over blocks):

  per kernel (ORF "hd")   pta_os_project, pta_clnl_mix, pta_clnl_assemble, pta_potrf_batched_ex, pta_clnl_rhs, pta_clnl_solve, pta_clnl_finish
  factorisation           beside pta_potrf_batched_ex alone on random SPD matrices of the same order and batch, same flags
  solve                   beside the sweep of pta_dgemm calls (transB = 0, beta = 1, batch = G) over the same off-diagonal block shapes
  whole                   generate_correlated_lnl(R, G) beside generate_lnl(R, G) and generate(R)

FLOP counts are the algorithm's: n^3 / 3 per factorisation, n^2 per (grid point, realisation) of the solve (2 flops per entry of the
lower triangle); the assembly is quoted in GB/s over the G n^2 8 bytes it writes.  Prints one JSON line; --out also writes it to a file.

    timeout -k 10 900 python scripts/gpu_clnl_throughput.py --steps 7 --warmup 2 --out profiles/r25_clnl_throughput.json
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

BLK = 64   # PTA_CLNL_BLK


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def summary(ts):
    return dict(median_ms=round(float(np.median(ts)), 4), range_ms=[round(min(ts), 4), round(max(ts), 4)])


def alternate(runs, steps, warmup):
    """{name: [ms per block]}: every block times each run once, in the order given"""
    for _ in range(warmup):
        for f in runs.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(steps):
        for k, f in runs.items():
            times[k].append(event_ms(f))
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--components", type=int, default=14)
    ap.add_argument("--psrs", type=int, default=68)
    ap.add_argument("--toas", type=int, default=5000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    R, G = a.batch, a.grid
    eng, _, _ = build_engine(a.psrs, a.toas, seed=1234)
    eng.workspace_bytes = 32 << 30          # the factors of both ORFs at G = 64 (3.7 GB) in one grid chunk
    eng.prepare_correlated_likelihood(components=a.components, orfs=("hd", "curn"))
    eng.prepare_likelihood(components=a.components)
    rng = np.random.default_rng(1)
    grid = {"gwb_log10_A": rng.uniform(-15.0, -14.0, G), "gwb_gamma": rng.uniform(3.5, 5.0, G)}
    rows = dv.empty((R, eng.n_toa))
    eng.generate(R, out=rows)
    st = eng._clnl
    P, C, n, rho = eng.P, st["C"], st["n"][0], st["rho"][0]
    Rc, Gc = eng._clnl_chunks(st, R, G, with_rows=True, chunk=R)
    assert (Rc, Gc) == (R, G), (Rc, Gc)
    for _ in range(a.warmup):
        eng.correlated_log_likelihood(rows, grid)
    ws = st["ws"]
    dev, _ = eng._clnl_grid(st, grid)
    s = dv.stream_ptr()
    lA, gam = dv.ptr(dev["lA"]), dv.ptr(dev["gamma"])
    M, ntot = ws["M"][0], int(st["off_yp"][-1])
    flags = _lib.POTRF_SUBSTITUTION if n <= 2048 else 0
    out = dv.empty((G, R))
    kernels = {
        "os_project": lambda: eng._stats_project(st["Wt"], C, st["off"], rows, R, ws["Y"]),
        "clnl_mix": lambda: _lib.call("pta_clnl_mix", dv.ptr(ws["Y"]), P * C, P, C, R, dv.ptr(st["Bt"][0]), rho, dv.ptr(ws["Yp"]), ntot, s),
        "clnl_assemble": lambda: _lib.call("pta_clnl_assemble", dv.ptr(st["To"][0]), rho, C, st["gamma"], st["T"], lA, gam, G, dv.ptr(M), s),
        "potrf": lambda: _lib.call("pta_potrf_batched_ex", dv.ptr(M), n, n, n * n, G, dv.ptr(ws["info"]), flags, s),
        "clnl_rhs": lambda: _lib.call("pta_clnl_rhs", dv.ptr(ws["Yp"]), ntot, rho, C, R, st["gamma"], st["T"], lA, gam, G, dv.ptr(ws["V"]), R, s),
        "clnl_solve": lambda: _lib.call("pta_clnl_solve", dv.ptr(M), n, G, dv.ptr(ws["V"]), R, R, dv.ptr(ws["quad"]), R, s),
        "clnl_finish": lambda: _lib.call("pta_clnl_finish", dv.ptr(M), n, G, dv.ptr(ws["quad"]), R, R, dv.ptr(out), R, s),
    }
    # the factorisation alone, on random SPD matrices of the same order and batch: X X^T / n + I, copied into the work buffer before each timing
    X = torch.randn((G, n, n), dtype=torch.float64, device=rows.device)
    spd = torch.baddbmm(torch.eye(n, dtype=torch.float64, device=rows.device).expand(G, n, n), X, X.transpose(1, 2), alpha=1.0 / n)
    del X
    work = torch.empty_like(spd)

    def potrf_alone():
        _lib.call("pta_potrf_batched_ex", dv.ptr(work), n, n, n * n, G, dv.ptr(ws["info"]), flags, s)
    # the sweep of tile products of the same block shapes as the solve's off-diagonal updates: V_j -= L[j, < j] V[< j], j = 1 ..
    Vg = dv.empty((G, n, R))

    def dgemm_sweep():
        for j0 in range(BLK, n, BLK):
            rws = min(BLK, n - j0)
            _lib.call("pta_dgemm", 0, rws, R, j0, -1.0, ctypes.c_void_p(M.data_ptr() + 8 * j0 * n), n, 1, dv.ptr(Vg), R, 1.0,
                      ctypes.c_void_p(Vg.data_ptr() + 8 * j0 * R), R, 0, G, n * n, n * R, n * R, 1, s)
    for _ in range(a.warmup):
        for f in kernels.values():
            f()
        work.copy_(spd)
        potrf_alone()
        Vg.copy_(ws["V"].view(G, n, R))
        dgemm_sweep()
    torch.cuda.synchronize()
    kt = {k: [] for k in kernels}
    kt["potrf_alone_random_spd"], kt["dgemm_sweep_same_blocks"] = [], []
    for _ in range(a.steps):
        for k, f in kernels.items():
            kt[k].append(event_ms(f))
        work.copy_(spd)
        kt["potrf_alone_random_spd"].append(event_ms(potrf_alone))
        Vg.copy_(ws["V"].view(G, n, R))
        kt["dgemm_sweep_same_blocks"].append(event_ms(dgemm_sweep))
    assert int(ws["info"].abs().max()) == 0
    del spd, work, Vg
    flop_factor = G * n ** 3 / 3.0
    flop_solve = float(G) * R * n * n
    flop_sweep = sum(2.0 * min(BLK, n - j0) * R * j0 * G for j0 in range(BLK, n, BLK))
    bytes_assemble = 8.0 * G * n * n

    def rate(x, ts):
        return round(x / (float(np.median(ts)) * 1e-3) / 1e12, 3)
    res = dict(config=f"{a.psrs} x {a.toas}, HD GWB + RN + EFAC/EQUAD + ECORR; correlated likelihood: spin model, {a.components} frequencies, ORFs hd and curn, "
                      f"n = {n}; per-kernel figures for one ORF", device=torch.cuda.get_device_name(0), batch=R, grid=G, steps=a.steps, warmup=a.warmup, n=n, rho=rho, C=C,
               kernels={k: summary(v) for k, v in kt.items()},
               factor_GFLOP=round(flop_factor / 1e9, 1), factor_TFLOPs=rate(flop_factor, kt["potrf"]), potrf_alone_TFLOPs=rate(flop_factor, kt["potrf_alone_random_spd"]),
               solve_GFLOP=round(flop_solve / 1e9, 1), solve_TFLOPs=rate(flop_solve, kt["clnl_solve"]),
               dgemm_sweep_GFLOP=round(flop_sweep / 1e9, 1), dgemm_sweep_TFLOPs=rate(flop_sweep, kt["dgemm_sweep_same_blocks"]),
               assemble_GB=round(bytes_assemble / 1e9, 3), assemble_TBps=rate(bytes_assemble, kt["clnl_assemble"]),
               rhs_GB_written=round(8.0 * G * n * R / 1e9, 3), rhs_TBps=rate(8.0 * G * n * R, kt["clnl_rhs"]))
    out_rows = dv.empty((R, eng.n_toa))
    whole = alternate({"generate": lambda: eng.generate(R, out=out_rows), "generate_lnl": lambda: eng.generate_lnl(R, grid, chunk=R),
                       "generate_correlated_lnl": lambda: eng.generate_correlated_lnl(R, grid, chunk=R),
                       "correlated_log_likelihood": lambda: eng.correlated_log_likelihood(rows, grid)}, a.steps, a.warmup)
    res["whole"] = {k: summary(v) for k, v in whole.items()}
    med = {k: float(np.median(v)) for k, v in whole.items()}
    res.update(generate_realisations_per_s=round(R / med["generate"] * 1e3, 1), generate_lnl_realisations_per_s=round(R / med["generate_lnl"] * 1e3, 1),
               generate_correlated_lnl_realisations_per_s=round(R / med["generate_correlated_lnl"] * 1e3, 1),
               correlated_evaluations_per_s=round(R * G * st["n_orf"] / med["correlated_log_likelihood"] * 1e3, 1))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
