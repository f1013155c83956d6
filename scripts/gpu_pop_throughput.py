"""The population path on the headline workload (68 x 5000, R = 1024, F = 40 bins of 10^5 cells, log-uniform expected counts over
[1e-6, 1e8], 10 loudest per bin): ONE process, blocks alternating between the things compared (the method of
scripts/gpu_mix_stream_ab.py), device events, median [min, max] per item.

    python scripts/gpu_pop_throughput.py [--reps 5] [--R 1024] [--cells 100000] [--out profiles/r26_pop_throughput.json]

Timed: population_theta(R) and its two kernels alone; generate_sampled(R) with the population against generate(R, theta) with the same
labels precomputed; the Philox + Box-Muller microbenchmark of the same process (the yardstick of the draw rate); and what the feature
replaces, NumPy's rng.poisson + split_population for ONE realisation of the same population on this machine's host.  Counted from the
shapes: the table bytes pta_pop_draw_select reads per call and the bandwidth the measured time implies."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12


def summary(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def population(F, cells, T_obs, seed=26):
    """a synthetic population in the layout of the reference's inputs: vals [4, B] (Mtot [g], q, z, f_obs [Hz]), number [B], fobs [F + 1]"""
    import numpy as np
    rng = np.random.default_rng(seed)
    fobs = np.arange(1, F + 2) / T_obs
    B = F * cells
    fo = (fobs[:-1, None] + rng.uniform(0.001, 0.999, (F, cells)) * np.diff(fobs)[:, None]).ravel()
    perm = rng.permutation(B)
    vals = np.array([10 ** rng.uniform(8.5, 10.3, B) * 1.988409870698051e33, rng.uniform(0.1, 1.0, B), rng.uniform(0.02, 2.0, B), fo[perm]])
    return vals, 10 ** rng.uniform(-6.0, 8.0, B), fobs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--R", type=int, default=1024)
    ap.add_argument("--bins", type=int, default=40)
    ap.add_argument("--cells", type=int, default=100000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--psrs", type=int, default=68)
    ap.add_argument("--toas", type=int, default=5000)
    ap.add_argument("--out")
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from pta_replicator_amd import _lib, _pop, _population, device as dv
    from pta_replicator_amd.deterministic import split_population
    from pta_replicator_amd.engine import ReplicaEngine
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    R, F, k = args.R, args.bins, args.k
    T_obs = (58478.0 - 53000.0) * 86400.0
    vals, number, fobs = population(F, args.cells, T_obs)
    fc = _population.f_centers(fobs)
    psrs, noise = bench.headline_array(args.psrs, args.toas)
    eng = bench.configure_engine(ReplicaEngine(psrs, seed=20261021), noise)
    eng.set_gwb(None, None, userSpec=np.array([fc, 1e-15 * (fc / fc[0]) ** (-2.0 / 3.0)]).T)
    eng.set_cw(psrTerm=True, evolve=True, phase_approx=False, tref=53000 * 86400.0, pdist=1.0)
    t0 = time.perf_counter()
    eng.set_population(vals, number, fobs, T_obs, outlier_per_bin=k)
    t_tables = time.perf_counter() - t0
    eng.td_warmup = False
    eng.prepare()
    out = dv.empty((R, eng.n_toa))
    labels = eng.population_theta(R)
    s = dv.stream_ptr()
    d = eng._popd
    S = F * k
    sel_number, sel_w, sel_cell = dv.empty((R * S,)), dv.empty((R * S,)), dv.empty((R * S,), dtype=torch.int32)
    sel_count, free_spec = dv.empty((R, F), dtype=torch.int32), dv.empty((R, F))
    th = {key: torch.empty_like(labels[key]) for key in ("cw_log10_mc", "cw_log10_fgw", "cw_log10_dist", "pop_number", "pop_cell", "cw_count", "gwb_log10_hc")}

    def draw_select(i):
        _lib.call("pta_pop_draw_select", ctypes.byref(d["plan"]), eng.seed, i * R, R, None, 0, None, 0, dv.ptr(sel_cell), dv.ptr(sel_number), dv.ptr(sel_w),
                  dv.ptr(sel_count), dv.ptr(free_spec), s)

    def theta_kernel(i):
        _lib.call("pta_pop_theta", ctypes.byref(d["plan"]), R, dv.ptr(sel_cell), dv.ptr(sel_number), dv.ptr(sel_count), dv.ptr(free_spec),
                  dv.ptr(th["cw_log10_mc"]), dv.ptr(th["cw_log10_fgw"]), dv.ptr(th["cw_log10_dist"]), dv.ptr(th["pop_number"]), dv.ptr(th["pop_cell"]),
                  dv.ptr(th["cw_count"]), dv.ptr(th["gwb_log10_hc"]), F, s)

    items = {
        "population_theta(R)": lambda i: eng.population_theta(R, r0=i * R),
        "pta_pop_draw_select": draw_select,
        "pta_pop_theta": theta_kernel,
        "generate_sampled(R), with the population": lambda i: eng.generate_sampled(R, r0=i * R, out=out),
        "generate(R, theta), the same labels precomputed": lambda i: eng.generate(R, r0=i * R, out=out, theta=labels),
    }
    for fn in items.values():   # warm up every shape
        fn(0)
    torch.cuda.synchronize()

    def block(fn, i):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(i)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    times = {name: [] for name in items}
    for rep in range(args.reps):
        for name, fn in items.items():
            times[name].append(block(fn, rep + 1))
    res = {name: summary(v) for name, v in times.items()}
    micro = ctypes.c_double(0.0)
    _lib.call("pta_microbench", 4, 1 << 30, 200, 0, ctypes.byref(micro))   # Philox + Box-Muller, T normals / s (two per Philox block)
    # the host path of one realisation: the counts, then the reference's bookkeeping
    rng = np.random.default_rng(1)
    t0 = time.perf_counter()
    weights = rng.poisson(number).astype(np.float64)
    t_poisson = time.perf_counter() - t0
    t0 = time.perf_counter()
    split_population(vals, weights, fobs, T_obs, outlier_per_bin=k)
    t_split = time.perf_counter() - t0
    n_sorted = len(d["orig"])
    draws = R * int(np.count_nonzero(number[eng._pop["orig"]] > 0))
    t_draw = res["pta_pop_draw_select"]["median_ms"] * 1e-3
    table_bytes = R * n_sorted * (3 * 8 + 4)
    reg = np.bincount(_pop.regime(number), minlength=4)
    line = {"config": "%d x %d, R = %d, F = %d, %d cells per bin, number log-uniform over [1e-6, 1e8], k = %d" % (len(psrs), args.toas, R, F, args.cells, k),
            "device": torch.cuda.get_device_name(0), "blocks_per_item": args.reps, "launches_per_block": 1, "times": res,
            "cells_by_regime (none, inversion, PTRS, normal)": [int(x) for x in reg],
            "poisson_draws_per_call": draws,
            "poisson_G_draws_per_s": {"median": round(draws / t_draw * 1e-9, 3),
                                      "range": [round(draws / (res["pta_pop_draw_select"]["max_ms"] * 1e-3) * 1e-9, 3),
                                                round(draws / (res["pta_pop_draw_select"]["min_ms"] * 1e-3) * 1e-9, 3)]},
            "microbench_philox_box_muller_G_blocks_per_s": round(micro.value * 1e3 / 2, 3),
            "draw_select_table_bytes_per_call": table_bytes,
            "draw_select_table_TB_per_s_implied": round(table_bytes / t_draw * 1e-12, 3),
            "draw_select_hbm_floor_ms_if_every_row_came_from_hbm": round(table_bytes / HBM_BYTES_PER_S * 1e3, 3),
            "table_bytes_of_one_realisation": n_sorted * 28,
            "realisations_per_s": {"population_theta": round(R / (res["population_theta(R)"]["median_ms"] * 1e-3), 1),
                                   "generate_sampled": round(R / (res["generate_sampled(R), with the population"]["median_ms"] * 1e-3), 1),
                                   "generate_theta": round(R / (res["generate(R, theta), the same labels precomputed"]["median_ms"] * 1e-3), 1)},
            "host_one_realisation_s": {"rng.poisson": round(t_poisson, 3), "split_population": round(t_split, 3),
                                       "set_population tables (once)": round(t_tables, 3)},
            "host_over_device_per_realisation": round((t_poisson + t_split) / (res["population_theta(R)"]["median_ms"] * 1e-3 / R), 1)}
    txt = json.dumps(line, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
