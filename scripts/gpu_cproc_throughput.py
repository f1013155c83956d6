"""The common-process term on the headline workload (68 x 5000, R = 1024, n_f = 14 and 30): ONE process, blocks alternating between the
things compared (the method of scripts/gpu_chrom_throughput.py), device events, median [min, max] per item.

    python scripts/gpu_cproc_throughput.py [--reps 15] [--steps 4] [--out profiles/r27_cproc_throughput.json]

Timed per n_f: pta_engine_cproc_add (harmonics by rotation in registers); pta_engine_bwm_add on the same rows (the same
read-modify-write traffic, no arithmetic to speak of) - the floor; pta_engine_chrom_add fed the same coef and a tabulated Ft of the
same 2 n_f columns - the existing kernel that could have done the job; pta_engine_cproc_coef; generate(R) with three processes
(monopole, dipole, CURN) and without them.  Counted from shapes: the algorithmic bytes 2 x 8 x N x R, the multiply-adds per element (2
n_f of the sums plus 4 n_f / (RG / 2) of the rotations), and which of the two bounds the kernel (peaks: 8 TB/s HBM, 78.6 TFLOP/s fp64).

The decision rule, fixed before the first number: the in-register basis is kept only if the [min, max] range of pta_engine_cproc_add
lies below that of pta_engine_chrom_add at both n_f."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NFS = (14, 30)
HBM_BYTES_PER_S, FP64_FLOPS = 8.0e12, 78.6e12


def summary(v):
    return {"median_ms": round(statistics.median(v), 5), "min_ms": round(min(v), 5), "max_ms": round(max(v), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--R", type=int, default=1024)
    ap.add_argument("--psrs", type=int, default=68)
    ap.add_argument("--toas", type=int, default=5000)
    ap.add_argument("--out")
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from pta_replicator_amd import _lib, device as dv
    from pta_replicator_amd import optimal_statistic as ost
    from pta_replicator_amd.engine import ReplicaEngine
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    R = args.R
    psrs, noise = bench.headline_array(args.psrs, args.toas)
    P = len(psrs)
    rng = np.random.default_rng(27)
    s = dv.stream_ptr()
    plain = bench.configure_engine(ReplicaEngine(psrs, seed=20261021), noise)
    plain.td_warmup = False
    plain.prepare()
    N = plain.n_toa
    out, src = dv.empty((R, N)), dv.zeros((R, N))
    b = _lib.BwmEngine()
    bcoef, bt0 = dv.f64(rng.normal(0, 1e-15, (R, P))), dv.f64(rng.uniform(53000, 58478, R) * 86400.0)
    b.n_psr, b.toa_s, b.coef, b.t0_s = P, plain.d_toa_s.data_ptr(), bcoef.data_ptr(), bt0.data_ptr()
    items, keep, agree = {}, [], {}
    items["generate(R), without the processes"] = lambda i: plain.generate(R, r0=i * R, out=out)
    items["pta_engine_bwm_add"] = lambda i: _lib.call("pta_engine_bwm_add", ctypes.byref(plain.plan), ctypes.byref(b), R, out.data_ptr(),
                                                      out.stride(0), 1, s)
    items["device-to-device copy of the rows"] = lambda i: out.copy_(src)
    for nf in NFS:
        K = 2 * nf
        eng = bench.configure_engine(ReplicaEngine(psrs, seed=20261021), noise)
        eng.td_warmup = False
        for orf, lA, g in (("monopole", -13.8, 3.0), ("dipole", -13.9, 2.0), ("curn", -14.2, 13. / 3.)):
            eng.add_common_process(lA, g, orf=orf, components=nf)
        eng.prepare()
        t = eng._cproc_t
        c = eng._cproc_struct()
        coef = dv.empty((R, P, K))
        c.coef = coef.data_ptr()
        _lib.call("pta_engine_cproc_coef", ctypes.byref(c), eng.seed, 0, R, s)
        # the tabulated design matrix of the same columns for pta_engine_chrom_add: Ft [K, N], NumPy's float64 sin / cos
        Ft = dv.f64(np.ascontiguousarray(np.concatenate([ost.fourier_basis(x, nf, t["T"]) for x in eng._cproc_toas()]).T))
        ch = _lib.ChromEngine()
        ch.n_psr, ch.k, ch.Ft, ch.ldf, ch.coef = P, K, Ft.data_ptr(), N, coef.data_ptr()
        keep += [eng, coef, Ft, c, ch]
        # the two routes agree to what the two bases differ by (NumPy's float64 argument 2 pi f t at t ~ 4.6e9 s against frac(t / T))
        a0, a1 = dv.zeros((8, N)), dv.zeros((8, N))
        _lib.call("pta_engine_cproc_add", ctypes.byref(eng.plan), ctypes.byref(c), 8, a0.data_ptr(), N, 0, s)
        _lib.call("pta_engine_chrom_add", ctypes.byref(eng.plan), ctypes.byref(ch), 8, a1.data_ptr(), N, 0, s)
        agree[nf] = float((a0 - a1).abs().max() / a0.abs().max())
        items[f"pta_engine_cproc_add, n_f = {nf}"] = lambda i, eng=eng, c=c: _lib.call(
            "pta_engine_cproc_add", ctypes.byref(eng.plan), ctypes.byref(c), R, out.data_ptr(), out.stride(0), 1, s)
        items[f"pta_engine_chrom_add on a tabulated Ft, n_f = {nf}"] = lambda i, eng=eng, ch=ch: _lib.call(
            "pta_engine_chrom_add", ctypes.byref(eng.plan), ctypes.byref(ch), R, out.data_ptr(), out.stride(0), 1, s)
        items[f"pta_engine_cproc_coef, n_f = {nf}"] = lambda i, eng=eng, c=c: _lib.call("pta_engine_cproc_coef", ctypes.byref(c), eng.seed, i * R, R, s)
        items[f"generate(R), with three processes, n_f = {nf}"] = lambda i, eng=eng: eng.generate(R, r0=i * R, out=out)
    for fn in items.values():   # warm up every shape
        for i in range(2):
            fn(i)
    torch.cuda.synchronize()

    def block(fn, k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(args.steps):
            fn(k * args.steps + i)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.steps

    times = {k: [] for k in items}
    for rep in range(args.reps):
        for name, fn in items.items():
            times[name].append(block(fn, rep))
    res = {k: summary(v) for k, v in times.items()}
    counts, decision = {"rows_bytes": 2 * 8 * N * R, "rows_hbm_floor_ms": round(2 * 8 * N * R / HBM_BYTES_PER_S * 1e3, 4)}, {}
    half = _lib.CPROC_RG // 2
    for nf in NFS:
        fma = (2 * nf + 4 * nf / half) * N * R   # one per column of the sums, four per harmonic of the rotation shared by RG / 2 rows
        counts[f"n_f = {nf}"] = {"fp64_fma": int(fma), "fp64_vector_floor_ms": round(2 * fma / FP64_FLOPS * 1e3, 4),
                                 "chrom_add_matrix_floor_ms": round(2 * 2 * nf * N * R / FP64_FLOPS * 1e3, 4)}
        new, old, floor = res[f"pta_engine_cproc_add, n_f = {nf}"], res[f"pta_engine_chrom_add on a tabulated Ft, n_f = {nf}"], res["pta_engine_bwm_add"]
        decision[f"n_f = {nf}"] = {"cproc_add_range_ms": [new["min_ms"], new["max_ms"]], "chrom_add_range_ms": [old["min_ms"], old["max_ms"]],
                                   "cproc_range_below_chrom_range": bool(new["max_ms"] < old["min_ms"]),
                                   "cproc_add_over_bwm_add": round(new["median_ms"] / floor["median_ms"], 4),
                                   "chrom_add_over_bwm_add": round(old["median_ms"] / floor["median_ms"], 4),
                                   "generate_with_minus_without_ms": round(res[f"generate(R), with three processes, n_f = {nf}"]["median_ms"]
                                                                           - res["generate(R), without the processes"]["median_ms"], 5)}
    decision["keep_in_register_basis"] = all(d["cproc_range_below_chrom_range"] for d in decision.values())
    line = {"config": "%d x %d, R = %d, %d tiles, throughput mode, three processes (monopole, dipole, curn)" % (P, args.toas, R, int(plain.plan.n_tiles)),
            "device": torch.cuda.get_device_name(0), "blocks_per_item": args.reps, "launches_per_block": args.steps, "library_RG": _lib.CPROC_RG,
            "routes_agree_rel": agree, "times": res, "counts": counts, "decision": decision}
    txt = json.dumps(line, indent=1)
    if args.out:
        open(args.out, "w").write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
