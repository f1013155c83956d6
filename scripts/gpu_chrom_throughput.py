"""The chromatic term on the headline workload (68 x 5000, two radio bands, K_c = 60, R = 1024): ONE process, blocks alternating between
the things compared (the method of scripts/gpu_mix_stream_ab.py), device events, median [min, max] per item.

    python scripts/gpu_chrom_throughput.py --build-probes DIR          (where hipcc is; no GPU needed)
    python scripts/gpu_chrom_throughput.py [--probes DIR] [--reps 15] [--steps 4] [--out profiles/r24_chrom_throughput.json]

Timed: generate(R) with the process and without it; generate(R, theta) with the chromatic keys and without them; pta_engine_chrom_add at
PTA_CHROM_RG = 16, 32, 64 (probe builds of csrc/pta_chrom_kernels.hip alone, linked against the library: for this measurement only);
pta_engine_bwm_add on the same rows (the same read-modify-write traffic, no product) - the yardstick; a device-to-device copy of the
rows; pta_engine_chrom_coef against pta_engine_rn_coef.  Counted from shapes: the algorithmic bytes 2 x 8 x N x R plus the design-matrix
slab a realisation group reads, the flops 2 K_c N R, and which of the two bounds the kernel (peaks: 8 TB/s HBM, 78.6 TFLOP/s fp64 matrix)."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RGS = (16, 32, 64)
HBM_BYTES_PER_S, FP64_MATRIX_FLOPS = 8.0e12, 78.6e12


def build_probes(outdir):
    from pta_replicator_amd import build as b
    b.build()
    os.makedirs(outdir, exist_ok=True)
    pkg = os.path.join(ROOT, "pta_replicator_amd")
    for rg in RGS:
        obj = os.path.join(outdir, f"chrom_rg{rg}.o")
        subprocess.check_call([b.HIPCC] + b.FLAGS + [f"-DPTA_CHROM_RG={rg}", "-c", os.path.join(b.CSRC, "pta_chrom_kernels.hip"), "-o", obj])
        subprocess.check_call([b.HIPCC, f"--offload-arch={b.ARCH}", "-shared", "-fPIC", "-o", os.path.join(outdir, f"libpta_chrom_rg{rg}.so"), obj,
                               "-L" + pkg, "-l:libpta_replicator_amd.so", "-Wl,-rpath," + pkg])
        os.remove(obj)
        print("built", os.path.join(outdir, f"libpta_chrom_rg{rg}.so"))


def summary(v):
    return {"median_ms": round(statistics.median(v), 5), "min_ms": round(min(v), 5), "max_ms": round(max(v), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-probes")
    ap.add_argument("--probes")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--R", type=int, default=1024)
    ap.add_argument("--psrs", type=int, default=68)
    ap.add_argument("--toas", type=int, default=5000)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.build_probes:
        return build_probes(args.build_probes)
    import numpy as np
    import torch
    import bench
    from pta_replicator_amd import _lib, device as dv
    from pta_replicator_amd.engine import ReplicaEngine
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    R, Kc = args.R, 60
    psrs, noise = bench.headline_array(args.psrs, args.toas)
    rng = np.random.default_rng(24)
    for p in psrs:   # two radio bands
        p.toas.freqs_mhz = np.where(rng.integers(0, 2, len(p.toas.freqs_mhz)) == 1, 1440.0, 820.0)
    P = len(psrs)
    plain = bench.configure_engine(ReplicaEngine(psrs, seed=20261020), noise)
    chrom = bench.configure_engine(ReplicaEngine(psrs, seed=20261020), noise)
    chrom.set_chromatic_noise(list(np.linspace(-13.9, -13.1, P)), list(np.linspace(1.5, 4.0, P)), components=Kc // 2)
    for e in (plain, chrom):
        e.td_warmup = False
        e.prepare()
    N = chrom.n_toa
    out = dv.empty((R, N))
    th_rn = dict(rn_log10_A=rng.uniform(-15, -13, (R, P)), rn_gamma=rng.uniform(1, 5, (R, P)))
    th_ch = dict(th_rn, chrom_log10_A=rng.uniform(-14.5, -13, (R, P)), chrom_gamma=rng.uniform(1, 5, (R, P)))
    th_rn = {k: dv.f64(v) for k, v in th_rn.items()}
    th_ch = {k: dv.f64(v) for k, v in th_ch.items()}
    s = dv.stream_ptr()
    # the structs of the launches timed alone, on the engine's own tables
    t = chrom._chrom_t
    coef = dv.empty((R, P, Kc))
    c = _lib.ChromEngine()
    c.n_psr, c.k, c.rng_fast, c.Ft, c.ldf, c.amp, c.coef = P, Kc, 0, t["Ft"].data_ptr(), N, t["amp"].data_ptr(), coef.data_ptr()
    _lib.call("pta_engine_chrom_coef", ctypes.byref(c), chrom.seed, 0, R, s)
    rn_coef = dv.empty((R, P, chrom.K))
    b = _lib.BwmEngine()
    bcoef, bt0 = dv.f64(rng.normal(0, 1e-15, (R, P))), dv.f64(rng.uniform(53000, 58478, R) * 86400.0)
    b.n_psr, b.toa_s, b.coef, b.t0_s = P, chrom.d_toa_s.data_ptr(), bcoef.data_ptr(), bt0.data_ptr()
    src = torch.zeros_like(out)
    probes = {}
    for rg in RGS:
        path = os.path.join(args.probes, f"libpta_chrom_rg{rg}.so") if args.probes else None
        if path and os.path.exists(path):
            fn = ctypes.CDLL(path).pta_engine_chrom_add
            fn.restype, fn.argtypes = _lib.lib.pta_engine_chrom_add.restype, _lib.lib.pta_engine_chrom_add.argtypes
            probes[rg] = fn

    def probe(fn):
        _lib.check(fn(ctypes.byref(chrom.plan), ctypes.byref(c), R, out.data_ptr(), out.stride(0), 1, s), "pta_engine_chrom_add (probe)")

    items = {
        "generate(R), with the process": lambda i: chrom.generate(R, r0=i * R, out=out),
        "generate(R), without it": lambda i: plain.generate(R, r0=i * R, out=out),
        "generate(R, theta), rn_* and chrom_* keys": lambda i: chrom.generate(R, r0=i * R, out=out, theta=th_ch),
        "generate(R, theta), rn_* keys alone": lambda i: chrom.generate(R, r0=i * R, out=out, theta=th_rn),
        "pta_engine_chrom_add (library, RG = %d)" % _lib.CHROM_RG:
            lambda i: _lib.call("pta_engine_chrom_add", ctypes.byref(chrom.plan), ctypes.byref(c), R, out.data_ptr(), out.stride(0), 1, s),
        "pta_engine_bwm_add": lambda i: _lib.call("pta_engine_bwm_add", ctypes.byref(chrom.plan), ctypes.byref(b), R, out.data_ptr(), out.stride(0), 1, s),
        "device-to-device copy of the rows": lambda i: out.copy_(src),
        "pta_engine_chrom_coef": lambda i: _lib.call("pta_engine_chrom_coef", ctypes.byref(c), chrom.seed, i * R, R, s),
        "pta_engine_rn_coef": lambda i: _lib.call("pta_engine_rn_coef", chrom.seed, i * R, R, P, chrom.K, dv.ptr(chrom.d_amp), dv.ptr(rn_coef), 0, s),
    }
    for rg, fn in probes.items():
        items["pta_engine_chrom_add (probe, RG = %d)" % rg] = lambda i, fn=fn: probe(fn)
    # the probes compute what the library computes
    ref = torch.zeros_like(out)
    _lib.call("pta_engine_chrom_add", ctypes.byref(chrom.plan), ctypes.byref(c), R, ref.data_ptr(), ref.stride(0), 0, s)
    same = {}
    for rg, fn in probes.items():
        out.zero_()
        probe(fn)
        same[rg] = bool(torch.equal(out, ref))
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
    med = lambda k: res[k]["median_ms"]   # noqa: E731
    n_tiles = int(chrom.plan.n_tiles)
    counts = {"rows_bytes": 2 * 8 * N * R, "flops": 2 * Kc * N * R}
    floor = {}
    for rg in RGS:
        by = counts["rows_bytes"] + 8 * Kc * N * ((R + rg - 1) // rg)   # every realisation group reads its tile's design-matrix slab (L2 or HBM)
        floor[rg] = {"bytes_with_design_matrix": by, "hbm_ms": round(by / HBM_BYTES_PER_S * 1e3, 4)}
    counts["matrix_core_floor_ms"] = round(counts["flops"] / FP64_MATRIX_FLOPS * 1e3, 4)
    counts["rows_hbm_floor_ms"] = round(counts["rows_bytes"] / HBM_BYTES_PER_S * 1e3, 4)
    counts["bound"] = "HBM (read-modify-write of the rows)" if counts["rows_hbm_floor_ms"] > counts["matrix_core_floor_ms"] else "fp64 matrix cores"
    lib_key = "pta_engine_chrom_add (library, RG = %d)" % _lib.CHROM_RG
    ratio = {"chrom_add_over_bwm_add": round(med(lib_key) / med("pta_engine_bwm_add"), 4),
             "range": [round(res[lib_key]["min_ms"] / res["pta_engine_bwm_add"]["max_ms"], 4), round(res[lib_key]["max_ms"] / res["pta_engine_bwm_add"]["min_ms"], 4)],
             "chrom_add_minus_bwm_add_minus_matrix_floor_ms": round(med(lib_key) - med("pta_engine_bwm_add") - counts["matrix_core_floor_ms"], 5),
             "generate_with_over_without": round(med("generate(R), with the process") / med("generate(R), without it"), 4),
             "chrom_coef_over_rn_coef": round(med("pta_engine_chrom_coef") / med("pta_engine_rn_coef"), 4)}
    line = {"config": "%d x %d, two bands, K_c = %d, R = %d, %d tiles, throughput mode" % (P, args.toas, Kc, R, n_tiles),
            "device": torch.cuda.get_device_name(0), "blocks_per_item": args.reps, "launches_per_block": args.steps, "library_RG": _lib.CHROM_RG,
            "probe_equals_library": same, "times": res, "counts": counts, "per_RG": floor, "ratios": ratio}
    txt = json.dumps(line, indent=1)
    if args.out:
        open(args.out, "w").write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
