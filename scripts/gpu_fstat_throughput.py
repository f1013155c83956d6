"""Throughput of the continuous-wave F-statistics, headline configuration (68 pulsars x 5000 TOAs, HD GWB + RN + EFAC/EQUAD + ECORR),
R realisations, J frequencies, S sky points, timed with HIP events in ONE process:

  per kernel, for J in --freqs, S in --sky   pta_fstat_project, pta_fstat_fp, pta_fstat_fe (full map and sky_max) on one batch of residuals
  projection baselines (same operands)       (a) pta_os_project looped over 64-column slices, (b) one batched pta_dgemm (algo 2) over
                                             the 68 equal-length pulsars
  ragged array (bench_extras.ragged_counts)  pta_fstat_project against (a) and against P separate pta_dgemm launches
  generate_f_statistic                       against eng.generate(R, theta=theta), alternating step by step after a warm-up

The kernels are timed through the C ABI on operands of the headline shapes: the residuals are the engine's, W, G^-1, phi and M^-1 are
random (no kernel's time depends on their values); the engine section goes through prepare_f_statistic / generate_f_statistic alone.

Every timing is the median and the minimum of --reps repetitions after --warmup.  pta_fstat_project is quoted in TFLOP/s of useful
work (2 R 2J sum N_a) and of the work the matrix cores execute (rows and columns padded to the tile, every pulsar's TOAs to 16),
next to the fp64 MFMA rate pta_microbench kind 0 measures in the same process; pta_fstat_fe in TFLOP/s (8 R J S P useful; 2 ceil(P / 4) MFMAs
per 16 x 16 tile executed) and in bytes moved (Q once per 64-point sky tile, plus the map or the per-tile maxima).  Prints one JSON
line; --out also writes it to a file (after every section, so that a cut run keeps what it measured).

    timeout -k 10 1100 python scripts/gpu_fstat_throughput.py --out profiles/r11_fstat_throughput.json
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
from bench_extras import ragged_counts  # noqa: E402
from pta_replicator_amd import _lib, device as dv  # noqa: E402


def timed(fn, reps, warmup):
    """(median, min, max) ms of `reps` single launches of fn after `warmup`"""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return dict(median=round(float(np.median(out)), 4), min=round(min(out), 4), max=round(max(out), 4))


def project_fns(Wt, off, counts, rows, Q, R, C, n_toa, uniform):
    """the new kernel and the parent-commit baselines on the same operands -> {name: launcher}"""
    P = len(counts)
    s = dv.stream_ptr()
    Qs = dv.empty((R, P * 64))         # baseline (a) writes one 64-column slice at a time, [R, P, 64]
    fns = {"fstat_project": lambda: _lib.call("pta_fstat_project", dv.ptr(Wt), n_toa, C, dv.ptr(off), P, dv.ptr(rows), rows.stride(0), R, dv.ptr(Q), P * C, s)}

    def sliced():
        for c0 in range(0, C, 64):
            _lib.call("pta_os_project", ctypes.c_void_p(Wt.data_ptr() + 8 * c0 * n_toa), n_toa, min(64, C - c0), dv.ptr(off), P, dv.ptr(rows), rows.stride(0), R,
                      dv.ptr(Qs), P * 64, s)
    fns["os_project_sliced"] = sliced
    if uniform:
        n = int(counts[0])
        fns["dgemm_batched"] = lambda: _lib.call("pta_dgemm", 1, R, C, n, 1.0, dv.ptr(rows), rows.stride(0), 1, dv.ptr(Wt), n_toa, 0.0, dv.ptr(Q), P * C, 0, P,
                                                 n, n, C, 2, s)
    else:
        o = np.concatenate([[0], np.cumsum(counts)])

        def loop():
            for a in range(P):
                _lib.call("pta_dgemm", 1, R, C, int(counts[a]), 1.0, ctypes.c_void_p(rows.data_ptr() + 8 * int(o[a])), rows.stride(0), 1,
                          ctypes.c_void_p(Wt.data_ptr() + 8 * int(o[a])), n_toa, 0.0, ctypes.c_void_p(Q.data_ptr() + 8 * a * C), P * C, 0, 1, 0, 0, 0, 2, s)
        fns["dgemm_per_pulsar"] = loop
    return fns


def project_flops(R, C, counts):
    useful = 2.0 * R * C * float(np.sum(counts))
    ct = 64 if C > 32 else 32     # the tiles of a launch are multiples of 64 rows and of this many columns
    padded = 2.0 * (-(-R // 64) * 64) * (-(-C // ct) * ct) * float(np.sum(-(-np.asarray(counts) // 16) * 16))
    return useful, padded


def rate(entry, useful, padded, mfma):
    t = entry["fstat_project"]["median"] * 1e-3
    entry.update(GFLOP_useful=round(useful / 1e9, 1), GFLOP_padded=round(padded / 1e9, 1), TFLOPs_useful=round(useful / t / 1e12, 2),
                 TFLOPs_padded=round(padded / t / 1e12, 2), fraction_of_mfma_rate=round(padded / t / 1e12 / mfma, 3))


def faster(entry, base):
    """is fstat_project faster than `base` by more than either's spread between repetitions?"""
    new, old = entry["fstat_project"], entry[base]
    return bool(old["median"] - new["median"] > max(new["max"] - new["min"], old["max"] - old["min"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--freqs", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--sky", type=int, nargs="+", default=[0, 192, 768])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    R = a.batch
    eng, _, _ = build_engine(68, 5000, seed=1234)
    eng.workspace_bytes = 32 << 30          # one chunk of R realisations: rows, Q and the per-tile maxima
    P = eng.P
    mfma = ctypes.c_double(0.0)
    _lib.call("pta_microbench", 0, 1 << 30, 2000, 0, ctypes.byref(mfma))
    mfma = mfma.value
    eng.set_cw(psrTerm=False, evolve=False)
    eng.set_hyper_prior(gwb_log10_A=(-15.0, -14.0), gwb_gamma=(3.5, 5.0), rn_log10_A=(-15.5, -13.0), rn_gamma=(2.0, 6.0))
    eng.set_cw_prior(log10_mc=(8.5, 9.5), log10_fgw=(-8.5, -7.0), log10_h=(-15.0, -13.5))
    theta = eng.sample_theta(R)
    rows = dv.empty((R, eng.n_toa))
    eng.generate(R, out=rows, theta=theta)
    s = dv.stream_ptr()
    rng = np.random.default_rng(1)
    Smax = max(a.sky)
    sky_all = (rng.uniform(-1, 1, Smax), rng.uniform(0, 2 * np.pi, Smax)) if Smax else None
    res = dict(config="68 x 5000, HD GWB + RN(67) + EFAC/EQUAD + ECORR; F-statistic: spin model, GWB auto-term on 14 frequencies, log-spaced GW "
                      "frequencies 4 nHz .. 300 nHz, isotropic random sky grid", device=torch.cuda.get_device_name(0), batch=R, reps=a.reps,
               warmup=a.warmup, fp64_mfma_tflops=round(mfma, 2), uniform={}, ragged={}, engine={}, acceptance={})

    def save():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write(json.dumps(res) + "\n")

    def rand(*shape):
        return torch.randn(shape, dtype=torch.float64, device="cuda")
    ks = (P + 3) // 4
    off = dv.i32(eng.off)
    for J in a.freqs:
        C = 2 * J
        entry = res["uniform"][f"J{J}"] = {}
        Wt, Q, Ginv, fp = rand(C, eng.n_toa), dv.empty((R, P * C)), rand(P * J * 3), dv.empty((R, J))
        useful, padded = project_flops(R, C, eng.counts)
        pr = entry["project"] = {k: timed(f, a.reps, a.warmup) for k, f in project_fns(Wt, off, eng.counts, rows, Q, R, C, eng.n_toa, uniform=True).items()}
        rate(pr, useful, padded, mfma)
        entry["fp_ms"] = timed(lambda: _lib.call("pta_fstat_fp", dv.ptr(Q), P * C, P, J, R, dv.ptr(Ginv), dv.ptr(fp), J, s), a.reps, a.warmup)
        print(f"J={J}: projection {pr}", flush=True)
        for S in [x for x in a.sky if x]:
            ntile = int(_lib.lib.pta_fstat_fe_tiles(S))
            phi, Minv, fe = rand(P, S, 2), rand(J * S * 10), dv.empty((R, J * S))
            fe_max, fe_arg = dv.empty((R, J)), dv.empty((R, J), dtype=torch.int32)
            pv, pa = dv.empty((R * J * ntile,)), dv.empty((R * J * ntile,), dtype=torch.int32)
            full = lambda: _lib.call("pta_fstat_fe", dv.ptr(Q), P * C, P, J, R, dv.ptr(phi), S, dv.ptr(Minv), dv.ptr(fe), J * S, None, 0, None, 0,  # noqa: E731
                                     None, None, s)
            smax = lambda: _lib.call("pta_fstat_fe", dv.ptr(Q), P * C, P, J, R, dv.ptr(phi), S, dv.ptr(Minv), None, 0, dv.ptr(fe_max), J,  # noqa: E731
                                     dv.ptr(fe_arg), J, dv.ptr(pv), dv.ptr(pa), s)
            t_full, t_max = timed(full, a.reps, a.warmup), timed(smax, a.reps, a.warmup)
            useful = 8.0 * R * J * S * P
            executed = 2.0 * ks * 2048.0 * R * (-(-J // 8)) * (-(-S // 64)) * 4
            q_bytes = 8.0 * R * P * C * (-(-S // 64))
            entry[f"fe_S{S}"] = dict(full_ms=t_full, sky_max_ms=t_max, GFLOP_useful=round(useful / 1e9, 1), GFLOP_mfma=round(executed / 1e9, 1),
                                     full_TFLOPs_useful=round(useful / (t_full["median"] * 1e-3) / 1e12, 2),
                                     sky_max_TFLOPs_useful=round(useful / (t_max["median"] * 1e-3) / 1e12, 2),
                                     full_fraction_of_mfma_rate=round(executed / (t_full["median"] * 1e-3) / 1e12 / mfma, 3),
                                     sky_max_fraction_of_mfma_rate=round(executed / (t_max["median"] * 1e-3) / 1e12 / mfma, 3),
                                     full_GB_moved=round((q_bytes + 8.0 * R * J * S) / 1e9, 3),
                                     sky_max_GB_moved=round((q_bytes + 12.0 * R * J * ntile) / 1e9, 3))
            print(f"J={J} S={S}: Fe full {t_full}, sky_max {t_max}", flush=True)
            res["acceptance"][f"sky_max_not_slower_than_full_map_J{J}_S{S}"] = bool(t_max["median"] <= t_full["median"])
            del phi, Minv, fe, fe_max, fe_arg, pv, pa
        res["acceptance"][f"uniform_J{J}_not_slower_than_os_project_sliced"] = bool(pr["fstat_project"]["median"] <= pr["os_project_sliced"]["median"])
        res["acceptance"][f"uniform_J{J}_fstat_project_over_dgemm_batched"] = round(pr["fstat_project"]["median"] / pr["dgemm_batched"]["median"], 3)
        del Wt, Q, Ginv, fp
        torch.cuda.empty_cache()
        save()
    # the ragged array: an ng15-like spread of TOA counts (bench_extras.ragged_counts), random operands (timing only)
    del rows
    torch.cuda.empty_cache()
    counts = np.array(ragged_counts(42))
    n_toa = int(counts.sum())
    roff = dv.i32(np.concatenate([[0], np.cumsum(counts)]))
    rrows = rand(R, n_toa)
    res["ragged"]["counts"] = dict(P=len(counts), min=int(counts.min()), max=int(counts.max()), n_toa=n_toa)
    for J in a.freqs:
        C = 2 * J
        Wt, Q = rand(C, n_toa), dv.empty((R, len(counts) * C))
        useful, padded = project_flops(R, C, counts)
        entry = {k: timed(f, a.reps, a.warmup) for k, f in project_fns(Wt, roff, counts, rrows, Q, R, C, n_toa, uniform=False).items()}
        rate(entry, useful, padded, mfma)
        res["ragged"][f"J{J}"] = entry
        res["acceptance"][f"ragged_J{J}_faster_than_os_project_sliced"] = faster(entry, "os_project_sliced")
        res["acceptance"][f"ragged_J{J}_faster_than_dgemm_per_pulsar"] = faster(entry, "dgemm_per_pulsar")
        print(f"ragged J={J}: {entry}", flush=True)
        del Wt, Q
        torch.cuda.empty_cache()
        save()
    del rrows
    torch.cuda.empty_cache()
    # the engine's whole path against generate, alternating step by step
    buf = dv.empty((R, eng.n_toa))
    for J in a.freqs:
        freqs = np.geomspace(4e-9, 3e-7, J)
        for S in a.sky:
            eng.prepare_f_statistic(freqs, sky=None if S == 0 else (sky_all[0][:S], sky_all[1][:S]))
            runs = [lambda: eng.generate(R, out=buf, theta=theta), lambda: eng.generate_f_statistic(R, theta=theta, chunk=R)]
            if S:
                runs.append(lambda: eng.generate_f_statistic(R, theta=theta, chunk=R, sky_max=True))
            for _ in range(a.warmup):
                for f in runs:
                    f()
            torch.cuda.synchronize()
            times = [[] for _ in runs]
            for _ in range(a.reps):
                for t, f in zip(times, runs):
                    t.append(timed(f, 1, 0)["median"])
            med = [float(np.median(t)) for t in times]
            e = dict(generate_theta_ms=dict(median=round(med[0], 4), min=round(min(times[0]), 4)),
                     generate_f_statistic_ms=dict(median=round(med[1], 4), min=round(min(times[1]), 4)),
                     generate_theta_realisations_per_s=round(R / med[0] * 1e3, 1), generate_f_statistic_realisations_per_s=round(R / med[1] * 1e3, 1),
                     generate_f_statistic_over_generate=round(med[1] / med[0], 3))
            if S:
                e.update(generate_f_statistic_sky_max_ms=dict(median=round(med[2], 4), min=round(min(times[2]), 4)),
                         generate_f_statistic_sky_max_realisations_per_s=round(R / med[2] * 1e3, 1),
                         generate_f_statistic_sky_max_over_generate=round(med[2] / med[0], 3))
            res["engine"][f"J{J}_S{S}"] = e
            print(f"engine J={J} S={S}: {e}", flush=True)
            torch.cuda.empty_cache()
            save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
