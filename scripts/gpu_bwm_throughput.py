"""Throughput of the per-realisation burst with memory, headline configuration (68 pulsars x 5000 TOAs, HD GWB + RN + EFAC/EQUAD +
ECORR), R realisations, timed with HIP events in ONE process, every comparison alternating step by step after a warm-up:

  injection    generate(R, theta=bwm) against generate(R): the difference is pta_engine_bwm_params + pta_engine_bwm_add; the add kernel
               alone (through the C ABI on the engine's rows, accumulate = 1 and 0) with the bytes it moves, 16 R n_toa (8 with
               accumulate = 0), and the achieved TB/s; generate_sampled with all five labels drawn against generate(R, theta=bwm)
  statistic    pta_bwm_stat against pta_fstat_fe on operands of the same shape (J epochs / frequencies, S sky points; full map and
               sky_max), pta_fstat_project with J against 2 J operator rows
  engine       generate_bwm_statistic (full map and sky_max) against generate alone

The kernels are timed on operands of the headline shapes: the residuals are the engine's, W, phi and M^-1 are random (no kernel's
time depends on their values); the engine section goes through prepare_bwm_statistic / generate_bwm_statistic alone.  Every timing is
the median with the [min, max] range of --reps repetitions.  Prints one JSON line; --out also writes it to a file (after every
section, so that a cut run keeps what it measured).

    timeout -k 10 900 python scripts/gpu_bwm_throughput.py --out profiles/r18_bwm_throughput.json
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


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(fns, reps, warmup):
    """{name: dict(median, min, max) ms}: the launchers run in turn, `reps` rounds after `warmup` rounds"""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            times[k].append(once(f))
    return {k: dict(median=round(float(np.median(t)), 4), min=round(min(t), 4), max=round(max(t), 4)) for k, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--epochs", type=int, default=256)
    ap.add_argument("--sky", type=int, default=768)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--psrs", type=int, default=68)
    ap.add_argument("--toas", type=int, default=5000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    R, J, S = a.batch, a.epochs, a.sky
    eng, _, _ = build_engine(a.psrs, a.toas, seed=1234)
    eng.workspace_bytes = 32 << 30          # one chunk of R realisations: rows, Q and the per-tile maxima
    P, N = eng.P, eng.n_toa
    eng.set_bwm()
    first, last = max(m.min() for m in eng.mjd), min(m.max() for m in eng.mjd)
    eng.set_bwm_prior(log10_h=(-15.0, -13.5), t0_mjd=(first + 0.1 * (last - first), last - 0.1 * (last - first)))
    theta = eng.sample_theta(R)
    res = dict(config=f"{P} x {a.toas}, HD GWB + RN + EFAC/EQUAD + ECORR; burst with memory per realisation from set_bwm_prior; statistic: spin "
                      f"model, GWB auto-term on 14 frequencies, {J} epochs over the inner 80 % of the span, {S} random sky points",
               device=torch.cuda.get_device_name(0), batch=R, reps=a.reps, warmup=a.warmup, n_toa=N, injection={}, statistic={}, engine={},
               acceptance={})

    def save():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write(json.dumps(res) + "\n")

    # ---- injection
    buf = dv.empty((R, N))
    inj = alternate({"generate": lambda: eng.generate(R, out=buf), "generate_theta_bwm": lambda: eng.generate(R, out=buf, theta=theta),
                     "generate_sampled": lambda: eng.generate_sampled(R, out=buf)}, a.reps, a.warmup)
    inj["bwm_minus_plain_ms"] = round(inj["generate_theta_bwm"]["median"] - inj["generate"]["median"], 4)
    inj["sampled_over_theta"] = round(inj["generate_sampled"]["median"] / inj["generate_theta_bwm"]["median"], 4)
    coef, t0 = torch.randn((R, P), dtype=torch.float64, device="cuda") * 1e-15, dv.as_f64(theta["bwm_t0_mjd"]) * 86400.0
    b = _lib.BwmEngine()
    b.n_psr, b.toa_s, b.coef, b.t0_s = P, eng.d_toa_s.data_ptr(), coef.data_ptr(), t0.data_ptr()
    s = dv.stream_ptr()
    buf2 = dv.zeros((R, N))                 # a device-to-device copy of the same rows reads 8 and writes 8 bytes per element too
    add = alternate({"accumulate": lambda: _lib.call("pta_engine_bwm_add", ctypes.byref(eng.plan), ctypes.byref(b), R, dv.ptr(buf), N, 1, s),
                     "write": lambda: _lib.call("pta_engine_bwm_add", ctypes.byref(eng.plan), ctypes.byref(b), R, dv.ptr(buf), N, 0, s),
                     "device_copy_same_bytes": lambda: buf.copy_(buf2)}, a.reps, a.warmup)
    for k, nbytes in (("accumulate", 16.0 * R * N), ("write", 8.0 * R * N), ("device_copy_same_bytes", 16.0 * R * N)):
        add[k].update(GB_moved=round(nbytes / 1e9, 3), TB_per_s=round(nbytes / (add[k]["median"] * 1e-3) / 1e12, 3))
    inj["bwm_add_kernel"] = add
    res["injection"] = inj
    res["acceptance"]["bwm_add_accumulate_fraction_of_device_copy_rate"] = round(add["accumulate"]["TB_per_s"] / add["device_copy_same_bytes"]["TB_per_s"], 3)
    print(f"injection: {inj}", flush=True)
    del buf2
    save()

    # ---- statistic kernels on one batch of residuals
    def rand(*shape):
        return torch.randn(shape, dtype=torch.float64, device="cuda")
    eng.generate(R, out=buf, theta=theta)
    off = dv.i32(eng.off)
    C = J + (J & 1)
    ntile = int(_lib.lib.pta_fstat_fe_tiles(S))
    Wb, Wf = rand(C, N), rand(2 * J, N)
    Qb, Qf = dv.empty((R, P * C)), dv.empty((R, P * 2 * J))
    phi, Mb, Mf = rand(P, S, 2), rand(J * S * 3), rand(J * S * 10)
    fmap = dv.empty((R, J * S))
    amp = dv.empty((R, 2 * J * S))
    mx, arg = dv.empty((R, J)), dv.empty((R, J), dtype=torch.int32)
    pv, pa = dv.empty((R * J * ntile,)), dv.empty((R * J * ntile,), dtype=torch.int32)
    st = alternate({
        "project_bwm": lambda: _lib.call("pta_fstat_project", dv.ptr(Wb), N, C, dv.ptr(off), P, dv.ptr(buf), N, R, dv.ptr(Qb), P * C, s),
        "project_fstat": lambda: _lib.call("pta_fstat_project", dv.ptr(Wf), N, 2 * J, dv.ptr(off), P, dv.ptr(buf), N, R, dv.ptr(Qf), P * 2 * J, s),
        "bwm_stat_full": lambda: _lib.call("pta_bwm_stat", dv.ptr(Qb), P * C, P, C, J, R, dv.ptr(phi), S, dv.ptr(Mb), dv.ptr(fmap), J * S, None, 0, None, 0,
                                           None, 0, None, None, s),
        "bwm_stat_full_amp": lambda: _lib.call("pta_bwm_stat", dv.ptr(Qb), P * C, P, C, J, R, dv.ptr(phi), S, dv.ptr(Mb), dv.ptr(fmap), J * S, dv.ptr(amp),
                                               2 * J * S, None, 0, None, 0, None, None, s),
        "bwm_stat_sky_max": lambda: _lib.call("pta_bwm_stat", dv.ptr(Qb), P * C, P, C, J, R, dv.ptr(phi), S, dv.ptr(Mb), None, 0, None, 0, dv.ptr(mx), J,
                                              dv.ptr(arg), J, dv.ptr(pv), dv.ptr(pa), s),
        "fstat_fe_full": lambda: _lib.call("pta_fstat_fe", dv.ptr(Qf), P * 2 * J, P, J, R, dv.ptr(phi), S, dv.ptr(Mf), dv.ptr(fmap), J * S, None, 0, None, 0,
                                           None, None, s),
        "fstat_fe_sky_max": lambda: _lib.call("pta_fstat_fe", dv.ptr(Qf), P * 2 * J, P, J, R, dv.ptr(phi), S, dv.ptr(Mf), None, 0, dv.ptr(mx), J, dv.ptr(arg), J,
                                              dv.ptr(pv), dv.ptr(pa), s)}, a.reps, a.warmup)
    ks = (P + 3) // 4
    useful = 4.0 * R * J * S * P                                           # 2 chains x (multiply + add) per (r, j, s, a)
    executed = 2.0 * ks * 2048.0 * R * (-(-J // 16)) * (-(-S // 64)) * 4   # 2 MFMAs of 16 x 16 x 4 per step and 16 x 16 tile
    q_bytes = 8.0 * R * P * J * (-(-S // 64))                              # Q once per 64-point sky tile
    st.update(J=J, S=S, GFLOP_useful=round(useful / 1e9, 1), GFLOP_mfma=round(executed / 1e9, 1),
              full_GB_moved=round((q_bytes + 8.0 * R * J * S) / 1e9, 3), full_amp_GB_moved=round((q_bytes + 24.0 * R * J * S) / 1e9, 3),
              sky_max_GB_moved=round((q_bytes + 12.0 * R * J * ntile) / 1e9, 3),
              full_TFLOPs_useful=round(useful / (st["bwm_stat_full"]["median"] * 1e-3) / 1e12, 2),
              sky_max_TFLOPs_useful=round(useful / (st["bwm_stat_sky_max"]["median"] * 1e-3) / 1e12, 2),
              full_TB_per_s=round((q_bytes + 8.0 * R * J * S) / (st["bwm_stat_full"]["median"] * 1e-3) / 1e12, 3))
    res["statistic"] = st
    res["acceptance"]["bwm_stat_full_over_fstat_fe_full"] = round(st["bwm_stat_full"]["median"] / st["fstat_fe_full"]["median"], 3)
    res["acceptance"]["bwm_stat_sky_max_over_fstat_fe_sky_max"] = round(st["bwm_stat_sky_max"]["median"] / st["fstat_fe_sky_max"]["median"], 3)
    res["acceptance"]["bwm_stat_not_slower_than_fstat_fe"] = bool(st["bwm_stat_full"]["median"] <= st["fstat_fe_full"]["median"] and
                                                                  st["bwm_stat_sky_max"]["median"] <= st["fstat_fe_sky_max"]["median"])
    print(f"statistic: {st}", flush=True)
    del Wb, Wf, Qb, Qf, phi, Mb, Mf, fmap, amp, mx, arg, pv, pa
    torch.cuda.empty_cache()
    save()

    # ---- the engine's whole path against generate alone
    rng = np.random.default_rng(1)
    span = last - first
    eng.prepare_bwm_statistic(np.linspace(first + 0.1 * span, last - 0.1 * span, J), sky=(rng.uniform(-1, 1, S), rng.uniform(0, 2 * np.pi, S)))
    e = alternate({"generate": lambda: eng.generate(R, out=buf), "generate_theta_bwm": lambda: eng.generate(R, out=buf, theta=theta),
                   "generate_bwm_statistic": lambda: eng.generate_bwm_statistic(R, theta=theta, chunk=R),
                   "generate_bwm_statistic_sky_max": lambda: eng.generate_bwm_statistic(R, theta=theta, chunk=R, sky_max=True)}, a.reps, a.warmup)
    for k in ("generate_bwm_statistic", "generate_bwm_statistic_sky_max"):
        e[k + "_over_generate"] = round(e[k]["median"] / e["generate"]["median"], 3)
        e[k + "_realisations_per_s"] = round(R / e[k]["median"] * 1e3, 1)
    e["generate_realisations_per_s"] = round(R / e["generate"]["median"] * 1e3, 1)
    res["engine"] = e
    print(f"engine: {e}", flush=True)
    save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
