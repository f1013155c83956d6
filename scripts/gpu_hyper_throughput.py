"""Throughput of per-realisation hyperparameters against the fixed-parameter engine, headline configuration (68 pulsars x 5000
TOAs, HD GWB + RN + EFAC/EQUAD + ECORR), R realisations per batch, timed with HIP events in ONE process:

  fixed    eng.generate(R)                              (the bench.py headline path)
  sampled  eng.generate_sampled(R)                      (theta drawn on chip: GWB log10_A, gamma and all 68 RN log10_A, gamma)

The two modes alternate step by step after a warm-up, so clock drift hits both alike.  The new stages are also timed on their own
(pta_gwb_spectrum_scale, pta_gwb_czt_scaled, pta_engine_rn_coef_hyper) beside their fixed-parameter counterparts.  Prints one
JSON line; --out also writes it to a file.

    timeout -k 10 300 python scripts/gpu_hyper_throughput.py --steps 20 --warmup 3 --out profiles/r07_hyper_throughput.json
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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20, help="launches per per-kernel timing")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    R = a.batch
    eng, _, _ = build_engine(68, 5000, seed=1234)
    eng.set_hyper_prior(gwb_log10_A=(-15.0, -14.0), gwb_gamma=(3.0, 5.0), rn_log10_A=(-15.0, -13.0), rn_gamma=(1.0, 5.0))
    out = dv.empty((R, eng.n_toa))
    r0 = 0
    for _ in range(a.warmup):
        eng.generate(R, r0=r0, out=out)
        eng.generate_sampled(R, r0=r0, out=out)
        r0 += R
    torch.cuda.synchronize()
    t_fixed, t_sampled = [], []
    for _ in range(a.steps):
        t_fixed.append(event_ms(lambda: eng.generate(R, r0=r0, out=out)))
        t_sampled.append(event_ms(lambda: eng.generate_sampled(R, r0=r0, out=out)))
        r0 += R

    # the new stages on their own, beside their fixed-parameter counterparts (same batch, same workspace)
    s = dv.stream_ptr()
    _, theta = eng.generate_sampled(R, r0=r0, out=out)
    ws, hy, tb, pl = eng._ws, eng._hyper_tables(), eng._ws["tables"], eng.plan
    Nf, gw = eng.grid["Nf"], eng._gw
    assert tb.use_czt
    czt_args = (tb.czt_pre, tb.czt_FB, tb.czt_tw, tb.czt_post, tb.ws_G0, pl.gw_npts, tb.czt_variant, pl.rng_fast)
    kern = {
        "gwb_spectrum_scale_ms": lambda: _lib.call(
            "pta_gwb_spectrum_scale", dv.ptr(hy["gw_f"]), dv.ptr(hy["gw_hcf0"]), Nf, R, dv.ptr(theta["gwb_log10_A"]),
            dv.ptr(theta["gwb_gamma"]), int(bool(gw["turnover"])), float(gw["f0"]), float(gw["beta"]), float(gw["power"]),
            dv.ptr(ws["scale"]), Nf, s),
        "gwb_czt_scaled_ms": lambda: _lib.call(
            "pta_gwb_czt_scaled", eng.seed, r0, None, 0, R, eng.P, Nf, pl.gw_npts, tb.gw_i0, *czt_args, dv.ptr(ws["scale"]), Nf, s),
        "gwb_czt_fixed_ms": lambda: _lib.call("pta_gwb_czt", eng.seed, r0, None, 0, R, eng.P, Nf, pl.gw_npts, tb.gw_i0, *czt_args, s),
        "rn_coef_hyper_ms": lambda: _lib.call(
            "pta_engine_rn_coef_hyper", eng.seed, r0, R, eng.P, eng.K, dv.ptr(hy["rn_f"]), dv.ptr(hy["rn_tspan"]),
            dv.ptr(theta["rn_log10_A"]), dv.ptr(theta["rn_gamma"]), dv.ptr(eng.d_amp), dv.ptr(ws["coef"]), int(eng.rng_fast), s),
        "rn_coef_fixed_ms": lambda: _lib.call("pta_engine_rn_coef", eng.seed, r0, R, eng.P, eng.K, dv.ptr(eng.d_amp), dv.ptr(ws["coef"]),
                                              int(eng.rng_fast), s),
        "hyper_uniform_ms": lambda: _lib.call("pta_hyper_uniform", eng.seed, r0, R, 2 + 2 * eng.P, dv.ptr(eng._boxes["hyper"][1][0]),
                                              dv.ptr(eng._boxes["hyper"][1][1]), ctypes.c_void_p(ws["G0"].data_ptr()), s),
    }
    kernels = {}
    for name, fn in kern.items():
        fn()
        kernels[name] = round(event_ms(fn, a.reps), 4)
    torch.cuda.synchronize()

    mf, ms = float(np.median(t_fixed)), float(np.median(t_sampled))
    res = dict(
        config="68 x 5000, HD GWB + RN(67) + EFAC/EQUAD + ECORR, throughput mode, czt transform",
        device=torch.cuda.get_device_name(0), batch=R, steps=a.steps, warmup=a.warmup,
        fixed_ms_per_batch_median=round(mf, 4), sampled_ms_per_batch_median=round(ms, 4),
        fixed_ms_min=round(min(t_fixed), 4), sampled_ms_min=round(min(t_sampled), 4),
        fixed_realisations_per_s=round(R / mf * 1e3, 1), sampled_realisations_per_s=round(R / ms * 1e3, 1),
        sampled_over_fixed=round(mf / ms, 4), sampled_params="gwb_log10_A, gwb_gamma, rn_log10_A x 68, rn_gamma x 68",
        kernels_ms=kernels,
    )
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
