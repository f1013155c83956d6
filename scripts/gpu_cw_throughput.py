"""Throughput of one CW source per realisation against the fixed-parameter engine, headline configuration (68 pulsars x 5000 TOAs,
HD GWB + RN + EFAC/EQUAD + ECORR at their configured values), R realisations per batch, timed with HIP events in ONE process:

  fixed    eng.generate(R)                              (the bench.py headline path)
  sampled  eng.generate_sampled(R)                      (a CW source per realisation drawn on chip from set_cw_prior)

for each CW mode (evolve + pulsar term, phase_approx + pulsar term, monochromatic + pulsar term, evolve Earth term only).  The two
paths alternate step by step after a warm-up, so clock drift hits both alike.  The CW kernels are also timed on their own
(pta_cw_uniform, pta_engine_cw_params, pta_engine_cw_add writing its own buffer).  Prints one JSON line; --out also writes it.

    timeout -k 10 600 python scripts/gpu_cw_throughput.py --steps 10 --warmup 2 --out profiles/r08_cw_throughput.json
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
from pta_replicator_amd import _cw, _lib, device as dv  # noqa: E402

MODES = {
    "evolve_psrterm": dict(evolve=True, phase_approx=False, psrTerm=True),
    "phase_approx_psrterm": dict(evolve=False, phase_approx=True, psrTerm=True),
    "monochromatic_psrterm": dict(evolve=False, phase_approx=False, psrTerm=True),
    "evolve_earth_only": dict(evolve=True, phase_approx=False, psrTerm=False),
}


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
    ap.add_argument("--reps", type=int, default=10, help="launches per per-kernel timing")
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    R = a.batch
    eng, _, _ = build_engine(68, 5000, seed=1234)
    tref = float(min(m.min() for m in eng.mjd)) * 86400.0
    eng.set_cw_prior(log10_mc=(7.0, 10.0), log10_fgw=(-9.0, -7.0), log10_h=(-16.0, -13.0))
    out = dv.empty((R, eng.n_toa))
    s = dv.stream_ptr()
    res_modes = {}
    r0 = 0
    for name in a.modes.split(","):
        eng.set_cw(tref=tref, pdist=1.0, **MODES[name])
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
        # the CW kernels on their own (the source table of the last batch, a separate output buffer)
        _, theta = eng.generate_sampled(R, r0=r0, out=out)
        cw = _cw.check_theta({k: v for k, v in theta.items() if k in _cw.KEYS}, R, eng.P, eng._cw, check_values=False)
        buf = dv.empty((R, eng.n_toa))
        eng._cw_apply(cw, R, buf, accumulate=False)
        src, par, tb = eng._keep["cw"], eng._scratch("cw_par", (R, eng.P, _lib.CW_ENGINE_NPAR)), eng._cw_tables()
        c = _lib.CwEngine()
        c.n_psr, c.mode, c.psr_term, c.amp_is_h, c.has_pdist = eng.P, _cw.mode(eng._cw), int(eng._cw["psrTerm"]), 1, 0
        c.tref, c.phat, c.pdist, c.toa_s = tref, tb["phat"].data_ptr(), tb["pdist"].data_ptr(), eng.d_toa_s.data_ptr()
        c.src, c.ld_src, c.par = src.data_ptr(), src.stride(0), par.data_ptr()
        lo, hi = eng._boxes["cw"][1]
        kern = {
            "cw_uniform_ms": lambda: _lib.call("pta_cw_uniform", eng.seed, r0, R, lo.shape[0], dv.ptr(lo), dv.ptr(hi),
                                               ctypes.c_void_p(buf.data_ptr()), s),
            "cw_params_ms": lambda: _lib.call("pta_engine_cw_params", ctypes.byref(c), R, s),
            "cw_add_ms": lambda: _lib.call("pta_engine_cw_add", ctypes.byref(eng.plan), ctypes.byref(c), R, dv.ptr(buf), buf.stride(0), 0, s),
        }
        kernels = {}
        for k, fn in kern.items():
            fn()
            kernels[k] = round(event_ms(fn, a.reps), 4)
        torch.cuda.synchronize()
        mf, ms = float(np.median(t_fixed)), float(np.median(t_sampled))
        res_modes[name] = dict(
            fixed_ms_per_batch_median=round(mf, 4), sampled_ms_per_batch_median=round(ms, 4),
            fixed_realisations_per_s=round(R / mf * 1e3, 1), sampled_realisations_per_s=round(R / ms * 1e3, 1),
            sampled_over_fixed=round(mf / ms, 4), kernels_ms=kernels,
            cw_add_ns_per_element=round(kernels["cw_add_ms"] * 1e6 / (R * eng.n_toa), 5))
        print(name, json.dumps(res_modes[name]), flush=True)
    res = dict(
        config="68 x 5000, HD GWB + RN(67) + EFAC/EQUAD + ECORR at configured values, throughput mode, czt transform; one CW source per "
               "realisation from set_cw_prior(log10_mc (7, 10), log10_fgw (-9, -7), log10_h (-16, -13), isotropic angles), tref = first TOA",
        device=torch.cuda.get_device_name(0), batch=R, steps=a.steps, warmup=a.warmup, modes=res_modes)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
