"""Throughput of a catalogue of S CW sources per realisation, headline configuration (68 pulsars x 5000 TOAs), R = 1024 realisations
per batch, S in {1, 16, 128}, timed with HIP events in ONE process, for the four CW configurations of gpu_cw_throughput.py:

  catalogue  pta_engine_cw_catalog_params + pta_engine_cw_catalog_add, accumulating into out[R, n_toa]       (this path)
  baseline   S successive pta_engine_cw_params + pta_engine_cw_add launches on the columns of the SAME source table, accumulating into
             the same buffer (the single-source kernels: what S passes of the single-source path cost)

The two alternate step by step after the warm-up, so clock drift hits both alike; median of --steps with minimum .. maximum.  A gain is
claimed only where the two [min, max] ranges do not overlap.  Per cell also generate_sampled(R) with set_cw_prior(n_sources=S) against
generate(R) (realisations / s).  Prints one JSON line; --out also writes it.

    timeout -k 10 900 python scripts/gpu_cw_catalogue_throughput.py --out profiles/r12_cw_catalogue_throughput.json
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
    "evolve_earth_only": dict(evolve=True, phase_approx=False, psrTerm=False),
    "phase_approx_psrterm": dict(evolve=False, phase_approx=True, psrTerm=True),
    "monochromatic_psrterm": dict(evolve=False, phase_approx=False, psrTerm=True),
}


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ts):
    return dict(median=round(float(np.median(ts)), 4), min=round(float(np.min(ts)), 4), max=round(float(np.max(ts)), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--sources", default="1,16,128")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    R = a.batch
    eng, _, _ = build_engine(68, 5000, seed=1234)
    P = eng.P
    tref = float(min(m.min() for m in eng.mjd)) * 86400.0
    box = dict(log10_mc=(7.0, 10.0), log10_fgw=(-9.0, -7.0), log10_h=(-16.0, -13.0))
    out = dv.empty((R, eng.n_toa))
    s = dv.stream_ptr()
    optr = ctypes.c_void_p(out.data_ptr())
    res_modes = {}
    for name in a.modes.split(","):
        eng.set_cw(tref=tref, pdist=1.0, **MODES[name])
        mode = _cw.mode(eng._cw)
        cells = {}
        for S in (int(x) for x in a.sources.split(",")):
            eng.set_cw_prior(n_sources=S, **box)
            theta = eng.sample_theta(R)
            cw = _cw.check_theta(theta, R, P, eng._cw, check_values=False)
            eng.generate(R, out=out)
            eng._cw_apply(cw, R, out)                       # builds the tables of both paths' shared inputs
            src, _, _ = eng._keep["cw"]                     # [R, S, 8]
            tb = eng._cw_tables()
            c = _lib.CwCatalogEngine()
            c.n_psr, c.n_src, c.mode, c.psr_term, c.amp_is_h, c.has_pdist = P, S, mode, int(eng._cw["psrTerm"]), 1, 0
            c.tref, c.phat, c.pdist, c.toa_s = tref, tb["phat"].data_ptr(), tb["pdist"].data_ptr(), eng.d_toa_s.data_ptr()
            c.src, c.ld_src, c.par = src.data_ptr(), src.stride(0), eng._scratch("cwc_par", (1,)).data_ptr()
            par1 = dv.empty((R, P, _lib.CW_ENGINE_NPAR))
            b = _lib.CwEngine()
            b.n_psr, b.mode, b.psr_term, b.amp_is_h, b.has_pdist = P, mode, int(eng._cw["psrTerm"]), 1, 0
            b.tref, b.phat, b.pdist, b.toa_s = tref, tb["phat"].data_ptr(), tb["pdist"].data_ptr(), eng.d_toa_s.data_ptr()
            b.ld_src, b.par = src.stride(0), par1.data_ptr()

            def catalogue():
                _lib.call("pta_engine_cw_catalog_params", ctypes.byref(c), R, s)
                _lib.call("pta_engine_cw_catalog_add", ctypes.byref(eng.plan), ctypes.byref(c), R, optr, out.stride(0), 1, s)

            def baseline():
                for k in range(S):                          # column k of the same table: source k of every realisation
                    b.src = src.data_ptr() + 8 * _cw.N_SRC * k
                    _lib.call("pta_engine_cw_params", ctypes.byref(b), R, s)
                    _lib.call("pta_engine_cw_add", ctypes.byref(eng.plan), ctypes.byref(b), R, optr, out.stride(0), 1, s)
            for _ in range(a.warmup):
                catalogue()
                baseline()
            torch.cuda.synchronize()
            t_cat, t_base = [], []
            for _ in range(a.steps):
                t_cat.append(event_ms(catalogue))
                t_base.append(event_ms(baseline))
            # end to end: generate_sampled with the catalogue against the fixed-parameter generate, alternating
            for _ in range(a.warmup):
                eng.generate(R, out=out)
                eng.generate_sampled(R, out=out)
            torch.cuda.synchronize()
            t_fixed, t_sampled = [], []
            for _ in range(a.steps):
                t_fixed.append(event_ms(lambda: eng.generate(R, out=out)))
                t_sampled.append(event_ms(lambda: eng.generate_sampled(R, out=out)))
            sc, sb = stats(t_cat), stats(t_base)
            mf, ms = float(np.median(t_fixed)), float(np.median(t_sampled))
            cells[f"S={S}"] = dict(
                catalogue_ms=sc, baseline_ms=sb, catalogue_ms_per_source=round(sc["median"] / S, 4),
                baseline_ms_per_source=round(sb["median"] / S, 4), baseline_over_catalogue=round(sb["median"] / sc["median"], 4),
                ranges_overlap=bool(sc["min"] <= sb["max"] and sb["min"] <= sc["max"]),
                gain_claimed=bool(sc["max"] < sb["min"]), slower=bool(sc["min"] > sb["max"]),
                fixed_realisations_per_s=round(R / mf * 1e3, 1), sampled_realisations_per_s=round(R / ms * 1e3, 1),
                fixed_ms=stats(t_fixed), sampled_ms=stats(t_sampled))
            print(name, S, json.dumps(cells[f"S={S}"]), flush=True)
            del par1
        res_modes[name] = cells
    res = dict(
        config="68 x 5000, HD GWB + RN(67) + EFAC/EQUAD + ECORR at configured values, throughput mode; S CW sources per realisation from "
               "set_cw_prior(n_sources=S, log10_mc (7, 10), log10_fgw (-9, -7), log10_h (-16, -13), isotropic angles), tref = first TOA; "
               "catalogue = pta_engine_cw_catalog_params + _add, baseline = S x (pta_engine_cw_params + pta_engine_cw_add), both accumulating",
        device=torch.cuda.get_device_name(0), batch=R, steps=a.steps, warmup=a.warmup, timing="HIP events, median [min, max] of steps",
        modes=res_modes)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
