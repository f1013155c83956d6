"""Throughput of the per-realisation white noise (theta's wn_efac / wn_log10_equad / wn_log10_ecorr per backend group), headline
configuration (68 pulsars x 5000 TOAs, HD GWB + RN + EFAC/EQUAD + ECORR), R realisations, timed with HIP events in ONE process, every
comparison alternating step by step after a warm-up:

  generation   generate(R, theta=all three keys) against generate(R) and generate(R, theta=rn keys); the same with one key group alone
               (the other term stays fused); generate_sampled with every group sampled against generate(R)
  kernels      pta_engine_wn_add (accumulate = 1 and 0, through the C ABI on the engine's rows) against pta_engine_synth on a plan
               with only white noise + ECORR (the same draws, half the traffic: it writes and does not read) and against
               pta_engine_bwm_add (the same traffic, no draws); pta_engine_wn_params beside them

Every timing is the median with the [min, max] range of --reps repetitions.  Prints one JSON line; --out also writes it to a file
(after every section, so that a cut run keeps what it measured).

    timeout -k 10 600 python scripts/gpu_wn_hyper_throughput.py --out profiles/r20_wn_hyper_throughput.json
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
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--psrs", type=int, default=68)
    ap.add_argument("--toas", type=int, default=5000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    R = a.batch
    eng, _, _ = build_engine(a.psrs, a.toas, seed=1234)
    P, N = eng.P, eng.n_toa
    G_wn, G_ec = len(eng.wn_groups), len(eng.ecorr_groups)
    eng.set_hyper_prior(wn_efac=(0.5, 2.0), wn_log10_equad=(-8.0, -6.0), wn_log10_ecorr=(-8.0, -6.0))
    th_wn = eng.sample_theta(R)
    rng = np.random.default_rng(3)
    th_rn = {"rn_log10_A": dv.f64(rng.uniform(-15, -13, (R, P))), "rn_gamma": dv.f64(rng.uniform(1, 5, (R, P)))}
    res = dict(config=f"{P} x {a.toas}, HD GWB + RN + EFAC/EQUAD + ECORR; {G_wn} white-noise groups, {G_ec} ECORR groups, every label from "
                      "set_hyper_prior boxes", device=torch.cuda.get_device_name(0), batch=R, reps=a.reps, warmup=a.warmup, n_toa=N,
               generation={}, kernels={}, ratios={})

    def save():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write(json.dumps(res) + "\n")

    # ---- generation
    buf = dv.empty((R, N))
    only = lambda *keys: {k: th_wn[k] for k in keys}   # noqa: E731
    gen = alternate({"generate": lambda: eng.generate(R, out=buf),
                     "generate_theta_rn": lambda: eng.generate(R, out=buf, theta=th_rn),
                     "generate_theta_wn": lambda: eng.generate(R, out=buf, theta=th_wn),
                     "generate_theta_efac_equad": lambda: eng.generate(R, out=buf, theta=only("wn_efac", "wn_log10_equad")),
                     "generate_theta_ecorr": lambda: eng.generate(R, out=buf, theta=only("wn_log10_ecorr")),
                     "generate_sampled": lambda: eng.generate_sampled(R, out=buf)}, a.reps, a.warmup)
    res["generation"] = gen
    m = lambda k: gen[k]["median"]   # noqa: E731
    res["ratios"].update(theta_wn_over_generate=round(m("generate_theta_wn") / m("generate"), 3),
                         theta_wn_over_theta_rn=round(m("generate_theta_wn") / m("generate_theta_rn"), 3),
                         theta_wn_minus_generate_ms=round(m("generate_theta_wn") - m("generate"), 4),
                         sampled_over_generate=round(m("generate_sampled") / m("generate"), 3),
                         realisations_per_s=dict(generate=round(R / m("generate") * 1e3, 1), theta_wn=round(R / m("generate_theta_wn") * 1e3, 1),
                                                 sampled=round(R / m("generate_sampled") * 1e3, 1)))
    print(f"generation: {gen}", flush=True)
    save()

    # ---- the kernels alone
    s = dv.stream_ptr()
    eng.generate(R, out=buf, theta=th_wn)    # fills the workspace, builds the tables
    wdev = eng._wn_theta_device(th_wn, R)
    w = eng._wn_struct(wdev, 0, R)
    _lib.call("pta_engine_wn_params", ctypes.byref(w), R, s)
    w_wn, w_ec = eng._wn_struct(wdev, 0, R, ecorr=False), eng._wn_struct(wdev, 0, R, wn=False)
    white = _lib.EnginePlan.from_buffer_copy(eng.plan)     # the fused kernel with only white noise + ECORR: the same draws
    white.rn_k = white.gw_npts = 0
    white.det = None
    coef, t0 = torch.randn((R, P), dtype=torch.float64, device="cuda") * 1e-15, dv.f64(np.full(R, 55000.0 * 86400.0))
    b = _lib.BwmEngine()
    b.n_psr, b.toa_s, b.coef, b.t0_s = P, eng.d_toa_s.data_ptr(), coef.data_ptr(), t0.data_ptr()
    add = lambda ww, acc: _lib.call("pta_engine_wn_add", ctypes.byref(eng.plan), ctypes.byref(ww), eng.seed, 0, R, dv.ptr(buf), N, acc, s)   # noqa: E731
    k = alternate({"wn_add_accumulate": lambda: add(w, 1), "wn_add_write": lambda: add(w, 0),
                   "wn_add_efac_equad_only": lambda: add(w_wn, 1), "wn_add_ecorr_only": lambda: add(w_ec, 1),
                   "synth_white_only": lambda: _lib.call("pta_engine_synth", ctypes.byref(white), eng.seed, 0, R, dv.ptr(buf), N, s),
                   "bwm_add_accumulate": lambda: _lib.call("pta_engine_bwm_add", ctypes.byref(eng.plan), ctypes.byref(b), R, dv.ptr(buf), N, 1, s),
                   "wn_params": lambda: _lib.call("pta_engine_wn_params", ctypes.byref(w), R, s)}, a.reps, a.warmup)
    for name, nbytes in (("wn_add_accumulate", 16.0), ("wn_add_write", 8.0), ("synth_white_only", 8.0), ("bwm_add_accumulate", 16.0)):
        k[name].update(GB_moved=round(nbytes * R * N / 1e9, 3), TB_per_s=round(nbytes * R * N / (k[name]["median"] * 1e-3) / 1e12, 3))
    res["kernels"] = k
    km = lambda name: k[name]["median"]   # noqa: E731
    res["ratios"].update(wn_add_over_synth_white_only=round(km("wn_add_accumulate") / km("synth_white_only"), 3),
                         wn_add_over_bwm_add=round(km("wn_add_accumulate") / km("bwm_add_accumulate"), 3),
                         wn_add_over_sum_of_both=round(km("wn_add_accumulate") / (km("synth_white_only") + km("bwm_add_accumulate")), 3))
    print(f"kernels: {k}", flush=True)
    save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
