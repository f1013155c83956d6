"""Throughput of the per-realisation sine-Gaussian wavelets, headline configuration (68 pulsars x 5000 TOAs, HD GWB + RN + EFAC/EQUAD +
ECORR), R realisations, timed with HIP events in ONE process, every comparison alternating step by step after a warm-up:

  kernels      pta_engine_burst_add at W = 1, 4, 16 wavelets (accumulate = 1, no wavelet skipped: every envelope is a normal number over
               the whole span), pta_engine_transient_add at V = 16 and the remove_quad pair (pta_engine_burst_quad + the add kernel's
               quad instance) at W = 4, each on the same rows beside two yardsticks of kernels the wavelets never touch:
               pta_engine_bwm_add (the same traffic and no arithmetic: the floor) and pta_engine_cw_catalog_add in monochromatic mode
               at S = W sources (one sin / cos per source and TOA; the wavelet adds one exp)
  generate     generate(R) against generate(R, theta = burst W = 4 + V = 16 transients) and generate_sampled with both priors

Every timing is the median with the [min, max] range of --reps repetitions.  Prints one JSON line; --out also writes it to a file
(after every section, so that a cut run keeps what it measured).

    timeout -k 10 900 python scripts/gpu_burst_throughput.py --out profiles/r28_burst_throughput.json
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
from gpu_bwm_throughput import alternate  # noqa: E402


def ratio(a, b):
    """median ratio a / b with the range [min a / max b, max a / min b]"""
    return dict(median=round(a["median"] / b["median"], 3), min=round(a["min"] / b["max"], 3), max=round(a["max"] / b["min"], 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--psrs", type=int, default=68)
    ap.add_argument("--toas", type=int, default=5000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    R = a.batch
    eng, _, _ = build_engine(a.psrs, a.toas, seed=1234)
    eng.workspace_bytes = 32 << 30          # one batch of R realisations
    P, N = eng.P, eng.n_toa
    first, last = min(m.min() for m in eng.mjd), max(m.max() for m in eng.mjd)
    res = dict(config=f"{P} x {a.toas}, HD GWB + RN + EFAC/EQUAD + ECORR; wavelets with t0 over the span, tau in [1.3e7, 1e8] s (no envelope "
                      "underflows: no wavelet is skipped), f in [3e-9, 1e-7] Hz",
               device=torch.cuda.get_device_name(0), batch=R, reps=a.reps, warmup=a.warmup, n_toa=N, kernels={}, generate={})

    def save():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write(json.dumps(res) + "\n")

    s = dv.stream_ptr()
    gen = torch.Generator(device="cuda").manual_seed(1)

    def uni(lo, hi, *shape):
        return lo + (hi - lo) * torch.rand(shape, dtype=torch.float64, device="cuda", generator=gen)

    def wavelet_rows(n, ncoef):
        tau = 10 ** uni(np.log10(1.3e7), 8.0, R, n)
        cols = [uni(first, last, R, n) * 86400.0, -0.5 / tau ** 2, 10 ** uni(np.log10(3e-9), -7.0, R, n)]
        return cols + [uni(-1e-7, 1e-7, R, n) for _ in range(ncoef)]

    buf = dv.empty((R, N))
    eng.generate(R, out=buf)
    # the floor: the ramp kernel on the same rows
    coef, t0 = uni(-1e-15, 1e-15, R, P), uni(first, last, R) * 86400.0
    bw = _lib.BwmEngine()
    bw.n_psr, bw.toa_s, bw.coef, bw.t0_s = P, eng.d_toa_s.data_ptr(), coef.data_ptr(), t0.data_ptr()
    bwm_add = lambda: _lib.call("pta_engine_bwm_add", ctypes.byref(eng.plan), ctypes.byref(bw), R, dv.ptr(buf), N, 1, s)   # noqa: E731
    eng.set_cw(psrTerm=False, evolve=False, phase_approx=False, tref=53000 * 86400.0)
    assert _cw.mode(eng._cw) == 2
    keep = []

    def catalog_add(S):
        """pta_engine_cw_catalog_add alone on the table one _cw_catalog_apply of S sources per realisation left in the engine's scratch"""
        eng.set_cw_prior(log10_mc=(8, 9.5), log10_fgw=(-8.7, -7.5), log10_h=(-15, -14), n_sources=S)
        cw = {k: v for k, v in eng.sample_theta(R).items() if k.startswith("cw_")}
        eng._cw_prior = None
        _, det = eng._theta_parts(cw, R)
        eng._cw_catalog_apply(det, R, buf)
        torch.cuda.synchronize()
        src, pdist, _ = eng._keep["cw"]
        par = eng._scratch_tabs["cwc_par"][0].clone()
        keep.append((src, pdist, par))
        c = _lib.CwCatalogEngine()
        c.n_psr, c.n_src, c.mode, c.psr_term, c.amp_is_h, c.has_pdist = P, S, 2, 0, 1, 0
        c.tref, c.phat, c.toa_s = eng._cw["tref"], eng._phat_device().data_ptr(), eng.d_toa_s.data_ptr()
        c.src, c.ld_src, c.pdist, c.ld_pdist, c.par = src.data_ptr(), src.stride(0), pdist.data_ptr(), 0, par.data_ptr()
        return lambda: _lib.call("pta_engine_cw_catalog_add", ctypes.byref(eng.plan), ctypes.byref(c), R, dv.ptr(buf), N, 1, s)

    def burst_add(W, quad=False):
        wav = torch.stack(wavelet_rows(W, 4), dim=2).contiguous()
        kk = uni(-1, 1, R, P, 2)
        b = _lib.BurstEngine()
        b.n_psr, b.n_wav, b.toa_s, b.wav, b.kk = P, W, eng.d_toa_s.data_ptr(), wav.data_ptr(), kk.data_ptr()
        keep.append((wav, kk))
        if quad:
            eng.set_burst(W, remove_quad=True)
            off, q = eng._burst_quad_tables()
            c = dv.empty((R, P, 3))
            keep.append(c)
            b.psr_off, b.quad_q, b.quad_c = off.data_ptr(), q.data_ptr(), c.data_ptr()
        return lambda: _lib.call("pta_engine_burst_add", ctypes.byref(eng.plan), ctypes.byref(b), R, dv.ptr(buf), N, 1, s)

    def transient_add(V):
        tab = torch.stack([torch.floor(uni(0, P, R, V)).clamp(max=P - 1)] + wavelet_rows(V, 2), dim=2).contiguous()
        t = _lib.TransientEngine()
        t.n_psr, t.n_wav, t.toa_s, t.tab = P, V, eng.d_toa_s.data_ptr(), tab.data_ptr()
        keep.append(tab)
        return lambda: _lib.call("pta_engine_transient_add", ctypes.byref(eng.plan), ctypes.byref(t), R, dv.ptr(buf), N, 1, s)

    for W in (1, 4, 16):
        fns = {"bwm_add": bwm_add, "cw_catalog_add_mono": catalog_add(W), "burst_add": burst_add(W)}
        if W == 4:
            fns["burst_quad_plus_add"] = burst_add(W, quad=True)
        if W == 16:
            fns["transient_add"] = transient_add(W)
        k = alternate(fns, a.reps, a.warmup)
        k["burst_over_bwm"] = ratio(k["burst_add"], k["bwm_add"])
        k["burst_over_catalog"] = ratio(k["burst_add"], k["cw_catalog_add_mono"])
        k["burst_ns_per_wavelet_toa"] = round(k["burst_add"]["median"] * 1e6 / (R * N * W), 5)
        k["catalog_ns_per_source_toa"] = round(k["cw_catalog_add_mono"]["median"] * 1e6 / (R * N * W), 5)
        if W == 4:
            k["quad_pair_over_burst"] = ratio(k["burst_quad_plus_add"], k["burst_add"])
        if W == 16:
            k["transient_over_bwm"] = ratio(k["transient_add"], k["bwm_add"])
            k["burst_exceeds_two_catalog_passes"] = bool(k["burst_add"]["median"] > 2 * k["cw_catalog_add_mono"]["median"])
        res["kernels"][f"W={W}"] = k
        print(f"W={W}: {k}", flush=True)
        save()
    keep.clear()
    torch.cuda.empty_cache()

    # ---- generate with and without the keys
    eng.set_burst(4).set_transients(16)
    span = last - first
    eng.set_burst_prior(t0_mjd=(first, last), log10_tau=(np.log10(1.3e7), 8.0), log10_f=(-8.5, -7.0), log10_a_plus=(-8, -7), log10_a_cross=(-8, -7))
    eng.set_transient_prior(t0_mjd=(first + 0.05 * span, last - 0.05 * span), log10_tau=(6.0, 7.0), log10_f=(-8.0, -7.0), log10_a=(-7, -6))
    theta = eng.sample_theta(R)
    g = alternate({"generate": lambda: eng.generate(R, out=buf), "generate_theta": lambda: eng.generate(R, out=buf, theta=theta),
                   "generate_sampled": lambda: eng.generate_sampled(R, out=buf)}, a.reps, a.warmup)
    g["theta_over_plain"] = ratio(g["generate_theta"], g["generate"])
    g["sampled_over_theta"] = ratio(g["generate_sampled"], g["generate_theta"])
    g["theta_minus_plain_ms"] = round(g["generate_theta"]["median"] - g["generate"]["median"], 4)
    g["note"] = "burst W = 4 (tau >= 1.3e7 s, nothing skipped) + V = 16 transients (tau 1e6 .. 1e7 s: most tiles skip most transients)"
    res["generate"] = g
    print(f"generate: {g}", flush=True)
    save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
