"""Throughput of the per-frequency optimal statistic against the broadband one, headline configuration (68 pulsars x 5000 TOAs, HD GWB
+ RN + EFAC/EQUAD + ECORR; n_f = 14, ORFs hd / monopole / dipole), R realisations per batch, timed with HIP events in ONE process:

  generate_os                    eng.generate_os(R, chunk=R)                                            fixed noise, broadband
  generate_os_spectrum           eng.generate_os_spectrum(R, chunk=R)                                   fixed noise, per frequency
  generate_os matched            eng.generate_os(R, theta=theta, matched=True, chunk=R)
  generate_os_spectrum matched   eng.generate_os_spectrum(R, theta=theta, matched=True, chunk=R)

The four alternate step by step after a warm-up, so clock drift hits all alike.  The pair kernels are also timed on their own on one
batch: pta_os_pairs against pta_os_pairs_pf, and pta_os_matched_pairs against pta_os_matched_pairs_pf (full, narrowband, full with the
Fisher matrices written out).  Every figure is a median with [min, max].  Prints one JSON line; --out also writes it to a file.

    timeout -k 10 600 python scripts/gpu_os_spectrum_throughput.py --out profiles/r14_os_spectrum_throughput.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench import build_engine  # noqa: E402
from pta_replicator_amd import _lib, device as dv  # noqa: E402


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(runs, steps, warmup):
    """{name: [ms per step]} of the callables, alternating step by step"""
    for _ in range(warmup):
        for f in runs.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(steps):
        for k, f in runs.items():
            times[k].append(event_ms(f))
    return times


def stats(t):
    return dict(median=round(float(np.median(t)), 4), min=round(min(t), 4), max=round(max(t), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--components", type=int, default=14)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    R = a.batch
    eng, _, _ = build_engine(68, 5000, seed=1234)
    eng.prepare_optimal_statistic(components=a.components, matched=True)
    eng.set_hyper_prior(gwb_log10_A=(-15.0, -14.0), gwb_gamma=(3.5, 5.0), rn_log10_A=(-15.5, -13.0), rn_gamma=(2.0, 6.0))
    theta = eng.sample_theta(R)
    calls = alternate({
        "generate_os": lambda: eng.generate_os(R, chunk=R),
        "generate_os_spectrum": lambda: eng.generate_os_spectrum(R, chunk=R),
        "generate_os_matched": lambda: eng.generate_os(R, theta=theta, matched=True, chunk=R),
        "generate_os_spectrum_matched": lambda: eng.generate_os_spectrum(R, theta=theta, matched=True, chunk=R),
    }, a.steps, a.warmup)

    # the pair kernels on their own, on the operands the last matched call left (X, Z of the batch) and on Y of one batch
    rows = eng.generate(R, theta=theta)
    st = eng._os
    m, sp = st["matched"], eng._os_spectrum_state(st)
    ws = eng._os_matched_front(rows, R, eng._os_matched_theta(st, theta, R, "bench"), 0)
    Y = eng._os_project(rows, R)
    P, C, n_orf, s = eng.P, st["C"], st["n_orf"], dv.stream_ptr()
    nf, npairs = C // 2, len(st["plan"].den)
    A2, sg = dv.empty((R, n_orf)), dv.empty((R, n_orf))
    a2, sgf, fi = dv.empty((R, n_orf * nf)), dv.empty((R, n_orf * nf)), dv.empty((R, n_orf * nf * nf))

    def pf(mode, fisher):
        return lambda: _lib.call("pta_os_matched_pairs_pf", dv.ptr(ws["X"]), dv.ptr(ws["Z"]), P, C, R, dv.ptr(st["pa"]), dv.ptr(st["pb"]), npairs,
                                 dv.ptr(m["G"]), dv.ptr(m["G2"]), n_orf, mode, dv.ptr(a2), n_orf * nf, dv.ptr(sgf), n_orf * nf,
                                 dv.ptr(fi) if fisher else None, n_orf * nf * nf if fisher else 0, s)
    kernels = alternate({
        "pta_os_pairs": lambda: _lib.call("pta_os_pairs", dv.ptr(Y), P * C, P, C, R, dv.ptr(st["pa"]), dv.ptr(st["pb"]), npairs, dv.ptr(st["wt"]), n_orf,
                                          dv.ptr(A2), n_orf, None, None, 0, s),
        "pta_os_pairs_pf": lambda: _lib.call("pta_os_pairs_pf", dv.ptr(Y), P * C, P, C, R, dv.ptr(st["pa"]), dv.ptr(st["pb"]), npairs, dv.ptr(sp["G"]),
                                             n_orf, dv.ptr(sp["op"][0]), 0, dv.ptr(a2), n_orf * nf, s),
        "pta_os_matched_pairs": lambda: _lib.call("pta_os_matched_pairs", dv.ptr(ws["X"]), dv.ptr(ws["Z"]), P, C, R, dv.ptr(st["pa"]), dv.ptr(st["pb"]),
                                                  npairs, dv.ptr(m["G"]), dv.ptr(m["G2"]), n_orf, dv.ptr(A2), n_orf, dv.ptr(sg), n_orf, None, None, 0, s),
        "pta_os_matched_pairs_pf": pf(0, False),
        "pta_os_matched_pairs_pf_narrowband": pf(1, False),
        "pta_os_matched_pairs_pf_fisher": pf(0, True),
    }, a.steps, a.warmup)
    torch.cuda.synchronize()

    def ratio(t, num, den):
        return round(float(np.median(t[num]) / np.median(t[den])), 3)
    res = dict(
        config="68 x 5000, HD GWB + RN(67) + EFAC/EQUAD + ECORR, throughput mode; OS: spin model, GWB auto-term, ORFs hd/monopole/dipole; matched: "
               "theta ~ prior (gwb_log10_A, gwb_gamma, rn_log10_A, rn_gamma)",
        device=torch.cuda.get_device_name(0), batch=R, steps=a.steps, warmup=a.warmup, components=a.components, C=C, n_pairs=npairs,
        n_blocks=nf * (nf + 1) // 2, calls_ms={k: stats(t) for k, t in calls.items()},
        calls_realisations_per_s={k: dict(median=round(R / float(np.median(t)) * 1e3, 1), min=round(R / max(t) * 1e3, 1), max=round(R / min(t) * 1e3, 1))
                                  for k, t in calls.items()},
        spectrum_over_broadband_fixed=ratio(calls, "generate_os_spectrum", "generate_os"),
        spectrum_over_broadband_matched=ratio(calls, "generate_os_spectrum_matched", "generate_os_matched"),
        kernels_ms={k: stats(t) for k, t in kernels.items()},
        pairs_pf_over_pairs=ratio(kernels, "pta_os_pairs_pf", "pta_os_pairs"),
        matched_pairs_pf_over_matched_pairs=ratio(kernels, "pta_os_matched_pairs_pf", "pta_os_matched_pairs"),
    )
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
