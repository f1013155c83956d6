"""Throughput of the per-realisation chromatic events, headline configuration (68 pulsars x 5000 TOAs in two radio bands, HD GWB + RN +
EFAC/EQUAD + ECORR), R realisations, timed with HIP events in ONE process, every comparison alternating step by step after a warm-up:

  sparse       a decay and a cusp per realisation in two drawn pulsars (E = 2): pta_engine_chrom_event_add (accumulate = 1), which
               leaves the (tile, realisation) pairs of a pulsar without a live event alone, beside pta_engine_transient_add at V = 2 on
               the same rows (the existing kernel that read-modify-writes every row of every pulsar) and pta_engine_bwm_add (that
               traffic and no arithmetic)
  dense        an annual term in every pulsar plus the two events (E = P + 2): the same kernels (the transient kernel at V = 2 and the
               ramp kernel as the yardsticks of the traffic)
  generate     generate(R) against generate(R, theta = the sparse / the dense events), and generate_sampled with and without the
               event prior

A library built with the measurement's second instance of the add kernel (the template parameter that switches the skip of untouched
(tile, realisation) pairs off, exported as pta_engine_chrom_event_add_noskip) is measured with it; the committed library holds the winner
alone.  Every timing is the median with the [min, max] range of --reps repetitions; a ratio is the median ratio with the
range [min / max, max / min].  Prints one JSON line; --out also writes it to a file (after every section, so that a cut run keeps what
it measured).

    timeout -k 10 900 python scripts/gpu_chrom_event_throughput.py --out profiles/r29_chrom_event_throughput.json
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
from gpu_burst_throughput import ratio  # noqa: E402
from gpu_bwm_throughput import alternate  # noqa: E402


def overlap(a, b):
    """True if the [min, max] ranges of two timings overlap"""
    return a["min"] <= b["max"] and b["min"] <= a["max"]


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
    rng = np.random.default_rng(7)
    for p in eng.psrs:
        p.toas.freqs_mhz = np.where(rng.integers(0, 2, len(p.toas.freqs_mhz)) == 1, 1440.0, 820.0)
    eng.workspace_bytes = 32 << 30          # one batch of R realisations
    P, N = eng.P, eng.n_toa
    first, last = min(m.min() for m in eng.mjd), max(m.max() for m in eng.mjd)
    res = dict(config=f"{P} x {a.toas} in two bands (820 / 1440 MHz), HD GWB + RN + EFAC/EQUAD + ECORR; sparse: a decay and a cusp per realisation "
                      "in two drawn pulsars, t0 over the span, tau in [1e6, 3e7] s; dense: plus an annual term in every pulsar",
               device=torch.cuda.get_device_name(0), batch=R, reps=a.reps, warmup=a.warmup, n_toa=N, kernels={}, generate={})

    def save():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write(json.dumps(res) + "\n")

    s = dv.stream_ptr()
    noskip = getattr(_lib.lib, "pta_engine_chrom_event_add_noskip", None)   # only in a library built for the A/B
    if noskip is not None:
        noskip.restype, noskip.argtypes = ctypes.c_int, _lib.lib.pta_engine_chrom_event_add.argtypes
    res["noskip_instance_measured"] = noskip is not None
    buf = dv.empty((R, N))
    eng.generate(R, out=buf)
    eng.set_chromatic_events(2)
    lnu = eng._ce_lnu_device()
    keep = []

    # the sparse theta: slot 0 a decay, slot 1 a cusp, each in a drawn pulsar
    box = dict(log10_a=(-6.5, -5.5), t0_mjd=(float(first), float(last)), log10_tau=(6.0, 7.5))
    eng.set_chromatic_event_prior(["decay", "cusp"], **box)
    sparse = eng.sample_theta(R)
    # the dense theta: slots 0 .. P-1 the annual term of pulsar a, then the two events
    E2 = P + 2
    dense_prior = dict(kind=["annual"] * P + ["decay", "cusp"], log10_a=[(-7.0, -6.0)] * P + [box["log10_a"]] * 2, psr=list(range(P)) + [None, None],
                       t0_mjd=[None] * P + [box["t0_mjd"]] * 2, log10_tau=[None] * P + [box["log10_tau"]] * 2)

    def ce_table(theta, E):
        """the table rows of theta, left in the engine's scratch by one _ce_apply, and the struct the add entry takes"""
        _, det = eng._theta_parts(theta, R, check_values=False)
        eng._ce_apply(det, R, buf)
        torch.cuda.synchronize()
        tab = eng._scratch_tabs["ce_tab"][0][:R].clone()
        keep.append(tab)
        c = _lib.ChromEventEngine()
        c.n_psr, c.n_ev, c.toa_s, c.lnu, c.tab = P, E, eng.d_toa_s.data_ptr(), lnu.data_ptr(), tab.data_ptr()
        return c

    def transient_add():
        """pta_engine_transient_add at V = 2 on the same rows: two wavelets per realisation in two drawn pulsars"""
        gen = torch.Generator(device="cuda").manual_seed(1)

        def uni(lo, hi, *shape):
            return lo + (hi - lo) * torch.rand(shape, dtype=torch.float64, device="cuda", generator=gen)
        tau = 10 ** uni(6.0, 7.5, R, 2)
        tab = torch.stack([torch.floor(uni(0, P, R, 2)).clamp(max=P - 1), uni(first, last, R, 2) * 86400.0, -0.5 / tau ** 2, 10 ** uni(-8.5, -7.0, R, 2),
                           uni(-1e-6, 1e-6, R, 2), uni(-1e-6, 1e-6, R, 2)], dim=2).contiguous()
        t = _lib.TransientEngine()
        t.n_psr, t.n_wav, t.toa_s, t.tab = P, 2, eng.d_toa_s.data_ptr(), tab.data_ptr()
        keep.append(tab)
        return lambda: _lib.call("pta_engine_transient_add", ctypes.byref(eng.plan), ctypes.byref(t), R, dv.ptr(buf), N, 1, s)

    gen = torch.Generator(device="cuda").manual_seed(2)
    coef = (torch.rand((R, P), dtype=torch.float64, device="cuda", generator=gen) - 0.5) * 2e-15
    t0 = (first + (last - first) * torch.rand((R,), dtype=torch.float64, device="cuda", generator=gen)) * 86400.0
    bw = _lib.BwmEngine()
    bw.n_psr, bw.toa_s, bw.coef, bw.t0_s = P, eng.d_toa_s.data_ptr(), coef.data_ptr(), t0.data_ptr()
    bwm_add = lambda: _lib.call("pta_engine_bwm_add", ctypes.byref(eng.plan), ctypes.byref(bw), R, dv.ptr(buf), N, 1, s)   # noqa: E731
    nt_add = transient_add()

    def section(name, theta, E):
        c = ce_table(theta, E)
        fns = {"chrom_event_add": lambda: _lib.call("pta_engine_chrom_event_add", ctypes.byref(eng.plan), ctypes.byref(c), R, dv.ptr(buf), N, 1, s)}
        if noskip is not None:
            fns["chrom_event_add_noskip"] = lambda: _lib.check(noskip(ctypes.byref(eng.plan), ctypes.byref(c), R, dv.ptr(buf), N, 1, s))
        fns.update({"transient_add_v2": nt_add, "bwm_add": bwm_add})
        k = alternate(fns, a.reps, a.warmup)
        k["events_per_realisation"] = E
        k["skip_over_transient"] = ratio(k["chrom_event_add"], k["transient_add_v2"])
        k["skip_over_bwm"] = ratio(k["chrom_event_add"], k["bwm_add"])
        if noskip is not None:
            k["skip_over_noskip"] = ratio(k["chrom_event_add"], k["chrom_event_add_noskip"])
            k["skip_range_below_noskip"] = bool(k["chrom_event_add"]["max"] < k["chrom_event_add_noskip"]["min"])
            k["skip_range_above_noskip"] = bool(k["chrom_event_add"]["min"] > k["chrom_event_add_noskip"]["max"])
            k["ranges_overlap"] = overlap(k["chrom_event_add"], k["chrom_event_add_noskip"])
        res["kernels"][name] = k
        print(f"{name}: {k}", flush=True)
        save()

    section("sparse", sparse, 2)
    eng.set_chromatic_events(E2)
    eng.set_chromatic_event_prior(**dense_prior)
    dense = eng.sample_theta(R)
    section("dense", dense, E2)
    if noskip is not None:
        res["keep_skip"] = bool(res["kernels"]["sparse"]["skip_range_below_noskip"] and not res["kernels"]["dense"]["skip_range_above_noskip"])
    keep.clear()
    torch.cuda.empty_cache()

    # ---- generate with and without the keys (the engine is at E = P + 2: the sparse theta is padded with a count of 2)
    pad = {k: torch.cat([v, dense[k][:, 2:]], dim=1) for k, v in sparse.items()}
    pad["ce_count"] = torch.full((R,), 2, dtype=torch.int32, device="cuda")
    g = alternate({"generate": lambda: eng.generate(R, out=buf), "generate_sparse": lambda: eng.generate(R, out=buf, theta=pad),
                   "generate_dense": lambda: eng.generate(R, out=buf, theta=dense), "generate_sampled_dense": lambda: eng.generate_sampled(R, out=buf)},
                  a.reps, a.warmup)
    eng.set_hyper_prior(gwb_log10_A=(-15, -14))
    prior = eng._ce_prior

    def sampled(events):
        eng._ce_prior = prior if events else None
        return eng.generate_sampled(R, out=buf)
    g.update(alternate({"generate_sampled_hyper": lambda: sampled(False), "generate_sampled_hyper_events": lambda: sampled(True)}, a.reps, a.warmup))
    g["sparse_over_plain"] = ratio(g["generate_sparse"], g["generate"])
    g["dense_over_plain"] = ratio(g["generate_dense"], g["generate"])
    g["sampled_events_over_sampled"] = ratio(g["generate_sampled_hyper_events"], g["generate_sampled_hyper"])
    for k, (x, y) in {"sparse_vs_plain": ("generate_sparse", "generate"), "dense_vs_plain": ("generate_dense", "generate"),
                      "sampled_events_vs_sampled": ("generate_sampled_hyper_events", "generate_sampled_hyper")}.items():
        g[k + "_ranges_overlap"] = overlap(g[x], g[y])
    res["generate"] = g
    print(f"generate: {g}", flush=True)
    save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
