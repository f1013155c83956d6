"""Sine-Gaussian wavelets per realisation on the GPU: a GW burst (a coherent sum of wavelets from one sky position) and glitch-like
noise transients (single wavelets, each in one pulsar), drawn per realisation from uniform boxes, and what the transients do to the
null distribution of the Hellings-Downs optimal statistic evaluated under the fixed noise model.

    python examples/burst_wavelets.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from bench import configure_engine, headline_array                      # synthetic array with the NANOGrav 15-yr noise dictionary's shape
from pta_replicator_amd.engine import ReplicaEngine

psrs, noise = headline_array(68, 5000)
R = 4096

eng = configure_engine(ReplicaEngine(psrs, seed=21), noise)
eng._gw = None                                                         # no GWB: the null of the optimal statistic
eng.prepare()
first, last = min(m.min() for m in eng.mjd), max(m.max() for m in eng.mjd)
span = last - first

# ---- inject: a burst of 3 wavelets and 8 glitches per realisation, every parameter drawn on chip, keyed by (seed, realisation)
eng.set_burst(n_wavelets=3).set_transients(n=8)
eng.set_burst_prior(t0_mjd=(first + 0.2 * span, last - 0.2 * span), log10_tau=(6.5, 7.5), log10_f=(-8.3, -7.3),
                    log10_a_plus=(-7.5, -6.5), log10_a_cross=(-7.5, -6.5))
eng.set_transient_prior(t0_mjd=(first, last), log10_tau=(5.5, 6.5), log10_f=(-7.5, -6.5), log10_a=(-6.5, -5.5))
rows, theta = eng.generate_sampled(8)
sig = eng.generate_per_signal(8, theta=theta)
print("labels of realisation 0:")
for k in ("burst_cos_gwtheta", "burst_gwphi", "burst_t0_mjd", "burst_log10_tau", "nt_psr", "nt_t0_mjd"):
    print(f"  {k:18s} {theta[k][0].cpu().numpy()}")
print(f"rms [s] over 8 realisations: burst {float(sig['burst'].square().mean().sqrt()):.3g}, transients "
      f"{float(sig['transient'].square().mean().sqrt()):.3g}, everything {float(rows.square().mean().sqrt()):.3g}")

# ---- the fixed-noise OS null distribution with and without transient contamination (the same noise realisations in both)
eng.prepare_optimal_statistic(components=14, gwb_auto=False)
clean = eng.generate_os(R)["snr"].cpu().numpy()[:, 0]
theta = eng.sample_theta(R)
glitches = {k: v for k, v in theta.items() if k.startswith("nt_")}
dirty = eng.generate_os(R, theta=glitches)["snr"].cpu().numpy()[:, 0]
both = eng.generate_os(R, theta=theta)["snr"].cpu().numpy()[:, 0]
thr = np.quantile(clean, 1 - 1.35e-3)
print(f"HD SNR, {R} realisations, threshold at the clean null's 3-sigma level {thr:.2f}:")
for name, snr in (("noise only", clean), ("+ 8 glitches", dirty), ("+ glitches + burst", both)):
    print(f"  {name:20s} mean {snr.mean():6.3f}  std {snr.std():5.3f}  false-alarm fraction {np.mean(snr > thr):.4f}")
