"""Null and signal distributions of the Hellings-Downs optimal statistic, computed per realisation on the GPU: 68 synthetic pulsars x
5000 TOAs with the NANOGrav 15-yr noise dictionary's per-backend white noise, ECORR and red noise.

  null    no GWB injected, no GW term in the model: the SNR is unit-variance by construction (its false-alarm levels follow)
  signal  the dictionary's HD GWB injected: the SNR distribution shifts, and the fraction above the null's 3-sigma level is the
          detection probability at that amplitude

    python examples/os_null_distribution.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from bench import configure_engine, headline_array                      # synthetic array with the NANOGrav 15-yr noise dictionary's shape
from pta_replicator_amd.engine import ReplicaEngine

psrs, noise = headline_array(68, 5000)
R = 8192


def histogram(snr, lo=-5.0, hi=10.0, bins=30):
    h, edges = np.histogram(snr, bins=bins, range=(lo, hi))
    for c, e in zip(h, edges):
        print(f"  {e:6.2f} {'#' * int(60 * c / max(h.max(), 1))}")


# null: white noise + ECORR + red noise only
eng = configure_engine(ReplicaEngine(psrs, seed=11), noise)
eng._gw = None                                                         # no GWB in the injection
eng.prepare()
eng.prepare_optimal_statistic(components=14, gwb_auto=False)            # model = data covariance
null = eng.generate_os(R)
snr0 = null["snr"].cpu().numpy()
print(f"null, {R} realisations: SNR mean {snr0.mean(0).round(3)}, std {snr0.std(0).round(3)} ({null['names']})")
thr = np.quantile(snr0[:, 0], 1 - 1.35e-3)                              # the empirical one-sided 3-sigma level of the HD SNR
print(f"HD SNR at false-alarm probability 1.35e-3: {thr:.2f}")
histogram(snr0[:, 0])

# signal: the dictionary's GWB amplitude, HD-correlated
eng = configure_engine(ReplicaEngine(psrs, seed=12), noise)
eng.prepare()
eng.prepare_optimal_statistic(components=14)                            # GW auto-term at the configured amplitude
sig = eng.generate_os(R)
snr1 = sig["snr"].cpu().numpy()
A2 = sig["A2"].cpu().numpy()[:, 0]
print(f"signal (log10_A = {noise['gw_log10_A']:.2f}): mean A2_HD / A^2 = {A2.mean() / 10 ** (2 * noise['gw_log10_A']):.3f}, "
      f"HD SNR mean {snr1[:, 0].mean():.2f}, detection probability at the null's 3-sigma level {np.mean(snr1[:, 0] > thr):.3f}")
histogram(snr1[:, 0])
