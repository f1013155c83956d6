"""Chromatic events per realisation on the GPU: a J1713+0747-like exponential DM dip in one pulsar plus the yearly DM sinusoid in every
pulsar, every parameter drawn per realisation from a prior, the term alone beside the other signals, and its chromatic signature: the
ratio of the term between the two radio bands is (nu_high / nu_low)^2.

    python examples/chromatic_events.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from bench import configure_engine, headline_array                      # synthetic array with the NANOGrav 15-yr noise dictionary's shape
from pta_replicator_amd.engine import ReplicaEngine

psrs, noise = headline_array(68, 5000)
rng = np.random.default_rng(3)
for p in psrs:                                                          # two receivers per pulsar
    p.toas.freqs_mhz = np.where(rng.integers(0, 2, len(p.toas.freqs_mhz)) == 1, 1440.0, 820.0)
P, R, DIP = len(psrs), 8, 11                                            # the dip lives in pulsar 11

eng = configure_engine(ReplicaEngine(psrs, seed=21), noise)
eng.prepare()
first, last = min(m.min() for m in eng.mjd), max(m.max() for m in eng.mjd)
span = last - first

# ---- slots 0 .. P-1: the annual DM term of pulsar a; slot P: the dip.  kind and pulsar are fixed per slot, the rest is drawn.
eng.set_chromatic_events(n=P + 1, ref_freq_mhz=1400.0)
eng.set_chromatic_event_prior(kind=["annual"] * P + ["decay"],
                              psr=list(range(P)) + [DIP],
                              log10_a=[(-7.5, -6.5)] * P + [(-6.0, -5.3)],                      # seconds at 1400 MHz
                              t0_mjd=[None] * P + [(first + 0.3 * span, first + 0.7 * span)],
                              log10_tau=[None] * P + [(np.log10(20 * 86400.0), np.log10(120 * 86400.0))],   # 20 .. 120 days
                              sign=-1, index=2.0)                                               # a dip: the TOAs come early; DM: nu^-2
rows, theta = eng.generate_sampled(R)
sig = eng.generate_per_signal(R, theta=theta)
print("the dip of realisation 0:", {k: float(theta[k][0, P]) for k in ("ce_psr", "ce_t0_mjd", "ce_log10_tau", "ce_log10_a")})
term = sig["chrom_event"].cpu().numpy()
print(f"rms [s] over {R} realisations: chromatic events {np.sqrt(np.mean(term ** 2)):.3g}, everything {float(rows.square().mean().sqrt()):.3g}")

# ---- the chromatic signature in the dip's pulsar, just after the epoch
sl = slice(eng.off[DIP], eng.off[DIP + 1])
mjd, nu = eng.mjd[DIP], psrs[DIP].toas.freqs_mhz
t0 = float(theta["ce_t0_mjd"][0, P])
after = (mjd > t0) & (mjd < t0 + 10)
annual_only = dict(theta, ce_count=np.full(R, P))                         # the same labels without the last slot
dip = term[0, sl] - eng.generate_per_signal(R, theta=annual_only)["chrom_event"].cpu().numpy()[0, sl]
lo, hi = dip[after & (nu < 1000)], dip[after & (nu > 1000)]
if len(lo) and len(hi):
    print(f"dip just after t0: {lo.mean():.3g} s at 820 MHz, {hi.mean():.3g} s at 1440 MHz, ratio {lo.mean() / hi.mean():.3f} "
          f"((1440 / 820)^2 = {(1440 / 820) ** 2:.3f} up to the decay between the TOAs)")
print(f"before t0 the dip is exactly zero: {bool(np.all(dip[mjd < t0] == 0))}")
