"""Chromatic (DM) red noise in the noise model: a two-band array whose pulsars carry dispersion-measure variations, and the null
distribution of the optimal statistic weighted with the chromatic term in the noise model and without it.

    python examples/chromatic_noise.py

The realisations hold white noise, ECORR, achromatic red noise and a DM process per pulsar, and NO common signal.  The statistic
prepared on the engine that generates them puts the columns (nu_ref / nu)^2 . F with their prior into C_a; the statistic prepared on
the same engine without the process believes the data are quieter than they are, and its "SNR" is no unit-variance variable any more.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from pta_replicator_amd.engine import ReplicaEngine
from pta_replicator_amd.simulate import ArrayTOAs, SimulatedPulsar, make_ideal

P, N, R = 20, 800, 4096
rng = np.random.default_rng(7)
psrs = []
for a in range(P):
    mjd = np.sort(rng.uniform(53000, 58000, N))
    band = np.where(rng.integers(0, 2, N) == 1, 1440.0, 820.0)          # two radio bands [MHz]
    psr = SimulatedPulsar(toas=ArrayTOAs(mjd, 0.5, freqs_mhz=band), name=f"J{a:04d}",
                          loc={"RAJ": float(rng.uniform(0, 24)), "DECJ": float(np.degrees(np.arcsin(rng.uniform(-1, 1))))})
    make_ideal(psr)
    psrs.append(psr)


rn_A, rn_g = rng.uniform(-14.5, -13.8, P), rng.uniform(2.0, 4.5, P)
dm_A, dm_g = rng.uniform(-13.8, -13.2, P), rng.uniform(1.5, 3.5, P)


def engine(chromatic):
    eng = ReplicaEngine(psrs, seed=2026)
    eng.set_white_noise(efac=1.0, log10_equad=-7.0)
    eng.set_jitter(log10_ecorr=-7.0)
    eng.set_red_noise(list(rn_A), list(rn_g), components=30)
    if chromatic:   # DM variations: index 2, referred to 1400 MHz; every pulsar its own amplitude and spectral index
        eng.set_chromatic_noise(list(dm_A), list(dm_g), components=30, index=2.0, ref_freq_mhz=1400.0)
    return eng.prepare()


with_dm, without = engine(True), engine(False)

rows = with_dm.generate(R)                                   # [R, 16000] seconds on the device: noise only
sig = with_dm.generate_per_signal(4)
a = 0
ch = with_dm.split(sig["chrom"])[a][0].cpu().numpy()
f = psrs[a].toas.freqs_mhz
print("pulsar 0, RMS of the chromatic term [us]: 820 MHz %.3f, 1440 MHz %.3f (ratio %.2f; (1440 / 820)^2 = %.2f)"
      % (1e6 * ch[f == 820.0].std(), 1e6 * ch[f == 1440.0].std(), ch[f == 820.0].std() / ch[f == 1440.0].std(), (1440.0 / 820.0) ** 2))

# the same rows through the optimal statistic with and without the chromatic columns in C_a (no GW auto-term: this is a null run)
for name, eng in (("with the chromatic term in the noise model", with_dm), ("without it", without)):
    eng.prepare_optimal_statistic(components=14, gwb_auto=False)
    snr = eng.optimal_statistic(rows)["snr"][:, 0].cpu().numpy()     # Hellings-Downs
    print("%-44s null SNR: mean %+.3f, std %.3f, P(SNR > 3) = %.4f" % (name + ":", snr.mean(), snr.std(), np.mean(snr > 3)))
print("(a correctly weighted null SNR has unit variance; its tail is heavier than a Gaussian's, for which P(SNR > 3) = 0.0013)")

# per-realisation amplitudes: theta's chrom_log10_A / chrom_gamma [R, P], or drawn on chip from uniform boxes with the labels returned
with_dm.set_hyper_prior(chrom_log10_A=(-14.5, -13.0), chrom_gamma=(1.0, 4.0))
res, theta = with_dm.generate_sampled(256)
print({k: tuple(v.shape) for k, v in theta.items()})
