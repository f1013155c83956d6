"""Burst-with-memory detection per realisation on the GPU: 68 synthetic pulsars x 5000 TOAs with the NANOGrav 15-yr noise
dictionary's per-backend white noise, ECORR and red noise (no GWB: the statistic's noise model is the data covariance).

  null       noise only: 2 Fb ~ chi^2(2) per (epoch, sky point); the false-alarm threshold of max_j max_s Fb (the trials over the
             epoch and sky grids included) is read off the ensemble
  detection  one burst per realisation from set_bwm_prior, isotropic sky and polarisation, epoch uniform over the grid's span, on
             a ladder of strains bwm_log10_h: the fraction of realisations whose max_j max_s Fb exceeds the null's threshold - a
             sensitivity curve point by point - and how often the best epoch is the grid epoch nearest to the injected one

Out of scope of the statistic: the pulsar term, a noise model matched to per-realisation theta, more than one burst, a continuous
epoch (the epochs are a grid).

    python examples/bwm_detection.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from bench import headline_array                                        # synthetic array with the NANOGrav 15-yr noise dictionary's shape
from pta_replicator_amd.engine import ReplicaEngine

psrs, noise = headline_array(68, 5000)
R = 4096
n_lat, n_lon = 12, 24                                                   # an equal-area grid: uniform in cos(theta) and in phi
cos_t = np.repeat((np.arange(n_lat) + 0.5) / n_lat * 2 - 1, n_lon)
phi = np.tile((np.arange(n_lon) + 0.5) / n_lon * 2 * np.pi, n_lat)

eng = ReplicaEngine(psrs, seed=11)                                      # no GWB in the injection, none in the model
eng.set_white_noise(efac=noise["efac"], log10_equad=noise["log10_equad"], flags=noise["flags"])
eng.set_jitter(log10_ecorr=noise["log10_ecorr"], flags=noise["flags"], coarsegrain=0.1)
eng.set_red_noise(noise["rn_log10_A"], noise["rn_gamma"], components=30)
eng.set_bwm()
eng.prepare()
first, last = max(m.min() for m in eng.mjd), min(m.max() for m in eng.mjd)
span = last - first
t0_grid = np.linspace(first + 0.1 * span, last - 0.1 * span, 32)        # burst epochs [MJD], inside every pulsar's data
eng.prepare_bwm_statistic(t0_grid, sky=(cos_t, phi))

# null: the threshold at false-alarm probability 1e-2 of the maximum over the whole (epoch, sky) grid
null = eng.generate_bwm_statistic(R, sky_max=True)["fb_max"].cpu().numpy()
print(f"null, {R} realisations: mean max_s Fb per epoch = {null.mean():.2f} (1 for a single sky point)")
thr = np.quantile(null.max(axis=1), 1 - 1e-2)
print(f"threshold at false-alarm probability 1e-2: max_j max_s Fb > {thr:.2f}")

# detection probability against strain
print("log10_h   P_det   epoch recovered")
for log10_h in np.arange(-15.0, -13.4, 0.2):
    eng.set_bwm_prior(log10_h=(log10_h, log10_h), t0_mjd=(t0_grid[0], t0_grid[-1]))
    theta = eng.sample_theta(1024, r0=100000)
    fb = eng.generate_bwm_statistic(1024, r0=100000, theta=theta, sky_max=True)["fb_max"].cpu().numpy()
    near = np.argmin(np.abs(t0_grid[None, :] - theta["bwm_t0_mjd"].cpu().numpy()[:, None]), axis=1)
    print(f"{log10_h:7.2f}   {np.mean(fb.max(axis=1) > thr):5.3f}   {np.mean(fb.argmax(axis=1) == near):5.3f}")
