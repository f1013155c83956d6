"""Continuous-wave F-statistics per realisation on the GPU: 68 synthetic pulsars x 5000 TOAs with the NANOGrav 15-yr noise
dictionary's per-backend white noise, ECORR and red noise (no GWB: the statistic's noise model is the data covariance).

  null       noise only: 2 Fp ~ chi^2(2 P) and 2 Fe ~ chi^2(4) per grid point; the false-alarm threshold of max_s Fe per frequency
             (the trials over the sky grid included) is read off the ensemble
  detection  one earth-term binary per realisation from set_cw_prior at a fixed frequency, isotropic sky and orientation, on a
             ladder of strains cw_log10_h: the fraction of realisations whose max_s Fe at that frequency exceeds the null's
             threshold - a sensitivity curve point by point
  sky map    Fe over the whole sky grid for one realisation with a loud source, as text

    python examples/cw_f_statistic.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from bench import headline_array                                        # synthetic array with the NANOGrav 15-yr noise dictionary's shape
from pta_replicator_amd.engine import ReplicaEngine

psrs, noise = headline_array(68, 5000)
R = 4096
freqs = np.geomspace(4e-9, 1e-7, 32)                                    # GW frequencies [Hz]
n_lat, n_lon = 12, 24                                                   # an equal-area grid: uniform in cos(theta) and in phi
cos_t = np.repeat((np.arange(n_lat) + 0.5) / n_lat * 2 - 1, n_lon)
phi = np.tile((np.arange(n_lon) + 0.5) / n_lon * 2 * np.pi, n_lat)
jstar = 20                                                              # the injected sources sit at freqs[jstar]

eng = ReplicaEngine(psrs, seed=11)                                      # no GWB in the injection, none in the model
eng.set_white_noise(efac=noise["efac"], log10_equad=noise["log10_equad"], flags=noise["flags"])
eng.set_jitter(log10_ecorr=noise["log10_ecorr"], flags=noise["flags"], coarsegrain=0.1)
eng.set_red_noise(noise["rn_log10_A"], noise["rn_gamma"], components=30)
eng.set_cw(psrTerm=False, evolve=False)                                 # what the statistic models: a monochromatic earth term
eng.prepare()
eng.prepare_f_statistic(freqs, sky=(cos_t, phi))

# null: thresholds at false-alarm probability 1e-3 per frequency
null = eng.generate_f_statistic(R, sky_max=True)
fp0, fe0 = null["fp"].cpu().numpy(), null["fe_max"].cpu().numpy()
print(f"null, {R} realisations: mean Fp / P = {fp0.mean() / len(psrs):.4f} (1), mean max_s Fe = {fe0.mean():.2f} (2 for a single sky point)")
thr_fe, thr_fp = np.quantile(fe0[:, jstar], 1 - 1e-3), np.quantile(fp0[:, jstar], 1 - 1e-3)
print(f"f = {freqs[jstar] * 1e9:.1f} nHz: thresholds at false-alarm probability 1e-3: max_s Fe > {thr_fe:.2f}, Fp > {thr_fp:.2f}")

# detection probability against strain
lg = np.log10(freqs[jstar])
print("log10_h   P_det(Fe)  P_det(Fp)  sky index recovered")
for log10_h in np.arange(-15.0, -13.4, 0.2):
    eng.set_cw_prior(log10_mc=(9.0, 9.0), log10_fgw=(lg, lg), log10_h=(log10_h, log10_h))
    theta = eng.sample_theta(1024, r0=100000)
    out = eng.generate_f_statistic(1024, r0=100000, theta=theta, sky_max=True)
    fe, fp, arg = out["fe_max"][:, jstar].cpu().numpy(), out["fp"][:, jstar].cpu().numpy(), out["fe_arg"][:, jstar].cpu().numpy()
    src = np.stack([theta["cw_cos_gwtheta"].cpu().numpy(), theta["cw_gwphi"].cpu().numpy()], axis=1)
    near = np.argmin((cos_t[None, :] - src[:, :1]) ** 2 * (n_lat / 2) ** 2 + (np.angle(np.exp(1j * (phi[None, :] - src[:, 1:]))) * n_lon / (2 * np.pi)) ** 2, axis=1)
    print(f"{log10_h:7.2f}   {np.mean(fe > thr_fe):8.3f}  {np.mean(fp > thr_fp):9.3f}  {np.mean(arg == near):8.3f}")

# a sky map of one realisation with a loud source
eng.set_cw_prior(log10_mc=(9.0, 9.0), log10_fgw=(lg, lg), log10_h=(-13.6, -13.6))
theta = eng.sample_theta(1, r0=7)
fe = eng.f_statistic(eng.generate(1, r0=7, theta=theta))["fe"][0, jstar].cpu().numpy().reshape(n_lat, n_lon)
print(f"Fe(f = {freqs[jstar] * 1e9:.1f} nHz) over the sky, source at cos(theta) = {float(theta['cw_cos_gwtheta'][0]):.2f}, phi = {float(theta['cw_gwphi'][0]):.2f} "
      f"(rows: cos(theta) from -1 to 1; columns: phi from 0 to 2 pi); maximum {fe.max():.1f}")
ramp = " .:-=+*#%@"
for row in fe:
    print("  " + "".join(ramp[min(len(ramp) - 1, int(len(ramp) * v / (fe.max() * 1.0001)))] for v in row))
