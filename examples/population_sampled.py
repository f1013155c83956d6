"""A binned supermassive-binary population per realisation: every realisation draws its own Poisson counts on the GPU, injects the
loudest binaries of every frequency bin one by one and the rest as a free-spectrum GWB - the reference's add_gwb_plus_outlier_cws with
the sampling of the population in front of it, for a whole ensemble.

  1. set_population: a synthetic population in the reference's layout (vals = [Mtot (g), q, z, f_obs (Hz)], the expected number of every
     cell, the bin edges), the reference's CW flags, set_gwb(userSpec=) on the bin centres;
  2. generate_sampled: residuals and labels (the sources of every realisation, its residual spectrum, the cells they came from);
  3. generate_os_spectrum on the same realisations: the cross-correlated power per frequency bin against the spectrum of the whole
     population - the loud sources are part of what the array correlates.

    python examples/population_sampled.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pta_replicator_amd import _population
from pta_replicator_amd.engine import ReplicaEngine
from pta_replicator_amd.simulate import ArrayTOAs, SimulatedPulsar, make_ideal

P, N, R, F, CELLS, K = 20, 300, 1024, 8, 4000, 5
rng = np.random.default_rng(26)
T_obs = 4500 * 86400.0
psrs = []
for a in range(P):
    p = SimulatedPulsar(toas=ArrayTOAs(np.sort(np.r_[53000.0, 57500.0, rng.uniform(53000, 57500, N - 2)]), 0.1), name=f"J{a:04d}",
                        loc={"RAJ": float(rng.uniform(0, 24)), "DECJ": float(np.degrees(np.arcsin(rng.uniform(-1, 1))))})
    make_ideal(p)
    psrs.append(p)

# ---- 1. the population: F bins of CELLS cells, expected counts falling with mass -----------------------------------------------------
fobs = np.arange(1, F + 2) / T_obs
B = F * CELLS
log_m = rng.uniform(8.5, 10.3, B)
vals = np.array([10 ** log_m * _population.MSOL_CGS, rng.uniform(0.1, 1.0, B), rng.uniform(0.02, 2.0, B),
                 10 ** rng.uniform(np.log10(fobs[0]), np.log10(fobs[-1]), B)])
number = 10 ** (3.0 - 2.5 * (log_m - 8.5)) * (vals[3] / fobs[0]) ** (-8.0 / 3.0)      # many light binaries, a few heavy ones
fc = _population.f_centers(fobs)

eng = ReplicaEngine(psrs, seed=2026)
eng.set_white_noise(efac=1.0)
eng.set_gwb(-14.0, 13. / 3., userSpec=np.array([fc, 1e-15 * (fc / fc[0]) ** (-2.0 / 3.0)]).T)     # the nodes; every realisation brings its own hc
eng.set_cw(psrTerm=True, evolve=True, phase_approx=False, tref=53000 * 86400.0, pdist=1.0)     # the reference's flags
eng.set_population(vals, number, fobs, T_obs, outlier_per_bin=K)

# ---- 2. an ensemble --------------------------------------------------------------------------------------------------------------
res, labels = eng.generate_sampled(R)                                                  # [R, P N] seconds; labels on the device
print("labels:", {k: tuple(v.shape) for k, v in labels.items()})
count = labels["cw_count"].cpu().numpy()
multi = (labels["pop_number"] > 1).sum(dim=1).cpu().numpy()
print(f"sources per realisation: {count.min()} .. {count.max()} of {F * K}; of them cells holding more than one binary: mean {multi.mean():.2f}")
hc = 10 ** labels["gwb_log10_hc"].cpu().numpy()
print("residual spectrum hc per bin, median over realisations:", np.array2string(np.median(hc, axis=0), precision=2))
assert bool((eng.generate(8, r0=40, theta={k: v[40:48] for k, v in labels.items()}) == res[40:48]).all())
print("labels reproduce the sampled realisations: identical")

# ---- 3. the per-frequency optimal statistic of the same realisations --------------------------------------------------------------
eng.prepare_optimal_statistic(components=F)
os_res = eng.generate_os_spectrum(R, theta=labels)
f = os_res["freqs"].cpu().numpy()
phi = os_res["phi"][:, 0].cpu().numpy()
_, _, hs, fo = _population.cell_quantities(vals)
k_of = np.digitize(fo, fobs) - 1
total = np.array([np.sum((number * hs ** 2 * fo * T_obs)[k_of == b]) for b in range(F)])    # <hc^2> of the whole population per bin
T = 1.0 / f[0]
print("per frequency, HD:   f [nHz]   population <hc^2>   mean(phi) 12 pi^2 f^3 T")
for b in range(F):
    print(f"    {f[b] * 1e9:8.2f}   {total[b]:.3e}   {phi[:, b].mean() * 12 * np.pi ** 2 * f[b] ** 3 * T:.3e}")
