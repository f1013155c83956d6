"""The per-frequency optimal statistic: a GWB whose spectrum turns over at f0 = 1e-8 Hz, searched under the usual power-law template.

  broadband       generate_os(R)            one amplitude A^2 under the template: a fraction of the injected A^2
  per frequency   generate_os_spectrum(R)   phi_k, the cross-correlated power of every Fourier bin: the injected spectrum

    python examples/os_spectrum.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pta_replicator_amd import red_noise as rn
from pta_replicator_amd.engine import ReplicaEngine
from pta_replicator_amd.simulate import ArrayTOAs, SimulatedPulsar, make_ideal

P, N, R, NF = 16, 200, 2048, 10
rng = np.random.default_rng(21)
psrs = []
for a in range(P):
    p = SimulatedPulsar(toas=ArrayTOAs(np.sort(rng.uniform(53000, 57500, N)), 0.1), name=f"J{a:04d}",       # 0.1 us white noise
                        loc={"RAJ": float(rng.uniform(0, 24)), "DECJ": float(np.degrees(np.arcsin(rng.uniform(-1, 1))))})
    make_ideal(p)
    psrs.append(p)
eng = ReplicaEngine(psrs, seed=8)
eng.set_white_noise(efac=1.0)
eng.set_gwb(-14.0, 13. / 3., turnover=True, f0=1e-8)
eng.prepare()
eng.prepare_optimal_statistic(components=NF)
A2 = eng.generate_os(R)["A2"][:, 0].cpu().numpy()
print(f"{P} pulsars x {N} TOAs, {R} realisations, GWB log10_A = -14 with a turnover at 1e-8 Hz")
print(f"broadband  A2_HD / A^2 = {A2.mean() / 1e-28:.3f} +- {A2.std() / np.sqrt(R) / 1e-28:.3f}")
for mode in ("full", "narrowband"):
    res = eng.generate_os_spectrum(R, mode=mode)
    f = res["freqs"].cpu().numpy()
    T = 1.0 / f[0]
    inj = rn.gwb_spectrum_hcf(f, -14.0, 13. / 3., True, 1e-8, 1, 1) ** 2 / (12 * np.pi ** 2 * f ** 3 * T)   # variance of one sin / cos coefficient
    phi = res["phi"][:, 0].cpu().numpy()
    print(f"per frequency ({mode}), HD:   f [nHz]   phi_injected [s^2]   mean(phi) / phi_injected")
    for k in range(NF):
        print(f"    {f[k] * 1e9:8.2f}   {inj[k]:.3e}   {phi[:, k].mean() / inj[k]:6.3f} +- {phi[:, k].std() / np.sqrt(R) / inj[k]:.3f}")
