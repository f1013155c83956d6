"""A free GWB spectrum per realisation, injected and recovered on the GPU.

The engine is configured with a userSpec of M nodes; set_hyper_prior(gwb_log10_hc=...) draws log10 hc at every node per realisation
(stream (7, 1)), generate_os_spectrum(matched=True) generates each realisation under its own spectrum and evaluates the per-frequency
optimal statistic with that spectrum in the noise model.  Printed per Fourier bin, averaged over the realisations: the injected
phi_k = hc_r(f_k)^2 / (12 pi^2 f_k^3 T) against the recovered phi_k.

    python examples/gwb_spectrum_sampled.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pta_replicator_amd import _hyper
from pta_replicator_amd.engine import ReplicaEngine
from pta_replicator_amd.simulate import ArrayTOAs, SimulatedPulsar, make_ideal

P, N, R, NF, M = 16, 200, 2048, 8, 10
rng = np.random.default_rng(21)
psrs = []
for a in range(P):
    p = SimulatedPulsar(toas=ArrayTOAs(np.sort(rng.uniform(53000, 57500, N)), 0.1), name=f"J{a:04d}",       # 0.1 us white noise
                        loc={"RAJ": float(rng.uniform(0, 24)), "DECJ": float(np.degrees(np.arcsin(rng.uniform(-1, 1))))})
    make_ideal(p)
    psrs.append(p)
nodes = 10 ** np.linspace(np.log10(1.5e-9), np.log10(4e-8), M)
base = -14.0 - (2. / 3.) * np.log10(nodes * 3.16e7)                      # a gamma = 13/3 power law of amplitude 1e-14 at the nodes
eng = ReplicaEngine(psrs, seed=8)
eng.set_white_noise(efac=1.0)
eng.set_gwb(-14.0, 13. / 3., userSpec=np.stack([nodes, 10 ** base], axis=1))
eng.prepare()
eng.prepare_optimal_statistic(components=NF, matched=True)
eng.set_hyper_prior(gwb_log10_hc=np.stack([base - 0.3, base + 0.3], axis=1))   # a free spectrum: every node in its own box
theta = eng.sample_theta(R)
res = eng.generate_os_spectrum(R, theta=theta, matched=True)
f = res["freqs"].cpu().numpy()
T = 1.0 / f[0]
_, xp = _hyper.spec_nodes(eng._gw["userSpec"])
hc = _hyper.spec_eval(_hyper.spec_tables(f, xp), theta["gwb_log10_hc"].cpu().numpy())    # [R, NF]: hc_r(f_k), the nodes given sorted
inj = hc ** 2 / (12 * np.pi ** 2 * f ** 3 * T)                                           # variance of one sin / cos coefficient
phi = res["phi"][:, 0].cpu().numpy()
print(f"{P} pulsars x {N} TOAs, {R} realisations, log10 hc at {M} nodes drawn within +-0.3 of a gamma = 13/3 power law")
print("per frequency (full), HD:   f [nHz]   mean phi_injected [s^2]   mean(phi) / mean(phi_injected)   corr(phi, phi_injected)")
for k in range(NF):
    ratio = phi[:, k].mean() / inj[:, k].mean()
    err = phi[:, k].std() / np.sqrt(R) / inj[:, k].mean()
    print(f"    {f[k] * 1e9:8.2f}   {inj[:, k].mean():.3e}   {ratio:6.3f} +- {err:.3f}   {np.corrcoef(phi[:, k], inj[:, k])[0, 1]:6.3f}")
