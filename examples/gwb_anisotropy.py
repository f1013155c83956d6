"""An anisotropic GWB per realisation, injected and recovered on the GPU: 68 synthetic pulsars x 5000 TOAs with the NANOGrav 15-yr
noise dictionary's per-backend white noise, ECORR and red noise, and a GWB whose angular power is isotropic plus a dipole drawn per
realisation.

  injection  set_gwb(lmax=1) + set_hyper_prior(gwb_clm=...): c_1m ~ U(-0.6, 0.6) per realisation, c_00 = sqrt(4 pi) as configured
             (3 * 0.6 * max|Y_1m| = 0.88 <= c_00 Y_00 = 1: the power stays positive, every ORF is positive definite); each realisation
             is mixed with the Cholesky factor of its own ORF = 2 sum_k c_k basis[k]
  recovery   prepare_optimal_statistic(anisotropy_lmax=1): the joint fit of the four basis ORFs to the pair correlations gives
             a2clm = estimates of A^2 c_lm per realisation; c_1m / c_00 = a2clm[:, k] / a2clm[:, 0]

One realisation constrains its dipole poorly; the ensemble shows the estimator following the injected value.

    python examples/gwb_anisotropy.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from bench import configure_engine, headline_array                      # synthetic array with the NANOGrav 15-yr noise dictionary's shape
from pta_replicator_amd.engine import ReplicaEngine

psrs, noise = headline_array(68, 5000)
R = 4096
c00 = np.sqrt(4.0 * np.pi)

eng = configure_engine(ReplicaEngine(psrs, seed=19), noise)
eng.set_gwb(-14.0, 13. / 3., clm=[c00, 0.0, 0.0, 0.0], lmax=1)          # a loud background: the dipole of one sky shows in the ensemble
eng.prepare()
eng.set_hyper_prior(gwb_clm=(-0.6, 0.6))
eng.prepare_optimal_statistic(components=14, anisotropy_lmax=1)

theta = eng.sample_theta(R)
assert not theta["gwb_orf_info"].any()                                  # every drawn sky is positive definite
res = eng.generate_os(R, theta=theta)
c = theta["gwb_clm"].cpu().numpy()
a2 = res["a2clm"].cpu().numpy()
sig = res["clm_sigma"].cpu().numpy()
print(f"{R} realisations, A^2 = 1e-28: mean a2clm[:, 0] / sqrt(4 pi) = {a2[:, 0].mean() / c00:.3e}  (null sigma of one realisation {sig[0] / c00:.1e})")
print("injected c_1m (bin centre)   mean recovered c_1m = sqrt(4 pi) <a2clm_k> / <a2clm_0>,   m = -1, 0, 1")
edges = np.linspace(-0.6, 0.6, 7)
for lo, hi in zip(edges[:-1], edges[1:]):
    row = []
    for k in (1, 2, 3):
        sel = (c[:, k] >= lo) & (c[:, k] < hi)
        row.append(c00 * a2[sel, k].mean() / a2[sel, 0].mean())
    print(f"{(lo + hi) / 2:+.2f}                         " + "   ".join(f"{v:+.3f}" for v in row))
