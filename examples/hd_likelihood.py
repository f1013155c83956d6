"""Hellings-Downs against uncorrelated common process: the log Bayes factor of each of R realisations by grid integration, on the GPU.
The realisations carry a GWB with Hellings-Downs correlations (or, with --uncorrelated, without them); the likelihood ratio of a
correlated common process against noise only is evaluated for both ORFs on a grid of (log10_A, gamma), and with the same flat prior on the
grid for both models the evidence ratio is the ratio of the grid sums:

    ln B_hd/curn = logsumexp_g Lambda_hd[g] - logsumexp_g Lambda_curn[g]

(the noise-only likelihood and the grid's measure cancel).  The intrinsic noise is held at its configured values.

    python examples/hd_likelihood.py [--uncorrelated]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import configure_engine, headline_array                      # synthetic array with the NANOGrav 15-yr noise dictionary's shape
from pta_replicator_amd.engine import ReplicaEngine

P, N, R = 24, 2000, 512
TRUE_A, TRUE_G = -14.2, 13. / 3.
uncorrelated = "--uncorrelated" in sys.argv[1:]
psrs, noise = headline_array(P, N)
eng = configure_engine(ReplicaEngine(psrs, seed=21), noise)
eng.set_gwb(TRUE_A, TRUE_G, no_correlations=uncorrelated)
eng.prepare()
eng.prepare_correlated_likelihood(components=10, orfs=("hd", "curn", "monopole", "dipole"))
axis_A, axis_g = np.linspace(-14.8, -13.6, 13), np.linspace(3.0, 6.0, 7)
grid, shape = eng.theta_grid(gwb_log10_A=axis_A, gwb_gamma=axis_g)      # 91 grid points
res = eng.generate_correlated_lnl(R, grid, chunk=256)                  # the residuals never leave the device
lam, names = res["lnl_ratio"], res["names"]                             # [R, n_orf, G]
lnZ = torch.logsumexp(lam, dim=2).cpu().numpy()                         # flat prior on the grid, the same for every model
print(f"{P} pulsars x {N} TOAs, {R} realisations, GWB at ({TRUE_A}, {TRUE_G:.3f}) {'without' if uncorrelated else 'with Hellings-Downs'} correlations, "
      f"grid {shape[0]} x {shape[1]}")
for k, name in enumerate(names):
    if name == "curn":
        continue
    lnB = lnZ[:, names.index(name)] - lnZ[:, names.index("curn")]
    print(f"  ln B {name:>8} / curn: mean {lnB.mean():+8.3f} +- {lnB.std() / np.sqrt(R):.3f}, median {np.median(lnB):+8.3f}, positive in "
          f"{100 * np.mean(lnB > 0):.1f} % of the realisations")
post = torch.softmax(lam[:, names.index("hd"), :], dim=1).reshape(R, *shape)
mean_A = (post.sum(dim=2).cpu().numpy() * axis_A[None, :]).sum(axis=1)
mean_g = (post.sum(dim=1).cpu().numpy() * axis_g[None, :]).sum(axis=1)
print(f"  HD posterior mean log10_A {mean_A.mean():.3f} +- {mean_A.std():.3f} (scatter over realisations), gamma {mean_g.mean():.3f} +- {mean_g.std():.3f}")
