"""Posterior of (log10_A, gamma) of a common process for each of R realisations, on the GPU: the realisations carry a common
uncorrelated process with a known amplitude and index, the marginalised likelihood is evaluated on a grid of the two and, with a flat
prior on the grid, normalised per realisation.  The coverage of the credible regions is the check that the posteriors are
calibrated: the true grid point should lie inside the x % highest-posterior-density region of x % of the realisations.

    python examples/lnl_grid_posterior.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import configure_engine, headline_array                      # synthetic array with the NANOGrav 15-yr noise dictionary's shape
from pta_replicator_amd.engine import ReplicaEngine

P, N, R = 24, 2000, 2048
TRUE_A, TRUE_G = -14.0, 13. / 3.
psrs, noise = headline_array(P, N)
eng = configure_engine(ReplicaEngine(psrs, seed=21), noise)
eng.set_gwb(TRUE_A, TRUE_G, no_correlations=True)                      # the likelihood's common process is uncorrelated between pulsars
eng.prepare()
eng.prepare_likelihood(components=14)
axis_A, axis_g = np.linspace(-14.6, -13.4, 25), np.linspace(2.5, 6.0, 15)
grid, shape = eng.theta_grid(gwb_log10_A=axis_A, gwb_gamma=axis_g)      # 375 grid points; red noise as configured
lnl = eng.generate_lnl(R, grid, chunk=1024)["lnl"]                      # [R, G]: the residuals never leave the device
post = torch.softmax(lnl, dim=1)                                        # flat prior on the grid
i_true = int(np.argmin(np.abs(axis_A - TRUE_A))) * len(axis_g) + int(np.argmin(np.abs(axis_g - TRUE_G)))
# HPD level of the true point: the posterior mass of all grid points that are more probable than it
level = (post * (post > post[:, i_true:i_true + 1])).sum(dim=1).cpu().numpy()
post = post.reshape(R, *shape)
mean_A = (post.sum(dim=2).cpu().numpy() * axis_A[None, :]).sum(axis=1)
mean_g = (post.sum(dim=1).cpu().numpy() * axis_g[None, :]).sum(axis=1)
print(f"{P} pulsars x {N} TOAs, {R} realisations, common process at ({TRUE_A}, {TRUE_G:.3f}), grid {shape[0]} x {shape[1]}")
print(f"  posterior mean log10_A {mean_A.mean():.3f} +- {mean_A.std():.3f} (scatter over realisations), gamma {mean_g.mean():.3f} +- {mean_g.std():.3f}")
for x in (0.5, 0.68, 0.9, 0.95):
    print(f"  truth inside the {100 * x:.0f} % HPD region of {100 * np.mean(level <= x):.1f} % of the realisations")
