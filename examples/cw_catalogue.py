"""A catalogue of continuous-wave sources per realisation: 68 synthetic pulsars x 5000 TOAs with the NANOGrav 15-yr noise dictionary's
noise and HD GWB, and on top of every realisation its own set of circular supermassive-binary sources, summed on the GPU in one pass.

  1. an explicit catalogue from theta: every realisation brings up to S sources (cw_* keys of shape [R, S]) and says how many of them
     it uses (cw_count [R]) - what a population synthesis hands over after picking each universe's loudest binaries;
  2. a sampled one: set_cw_prior(n_sources=S) draws S sources per realisation on the GPU, labels returned with the residuals.

    python examples/cw_catalogue.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bench import configure_engine, headline_array                      # synthetic array with the NANOGrav 15-yr noise dictionary's shape
from pta_replicator_amd.engine import ReplicaEngine

psrs, noise = headline_array(68, 5000)
eng = ReplicaEngine(psrs, seed=2026)
configure_engine(eng, noise)   # per-backend EFAC / EQUAD / ECORR, per-pulsar RN, HD GWB: values of ng15_dict.json
tref = float(min(m.min() for m in eng.mjd)) * 86400.0
eng.set_cw(psrTerm=True, evolve=True, tref=tref, pdist=1.0)

# ---- 1. an explicit catalogue -------------------------------------------------------------------------------------------------
R, S = 256, 16
rng = np.random.default_rng(7)
count = rng.poisson(6.0, R).clip(0, S)                      # outliers per universe; entries past the count are never read
theta = {
    "cw_cos_gwtheta": rng.uniform(-1, 1, (R, S)), "cw_gwphi": rng.uniform(0, 2 * np.pi, (R, S)),
    "cw_log10_mc": rng.uniform(8.5, 10.0, (R, S)), "cw_log10_fgw": rng.uniform(-9.0, -7.5, (R, S)),
    "cw_log10_dist": rng.uniform(1.5, 3.0, (R, S)),           # [Mpc]; cw_log10_h (strain) is the alternative
    "cw_phase0": rng.uniform(0, 2 * np.pi, (R, S)), "cw_psi": rng.uniform(0, np.pi, (R, S)), "cw_cos_inc": rng.uniform(-1, 1, (R, S)),
    "cw_count": count,
}
res = eng.generate(R, theta=theta)                            # [R, 340000] seconds on the device
sig = eng.generate_per_signal(8, theta={k: v[:8] for k, v in theta.items()})
rms = sig["cw"].square().mean(dim=1).sqrt().cpu().numpy() * 1e9
print("sources per realisation:", count[:8], " catalogue RMS [ns]:", np.round(rms, 3))
assert torch.equal(res[:8], eng.generate(8) + sig["cw"])     # the catalogue's sum is formed first and added once
assert torch.equal(res[count == 0], eng.generate(R)[count == 0])

# ---- 2. a sampled catalogue ---------------------------------------------------------------------------------------------------
eng.set_cw_prior(log10_mc=(8.0, 10.0), log10_fgw=(-9.0, -7.5), log10_h=(-15.5, -13.5), n_sources=8)
res, labels = eng.generate_sampled(1024)                      # labels: cw_* device tensors of shape [1024, 8]
print("labels:", {k: tuple(v.shape) for k, v in labels.items()})
assert torch.equal(eng.generate(4, r0=100, theta={k: v[100:104] for k, v in labels.items()}), res[100:104])
print("labels reproduce the sampled realisations: identical")
