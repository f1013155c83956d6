"""Realisations with their own noise model each: 68 synthetic pulsars x 5000 TOAs, HD GWB + RN + white noise, with the GWB
(log10_A, gamma) and the red noise (log10_A, gamma) of all 68 pulsars drawn per realisation from uniform priors on the GPU - a
training set for simulation-based inference, labels included.

    python examples/ensemble_sampled.py
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
eng.prepare()

# uniform boxes; white noise and ECORR stay as configured.  A pulsar without red noise in the dictionary keeps none (label NaN)
eng.set_hyper_prior(gwb_log10_A=(-15.5, -13.5), gwb_gamma=(2.0, 6.0), rn_log10_A=(-16.0, -12.5), rn_gamma=(0.5, 6.5))

n_batch, R = 4, 1024
features, labels = [], []
for b in range(n_batch):
    res, theta = eng.generate_sampled(R, r0=b * R)     # [R, 340000] seconds on the device, theta: dict of device tensors
    # a stand-in for the summary a pipeline would compute on the device: per-pulsar residual RMS
    rms = torch.stack([seg.square().mean(dim=1).sqrt() for seg in eng.split(res)], dim=1)
    features.append(rms.cpu().numpy())
    labels.append(np.concatenate([theta["gwb_log10_A"][:, None].cpu().numpy(), theta["gwb_gamma"][:, None].cpu().numpy()], axis=1))
features, labels = np.concatenate(features), np.concatenate(labels)
print(f"{len(features)} realisations, features {features.shape}, GWB labels {labels.shape}")
print("log10 median RMS vs gwb_log10_A correlation:", round(float(np.corrcoef(np.log10(np.median(features, axis=1)), labels[:, 0])[0, 1]), 3))

# realisation r and its theta are pure functions of (seed, r): regenerating one realisation alone gives the same numbers
one, th1 = eng.generate_sampled(1, r0=5)
again, _ = eng.generate_sampled(8, r0=0)
assert torch.equal(one[0], again[5]) and float(th1["gwb_gamma"][0]) == float(labels[5, 1])
print("realisation 5 regenerated alone: identical")
