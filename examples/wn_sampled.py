"""White noise as a nuisance parameter: 68 synthetic pulsars x 5000 TOAs, HD GWB + RN + white noise, with EFAC, EQUAD and ECORR of
every backend of every pulsar drawn per realisation from uniform priors on the GPU next to the GWB amplitude - a training set in
which the per-backend white-noise parameters vary as they do over a posterior, labels included, from one prepare().

    python examples/wn_sampled.py
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

# the groups the white-noise keys address: (pulsar index, backend flag), pulsar-major
print(f"{len(eng.wn_groups)} white-noise groups, {len(eng.ecorr_groups)} ECORR groups; pulsar 0: {[f for a, f in eng.wn_groups if a == 0]}")

# uniform boxes, one for all groups (or one per group: an array [G, 2]); red noise stays as configured
eng.set_hyper_prior(gwb_log10_A=(-15.5, -13.5), wn_efac=(0.7, 1.5), wn_log10_equad=(-8.0, -6.0), wn_log10_ecorr=(-8.0, -6.0))

R = 1024
res, theta = eng.generate_sampled(R)     # [R, 340000] seconds on the device, theta: dict of device tensors, the labels
print({k: tuple(v.shape) for k, v in theta.items()})

# the white-noise level of a pulsar follows its labels: RMS of the white part against the EFAC of its first backend
sig = eng.generate_per_signal(8, theta={k: v[:8] for k, v in theta.items()})
a = 0
wn_rms = eng.split(sig["wn"])[a].square().mean(dim=1).sqrt().cpu().numpy()
print("pulsar 0, white-noise RMS [us] of realisations 0..7:", np.round(wn_rms * 1e6, 3))
print("           EFAC of its first backend:               ", np.round(theta["wn_efac"][:8, 0].cpu().numpy(), 3))

# theta can also be given: NaN keeps a group as configured, a key that is left out keeps its parameter as configured
efac = np.full((4, len(eng.wn_groups)), np.nan)
efac[:, 0] = [0.5, 1.0, 2.0, 4.0]          # only the first backend of pulsar 0 varies
rows = eng.generate_per_signal(4, theta={"wn_efac": efac})["wn"]
first = np.array([f["f"] for f in psrs[0].toas.table["flags"].data]) == eng.wn_groups[0][1]
rms = rows[:, :eng.counts[0]][:, torch.as_tensor(first, device=rows.device)].square().mean(dim=1).sqrt().cpu().numpy()
print("white-noise RMS [us] of that backend for EFAC 0.5, 1, 2, 4:", np.round(rms * 1e6, 3))

# realisation r and its labels are pure functions of (seed, r): regenerating one realisation alone gives the same numbers
one, th1 = eng.generate_sampled(1, r0=5)
assert torch.equal(one[0], res[5]) and torch.equal(th1["wn_log10_ecorr"][0], theta["wn_log10_ecorr"][5])
print("realisation 5 regenerated alone: identical")
