"""A continuous-wave training set: 68 synthetic pulsars x 5000 TOAs with the NANOGrav 15-yr noise dictionary's noise and HD GWB, plus one
circular supermassive-binary source per realisation drawn on the GPU (isotropic sky and orientation, log10 mc, log10 fgw and log10 h
from uniform boxes), written as residuals + labels.  tref is the array's first TOA.

    python examples/cw_sampled.py [out.npz]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bench import configure_engine, headline_array                      # synthetic array with the NANOGrav 15-yr noise dictionary's shape
from pta_replicator_amd.engine import ReplicaEngine

out_path = sys.argv[1] if len(sys.argv) > 1 else "cw_training_set.npz"
psrs, noise = headline_array(68, 5000)
eng = ReplicaEngine(psrs, seed=2026)
configure_engine(eng, noise)   # per-backend EFAC / EQUAD / ECORR, per-pulsar RN, HD GWB: values of ng15_dict.json
tref = float(min(m.min() for m in eng.mjd)) * 86400.0
eng.set_cw(psrTerm=True, evolve=True, tref=tref, pdist=1.0)
eng.set_cw_prior(log10_mc=(8.0, 10.0), log10_fgw=(-9.0, -7.5), log10_h=(-15.5, -13.5))

n_batch, R, keep = 2, 1024, 64
res_out, labels = [], []
for b in range(n_batch):
    res, theta = eng.generate_sampled(R, r0=b * R)      # [R, 340000] seconds on the device, theta: dict of device tensors
    res_out.append(res[:keep].to(torch.float32).cpu().numpy())   # a slice of each batch, to keep the file small
    labels.append({k: v[:keep].cpu().numpy() for k, v in theta.items() if k.startswith("cw_")})
lab = {k: np.concatenate([d[k] for d in labels]) for k in labels[0]}
np.savez(out_path, residuals=np.concatenate(res_out), off=eng.off, **lab)
print(f"wrote {out_path}: residuals {np.concatenate(res_out).shape}, labels {sorted(lab)}")

# the CW term alone of the first realisations, and a check that the labels reproduce the residuals exactly
sig = eng.generate_per_signal(4, theta={k: torch.as_tensor(v[:4], device="cuda") for k, v in lab.items()})
print("CW term RMS of the first 4 realisations [ns]:", np.round(sig["cw"].square().mean(dim=1).sqrt().cpu().numpy() * 1e9, 3))
again = eng.generate(4, r0=0, theta={k: torch.as_tensor(v[:4], device="cuda") for k, v in lab.items()})
first, _ = eng.generate_sampled(4, r0=0)
assert torch.equal(again, first)
print("labels reproduce the sampled realisations: identical")
