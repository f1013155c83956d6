"""Generate tests/golden/aniso_basis_p81_l4.npz: the spherical-harmonic ORF basis of 81 random pulsar positions up to l = 4 from the
pure-Python oracle (oracle.pta_oracle.correlated_basis, 20 s), so that the GPU tests of the per-realisation ORF factor
(tests/test_gpu_gwb_anisotropy.py) have the oracle's basis at P = 68 and 81 without recomputing it.  The basis of the first P pulsars
up to lmax is the sub-array [:(lmax+1)^2, :P, :P].  tests/test_gwb_anisotropy_host.py re-derives a sample of pairs from the oracle.

    python scripts/gen_aniso_basis_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import pta_oracle as po  # noqa: E402

P, LMAX, SEED = 81, 4, 20


def main():
    rng = np.random.default_rng(SEED)
    locs = np.stack([rng.uniform(0, 2 * np.pi, P), np.arccos(rng.uniform(-1, 1, P))], axis=1)   # (phi, colatitude), isotropic
    basis = np.array(po.correlated_basis(locs, LMAX))
    assert np.array_equal(basis, basis.transpose(0, 2, 1))
    iu = np.triu_indices(P)
    out = os.path.join(ROOT, "tests", "golden", "aniso_basis_p81_l4.npz")
    np.savez_compressed(out, locs=locs, tri=basis[:, iu[0], iu[1]], lmax=LMAX)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
