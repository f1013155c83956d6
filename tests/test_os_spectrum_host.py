"""Host half of the per-frequency optimal statistic (optimal_statistic.pair_blocks, spectrum_fisher, spectrum_from_rows,
matched_spectrum_from_XZ): the blocks against brute-force selector matrices, the sum rule against the broadband OS, narrowband
against a diagonal Fisher matrix, independence of the template's index, a Monte Carlo on exact-model data, and the block <-> packed
triangle map of csrc/pta_os_spectrum.h compiled with g++.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from pta_replicator_amd import optimal_statistic as ost
from pta_replicator_amd.simulate import timing_design_matrix
from test_os_host import _array, _pos, _prepare, _rn_inputs

HERE = os.path.dirname(os.path.abspath(__file__))


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(np.asarray(b))))


CASES = [(5, 1), (5, 5), (6, 6)]     # (pulsars, n_f)


@pytest.mark.parametrize("P,nf", CASES)
def test_blocks_and_fisher_vs_selector_matrices(P, nf):
    arr = _array(P=P, seed=3 + P)
    plan = _prepare(arr, nf, "spin", 10 ** (2 * -14.3))
    C = 2 * nf
    sel = np.zeros((nf, C, C))
    for k in range(nf):
        sel[k, 2 * k, 2 * k] = sel[k, 2 * k + 1, 2 * k + 1] = 1.0
    D = ost.pair_blocks(plan.Z, plan.pair_a, plan.pair_b)
    ref = np.zeros_like(D)
    for p, (a, b) in enumerate(zip(plan.pair_a, plan.pair_b)):
        for k in range(nf):
            for j in range(nf):
                ref[p, k, j] = np.trace(sel[k] @ plan.Z[a] @ sel[j] @ plan.Z[b])
    assert D.shape == (len(plan.pair_a), nf, nf)
    assert _rel(D, ref) < 1e-12
    assert _rel(D.sum(axis=(1, 2)), plan.den) < 1e-12
    F = ost.spectrum_fisher(plan)
    assert F.shape == (len(plan.names), nf, nf)
    assert _rel(F, np.einsum("op,pkj->okj", plan.G ** 2, ref)) < 1e-12
    assert _rel(F.sum(axis=(1, 2)), plan.G ** 2 @ plan.den) < 1e-12
    assert np.allclose(F, np.swapaxes(F, 1, 2), rtol=0, atol=1e-14 * np.max(np.abs(F)))
    assert np.all(np.linalg.eigvalsh(D) > -1e-12 * np.max(np.abs(D)))          # every pair's block matrix is PSD


@pytest.mark.parametrize("P,nf", CASES)
def test_sum_rule_and_narrowband(P, nf):
    arr = _array(P=P, seed=5)
    plan = _prepare(arr, nf, "astrometric", 10 ** (2 * -14.5))
    rows = np.random.default_rng(2).normal(0, 1e-7, (9, int(plan.off[-1])))
    A2 = ost.os_from_rows(plan, rows)[0]
    full = ost.spectrum_from_rows(plan, rows)
    F = full["fisher"]
    one = np.ones(nf)
    assert _rel(np.einsum("okj,roj->ro", F, full["a2"]) / (F @ one @ one)[None, :], A2) < 1e-10
    assert _rel(full["b"].sum(axis=2) / (F @ one @ one)[None, :], A2) < 1e-10
    nb = ost.spectrum_from_rows(plan, rows, mode="narrowband")
    Fd = F * np.eye(nf)
    a2d, sgd = ost.spectrum_solve(Fd, full["b"], "full")
    assert _rel(nb["a2"], a2d) < 1e-13 and _rel(nb["sigma"], sgd) < 1e-13
    assert full["sigma"].shape == (len(plan.names), nf) and full["a2"].shape == (9, len(plan.names), nf)
    assert np.allclose(full["freqs"], np.arange(1, nf + 1) / plan.T, rtol=1e-15)
    # the two forms of the solve, and the matched evaluation on the fixed plan's own Z
    alt = ost.spectrum_solve(F, full["b"], "full", form="solve")
    assert _rel(alt[0], full["a2"]) < 1e-9 and _rel(alt[1], full["sigma"]) < 1e-9
    Y = ost.project(plan, rows)
    i, j = np.tril_indices(2 * nf)
    for Z in (np.broadcast_to(plan.Z, (9,) + plan.Z.shape), np.broadcast_to(plan.Z[:, i, j], (9, P, len(i)))):
        m = ost.matched_spectrum_from_XZ(plan, Y, Z)
        assert _rel(m["a2"], full["a2"]) < 1e-12 and _rel(m["sigma"][4], full["sigma"]) < 1e-12 and _rel(m["phi"], full["phi"]) < 1e-12


def test_not_positive_definite():
    arr = _array(P=5)
    plan = _prepare(arr, 4, "spin", 0.0)
    F = ost.spectrum_fisher(plan)
    bad = F.copy()
    bad[1] = -bad[1]
    a2, sg = ost.spectrum_solve(bad, np.ones((3, 3, 4)))
    assert np.all(np.isnan(a2[:, 1])) and np.all(np.isnan(sg[1])) and np.all(np.isfinite(a2[:, [0, 2]]))
    bad[1] = np.ones((4, 4))             # positive diagonal, rank one
    a2, sg = ost.spectrum_solve(bad, np.ones((3, 3, 4)))
    assert np.all(np.isnan(a2[:, 1])) and np.all(np.isfinite(a2[:, [0, 2]]))
    plan.G = plan.G.copy()
    plan.G[2] = 0.0
    with pytest.raises(ValueError, match="not positive definite"):
        ost.spectrum_fisher(plan)
    with pytest.raises(ValueError, match="mode"):
        ost.spectrum_solve(F, np.ones(4), mode="wide")


def test_phi_does_not_depend_on_the_template_index():
    arr = _array(P=6, seed=5)
    nf = 6
    rn = [_rn_inputs(p) for p in arr]
    rows = np.random.default_rng(7).normal(0, 2e-7, (5, sum(len(p["t"]) for p in arr)))
    res = []
    for gamma in (13. / 3., 2.0):
        plan = ost.prepare([p["t"] for p in arr], [p["sigma2"] for p in arr], _pos(arr), components=nf, gamma=gamma,
                           epoch_of=[p["epoch_of"] for p in arr], ecorr=[p["ecorr"] for p in arr], F_rn=[x[0] for x in rn],
                           phi_rn=[x[1] for x in rn], gw_amp2=0.0, M=[timing_design_matrix(p["t"], model="spin")[0] for p in arr])
        res.append(ost.spectrum_from_rows(plan, rows))
    dev = np.abs(res[0]["phi"] - res[1]["phi"]) / res[0]["phi_sigma"][None]
    print("largest |phi(13/3) - phi(2)| / phi_sigma:", dev.max())
    assert dev.max() < 1e-8
    assert _rel(res[1]["phi_sigma"], res[0]["phi_sigma"]) < 1e-8
    assert _rel(res[1]["a2"], res[0]["a2"]) > 0.5          # a2 itself follows the template


# ---------------------------------------------------------------- Monte Carlo on exact-model data ----------------------------
R_MC, P_MC, NF_MC = 4000, 10, 6
PHI_TRUE = np.array([3.0, 0.6, 1.8, 0.25, 0.9, 0.4]) * 1e-14      # s^2 per sin / cos coefficient, non-monotonic


@pytest.fixture(scope="module")
def mc():
    """white noise + coefficients of variance PHI_TRUE in the basis F (HD-correlated between pulsars, or not), a quadratic timing
    model; the noise model holds the GW auto-term as a red process in the same basis, so it is the data covariance exactly"""
    rng = np.random.default_rng(12)
    counts = 60 + 7 * np.arange(P_MC)
    toas = [np.sort(rng.uniform(0, 4.0e8, n)) for n in counts]
    sigma2 = [np.full(n, (2e-7) ** 2) * rng.uniform(0.5, 1.5, n) for n in counts]
    z, ph = rng.uniform(-1, 1, P_MC), rng.uniform(0, 2 * np.pi, P_MC)
    pos = np.stack([np.sqrt(1 - z ** 2) * np.cos(ph), np.sqrt(1 - z ** 2) * np.sin(ph), z], axis=1)
    T = max(t.max() for t in toas) - min(t.min() for t in toas)
    Fs = [ost.fourier_basis(t, NF_MC, T) for t in toas]
    phi2 = np.repeat(PHI_TRUE, 2)
    plan = ost.prepare(toas, sigma2, pos, components=NF_MC, orfs=("hd",), F_rn=Fs, phi_rn=[phi2] * P_MC, gw_amp2=0.0,
                       M=[timing_design_matrix(t, model="spin")[0] for t in toas], T=T)
    gam = np.zeros((P_MC, P_MC))
    gam[plan.pair_a, plan.pair_b] = plan.G[0]
    gam = gam + gam.T + np.eye(P_MC)                              # HD with the pulsar term: 1 on the diagonal
    out = {}
    for name, Lc in (("signal", np.linalg.cholesky(gam)), ("null", np.eye(P_MC))):
        c = np.einsum("ab,rbc->rac", Lc, rng.normal(size=(R_MC, P_MC, 2 * NF_MC))) * np.sqrt(phi2)
        rows = np.concatenate([c[:, a] @ Fs[a].T + rng.normal(size=(R_MC, counts[a])) * np.sqrt(sigma2[a]) for a in range(P_MC)], axis=1)
        out[name] = rows
    return plan, out


@pytest.mark.parametrize("mode", ["full", "narrowband"])
def test_monte_carlo_null_is_calibrated(mc, mode):
    plan, rows = mc
    snr = ost.spectrum_from_rows(plan, rows["null"], mode)["snr"][:, 0]
    m, s = snr.mean(axis=0), snr.std(axis=0)
    print(f"{mode}: null snr mean", m, "std", s)
    assert np.all(np.abs(m) < 5 / np.sqrt(R_MC)), m
    assert np.all((s > 0.94) & (s < 1.06)), s


def test_monte_carlo_recovers_the_spectrum(mc):
    plan, rows = mc
    phi = ost.spectrum_from_rows(plan, rows["signal"])["phi"][:, 0]
    ratio, err = phi.mean(axis=0) / PHI_TRUE, phi.std(axis=0) / np.sqrt(R_MC) / PHI_TRUE
    print("mean(phi) / phi_true", ratio, "+-", err)
    assert np.all(np.abs(ratio - 1) < 5 * err), (ratio, err)


# ---------------------------------------------------------------- device index header ----------------------------------------
@pytest.fixture(scope="module")
def osp(tmp_path_factory):
    out = tmp_path_factory.mktemp("os_spectrum") / "libosspectrumhost.so"
    src = os.path.join(HERE, "os_spectrum", "os_spectrum_host.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", str(out)])
    lib = ctypes.CDLL(str(out))
    lib.osp_blocks.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int32)]
    lib.osp_blocks.restype = ctypes.c_int
    return lib


@pytest.mark.parametrize("C", [2, 6, 28, 64])
def test_block_index_header_matches_numpy(osp, C):
    nf = C // 2
    nb = nf * (nf + 1) // 2
    out = np.full(6 * nb, -1, dtype=np.int32)
    assert osp.osp_blocks(C, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) == nb
    out = out.reshape(nb, 6)
    kk, jj = np.tril_indices(nf)                                  # blocks in ascending k, then j <= k
    assert np.array_equal(out[:, 0], kk) and np.array_equal(out[:, 1], jj)
    packed = np.zeros((C, C), dtype=np.int64)
    ti, tj = np.tril_indices(C)
    packed[ti, tj] = packed[tj, ti] = np.arange(len(ti))
    for e in range(nb):
        k, j = kk[e], jj[e]
        ref = sorted(packed[i, l] for i in (2 * k, 2 * k + 1) for l in (2 * j, 2 * j + 1))
        assert sorted(out[e, 2:]) == ref, (k, j)
    assert out[:, 2:].min() >= 0 and out[:, 2:].max() == C * (C + 1) // 2 - 1
    # the four products per block give pair_blocks of the unpacked matrices
    rng = np.random.default_rng(C)
    Zp = rng.normal(size=(2, C * (C + 1) // 2))
    D = (Zp[0][out[:, 2:]] * Zp[1][out[:, 2:]]).sum(axis=1)
    ref = ost.pair_blocks(ost.unpack_triangle(Zp, C), np.array([0]), np.array([1]))[0]
    assert _rel(D, ref[kk, jj]) < 1e-14
