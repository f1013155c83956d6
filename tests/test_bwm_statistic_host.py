"""CPU checks of the host half of the burst-with-memory matched filter (pta_replicator_amd/bwm_statistic.py) against dense NumPy:
explicit C_a, np.linalg.inv, the timing model projected out.  No GPU."""
import numpy as np
import pytest

T0_MJD = np.array([53100.0, 54000.0, 55250.0, 56500.0])
SKY = (np.array([-0.71, -0.2, 0.05, 0.44, 0.83]), np.array([0.3, 1.9, 3.3, 4.4, 5.8]))    # tests/test_gpu_fstat.py's grid


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def dense_projector(t, sigma2, F=None, phi=None, M=None):
    """P^-1 [N, N] of one pulsar: C = diag(sigma2) + F diag(phi) F^T inverted densely, the timing model M projected out"""
    C = np.diag(np.asarray(sigma2, dtype=np.float64))
    if F is not None:
        C = C + (F * phi[None, :]) @ F.T
    Ci = np.linalg.inv(C)
    if M is not None:
        CiM = Ci @ M
        Ci = Ci - CiM @ np.linalg.solve(M.T @ CiM, CiM.T)
    return 0.5 * (Ci + Ci.T)


def antenna(phat, cos_t, phi):
    """(F+, Fx) of one pulsar at one sky point, written out as deterministic.add_gw_memory does"""
    th = np.arccos(cos_t)
    m = np.array([np.sin(phi), -np.cos(phi), 0.0])
    n = np.array([-np.cos(th) * np.cos(phi), -np.cos(th) * np.sin(phi), np.sin(th)])
    om = np.array([-np.sin(th) * np.cos(phi), -np.sin(th) * np.sin(phi), -np.cos(th)])
    d = 1 + om @ phat
    return np.array([0.5 * ((m @ phat) ** 2 - (n @ phat) ** 2) / d, (m @ phat) * (n @ phat) / d])


def dense_bwm(Pinv, toas, phat, t0_s, sky, rows=None):
    """W (list of [J, N_a]), g [P, J], M [J, S, 2, 2] and, for rows [R, sum N_a], Fb [R, J, S] and A [R, J, S, 2] - pulsar by pulsar,
    epoch by epoch, sky point by sky point"""
    P, J, S = len(toas), len(t0_s), len(sky[0])
    off = np.concatenate([[0], np.cumsum([len(t) for t in toas])])
    W, g = [], np.zeros((P, J))
    for a in range(P):
        E = np.maximum(toas[a][:, None] - t0_s[None, :], 0.0)
        PE = Pinv[a] @ E
        W.append(PE.T)
        g[a] = np.einsum("ij,ij->j", E, PE)
    ph = np.array([[antenna(phat[a], sky[0][s], sky[1][s]) for s in range(S)] for a in range(P)])   # [P, S, 2]
    M = np.zeros((J, S, 2, 2))
    for j in range(J):
        for s in range(S):
            for a in range(P):
                M[j, s] += np.outer(ph[a, s], ph[a, s]) * g[a, j]
    if rows is None:
        return W, g, M
    R = rows.shape[0]
    fb, amp = np.zeros((R, J, S)), np.zeros((R, J, S, 2))
    q = [rows[:, off[a]:off[a + 1]] @ W[a].T for a in range(P)]      # [R, J] each
    for j in range(J):
        for s in range(S):
            N = sum(q[a][:, j, None] * ph[a, s][None, :] for a in range(P))
            A = np.linalg.solve(M[j, s], N.T).T
            fb[:, j, s], amp[:, j, s] = 0.5 * np.einsum("rp,rp->r", N, A), A
    return W, g, M, fb, amp


def _array(seed=11, late=()):
    """6 pulsars of 150 + 37 a TOAs over MJD 53000 - 57500, white noise and 20-component red noise, spin-down timing model; pulsars in
    `late` lose their TOAs before MJD 54500"""
    from pta_replicator_amd import optimal_statistic as ost
    from pta_replicator_amd.simulate import timing_design_matrix
    rng = np.random.default_rng(seed)
    toas, sigma2, F_rn, phi_rn, M, phat = [], [], [], [], [], []
    for a in range(6):
        mjd = np.sort(rng.uniform(53000, 57500, 150 + 37 * a))
        if a in late:
            mjd = mjd[mjd >= 54500]
        t = mjd * 86400.0
        T = t.max() - t.min()
        toas.append(t)
        sigma2.append(rng.uniform(0.3e-6, 0.8e-6, len(t)) ** 2)
        F_rn.append(ost.fourier_basis(t, 20, T))
        phi_rn.append(10.0 ** (2 * (-14.0 + 0.1 * a)) * ost.unit_spectrum(20, T, 3.0 + 0.2 * (a % 4)))
        M.append(timing_design_matrix(t, model="spin")[0])
        c, p = rng.uniform(-1, 1), rng.uniform(0, 2 * np.pi)
        phat.append([np.sqrt(1 - c * c) * np.cos(p), np.sqrt(1 - c * c) * np.sin(p), c])
    return toas, sigma2, F_rn, phi_rn, M, np.array(phat)


@pytest.fixture(scope="module")
def setup():
    from pta_replicator_amd import bwm_statistic as bst
    toas, sigma2, F_rn, phi_rn, M, phat = _array()
    plan = bst.prepare(toas, sigma2, T0_MJD * 86400.0, phat, SKY, F_rn=F_rn, phi_rn=phi_rn, M=M)
    Pinv = [dense_projector(toas[a], sigma2[a], F_rn[a], phi_rn[a], M[a]) for a in range(6)]
    return plan, Pinv, toas, sigma2, phat


def test_operands_match_dense_numpy(setup):
    plan, Pinv, toas, sigma2, phat = setup
    W, g, M = dense_bwm(Pinv, toas, phat, plan.t0_s, SKY)
    white = np.array([[np.sum(np.maximum(toas[a] - t0, 0.0) ** 2 / sigma2[a]) for t0 in plan.t0_s] for a in range(6)])
    Mn = plan.M / np.sqrt(np.einsum("jspp,jsqq->jspq", plan.M, plan.M))
    ev = np.linalg.eigvalsh(Mn)
    print(f"test grid: g / white >= {np.min(plan.g / white):.3g}, normalised M eigenvalue ratio >= {np.min(ev[..., 0] / ev[..., -1]):.3g}")
    assert np.min(plan.g / white) > 1e-9 and np.min(ev[..., 0] / ev[..., -1]) > 1e-6     # far from the 1e-12 refusal
    errs = [rel(np.concatenate(plan.W, axis=1), np.concatenate(W, axis=1)), rel(plan.g, g), rel(plan.M, M)]
    print("W, g, M against dense NumPy: rel = " + ", ".join(f"{e:.2e}" for e in errs))
    assert max(errs) <= 1e-9
    assert plan.C == 4 and plan.Wt().shape == (4, sum(len(t) for t in toas))
    assert plan.Minv_packed().shape == (4, 5, 3)
    assert rel(np.einsum("jspq,jsqr->jspr", plan.Minv, plan.M), np.broadcast_to(np.eye(2), (4, 5, 2, 2))) < 1e-9


def test_rows_match_dense_numpy_and_odd_grid_pads(setup):
    from pta_replicator_amd import bwm_statistic as bst
    plan, Pinv, toas, sigma2, phat = setup
    rng = np.random.default_rng(2)
    rows = rng.normal(size=(7, int(plan.off[-1]))) * 1e-6
    fb, amp = bst.bwm_from_rows(plan, rows)
    _, _, _, fbd, ampd = dense_bwm(Pinv, toas, phat, plan.t0_s, SKY, rows)
    print(f"Fb rel = {rel(fb, fbd):.2e}, A rel = {rel(amp, ampd):.2e}")
    assert fb.shape == (7, 4, 5) and amp.shape == (7, 4, 5, 2) and rel(fb, fbd) <= 1e-9 and rel(amp, ampd) <= 1e-9
    assert np.all(fb >= 0)
    odd = bst.prepare(toas, sigma2, plan.t0_s[:3], phat, SKY, M=[None] * 6)
    Wt = odd.Wt()
    assert odd.J == 3 and odd.C == 4 and Wt.shape[0] == 4 and np.all(Wt[3] == 0) and np.any(Wt[2] != 0)


def test_noiseless_ramp_identity(setup):
    """a noiseless ramp at grid point (j*, s*): Fb = rho^2 / 2 against the dense rho^2 and A = (h cos 2psi, h sin 2psi), to 1e-10
    (measured: Fb 2.1e-11 against the dense rho^2, A 1.5e-15), and no other cell exceeds it."""
    from pta_replicator_amd import bwm_statistic as bst
    plan, Pinv, toas, _, phat = setup
    worst_f = worst_a = 0.0
    for js, ss, h, psi in ((2, 3, 3e-14, 0.9), (0, 0, 1e-15, 2.5), (3, 4, 2e-13, 0.1)):
        sig = [h * (np.cos(2 * psi) * f[0] + np.sin(2 * psi) * f[1]) * np.maximum(toas[a] - plan.t0_s[js], 0.0)
               for a, f in enumerate(antenna(phat[a], SKY[0][ss], SKY[1][ss]) for a in range(6))]
        rho2 = sum(s @ Pinv[a] @ s for a, s in enumerate(sig))
        fb, amp = bst.bwm_from_rows(plan, np.concatenate(sig)[None, :])
        want = h * np.array([np.cos(2 * psi), np.sin(2 * psi)])
        worst_f = max(worst_f, abs(fb[0, js, ss] / (0.5 * rho2) - 1))
        worst_a = max(worst_a, float(np.max(np.abs(amp[0, js, ss] - want)) / h))
        assert np.unravel_index(np.argmax(fb[0]), fb[0].shape) == (js, ss)
    print(f"identity: |Fb / (rho^2 / 2) - 1| <= {worst_f:.2e}, |A - (h cos 2psi, h sin 2psi)| / h <= {worst_a:.2e}")
    assert worst_f <= 1e-10 and worst_a <= 1e-10


def test_epochs_outside_every_span_are_refused():
    from pta_replicator_amd import bwm_statistic as bst
    toas, sigma2, F_rn, phi_rn, M, phat = _array()
    for t0, j in (([52900.0, 57600.0], 0), ([54000.0, 57600.0], 1), ([52900.0], 0)):
        with pytest.raises(ValueError, match=rf"singular at epoch {j} \(MJD {t0[j]:.6f}\), sky point 0"):
            bst.prepare(toas, sigma2, np.array(t0) * 86400.0, phat, SKY, F_rn=F_rn, phi_rn=phi_rn, M=M)
    with pytest.raises(ValueError, match="two pulsars"):
        bst.prepare(toas[:1], sigma2[:1], T0_MJD * 86400.0, phat[:1], SKY)
    with pytest.raises(ValueError, match="sky grid"):
        bst.prepare(toas, sigma2, T0_MJD * 86400.0, phat, None)
    with pytest.raises(ValueError, match="finite"):
        bst.prepare(toas, sigma2, np.array([np.nan]), phat, SKY)


def test_insensitive_pulsars_get_exactly_zero_rows():
    """an epoch before the data of pulsars 4 and 5 alone: accepted, their W rows and g exactly zero, the others' unchanged"""
    from pta_replicator_amd import bwm_statistic as bst
    toas, sigma2, F_rn, phi_rn, M, phat = _array(late=(4, 5))
    t0 = np.array([54000.0, 55250.0]) * 86400.0
    assert all(toas[a].min() > t0[0] for a in (4, 5)) and all(toas[a].min() < t0[0] for a in range(4))
    plan = bst.prepare(toas, sigma2, t0, phat, SKY, F_rn=F_rn, phi_rn=phi_rn, M=M)
    for a in range(6):
        gone = a >= 4
        assert np.all(plan.W[a][0] == 0) == gone and (plan.g[a, 0] == 0) == gone, a
        assert np.any(plan.W[a][1] != 0) and plan.g[a, 1] > 0, a
    Pinv = [dense_projector(toas[a], sigma2[a], F_rn[a], phi_rn[a], M[a]) for a in range(6)]
    _, g, Md = dense_bwm(Pinv, toas, phat, t0, SKY)
    white = np.array([np.sum((toas[a] - t0[0]) ** 2 / sigma2[a]) for a in (4, 5)])
    print("dense g / white of the absorbed ramps:", g[4:, 0] / white)
    assert np.all(np.abs(g[4:, 0]) <= 1e-12 * white)
    assert rel(plan.M, Md) <= 1e-9
