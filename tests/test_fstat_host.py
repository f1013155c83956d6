"""Host preparation of the continuous-wave F-statistics (pta_replicator_amd.f_statistic) against an independent dense NumPy
evaluation (C_a assembled explicitly, np.linalg.solve, explicit projector, explicit antenna patterns), the span identity of Fe and
the refusals.  No GPU."""
import numpy as np
import pytest

from oracle import pta_oracle as po
from pta_replicator_amd import f_statistic as fst
from pta_replicator_amd.simulate import timing_design_matrix

FREQS = np.array([6.1e-9, 1.13e-8, 2.37e-8, 4.71e-8])
SKY = (np.array([-0.71, -0.2, 0.05, 0.44, 0.83]), np.array([0.3, 1.9, 3.3, 4.4, 5.8]))


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(np.asarray(b))))


def _array(P=5, seed=3):
    """a small ragged array: unequal TOA counts, two backends (EFAC / EQUAD / ECORR per backend), red noise on all but one pulsar"""
    rng = np.random.default_rng(seed)
    out = []
    for a in range(P):
        n = 60 + 29 * a + (a % 2)
        sess = np.sort(rng.uniform(53000, 57800, (n + 2) // 3))        # sessions of three TOAs within 0.05 d: ECORR epochs of 0.1 d
        mjd = np.sort(np.repeat(sess, 3)[:n] + rng.uniform(0, 0.05, n))
        be = rng.integers(0, 2, n)
        sig = np.where(be == 0, 0.4e-6, 0.9e-6) * rng.uniform(0.8, 1.2, n)
        efac, equad = np.array([1.1, 0.9])[be], np.array([10 ** -6.6, 10 ** -6.9])[be]
        epoch_of, ne, first, _ = po.quantize(mjd, dt=0.1)
        rn = None if a == 2 else (-14.2 + 0.1 * a, 2.5 + 0.3 * a)
        ra, dec = rng.uniform(0, 2 * np.pi), np.arcsin(rng.uniform(-1, 1))
        out.append(dict(t=mjd * 86400.0, sigma2=(efac * sig) ** 2 + (efac * equad) ** 2, epoch_of=np.asarray(epoch_of),
                        ecorr=np.array([10 ** -6.7, 10 ** -7.0])[be[first]], rn=rn,
                        phat=np.array([np.cos(dec) * np.cos(ra), np.cos(dec) * np.sin(ra), np.sin(dec)])))
    return out


def _rn_inputs(p, components=10):
    if p["rn"] is None:
        return None, None
    T = p["t"].max() - p["t"].min()
    F, freqs = po.fourier_design_matrix(p["t"], nmodes=components, Tspan=T)
    return F, po.red_noise_prior(freqs, p["rn"][0], p["rn"][1], T)


def _prepare(arr, model, freqs=FREQS, sky=SKY):
    rn = [_rn_inputs(p) for p in arr]
    M = None if model is None else [timing_design_matrix(p["t"], model=model)[0] for p in arr]
    return fst.prepare([p["t"] for p in arr], [p["sigma2"] for p in arr], freqs, phat=np.array([p["phat"] for p in arr]), sky=sky,
                       epoch_of=[p["epoch_of"] for p in arr], ecorr=[p["ecorr"] for p in arr], F_rn=[x[0] for x in rn],
                       phi_rn=[x[1] for x in rn], M=M)


def _dense_projectors(arr, model):
    """P_a^-1 by brute force: C_a explicit, inverse through solve, the timing model projected out"""
    out = []
    for p in arr:
        n = len(p["t"])
        C = np.diag(p["sigma2"]).astype(np.float64)
        C += (p["epoch_of"][:, None] == p["epoch_of"][None, :]) * (p["ecorr"][p["epoch_of"]] ** 2)[:, None]
        Frn, phi = _rn_inputs(p)
        if Frn is not None:
            C += (Frn * phi) @ Frn.T
        Pi = np.linalg.solve(C, np.eye(n))
        if model is not None:
            M = timing_design_matrix(p["t"], model=model)[0]
            CiM = Pi @ M
            Pi = Pi - CiM @ np.linalg.solve(M.T @ CiM, CiM.T)
        out.append(0.5 * (Pi + Pi.T))
    return out


def _dense_antenna(phat, cos_t, phi):
    """(F+, Fx) of one pulsar and one sky point from the vectors m, n, Omega written out"""
    th = np.arccos(cos_t)
    m = np.array([np.sin(phi), -np.cos(phi), 0.0])
    n = np.array([-np.cos(th) * np.cos(phi), -np.cos(th) * np.sin(phi), np.sin(th)])
    om = np.array([-np.sin(th) * np.cos(phi), -np.sin(th) * np.sin(phi), -np.cos(th)])
    d = 1 + om @ phat
    return 0.5 * ((m @ phat) ** 2 - (n @ phat) ** 2) / d, (m @ phat) * (n @ phat) / d


def _dense_fstat(arr, Pinv, rows, freqs, sky):
    """(Fp [R, J], Fe [R, J, S], cond(M) [J, S]) pulsar by pulsar, frequency by frequency, sky point by sky point"""
    P, J, S, R = len(arr), len(freqs), len(sky[0]), rows.shape[0]
    off = np.concatenate([[0], np.cumsum([len(p["t"]) for p in arr])])
    fp, fe, cond = np.zeros((R, J)), np.zeros((R, J, S)), np.zeros((J, S))
    for j, f in enumerate(freqs):
        q, G = [], []
        for a, p in enumerate(arr):
            E = np.stack([np.sin(2 * np.pi * f * p["t"]), np.cos(2 * np.pi * f * p["t"])], axis=1)
            q.append(rows[:, off[a]:off[a + 1]] @ (Pinv[a] @ E))
            G.append(E.T @ Pinv[a] @ E)
            fp[:, j] += 0.5 * np.einsum("rk,kl,rl->r", q[a], np.linalg.inv(G[a]), q[a])
        for s in range(S):
            N, M = np.zeros((R, 4)), np.zeros((4, 4))
            for a, p in enumerate(arr):
                ph = np.array(_dense_antenna(p["phat"], sky[0][s], sky[1][s]))
                N += np.kron(ph[None, :], q[a])
                M += np.kron(np.outer(ph, ph), G[a])
            cond[j, s] = np.linalg.cond(M)
            fe[:, j, s] = 0.5 * np.einsum("ru,ru->r", N, np.linalg.solve(M, N.T).T)
    return fp, fe, cond


@pytest.mark.parametrize("model", ["spin", "astrometric"])
def test_plan_matches_dense(model):
    arr = _array()
    plan = _prepare(arr, model)
    Pinv = _dense_projectors(arr, model)
    rng = np.random.default_rng(5)
    rows = rng.normal(size=(7, int(plan.off[-1]))) * 1e-6
    fp_ref, fe_ref, cond = _dense_fstat(arr, Pinv, rows, FREQS, SKY)
    assert cond.max() <= 1e4, cond.max()        # the inputs keep M_js well conditioned: the 1e-10 below is about the plan, not about M
    fp, fe = fst.fstat_from_rows(plan, rows)
    print(f"{model}: max cond(M) = {cond.max():.3g}, Fp rel = {_rel(fp, fp_ref):.2e}, Fe rel = {_rel(fe, fe_ref):.2e}")
    for a, p in enumerate(arr):
        E = fst.cw_basis(p["t"], FREQS)
        assert _rel(plan.W[a], E.T @ Pinv[a]) < 1e-10
    assert _rel(fp, fp_ref) < 1e-10
    assert _rel(fe, fe_ref) < 1e-10
    assert plan.Minv_packed().shape == (len(FREQS), len(SKY[0]), 10) and plan.Ginv_packed().shape == (len(arr), len(FREQS), 3)
    # the packed triangle is the upper triangle, row-major
    assert np.array_equal(plan.Minv_packed()[1, 2], plan.Minv[1, 2][np.triu_indices(4)])


def test_fp_alone_for_one_pulsar():
    arr = _array(P=1)
    plan = _prepare(arr, "spin", sky=None)
    rows = np.random.default_rng(1).normal(size=(3, int(plan.off[-1]))) * 1e-6
    fp, fe = fst.fstat_from_rows(plan, rows)
    assert fe is None and fp.shape == (3, len(FREQS)) and np.all(fp > 0)
    Pinv = _dense_projectors(arr, "spin")
    E = fst.cw_basis(arr[0]["t"], FREQS[:1])
    q = rows @ (Pinv[0] @ E)
    assert _rel(fp[:, 0], 0.5 * np.einsum("rk,kl,rl->r", q, np.linalg.inv(E.T @ Pinv[0] @ E), q)) < 1e-10


@pytest.mark.parametrize("model", ["spin", "astrometric"])
def test_span_identity(model):
    """a signal inside the span of phi_a (x) E_aj* (any polarisation angle mixes + and x, any phase mixes sin and cos) is recovered
    whole: Fe[j*, s*] = 1/2 sum_a s_a^T P_a^-1 s_a, and no other grid point exceeds it"""
    arr = _array()
    plan = _prepare(arr, model)
    Pinv = _dense_projectors(arr, model)
    js, ss = 2, 3
    alpha, beta, psi = 0.7e-7, -1.3e-7, 0.6
    c2, s2 = np.cos(2 * psi), np.sin(2 * psi)
    rows, rho2 = [], 0.0
    for a, p in enumerate(arr):
        Fp_, Fx_ = plan.phi[a, ss]
        wave = alpha * np.sin(2 * np.pi * FREQS[js] * p["t"]) + beta * np.cos(2 * np.pi * FREQS[js] * p["t"])
        wave2 = beta * np.sin(2 * np.pi * FREQS[js] * p["t"]) - 0.4 * alpha * np.cos(2 * np.pi * FREQS[js] * p["t"])
        s_a = (Fp_ * c2 + Fx_ * s2) * wave + (Fx_ * c2 - Fp_ * s2) * wave2
        rows.append(s_a)
        rho2 += s_a @ Pinv[a] @ s_a
    fp, fe = fst.fstat_from_rows(plan, np.concatenate(rows)[None, :])
    assert abs(fe[0, js, ss] - 0.5 * rho2) <= 1e-10 * 0.5 * rho2
    assert np.all(fe[0] <= 0.5 * rho2 * (1 + 1e-10))
    assert np.unravel_index(np.argmax(fe[0]), fe[0].shape) == (js, ss)


def test_refusals():
    arr = _array()
    for bad in ([1e-8, np.nan], [1e-8, np.inf], [0.0, 1e-8], [-1e-8], []):
        with pytest.raises(ValueError, match="freqs"):
            _prepare(arr, "spin", freqs=bad)
    with pytest.raises(ValueError, match=r"\|cos_gwtheta\| > 1"):
        _prepare(arr, "spin", sky=(np.array([0.1, 1.0001]), np.array([0.0, 1.0])))
    with pytest.raises(ValueError, match="sky"):
        _prepare(arr, "spin", sky=(np.array([0.1, 0.2]), np.array([0.0])))
    with pytest.raises(ValueError, match="sky"):
        _prepare(arr, "spin", sky=(np.array([0.1, np.nan]), np.array([0.0, 1.0])))
    # no white noise: the covariance is singular
    noisefree = [dict(p, sigma2=np.zeros_like(p["sigma2"])) for p in arr]
    with pytest.raises(ValueError, match="white-noise variances must be positive"):
        _prepare(noisefree, "spin")
    # a frequency the astrometric fit absorbs: sin / cos of one year are columns of M
    with pytest.raises(ValueError, match="singular"):
        _prepare(arr, "astrometric", freqs=[1e-8, 1.0 / (365.25 * 86400.0)])
    _prepare(arr, "spin", freqs=[1e-8, 1.0 / (365.25 * 86400.0)])          # the spin-down fit leaves it alone
    # two pulsars in one direction: phi_1 = phi_2, M_js has rank 2
    twins = [dict(p) for p in arr[:2]]
    twins[1]["phat"] = twins[0]["phat"]
    with pytest.raises(ValueError, match="M_js.*singular"):
        _prepare(twins, "spin")
    # Fe needs two pulsars; Fp alone works for one
    with pytest.raises(ValueError, match="at least two pulsars"):
        _prepare(arr[:1], "spin")
    _prepare(arr[:1], "spin", sky=None)
