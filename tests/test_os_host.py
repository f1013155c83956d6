"""Host preparation of the cross-correlation optimal statistic (pta_replicator_amd.optimal_statistic) against an independent dense
NumPy construction: C_a assembled explicitly, np.linalg.solve, timing model projected out.  No GPU."""
import numpy as np
import pytest

from oracle import pta_oracle as po
from pta_replicator_amd import optimal_statistic as os_
from pta_replicator_amd.simulate import timing_design_matrix

YR = 365.25 * 86400.0


def _array(P=5, seed=3):
    """a small ragged array: unequal TOA counts, two backends (EFAC / EQUAD / ECORR per backend), red noise on all but one pulsar"""
    rng = np.random.default_rng(seed)
    out = []
    for a in range(P):
        n = 40 + 29 * a + (a % 2)
        # observing sessions of a few TOAs within 0.05 d: ECORR epochs of 0.1 d hold several TOAs
        sess = np.sort(rng.uniform(53000, 57800, (n + 2) // 3))
        mjd = np.sort(np.repeat(sess, 3)[:n] + rng.uniform(0, 0.05, n))
        be = rng.integers(0, 2, n)
        sig = np.where(be == 0, 0.4e-6, 0.9e-6) * rng.uniform(0.8, 1.2, n)
        efac, equad = np.array([1.1, 0.9])[be], np.array([10 ** -6.6, 10 ** -6.9])[be]
        sigma2 = (efac * sig) ** 2 + (efac * equad) ** 2
        epoch_of, ne, first, _ = po.quantize(mjd, dt=0.1)
        ecorr = np.array([10 ** -6.7, 10 ** -7.0])[be[first]]
        rn = None if a == 2 else (-14.2 + 0.1 * a, 2.5 + 0.3 * a)
        ra, dec = rng.uniform(0, 2 * np.pi), np.arcsin(rng.uniform(-1, 1))
        out.append(dict(mjd=mjd, t=mjd * 86400.0, sigma2=sigma2, epoch_of=np.asarray(epoch_of), ecorr=np.asarray(ecorr), rn=rn,
                        ra=ra, dec=dec))
    return out


def _pos(arr):
    return np.array([[np.cos(p["dec"]) * np.cos(p["ra"]), np.cos(p["dec"]) * np.sin(p["ra"]), np.sin(p["dec"])] for p in arr])


def _rn_inputs(p, components=10):
    if p["rn"] is None:
        return None, None
    F, freqs = po.fourier_design_matrix(p["t"], nmodes=components, Tspan=p["t"].max() - p["t"].min())
    return F, po.red_noise_prior(freqs, p["rn"][0], p["rn"][1], p["t"].max() - p["t"].min())


def _prepare(arr, nf, model, gw_amp2, orfs=os_.ORF_NAMES):
    rn = [_rn_inputs(p) for p in arr]
    M = None if model is None else [timing_design_matrix(p["t"], model=model)[0] for p in arr]
    return os_.prepare([p["t"] for p in arr], [p["sigma2"] for p in arr], _pos(arr), components=nf, orfs=orfs,
                       epoch_of=[p["epoch_of"] for p in arr], ecorr=[p["ecorr"] for p in arr], F_rn=[x[0] for x in rn],
                       phi_rn=[x[1] for x in rn], gw_amp2=gw_amp2, M=M)


def _dense(arr, nf, model, gw_amp2, gamma=13. / 3.):
    """(W list, Z [P, C, C]) by brute force: C_a explicit, solve, project out M"""
    T = max(p["t"].max() for p in arr) - min(p["t"].min() for p in arr)
    Ws, Zs = [], []
    for p in arr:
        n = len(p["t"])
        F, freqs = po.fourier_design_matrix(p["t"], nmodes=nf, Tspan=T)
        S = (1 / YR) ** (gamma - 3) * freqs ** (-gamma) / (12 * np.pi ** 2 * T)
        C = np.diag(p["sigma2"]).astype(np.float64)
        C += (p["epoch_of"][:, None] == p["epoch_of"][None, :]) * (p["ecorr"][p["epoch_of"]] ** 2)[:, None]
        Frn, phi = _rn_inputs(p)
        if Frn is not None:
            C += (Frn * phi) @ Frn.T
        if gw_amp2:
            C += gw_amp2 * (F * S) @ F.T
        Ci = np.linalg.solve(C, np.eye(n))
        Pi = Ci
        if model is not None:
            M = timing_design_matrix(p["t"], model=model)[0]
            CiM = Ci @ M
            Pi = Ci - CiM @ np.linalg.solve(M.T @ CiM, CiM.T)
        W = np.sqrt(S)[:, None] * (F.T @ Pi)
        Ws.append(W)
        Zs.append(W @ F * np.sqrt(S)[None, :])
    return Ws, np.stack(Zs)


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


@pytest.mark.parametrize("model", ["spin", "astrometric", None])
@pytest.mark.parametrize("gw", [0.0, 10 ** (2 * -14.3)])
def test_operators_match_dense(model, gw):
    arr = _array()
    nf = 6
    plan = _prepare(arr, nf, model, gw)
    Wd, Zd = _dense(arr, nf, model, gw)
    for a in range(len(arr)):
        assert plan.W[a].shape == (2 * nf, len(arr[a]["t"]))
        assert _rel(plan.W[a], Wd[a]) < 1e-10, (a, _rel(plan.W[a], Wd[a]))
        assert _rel(plan.Z[a], Zd[a]) < 1e-10
    den = np.array([np.trace(Zd[a] @ Zd[b]) for a, b in zip(plan.pair_a, plan.pair_b)])
    assert _rel(plan.den, den) < 1e-10


def test_hd_matches_engine_orf_over_two():
    arr = _array(P=7, seed=9)
    plan = _prepare(arr, 4, "spin", 0.0)
    locs = np.array([[p["ra"], np.pi / 2 - p["dec"]] for p in arr])
    ref = po.hd_orf_closed_form(locs) / 2
    k = plan.names.index("hd")
    np.testing.assert_allclose(plan.G[k], ref[plan.pair_a, plan.pair_b], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(plan.G[plan.names.index("monopole")], 1.0)
    np.testing.assert_allclose(plan.G[plan.names.index("dipole")], np.cos(plan.zeta), atol=1e-14)
    # pairs: a < b, row-major upper triangle
    ia, ib = np.triu_indices(7, 1)
    assert np.array_equal(plan.pair_a, ia) and np.array_equal(plan.pair_b, ib)


@pytest.mark.parametrize("model", ["spin", "astrometric"])
def test_whole_os_matches_dense(model):
    arr = _array(P=6, seed=5)
    nf, gw = 5, 10 ** (2 * -14.5)
    user = np.random.default_rng(1).uniform(-1, 1, (6, 6))
    plan = _prepare(arr, nf, model, gw, orfs=("hd", "monopole", "dipole", user))
    Wd, Zd = _dense(arr, nf, model, gw)
    rng = np.random.default_rng(2)
    rows = rng.normal(0, 1e-7, (9, int(plan.off[-1])))
    A2, snr, num = os_.os_from_rows(plan, rows)
    # dense statistic
    Y = [rows[:, plan.off[a]:plan.off[a + 1]] @ Wd[a].T for a in range(6)]
    num_d = np.stack([np.sum(Y[a] * Y[b], axis=1) for a, b in zip(plan.pair_a, plan.pair_b)], axis=1)
    den_d = np.array([np.trace(Zd[a] @ Zd[b]) for a, b in zip(plan.pair_a, plan.pair_b)])
    _, _, cz = os_.pair_geometry(_pos(arr))
    for k, G in enumerate([os_.hd(cz), np.ones_like(cz), cz, user[plan.pair_a, plan.pair_b]]):
        ref = num_d @ G / np.sum(G ** 2 * den_d)
        sig = np.sum(G ** 2 * den_d) ** -0.5
        assert _rel(A2[:, k], ref) < 1e-10
        assert _rel(snr[:, k], ref / sig) < 1e-10
        assert abs(plan.sigma[k] / sig - 1) < 1e-10
    assert _rel(num, num_d) < 1e-10
    assert plan.names == ["hd", "monopole", "dipole", "orf3"]


def test_refusals():
    arr = _array(P=3)
    with pytest.raises(ValueError, match="components"):
        _prepare_nf(arr, 0)
    with pytest.raises(ValueError, match="components"):
        _prepare_nf(arr, 33)
    with pytest.raises(ValueError, match="unknown ORF"):
        _prepare(arr, 4, "spin", 0.0, orfs=("hd", "quadrupole"))
    with pytest.raises(ValueError, match="user ORF"):
        _prepare(arr, 4, "spin", 0.0, orfs=(np.ones((2, 2)),))
    # two TOAs cannot constrain offset + F0 + F1
    t = np.array([5.0e9, 5.1e9])
    with pytest.raises(ValueError, match="singular"):
        os_.pulsar_operator(np.ones(2) * 1e-12, os_.fourier_basis(t, 2, 1e8), np.ones(4), M=timing_design_matrix(t, model="spin")[0])


def _prepare_nf(arr, nf):
    return _prepare(arr, nf, "spin", 0.0)


def test_host_preparation_never_forms_n_by_n(monkeypatch):
    """the Woodbury / Sherman-Morrison path: no intermediate with two TOA-sized axes"""
    arr = _array(P=2, seed=4)
    biggest = [0]
    real = np.linalg.solve

    def watch(A, B):
        biggest[0] = max(biggest[0], np.asarray(A).shape[0])
        return real(A, B)
    monkeypatch.setattr(np.linalg, "solve", watch)
    _prepare(arr, 4, "spin", 1e-29)
    assert biggest[0] <= 2 * 10 + 2 * 4 + 3
