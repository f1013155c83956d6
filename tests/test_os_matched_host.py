"""Host half of the optimal statistic under per-realisation noise parameters (optimal_statistic.matched_*): the reduced-rank
evaluation against a dense NumPy OS that assembles C_a(theta_r) explicitly, against the fixed-noise plan at the configured theta,
the device math header csrc/pta_os_matched.h compiled with g++ against matched_prior, and the refusals.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import pta_oracle as po
from pta_replicator_amd import _hyper
from pta_replicator_amd import optimal_statistic as ost
from pta_replicator_amd.simulate import timing_design_matrix

HERE = os.path.dirname(os.path.abspath(__file__))
YR = 365.25 * 86400.0
NRN = 10          # red-noise frequencies


def _array(P=5, seed=3):
    """a small ragged array: ECORR sessions, two backends, errors of 0.3 - 0.8 us, red noise on all but pulsar 2"""
    rng = np.random.default_rng(seed)
    out = []
    for a in range(P):
        n = 40 + 29 * a + (a % 2)
        sess = np.sort(rng.uniform(53000, 57800, (n + 2) // 3))
        mjd = np.sort(np.repeat(sess, 3)[:n] + rng.uniform(0, 0.05, n))
        be = rng.integers(0, 2, n)
        sig = np.where(be == 0, 0.4e-6, 0.7e-6) * rng.uniform(0.8, 1.1, n)
        efac, equad = np.array([1.1, 0.9])[be], np.array([10 ** -6.6, 10 ** -6.9])[be]
        epoch_of, ne, first, _ = po.quantize(mjd, dt=0.1)
        t = mjd * 86400.0
        out.append(dict(t=t, sigma2=(efac * sig) ** 2 + (efac * equad) ** 2, epoch_of=np.asarray(epoch_of),
                        ecorr=np.asarray(np.array([10 ** -6.7, 10 ** -7.0])[be[first]]), rn=None if a == 2 else (-14.2 + 0.1 * a, 2.5 + 0.3 * a),
                        tspan=t.max() - t.min(), ra=rng.uniform(0, 2 * np.pi), dec=np.arcsin(rng.uniform(-1, 1))))
    return out


def _pos(arr):
    return np.array([[np.cos(p["dec"]) * np.cos(p["ra"]), np.cos(p["dec"]) * np.sin(p["ra"]), np.sin(p["dec"])] for p in arr])


def _rn_basis(p):
    return po.fourier_design_matrix(p["t"], nmodes=NRN, Tspan=p["tspan"])


def _tables(arr):
    """(rn_f [P, NRN], rn_tspan [P], rn_phi [P, 2 NRN]): what the engine uploads - frequencies, spans, configured prior variances"""
    rn_f = np.stack([np.arange(1, NRN + 1) / p["tspan"] for p in arr])
    tspan = np.array([p["tspan"] for p in arr])
    phi = np.zeros((len(arr), 2 * NRN))
    for a, p in enumerate(arr):
        if p["rn"] is not None:
            phi[a] = ost.rn_prior(np.repeat(rn_f[a], 2), tspan[a], p["rn"][0], p["rn"][1])
    return rn_f, tspan, phi


def _M(arr, model):
    return None if model is None else [timing_design_matrix(p["t"], model=model)[0] for p in arr]


def _matched_plan(arr, nf, model, gamma=13. / 3.):
    return ost.prepare_matched([p["t"] for p in arr], [p["sigma2"] for p in arr], _pos(arr), components=nf, gamma=gamma,
                               epoch_of=[p["epoch_of"] for p in arr], ecorr=[p["ecorr"] for p in arr],
                               F_rn=[_rn_basis(p)[0] for p in arr], M=_M(arr, model))


def _dense(arr, rows, off, nf, model, rn_lA, rn_g, gw_lA, gw_g, gamma=13. / 3.):
    """X [R, P, C], Z [R, P, C, C] by brute force per realisation: C_a(theta_r) explicit, np.linalg.solve, the timing model projected
    out.  rn_lA, rn_g [R, P] (NaN = no red noise); gw_lA, gw_g [R] or None"""
    T = max(p["t"].max() for p in arr) - min(p["t"].min() for p in arr)
    R, P = rn_lA.shape
    X, Z = np.zeros((R, P, 2 * nf)), np.zeros((R, P, 2 * nf, 2 * nf))
    for a, p in enumerate(arr):
        n = len(p["t"])
        F, freqs = po.fourier_design_matrix(p["t"], nmodes=nf, Tspan=T)
        S = (1 / YR) ** (gamma - 3) * freqs ** (-gamma) / (12 * np.pi ** 2 * T)
        C0 = np.diag(p["sigma2"]).astype(np.float64)
        C0 += (p["epoch_of"][:, None] == p["epoch_of"][None, :]) * (p["ecorr"][p["epoch_of"]] ** 2)[:, None]
        Frn, fr = _rn_basis(p)
        M = None if model is None else timing_design_matrix(p["t"], model=model)[0]
        for r in range(R):
            C = C0.copy()
            if not np.isnan(rn_lA[r, a]):
                C += (Frn * po.red_noise_prior(fr, rn_lA[r, a], rn_g[r, a], p["tspan"])) @ Frn.T
            if gw_lA is not None:
                Sr = (1 / YR) ** (gw_g[r] - 3) * freqs ** (-gw_g[r]) / (12 * np.pi ** 2 * T)
                C += 10 ** (2 * gw_lA[r]) * (F * Sr) @ F.T
            Pi = np.linalg.solve(C, np.eye(n))
            if M is not None:
                CiM = Pi @ M
                Pi = Pi - CiM @ np.linalg.solve(M.T @ CiM, CiM.T)
            W = np.sqrt(S)[:, None] * (F.T @ Pi)
            X[r, a] = W @ rows[r, off[a]:off[a + 1]]
            Z[r, a] = W @ F * np.sqrt(S)[None, :]
    return X, Z


def _nrel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


def _theta(arr, R, seed, nan_rows=True):
    """rn_log10_A <= -13, indices 2 .. 6; NaN amplitudes ("as configured") on a few (realisation, pulsar) entries"""
    rng = np.random.default_rng(seed)
    P = len(arr)
    lA, g = rng.uniform(-15.5, -13.0, (R, P)), rng.uniform(2, 6, (R, P))
    if nan_rows:
        lA[0, :] = np.nan
        lA[1::3, 1] = np.nan
        g[np.isnan(lA)] = np.nan
    return lA, g


def _effective_rn(arr, lA, g):
    """what the model holds per (r, a): theta where given, the configured values where NaN, nothing for a pulsar without red noise"""
    lA, g = lA.copy(), g.copy()
    for a, p in enumerate(arr):
        nan = np.isnan(lA[:, a])
        lA[nan, a], g[nan, a] = (np.nan, np.nan) if p["rn"] is None else p["rn"]
        if p["rn"] is None:
            lA[:, a], g[:, a] = np.nan, np.nan
    return lA, g


@pytest.mark.parametrize("model", ["spin", "astrometric"])
@pytest.mark.parametrize("gw", ["off", "template", "own_index"])
def test_matched_os_vs_dense(model, gw):
    arr = _array()
    nf, R, P = 6, 7, len(arr)
    plan = _matched_plan(arr, nf, model)
    assert plan.K == 2 * NRN + 2 * nf and plan.K_rn == 2 * NRN and plan.C == 2 * nf
    rng = np.random.default_rng(11)
    rows = rng.normal(0, 5e-7, (R, int(plan.off[-1])))
    lA, g = _theta(arr, R, 5)
    lA_in = lA.copy()
    lA_in[:, 2] = np.nan      # a pulsar without red noise: the engine masks its amplitudes to NaN
    gw_lA = gw_g = None
    if gw != "off":
        gw_lA = rng.uniform(-14.8, -14.0, R)
        gw_g = np.full(R, 13. / 3.) if gw == "template" else rng.uniform(3.0, 5.5, R)
    rn_f, tspan, phi = _tables(arr)
    b = ost.matched_prior(R, plan.s, rn_f, tspan, phi, lA_in, g, nf, plan.T, gw_lA, gw_g)
    assert b.shape == (R, P, plan.K) and np.all(b[:, 2, :plan.K_rn] == 0) and np.all(b >= 0)
    got = ost.matched_from_rows(plan, rows, b)
    elA, eg = _effective_rn(arr, lA, g)
    Xd, Zd = _dense(arr, rows, plan.off, nf, model, elA, eg, gw_lA, gw_g)
    ref = ost.matched_from_XZ(plan, Xd, Zd)
    worst = 0.0
    for r in range(R):                       # per realisation
        for k in ("X", "Z", "A2", "sigma"):
            e = _nrel(got[k][r], ref[k][r])
            worst = max(worst, e)
            assert e < 1e-9, (r, k, e)
    cond = max(np.linalg.cond(np.eye(plan.K) + np.sqrt(b[r, a])[:, None] * plan.A[a] * np.sqrt(b[r, a])[None, :]) for r in range(R) for a in range(P))
    print(f"model={model} gw={gw}: worst norm-wise relative error against dense {worst:.3e}, max cond(Mc) {cond:.3g}")
    # the two host forms (Cholesky / solve) agree at the same level
    alt = ost.matched_from_rows(plan, rows, b, form="solve")
    assert _nrel(alt["X"], got["X"]) < 1e-9 and _nrel(alt["Z"], got["Z"]) < 1e-9


@pytest.mark.parametrize("model", ["spin", "astrometric", None])
@pytest.mark.parametrize("gw_lA", [None, -14.3])
def test_configured_theta_reproduces_fixed_plan(model, gw_lA):
    arr = _array()
    nf, R, P = 6, 4, len(arr)
    mp = _matched_plan(arr, nf, model)
    rn_f, tspan, phi = _tables(arr)
    fixed = ost.prepare([p["t"] for p in arr], [p["sigma2"] for p in arr], _pos(arr), components=nf, epoch_of=[p["epoch_of"] for p in arr],
                        ecorr=[p["ecorr"] for p in arr], F_rn=[_rn_basis(p)[0] if p["rn"] is not None else None for p in arr],
                        phi_rn=[phi[a] if p["rn"] is not None else None for a, p in enumerate(arr)],
                        gw_amp2=0.0 if gw_lA is None else 10.0 ** (2 * gw_lA), M=_M(arr, model))
    rows = np.random.default_rng(2).normal(0, 5e-7, (R, int(mp.off[-1])))
    gw = (None, None) if gw_lA is None else (np.full(R, gw_lA), np.full(R, 13. / 3.))
    b = ost.matched_prior(R, mp.s, rn_f, tspan, phi, None, None, nf, mp.T, *gw)
    got = ost.matched_from_rows(mp, rows, b)
    Y = ost.project(fixed, rows)
    eX, eZ = _nrel(got["X"], Y), max(_nrel(got["Z"][r], fixed.Z) for r in range(R))
    print(f"model={model} gw={gw_lA}: X {eX:.3e} Z {eZ:.3e}")
    assert eX < 1e-9 and eZ < 1e-9
    A2, snr, num = ost.os_from_Y(fixed, Y)
    assert _nrel(got["A2"], A2) < 1e-9 and _nrel(got["snr"], snr) < 1e-9
    assert all(_nrel(got["sigma"][r], fixed.sigma) < 1e-9 for r in range(R))
    # sampled theta equal to the configured values gives the same b as "as configured" up to the rounding of sqrt(.)^2
    lA = np.array([[np.nan if p["rn"] is None else p["rn"][0] for p in arr]] * R)
    g = np.array([[np.nan if p["rn"] is None else p["rn"][1] for p in arr]] * R)
    b2 = ost.matched_prior(R, mp.s, rn_f, tspan, phi, lA, g, nf, mp.T, *gw)
    assert np.allclose(b2, b, rtol=1e-14, atol=0)


# ---------------------------------------------------------------- device math header ----------------------------------------
@pytest.fixture(scope="module")
def omh(tmp_path_factory):
    out = tmp_path_factory.mktemp("os_matched") / "libosmatchedhost.so"
    src = os.path.join(HERE, "os_matched", "os_matched_host.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", str(out)])
    lib = ctypes.CDLL(str(out))
    i, d, p = ctypes.c_int, ctypes.c_double, ctypes.POINTER(ctypes.c_double)
    lib.omh_prior.argtypes = [i, i, i, i, p, p, p, p, p, d, p, p, p, p]
    lib.omh_prior.restype = None
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


@pytest.mark.parametrize("rn_theta", [False, True])
@pytest.mark.parametrize("gw_theta", [False, True])
def test_prior_header_matches_numpy(omh, rn_theta, gw_theta):
    """b of pta_os_matched_prior against matched_prior.  Entries that go through pow agree to 1e-14 relative (the precedent of
    tests/test_hyper_host.py for pta_rn_amp); entries taken from the configured table and the zeros are bit-equal."""
    rng = np.random.default_rng(8)
    R, P, K_rn, nf = 9, 4, 12, 5
    C, T = 2 * nf, 4.6e8
    tspan = rng.uniform(3e8, 4.5e8, P)
    rn_f = np.ascontiguousarray(np.arange(1, K_rn // 2 + 1)[None, :] / tspan[:, None])
    phi = np.ascontiguousarray(rng.uniform(1e-16, 1e-12, (P, K_rn)))
    phi[1] = 0.0
    s = rng.uniform(1e-13, 1e-12, P)
    lA = g = gl = gg = None
    if rn_theta:
        lA, g = rng.uniform(-18, -11, (R, P)), rng.uniform(0.5, 7, (R, P))
        lA[2, :] = np.nan
        lA[:, 1] = np.nan
        g[np.isnan(lA)] = np.nan
    if gw_theta:
        gl, gg = rng.uniform(-18, -11, R), rng.uniform(0.5, 7, R)
    dev = np.full(R * P * (K_rn + C), np.nan)
    omh.omh_prior(R, P, K_rn, C, _p(rn_f), _p(tspan), _p(phi), _p(lA), _p(g), T, _p(gl), _p(gg), _p(s), _p(dev))
    dev = dev.reshape(R, P, K_rn + C)
    ref = ost.matched_prior(R, s, rn_f, tspan, phi, lA, g, nf, T, gl, gg)
    assert np.all(np.isfinite(dev)) and np.all(dev >= 0)
    fixed = np.ones((R, P), dtype=bool) if lA is None else np.isnan(lA)
    assert np.array_equal(dev[:, :, :K_rn][fixed], ref[:, :, :K_rn][fixed])
    if not gw_theta:
        assert np.all(dev[:, :, K_rn:] == 0) and np.all(ref[:, :, K_rn:] == 0)
    nz = ref > 0
    worst = float(np.max(np.abs(dev[nz] / ref[nz] - 1))) if np.any(nz) else 0.0
    print(f"rn_theta={rn_theta} gw_theta={gw_theta}: worst relative deviation {worst:.2e}")
    assert np.array_equal(dev == 0, ref == 0)
    assert worst < 1e-14, worst


# ---------------------------------------------------------------- refusals ----------------------------------------------------
def _rn_conf(P):
    return {"A": [-14.0] * (P - 1) + [None], "g": [3.0] * (P - 1) + [None]}


def test_theta_refusals():
    R, P = 3, 4
    rn = _rn_conf(P)
    ok = {"gwb_log10_A": np.full(R, -14.0), "gwb_gamma": np.full(R, 4.0), "rn_log10_A": np.full((R, P), -14.0), "rn_gamma": np.full((R, P), 3.0)}
    assert set(_hyper.check_theta_os(ok, R, P, rn, True)) == set(ok)
    # cw_* keys are accepted and ignored; the gwb_mode of the generator plays no role (there is no such argument)
    assert set(_hyper.check_theta_os(dict(ok, cw_log10_mc=np.zeros(R), cw_gwphi="anything"), R, P, rn, True)) == set(ok)
    cases = [
        ({"gwb_amplitude": np.zeros(R)}, "unknown"),
        ({"gwb_log10_A": np.zeros(R + 1)}, "shape"),
        ({"rn_log10_A": np.zeros((R, P - 1))}, "shape"),
        ({"rn_gamma": np.zeros(R)}, "shape"),
        ({"gwb_gamma": np.array([4.0, np.inf, 4.0])}, "non-finite"),
        ({"gwb_log10_A": np.array([-14.0, -np.inf, -14.0])}, "non-finite"),
        ({"gwb_log10_A": np.array([-14.0, np.nan, -14.0])}, "non-finite"),
        ({"rn_log10_A": np.full((R, P), np.inf)}, "infinite"),
        ({**ok, "rn_gamma": np.full((R, P), -np.inf)}, "non-finite"),
        ({**ok, "rn_gamma": np.where(np.eye(R, P) > 0, np.nan, 3.0)}, "non-finite"),
    ]
    for theta, msg in cases:
        with pytest.raises(ValueError, match=msg):
            _hyper.check_theta_os(theta, R, P, rn, True)
    with pytest.raises(ValueError, match="dict"):
        _hyper.check_theta_os([1, 2], R, P, rn, True)
    with pytest.raises(ValueError, match="without the GWB auto-term"):
        _hyper.check_theta_os({"gwb_log10_A": np.full(R, -14.0)}, R, P, rn, False)
    with pytest.raises(ValueError, match="no red noise"):
        _hyper.check_theta_os({"rn_gamma": np.full((R, P), 3.0)}, R, P, None, True)
    # NaN amplitude = "as configured", with the index left NaN there too; the pulsar without red noise is ignored
    th = dict(rn_log10_A=np.where(np.eye(R, P) > 0, np.nan, -14.0), rn_gamma=np.where(np.eye(R, P) > 0, np.nan, 3.0))
    assert set(_hyper.check_theta_os(th, R, P, rn, False)) == set(th)
    g = np.full((R, P), 3.0)
    g[:, P - 1] = np.nan
    assert "rn_gamma" in _hyper.check_theta_os({"rn_gamma": g}, R, P, rn, False)


def test_k_over_the_limit_is_refused():
    arr = _array(P=2)
    wide = [po.fourier_design_matrix(p["t"], nmodes=55, Tspan=p["tspan"])[0] for p in arr]     # 110 + 2 * 10 = 130 > 128
    with pytest.raises(ValueError, match="exceeds the limit"):
        ost.prepare_matched([p["t"] for p in arr], [p["sigma2"] for p in arr], _pos(arr), components=10, F_rn=wide)
    with pytest.raises(ValueError, match="components"):
        ost.prepare_matched([p["t"] for p in arr], [p["sigma2"] for p in arr], _pos(arr), components=33)


def _engine(components=10):
    from helpers import load, mjd_ld
    from pta_replicator_amd.engine import ReplicaEngine
    from pta_replicator_amd.simulate import ArrayTOAs, SimulatedPulsar, make_ideal
    z = load("c3_mini.npz")
    psrs = []
    for i in range(4):
        p = SimulatedPulsar(toas=ArrayTOAs(mjd_ld(z, "", i), z[f"err_us_{i}"]), name=str(z["names"][i]),
                            loc={"RAJ": float(z["raj_hours"][i]), "DECJ": float(z["decj_deg"][i])})
        make_ideal(p)
        psrs.append(p)
    eng = ReplicaEngine(psrs, seed=5)
    eng.set_white_noise(efac=1.1)
    eng.set_red_noise([-14.0, None, -13.5, -14.2], [3.0, None, 2.5, 4.0], components=components)
    return eng


def test_engine_refusals_before_any_launch():
    """configured, never prepared: every refusal comes before the device is touched"""
    eng = _engine(components=50)
    with pytest.raises(ValueError, match="exceeds the kernel limit"):
        eng.prepare_optimal_statistic(components=15, matched=True)           # 100 + 30 > 128
    assert not eng._prepared
    eng = _engine()
    R = 2
    theta = {"rn_log10_A": np.full((R, 4), -14.0), "rn_gamma": np.full((R, 4), 3.0)}
    with pytest.raises(ValueError, match="matched=True"):
        eng._os_matched_theta({"matched": None}, theta, R, "optimal_statistic")   # prepared without matched=True
    with pytest.raises(ValueError, match="not prepared"):
        eng.generate_os(R, theta=theta, matched=True)
    st = {"matched": {"gw": None, "K_rn": 20}}
    with pytest.raises(ValueError, match="without the GWB auto-term"):
        eng._os_matched_theta(st, {"gwb_log10_A": np.full(R, -14.0)}, R, "optimal_statistic")
    with pytest.raises(ValueError, match="unknown"):
        eng._os_matched_theta(st, {"rn_amp": np.zeros((R, 4))}, R, "optimal_statistic")
    with pytest.raises(ValueError, match="shape"):
        eng._os_matched_theta(st, {"rn_log10_A": np.zeros((R + 1, 4))}, R, "optimal_statistic")
    with pytest.raises(ValueError, match="infinite"):
        eng._os_matched_theta(st, {**theta, "rn_log10_A": np.full((R, 4), -np.inf)}, R, "optimal_statistic")
    assert not eng._prepared
