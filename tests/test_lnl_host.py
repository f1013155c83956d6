"""Host half of the marginalised log-likelihood on a theta grid (optimal_statistic.lnl_*): the reduced-rank evaluation against a
dense NumPy likelihood that assembles C_a(theta_g) explicitly, differences between grid points, theta_grid, the device math header
csrc/pta_lnl.h compiled with g++ against lnl_quad, and the refusals.  No GPU.

Bound: |d ln L| <= 1e-12 (|ln L| + r^T P0' r / s) per (realisation, pulsar, grid point): the two terms of the reduced-rank form
cancel when red noise is strong, so the error scales with r^T P0' r / s and not with ln L.  The dense side assembles and factors
C_a(theta) in extended precision: at the stiff corner (log10_A = -12.5, gamma = 6) C_a has a condition number near 1e10 and a float64
slogdet / solve of it is off by 5e-12 of that scale, five times the bound, while the form under test is within 1e-14 of the extended
reference.  The bound still widens to 8 delta where that is larger, delta = the disagreement of the two host forms (Cholesky /
np.linalg.solve) at that (pulsar, grid point); with the extended reference it never is (the test prints it)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import pta_oracle as po
from pta_replicator_amd import optimal_statistic as ost
from pta_replicator_amd.simulate import timing_design_matrix

HERE = os.path.dirname(os.path.abspath(__file__))
YR = 365.25 * 86400.0
NRN = 10          # red-noise frequencies
NF = 6            # frequencies of the common process


def _array(seed=7):
    """3 ragged pulsars whose TOAs are NOT in time order: sessions of 1 - 4 TOAs (multi-TOA and singleton ECORR epochs), the epochs
    numbered in a random order and the TOAs shuffled, so no epoch is contiguous; pulsar 1 has no red noise"""
    rng = np.random.default_rng(seed)
    out = []
    for a, n_sess in enumerate((30, 47, 38)):
        size = rng.integers(1, 5, n_sess)
        size[:3] = (1, 4, 1)
        sess = np.sort(rng.uniform(53000, 57800, n_sess))
        mjd = np.repeat(sess, size) + rng.uniform(0, 0.05, size.sum())
        epoch = np.repeat(rng.permutation(n_sess), size)
        shuffle = rng.permutation(len(mjd))
        mjd, epoch = mjd[shuffle], epoch[shuffle]
        n = len(mjd)
        be = rng.integers(0, 2, n)
        sig = np.where(be == 0, 0.4e-6, 0.7e-6) * rng.uniform(0.8, 1.1, n)
        efac, equad = np.array([1.1, 0.9])[be], np.array([10 ** -6.6, 10 ** -6.9])[be]
        t = mjd * 86400.0
        out.append(dict(t=t, sigma2=(efac * sig) ** 2 + (efac * equad) ** 2, epoch_of=epoch, ecorr=10 ** rng.uniform(-7.0, -6.5, n_sess),
                        rn=None if a == 1 else (-14.0 + 0.2 * a, 3.0 + 0.5 * a), tspan=t.max() - t.min()))
        assert np.any(np.diff(epoch) < 0) and np.any(np.bincount(epoch) == 1) and np.any(np.bincount(epoch) > 1)
    return out


def _rn_basis(p):
    return po.fourier_design_matrix(p["t"], nmodes=NRN, Tspan=p["tspan"])


def _tables(arr):
    rn_f = np.stack([np.arange(1, NRN + 1) / p["tspan"] for p in arr])
    tspan = np.array([p["tspan"] for p in arr])
    phi = np.zeros((len(arr), 2 * NRN))
    for a, p in enumerate(arr):
        if p["rn"] is not None:
            phi[a] = ost.rn_prior(np.repeat(rn_f[a], 2), tspan[a], p["rn"][0], p["rn"][1])
    return rn_f, tspan, phi


def _M(arr, model):
    return None if model is None else [timing_design_matrix(p["t"], model=model)[0] for p in arr]


def _plan(arr, model):
    return ost.prepare_lnl([p["t"] for p in arr], [p["sigma2"] for p in arr], components=NF, epoch_of=[p["epoch_of"] for p in arr],
                           ecorr=[p["ecorr"] for p in arr], F_rn=[_rn_basis(p)[0] for p in arr], M=_M(arr, model))


def _grid(arr, gw):
    """9 grid points: rn_log10_A x rn_gamma over (-15, -13.7, -12.5) x (2, 4, 6) (pulsar 2 shifted by 0.1 so that the pulsars differ),
    the common process, where it is on, running over the same span; the last point is the stiff corner (-12.5, 6)"""
    lA, g = np.meshgrid([-15.0, -13.7, -12.5], [2.0, 4.0, 6.0], indexing="ij")
    P = len(arr)
    rn_lA = np.repeat(lA.reshape(-1, 1), P, axis=1)
    rn_lA[:, 2] -= 0.1
    rn_g = np.repeat(g.reshape(-1, 1), P, axis=1)
    rn_lA[:, 1] = np.nan        # no red noise on pulsar 1: the engine masks its amplitudes to NaN
    gw_lA = gw_g = None
    if gw:
        gw_lA, gw_g = lA.reshape(-1)[::-1].copy(), g.reshape(-1)[[4, 0, 8, 2, 6, 1, 7, 3, 5]].copy()
    return rn_lA, rn_g, gw_lA, gw_g


def _dense(arr, rows, off, model, rn_lA, rn_g, gw_lA, gw_g):
    """ln L [R, P, G] by brute force: C_a(theta_g) explicit and factored in extended precision, the timing model marginalised with a
    flat prior: -2 ln L = r^T [C^-1 - C^-1 M (M^T C^-1 M)^-1 M^T C^-1] r + ln det C + ln det(M^T C^-1 M) + (N - m) ln 2 pi"""
    T = max(p["t"].max() for p in arr) - min(p["t"].min() for p in arr)
    G, P = rn_lA.shape
    R = rows.shape[0]
    out = np.zeros((R, P, G))
    for a, p in enumerate(arr):
        n = len(p["t"])
        F, freqs = po.fourier_design_matrix(p["t"], nmodes=NF, Tspan=T)
        C0 = np.diag(p["sigma2"]).astype(LD)               # assembled in extended precision too: rounding C to float64 already
        C0 += (p["epoch_of"][:, None] == p["epoch_of"][None, :]) * (p["ecorr"].astype(LD)[p["epoch_of"]] ** 2)[:, None]   # moves ln L by cond(C) eps
        Frn, fr = _rn_basis(p)
        Frn, F = Frn.astype(LD), F.astype(LD)
        M = None if model is None else timing_design_matrix(p["t"], model=model)[0]
        r = rows[:, off[a]:off[a + 1]].T
        for g in range(G):
            C = C0.copy()
            if not np.isnan(rn_lA[g, a]):
                C += (Frn * po.red_noise_prior(fr, rn_lA[g, a], rn_g[g, a], p["tspan"]).astype(LD)) @ Frn.T
            if gw_lA is not None:
                Sg = (1 / YR) ** (gw_g[g] - 3) * freqs ** (-gw_g[g]) / (12 * np.pi ** 2 * T)
                C += (F * (10 ** (2 * gw_lA[g]) * Sg).astype(LD)) @ F.T
            sc = np.mean(p["sigma2"])                      # factor an O(1) matrix; the scale goes back in analytically
            L = _chol_ld(C / sc)
            y = _fwd_ld(L, r)
            chi2 = np.sum(y * y, axis=0) / sc
            logdet = 2 * np.sum(np.log(np.diag(L))) + n * np.log(LD(sc))
            m = 0
            if M is not None:
                m = M.shape[1]
                nrm = np.linalg.norm(M, axis=0)
                Y = _fwd_ld(L, M / nrm[None, :])           # M^T C^-1 M = Y^T Y, M^T C^-1 r = Y^T y
                Lb = _chol_ld(Y.T @ Y)
                z = _fwd_ld(Lb, Y.T @ y)
                chi2 = chi2 - np.sum(z * z, axis=0) / sc
                logdet += 2 * np.sum(np.log(np.diag(Lb))) - m * np.log(LD(sc)) + 2 * np.sum(np.log(nrm.astype(LD)))
            out[:, a, g] = -0.5 * (chi2 + logdet + (n - m) * np.log(2 * np.pi))
    return out


LD = np.longdouble


def _chol_ld(C):
    """lower Cholesky factor in extended precision (x87 long double, eps 1e-19): at the stiff corner C_a has a condition number
    near 1e10 and a float64 slogdet / solve of it is less accurate than the reduced-rank form under test"""
    A = np.array(C, dtype=LD)
    n = A.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        v = A[j:, j] - L[j:, :j] @ L[j, :j]
        L[j:, j] = v / np.sqrt(v[0])
    return L


def _fwd_ld(L, B):
    """L^-1 B by forward substitution in extended precision"""
    X = np.array(B, dtype=LD)
    for i in range(L.shape[0]):
        X[i] = (X[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


def _b(arr, plan, grid):
    rn_lA, rn_g, gw_lA, gw_g = grid
    rn_f, tspan, phi = _tables(arr)
    return ost.matched_prior(rn_lA.shape[0], plan.s, rn_f, tspan, phi, rn_lA, rn_g, NF, plan.T, gw_lA, gw_g)


def _effective(arr, rn_lA, rn_g):
    lA, g = rn_lA.copy(), rn_g.copy()
    for a, p in enumerate(arr):
        if p["rn"] is None:
            lA[:, a] = np.nan
    return lA, g


def _rows(arr, plan, R, seed):
    """white noise at the level of the error bars plus a smooth red term, so that r^T P0' r / s is far larger than N_a at weak-noise
    grid points and the cancellation at strong-noise points is exercised"""
    rng = np.random.default_rng(seed)
    rows = rng.normal(0, 5e-7, (R, int(plan.off[-1])))
    for a, p in enumerate(arr):
        x = (p["t"] - p["t"].min()) / p["tspan"]
        rows[:, plan.off[a]:plan.off[a + 1]] += rng.normal(0, 3e-6, (R, 1)) * np.sin(2 * np.pi * x)[None, :] + rng.normal(0, 3e-6, (R, 1)) * np.cos(4 * np.pi * x)[None, :]
    return rows


@pytest.mark.parametrize("model", ["spin", None])
@pytest.mark.parametrize("gw", [False, True])
def test_lnl_vs_dense(model, gw):
    arr = _array()
    plan = _plan(arr, model)
    P, K, R = len(arr), 2 * NRN + 2 * NF, 5
    assert plan.K == K and plan.K_rn == 2 * NRN and plan.C == 2 * NF and plan.m == (3 if model == "spin" else 0)
    rows = _rows(arr, plan, R, 11)
    grid = _grid(arr, gw)
    b = _b(arr, plan, grid)
    G = b.shape[0]
    assert b.shape == (G, P, K) and np.all(b[:, 1, :2 * NRN] == 0)
    lp, tot = ost.lnl_from_rows(plan, rows, b)
    lp_s, tot_s = ost.lnl_from_rows(plan, rows, b, form="solve")
    assert lp.shape == (R, P, G) and tot.shape == (R, G)
    assert np.array_equal(tot, (lp[:, 0] + lp[:, 1]) + lp[:, 2])          # the fixed-order pulsar sum
    ref = _dense(arr, rows, plan.off, model, *_effective(arr, grid[0], grid[1]), grid[2], grid[3])
    r0 = ost.lnl_quad(plan, rows)
    scale = np.abs(ref) + (r0 / plan.s[None, :])[:, :, None]
    delta = np.max(np.abs(lp - lp_s), axis=0, keepdims=True)              # [1, P, G]
    err = np.abs(lp - ref)
    tol = np.maximum(1e-12 * scale, 8 * delta)
    cond = [max(np.linalg.cond(np.eye(K) + np.sqrt(b[g, a])[:, None] * plan.A[a] * np.sqrt(b[g, a])[None, :]) for a in range(P)) for g in range(G)]
    for g in range(G):
        print(f"model={model} gw={gw} g={g}: cond(Mc) {cond[g]:.3g}, max |d lnL| {err[:, :, g].max():.3e}, relative to scale "
              f"{(err / scale)[:, :, g].max():.3e}, delta {delta[0, :, g].max():.3e}, widened {bool(np.any(8 * delta[0, :, g] > 1e-12 * scale[:, :, g].min(axis=0)))}")
    assert np.all(err <= tol), float(np.max(err / tol))
    assert np.max(delta / scale) < 1e-10                                  # the two host forms themselves agree
    # differences between grid points (c_a cancels) obey the same bound
    d_got, d_ref = lp[:, :, 1:] - lp[:, :, :1], ref[:, :, 1:] - ref[:, :, :1]
    d_tol = np.maximum(1e-12 * (scale[:, :, 1:] + scale[:, :, :1]), 8 * (delta[:, :, 1:] + delta[:, :, :1]))
    assert np.all(np.abs(d_got - d_ref) <= d_tol), float(np.max(np.abs(d_got - d_ref) / d_tol))
    # and they are not trivially zero: the grid moves ln L by many units
    assert np.min(np.max(np.abs(d_ref[:, [0, 2]]), axis=2)) > 1.0          # (pulsar 1 has no red noise: without the common process nothing moves it)


def test_quad_and_constant_pieces():
    """lnl_quad against r^T P0' r with P0' formed densely, with and without ECORR / a timing model"""
    arr = _array()
    for model in ("spin", None):
        for with_ecorr in (True, False):
            plan = ost.prepare_lnl([p["t"] for p in arr], [p["sigma2"] for p in arr], components=NF,
                                   epoch_of=[p["epoch_of"] for p in arr] if with_ecorr else None, ecorr=[p["ecorr"] for p in arr] if with_ecorr else None,
                                   F_rn=None, M=_M(arr, model))
            assert plan.K_rn == 0 and plan.K == 2 * NF
            psr_ep, ep_ptr, ep_idx, ep_g = plan.epochs()
            assert len(psr_ep) == len(arr) + 1 and len(ep_ptr) == len(ep_g) + 1 and (len(ep_g) > 0) == with_ecorr
            rows = _rows(arr, plan, 4, 3)
            got = ost.lnl_quad(plan, rows)
            for a, p in enumerate(arr):
                N = np.diag(p["sigma2"]).astype(np.float64)
                if with_ecorr:
                    N += (p["epoch_of"][:, None] == p["epoch_of"][None, :]) * (p["ecorr"][p["epoch_of"]] ** 2)[:, None]
                Np = N / plan.s[a]
                Pi = np.linalg.inv(Np)
                if model is not None:
                    M = timing_design_matrix(p["t"], model=model)[0]
                    M = M / np.linalg.norm(M, axis=0)
                    Pi = Pi - Pi @ M @ np.linalg.solve(M.T @ Pi @ M, M.T @ Pi)
                r = rows[:, plan.off[a]:plan.off[a + 1]]
                ref = np.einsum("ri,ij,rj->r", r, Pi, r)
                assert np.max(np.abs(got[:, a] - ref) / np.abs(ref)) < 1e-9, (model, with_ecorr, a)
            if model is not None:
                # un-fitted rows: a component inside the span of M, 200 times the error bars, leaves r^T P0' r where it was (the
                # difference of r^T N'^-1 r and || G r ||^2 would keep 4e4 eps of it; the fit residual keeps 200 eps)
                big = rows.copy()
                for a, p in enumerate(arr):
                    M = timing_design_matrix(p["t"], model=model)[0]
                    M = M / np.max(np.abs(M), axis=0)
                    big[:, plan.off[a]:plan.off[a + 1]] += 1e-4 * (M @ np.array([0.3, -1.0, 0.7]))[None, :]
                assert np.max(np.abs(ost.lnl_quad(plan, big) - got) / got) < 1e-12, (model, with_ecorr)


def test_theta_grid_shapes_and_order():
    grid, shape = ost.theta_grid(P=4, gwb_log10_A=[-15.0, -14.0], gwb_gamma=[3.0, 4.0, 5.0])
    assert shape == (2, 3) and set(grid) == {"gwb_log10_A", "gwb_gamma"}
    assert np.array_equal(grid["gwb_log10_A"], [-15, -15, -15, -14, -14, -14]) and np.array_equal(grid["gwb_gamma"], [3, 4, 5, 3, 4, 5])
    grid, shape = ost.theta_grid(P=4, rn_gamma=np.linspace(2, 6, 5), gwb_log10_A=[-15.0, -14.0])
    assert shape == (5, 2) and grid["rn_gamma"].shape == (10, 4) and grid["gwb_log10_A"].shape == (10,)
    assert np.array_equal(grid["rn_gamma"][:, 0], np.repeat(np.linspace(2, 6, 5), 2)) and np.all(grid["rn_gamma"] == grid["rn_gamma"][:, :1])
    assert np.array_equal(grid["gwb_log10_A"], np.tile([-15.0, -14.0], 5))
    with pytest.raises(ValueError, match="needs the number of pulsars"):
        ost.theta_grid(rn_log10_A=[-14.0])
    with pytest.raises(ValueError, match="unknown axes"):
        ost.theta_grid(P=2, cw_log10_mc=[9.0])
    with pytest.raises(ValueError, match="1-D"):
        ost.theta_grid(P=2, gwb_gamma=[[3.0]])
    with pytest.raises(ValueError, match="at least one axis"):
        ost.theta_grid(P=2)


# ---------------------------------------------------------------- device math header ----------------------------------------
@pytest.fixture(scope="module")
def lh(tmp_path_factory):
    out = tmp_path_factory.mktemp("lnl") / "liblnlhost.so"
    src = os.path.join(HERE, "lnl", "lnl_host.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", str(out)])
    lib = ctypes.CDLL(str(out))
    i, i64, d = ctypes.c_int, ctypes.c_int64, ctypes.c_double
    pd, pi = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    lib.lh_quad.argtypes = [pd, i64, i, pi, i, pd, pi, pi, pi, pd, pd, i64, i, i, i, pd, i64, pd]
    lib.lh_quad.restype = None
    lib.lh_q_index.argtypes = [i64, i, i, i, i, i64, i]
    lib.lh_q_index.restype = i64
    lib.lh_value.argtypes = [d, d, d, d, d]
    lib.lh_value.restype = d
    return lib


def _pd(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _pi(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def _q_blocked(q, blk):
    """q [R, P, Kt] -> the layout pta_os_project leaves when called once per block of blk operator rows"""
    R = q.shape[0]
    return np.ascontiguousarray(np.concatenate([q[:, :, k0:k0 + blk].reshape(R, -1) for k0 in range(0, q.shape[2], blk)], axis=1))


@pytest.mark.parametrize("model", ["spin", None])
@pytest.mark.parametrize("with_ecorr", [True, False])
def test_quad_header_matches_numpy(lh, model, with_ecorr):
    """the fit residual, the thread partials and the butterfly of k_lnl_quad on the CPU against lnl_quad: the same sums in another
    order, 1e-13 of the white-noise term of the rows (the result itself is smaller: the fit and the ECORR term take their share)"""
    arr = _array()
    plan = ost.prepare_lnl([p["t"] for p in arr], [p["sigma2"] for p in arr], components=NF, epoch_of=[p["epoch_of"] for p in arr] if with_ecorr else None,
                           ecorr=[p["ecorr"] for p in arr] if with_ecorr else None, F_rn=[_rn_basis(p)[0] for p in arr], M=_M(arr, model))
    R, P, K, m = 6, plan.P, plan.K, plan.m
    rows = np.ascontiguousarray(_rows(arr, plan, R, 5))
    Vt = plan.Vt()
    assert Vt.shape == (K + m, rows.shape[1])
    q = np.stack([rows[:, plan.off[a]:plan.off[a + 1]] @ Vt[:, plan.off[a]:plan.off[a + 1]].T for a in range(P)], axis=1)   # [R, P, K + m]
    blk = 16                                             # the timing-model rows straddle a block boundary (K = 32: rows 32, 33, 34)
    qb = _q_blocked(q, blk)
    for r, a, k in ((0, 0, 0), (3, 2, 17), (5, 1, K + m - 1), (2, 2, K - 1)):
        assert qb[0, 0] == q[0, 0, 0] and qb.reshape(-1)[lh.lh_q_index(r, a, k, P, K + m, qb.shape[1], blk)] == q[r, a, k]
    psr_ep, ep_ptr, ep_idx, ep_g = plan.epochs()
    Ht = np.ascontiguousarray(plan.Ht_all())
    off = plan.off.astype(np.int32)
    out = np.full((R, P), np.nan)
    lh.lh_quad(_pd(rows), rows.shape[1], R, _pi(off), P, _pd(plan.dinv), _pi(psr_ep) if with_ecorr else None, _pi(ep_ptr) if with_ecorr else None,
               _pi(ep_idx) if with_ecorr else None, _pd(ep_g) if with_ecorr else None, _pd(qb), qb.shape[1], blk, K, m, _pd(Ht) if m else None, Ht.shape[1], _pd(out))
    ref = ost.lnl_quad(plan, rows)
    white = np.stack([np.sum(rows[:, plan.off[a]:plan.off[a + 1]] ** 2 * plan.dinv[plan.off[a]:plan.off[a + 1]], axis=1) for a in range(P)], axis=1)
    worst = float(np.max(np.abs(out - ref) / white))
    print(f"model={model} ecorr={with_ecorr}: worst deviation over the white-noise term {worst:.2e}")
    assert np.all(np.isfinite(out)) and worst < 1e-13
    assert lh.lh_value(10.0, 4.0, 2.0, 1.5, 0.25) == -0.5 * ((10.0 - 4.0) / 2.0 + 1.5 + 0.25)


# ---------------------------------------------------------------- refusals ----------------------------------------------------
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
        eng.prepare_likelihood(components=15)                                  # 100 + 30 > 128
    with pytest.raises(ValueError, match="components"):
        eng.prepare_likelihood(components=33)
    with pytest.raises(ValueError, match="timing_model"):
        eng.prepare_likelihood(timing_model="full")
    assert not eng._prepared
    eng = _engine()
    G, P = 3, 4
    grid = {"rn_log10_A": np.full((G, P), -14.0), "rn_gamma": np.full((G, P), 3.0)}
    with pytest.raises(ValueError, match="not prepared"):
        eng.log_likelihood(None, grid)
    with pytest.raises(ValueError, match="not prepared"):
        eng.generate_lnl(2, grid)
    # a prepared state that belongs to an earlier prepare() of the engine
    eng._lnl = {"engine_plan": object()}
    eng._prepared, eng.plan = True, object()
    with pytest.raises(ValueError, match="re-prepared since"):
        eng.log_likelihood(None, grid)
    with pytest.raises(ValueError, match="re-prepared since"):
        eng.generate_lnl(2, grid)
    eng._prepared = False
    del eng.plan
    st = {"gw": (-14.5, 13. / 3.), "K_rn": 20}
    th, n = eng._lnl_check_grid(st, dict(grid, gwb_log10_A=np.full(G, -14.5)))
    assert n == G and set(th) == {"rn_log10_A", "rn_gamma", "gwb_log10_A"}
    assert eng._lnl_check_grid(st, {})[1] == 1
    cases = [
        ({"rn_log10_A": np.zeros((G, P - 1))}, "shape"),
        ({"rn_gamma": np.zeros(G)}, "shape"),
        ({"gwb_log10_A": np.zeros((G, P))}, "shape"),
        ({**grid, "gwb_log10_A": np.full(G + 1, -14.0)}, "leading axis"),
        ({"gwb_gamma": 4.0}, "leading grid axis"),
        ({**grid, "cw_log10_mc": np.full(G, 9.0)}, "cw_"),
        ({"gwb_amplitude": np.zeros(G)}, "unknown"),
        ({**grid, "rn_log10_A": np.full((G, P), np.inf)}, "infinite"),
        ({"gwb_log10_A": np.array([-14.0, np.nan, -14.0])}, "non-finite"),
    ]
    for bad, msg in cases:
        with pytest.raises(ValueError, match=msg):
            eng._lnl_check_grid(st, bad)
    with pytest.raises(ValueError, match="dict"):
        eng._lnl_check_grid(st, [1, 2])
    with pytest.raises(ValueError, match="without the GWB auto-term"):
        eng._lnl_check_grid({"gw": None, "K_rn": 20}, {"gwb_log10_A": np.full(G, -14.0)})
    grid2, shape = eng.theta_grid(rn_log10_A=[-15.0, -14.0], gwb_gamma=[3.0, 4.0, 5.0])
    assert shape == (2, 3) and grid2["rn_log10_A"].shape == (6, 4) and grid2["gwb_gamma"].shape == (6,)
    assert not eng._prepared


def test_k_over_the_limit_is_refused():
    arr = _array()
    wide = [po.fourier_design_matrix(p["t"], nmodes=55, Tspan=p["tspan"])[0] for p in arr]     # 110 + 2 * 10 = 130 > 128
    with pytest.raises(ValueError, match="exceeds the limit"):
        ost.prepare_lnl([p["t"] for p in arr], [p["sigma2"] for p in arr], components=10, F_rn=wide)
    with pytest.raises(ValueError, match="components"):
        ost.prepare_lnl([p["t"] for p in arr], [p["sigma2"] for p in arr], components=33)
