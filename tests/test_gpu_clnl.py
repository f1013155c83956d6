"""Likelihood ratio of a correlated common process on a (log10_A, gamma) grid on the MI355X: pta_clnl_mix / assemble / rhs / solve / finish
(with pta_potrf_batched_ex between assemble and solve) against NumPy, bit-identity across sub-batches, the engine against the host twin
(optimal_statistic.clnl_from_rows) with and without a timing model and with a chromatic process, placement independence of
generate_correlated_lnl, the tie of the "curn" ratio to the uncorrelated likelihood (log_likelihood), and the discrimination between a
Hellings-Downs and an uncorrelated injection.

Calibrated bound (the convention of tests/test_gpu_lnl.py): every |d ratio| is taken relative to scale = v^T v / 2 + |ln det M_g| (the
two terms the ratio is the difference of, v = D_g Y') and held to max(1e-12, 8 delta), delta = the disagreement, on the same scale, of the
two independent CPU fp64 evaluations of clnl_ratio (Cholesky against np.linalg.solve / slogdet).  Every such test checks delta < 1e-8 itself.

Measured on one MI355X (worst |d ratio| / scale, device against host): kernels 1.3e-14 (n = 2 .. 272; delta up to 9.8e-13), engines with 16
pulsars 9.4e-14 with the spin timing model (delta 4.3e-14), 1.8e-15 without one, 8.9e-15 with a chromatic process; the "curn" tie 3.3e-16;
mean Delta = Lambda_hd - Lambda_curn +10.17 +- 0.33 for a Hellings-Downs injection and -11.07 +- 0.32 for an uncorrelated one (R = 256)."""
import ctypes

import numpy as np
import pytest
import torch

from pta_replicator_amd import optimal_statistic as ost
from pta_replicator_amd.constants import YEAR_IN_SEC
from test_gpu_os import _engine as _engine_all_rn, _psrs

pytestmark = pytest.mark.gpu

TSPAN, GREF = 10 * YEAR_IN_SEC, 13. / 3.


def _bound(delta):
    assert delta < 1e-8, f"the inputs are too ill-conditioned for this check: delta = {delta:.3e}"
    return max(1e-12, 8 * delta)


# ---------------------------------------------------------------- kernels ---------------------------------------------------
def _problem(rho, C, R, G):
    rng = np.random.default_rng(rho * 1000003 + C * 10007 + R * 101 + G)
    n = rho * C
    Q = np.linalg.qr(rng.normal(size=(n, n)))[0]
    T = (Q * 10.0 ** rng.uniform(-2, 3, n)) @ Q.T      # SPD with eigenvalues over five decades
    T = 0.5 * (T + T.T)
    Yp = rng.normal(size=(R, n))
    lA, gam = rng.uniform(-1.0, 0.3, G), rng.uniform(2.0, 6.0, G)
    lA[G // 2] = -40.0                                 # one grid point without a common process: M = I
    return T, Yp, lA, gam


def _device(T, Yp, rho, C, lA, gam, pad=3):
    """(ratio [G, R], L [G, n, n], quad [G, R]) through the kernels, Y' with a row stride wider than its rows"""
    from pta_replicator_amd import _lib, device as dv
    n, R, G = rho * C, Yp.shape[0], len(lA)
    dT, dlA, dg = dv.f64(T), dv.f64(lA), dv.f64(gam)
    dYp = dv.zeros((R, n + pad))
    dYp[:, :n] = dv.f64(Yp)
    M, V, quad, out = dv.empty((G, n, n)), dv.empty((G, n, R)), dv.empty((G, R)), dv.empty((G, R))
    info = dv.zeros((G,), dtype=torch.int32)
    s = dv.stream_ptr()
    _lib.call("pta_clnl_assemble", dv.ptr(dT), rho, C, GREF, TSPAN, dv.ptr(dlA), dv.ptr(dg), G, dv.ptr(M), s)
    _lib.call("pta_potrf_batched_ex", dv.ptr(M), n, n, n * n, G, dv.ptr(info), _lib.POTRF_SUBSTITUTION, s)
    _lib.call("pta_clnl_rhs", dv.ptr(dYp), n + pad, rho, C, R, GREF, TSPAN, dv.ptr(dlA), dv.ptr(dg), G, dv.ptr(V), R, s)
    _lib.call("pta_clnl_solve", dv.ptr(M), n, G, dv.ptr(V), R, R, dv.ptr(quad), R, s)
    _lib.call("pta_clnl_finish", dv.ptr(M), n, G, dv.ptr(quad), R, R, dv.ptr(out), R, s)
    assert int(info.abs().max()) == 0
    return out, M, quad


@pytest.mark.parametrize("G", [1, 3, 5])
@pytest.mark.parametrize("R", [1, 17, 65, 130])
@pytest.mark.parametrize("rho,C", [(1, 2), (3, 2), (5, 14), (5, 26), (9, 30), (1, 64), (17, 16)])
def test_kernels_vs_numpy(rho, C, R, G):
    """n = 2, 6, 70, 130, 270, 64, 272: below, at and across the 64-row blocks of the substitution and the 128-row blocks of the
    factorisation, and several blocks plus a remainder; R below, at and across the 64 realisations of a workgroup.
    Measured: worst device error / scale 1.3e-14 (delta 9.8e-13 at the most)."""
    T, Yp, lA, gam = _problem(rho, C, R, G)
    n = rho * C
    D = np.tile(ost.clnl_scale(C // 2, TSPAN, GREF, lA, gam), (1, rho))
    ref, scale = ost.clnl_ratio(T, Yp, D)
    alt, _ = ost.clnl_ratio(T, Yp, D, form="solve")
    delta = float(np.max(np.abs(alt - ref) / scale))
    out, L, quad = _device(T, Yp, rho, C, lA, gam)
    got = out.t().cpu().numpy()
    err = float(np.max(np.abs(got - ref) / scale))
    print(f"rho={rho} C={C} n={n} R={R} G={G}: delta {delta:.3e}, device {err:.3e}")
    assert np.all(np.isfinite(got)) and err < _bound(delta)
    # the grid point without a common process (d ~ 1e-40: d T d is lost against the unit diagonal and is 1e-77 off it): a unit diagonal, no
    # log-determinant, and the ratio is exactly half the squared norm of D Y' - n squares summed in sequence, d within 2 ulp of NumPy's
    g0 = G // 2
    Lg = torch.tril(L[g0]).cpu().numpy()
    assert np.array_equal(np.diag(Lg), np.ones(n)) and np.max(np.abs(Lg - np.eye(n))) < 1e-70
    assert torch.equal(out[g0], 0.5 * quad[g0])
    v2 = np.sum((D[g0][None, :] * Yp) ** 2, axis=1)
    assert np.max(np.abs(quad[g0].cpu().numpy() - v2) / v2) < (n + 16) * 2.3e-16
    if R == 17 and G == 5:   # a (realisation, grid point) value does not depend on the rows or grid points that share its launch
        sub, _, subq = _device(T, Yp[13:16], rho, C, lA[2:5], gam[2:5], pad=0)
        assert torch.equal(sub, out[2:5, 13:16]) and torch.equal(subq, quad[2:5, 13:16])


@pytest.mark.parametrize("P,C,rho,R", [(1, 2, 1, 1), (5, 6, 3, 17), (16, 28, 16, 33), (68, 28, 1, 5)])
def test_mix_vs_numpy(P, C, rho, R):
    from pta_replicator_amd import _lib, device as dv
    rng = np.random.default_rng(P * 100 + rho)
    B, Y = rng.normal(size=(P, rho)), rng.normal(size=(R, P, C))
    ref = np.einsum("ai,rac->ric", B, Y).reshape(R, rho * C)
    dY, dBt, out = dv.f64(Y.reshape(R, P * C)), dv.f64(np.ascontiguousarray(B.T)), dv.zeros((R, rho * C + 5))
    _lib.call("pta_clnl_mix", dv.ptr(dY), P * C, P, C, R, dv.ptr(dBt), rho, dv.ptr(out), rho * C + 5, dv.stream_ptr())
    got = out.cpu().numpy()
    size = np.einsum("ai,rac->ric", np.abs(B), np.abs(Y)).reshape(R, rho * C)
    assert np.max(np.abs(got[:, :rho * C] - ref) / size) < 2.3e-16 * (P + 2) and np.all(got[:, rho * C:] == 0)
    if R >= 17:
        sub = dv.zeros((3, rho * C))
        _lib.call("pta_clnl_mix", ctypes.c_void_p(dY.data_ptr() + 8 * 13 * P * C), P * C, P, C, 3, dv.ptr(dBt), rho, dv.ptr(sub), rho * C, dv.stream_ptr())
        assert torch.equal(sub, out[13:16, :rho * C])


# ---------------------------------------------------------------- engines -----------------------------------------------------
NAMES = ("hd", "monopole", "dipole", "curn")


def _chrom_engine():
    from pta_replicator_amd.engine import ReplicaEngine
    psrs = _psrs(16, 120, 11)
    for p in psrs:
        p.toas.freqs_mhz = np.where(np.arange(len(p.toas.freqs_mhz)) % 2, 820.0, 1440.0)
    eng = ReplicaEngine(psrs, seed=77)
    eng.td_warmup = False
    eng.set_white_noise(efac=1.05)
    eng.set_red_noise(-14.0, 3.5, components=10)
    eng.set_chromatic_noise(-13.6, 3.0, components=8)
    eng.set_gwb(-14.4, 13. / 3.)
    eng.prepare()
    return eng


def _compare(eng, rows, grid, what):
    res = eng.correlated_log_likelihood(rows, grid)
    plan = eng._clnl["plan"]
    from pta_replicator_amd import engine_clnl
    lA, gam = engine_clnl.check_grid(grid, None if eng._gw is None else eng._gw["A"], eng._clnl["gamma"])
    h = rows.cpu().numpy()
    ref, scale = ost.clnl_from_rows(plan, h, lA, gam, with_scale=True)
    alt = ost.clnl_from_rows(plan, h, lA, gam, form="solve")
    delta = float(np.max(np.abs(alt - ref) / scale))
    got = res["lnl_ratio"].cpu().numpy()
    assert got.shape == ref.shape == (h.shape[0], len(plan.names), len(lA)) and res["names"] == list(plan.names)
    err = float(np.max(np.abs(got - ref) / scale))
    print(f"{what}: delta {delta:.3e}, device {err:.3e}")
    assert np.all(np.isfinite(got)) and err < _bound(delta)
    return res, ref


@pytest.mark.parametrize("kind", ["spin", "no timing model", "chromatic"])
def test_engine_vs_host_twin(kind):
    """16 ragged pulsars; ECORR + red noise with the spin timing model, the same without a timing model, and white noise + red noise +
    a chromatic process (whose columns sit in the fixed low-rank part).  Four named ORFs (n = 448, 28, 84, 448), G = 6, R = 33.
    Measured: worst device error / scale 9.4e-14 (spin; delta 4.3e-14), 1.8e-15 (no timing model), 8.9e-15 (chromatic)."""
    eng = _chrom_engine() if kind == "chromatic" else _engine_all_rn(P=16, n0=120)
    eng.prepare_correlated_likelihood(components=14, orfs=NAMES, timing_model=None if kind == "no timing model" else "spin")
    st = eng._clnl
    assert st["rho"] == [16, 1, 3, 16] and st["n"] == [448, 28, 84, 448]
    rows = eng.generate(33, r0=5)
    grid, shape = eng.theta_grid(gwb_log10_A=[-15.2, -14.4, -13.6], gwb_gamma=[3.2, 5.0])
    assert shape == (3, 2)
    _compare(eng, rows, grid, f"{kind}, theta_grid")
    _compare(eng, rows[:3], {}, f"{kind}, one grid point as configured")
    _compare(eng, rows[:3], {"gwb_gamma": torch.as_tensor([3.0, 4.0])}, f"{kind}, index only")
    if kind == "chromatic":   # the refusals of an engine with a chromatic process stay what they were
        with pytest.raises(ValueError, match="chromatic"):
            eng.prepare_likelihood()
        with pytest.raises(ValueError, match="no TD mode"):
            eng.generate_correlated_lnl(4, grid, td=True)
        with pytest.raises(ValueError, match="configured one"):
            eng.correlated_log_likelihood(rows, {"chrom_log10_A": np.zeros((1, 16))})


def test_single_pulsar_and_user_orf():
    from pta_replicator_amd.engine import ReplicaEngine
    eng = ReplicaEngine(_psrs(1, 200, 5), seed=3)
    eng.td_warmup = False
    eng.set_white_noise(efac=1.0)
    eng.set_red_noise([-13.8], [3.5], components=15)
    eng.prepare()
    eng.prepare_correlated_likelihood(components=6, orfs=("hd", "curn", np.array([[2.5]])))
    assert eng._clnl["n"] == [12, 12, 12] and eng._clnl["names"] == ["hd", "curn", "orf2"]
    rows = eng.generate(9)
    with pytest.raises(ValueError, match="given nowhere"):
        eng.correlated_log_likelihood(rows, {"gwb_gamma": np.array([4.0])})
    res, _ = _compare(eng, rows, {"gwb_log10_A": np.linspace(-15, -13, 5)}, "one pulsar")
    assert torch.equal(res["lnl_ratio"][:, 0], res["lnl_ratio"][:, 1])           # one pulsar: every unit-diagonal ORF is the same model
    eng = _engine_all_rn(P=6)
    rng = np.random.default_rng(4)
    A = rng.normal(size=(6, 2))
    eng.prepare_correlated_likelihood(components=5, orfs=(A @ A.T, "hd"))
    assert eng._clnl["rho"] == [2, 6]
    _compare(eng, eng.generate(7), {"gwb_log10_A": [-14.5, -13.9]}, "user ORF of rank 2")


def test_placement_independence():
    """generate_correlated_lnl against correlated_log_likelihood(generate(...)), bit for bit: the chunk, a workspace so small that both
    the realisations and the grid are cut (no factor is then reused), r0, TD mode, and rows that are a strided view"""
    eng = _engine_all_rn(P=16, n0=120, gw=None)
    eng.prepare_td()
    eng.prepare_correlated_likelihood(components=5, orfs=("hd", "curn"))
    R, G = 33, 6
    grid, _ = eng.theta_grid(gwb_log10_A=[-15.0, -14.0, -13.5], gwb_gamma=[3.5, 13. / 3.])
    rows = eng.generate(R, r0=5)
    ref = eng.correlated_log_likelihood(rows, grid)["lnl_ratio"]
    assert ref.shape == (R, 2, G)
    for chunk in (7, 1024):
        assert torch.equal(eng.generate_correlated_lnl(R, grid, r0=5, chunk=chunk)["lnl_ratio"], ref), chunk
    assert torch.equal(eng.generate_correlated_lnl(9, grid, r0=12, chunk=4)["lnl_ratio"], ref[7:16])
    wide = torch.full((R, eng.n_toa + 7), float("nan"), dtype=torch.float64, device=rows.device)
    wide[:, :eng.n_toa] = rows
    assert torch.equal(eng.correlated_log_likelihood(wide[:, :eng.n_toa], grid)["lnl_ratio"], ref)
    assert torch.equal(eng.correlated_log_likelihood(rows[4:9], {k: v[2:5] for k, v in grid.items()})["lnl_ratio"], ref[4:9, :, 2:5])
    ws = eng.workspace_bytes
    try:
        eng.workspace_bytes = int(1.25 * 8 * sum(n * n for n in eng._clnl["n"]))
        for with_rows in (False, True):
            Rc, Gc = eng._clnl_chunks(eng._clnl, R, G, with_rows=with_rows)
            assert 1 <= Rc < R and 1 <= Gc < G, (Rc, Gc)
        assert torch.equal(eng.correlated_log_likelihood(rows, grid)["lnl_ratio"], ref)
        assert torch.equal(eng.generate_correlated_lnl(12, grid, r0=5)["lnl_ratio"], ref[:12])   # one realisation per chunk
    finally:
        eng.workspace_bytes = ws
    td = eng.correlated_log_likelihood(eng.generate_td(R, r0=5), grid)["lnl_ratio"]
    for chunk in (7, 1024):
        assert torch.equal(eng.generate_correlated_lnl(R, grid, r0=5, td=True, chunk=chunk)["lnl_ratio"], td), chunk
    eng.set_hyper_prior(rn_log10_A=(-14.5, -13.5))
    eng.prepare_correlated_likelihood(components=5, orfs=("hd", "curn"))      # set_hyper_prior re-prepares the engine
    theta = eng.sample_theta(R)
    th = eng.correlated_log_likelihood(eng.generate(R, theta=theta), grid)["lnl_ratio"]
    assert torch.equal(eng.generate_correlated_lnl(R, grid, theta=theta, chunk=7)["lnl_ratio"], th)


def test_curn_ties_to_the_uncorrelated_likelihood():
    """an engine without red noise: the fixed model of this likelihood and the grid model of log_likelihood coincide, and the "curn" ratio
    is ln L(grid point) - ln L(vanishing amplitude) of log_likelihood.  Bound: the calibrated one on the larger of the two scales (the
    uncorrelated likelihood's |ln L| + r^T P0' r / s, summed over the pulsars).  Measured: 3.3e-16 (delta 8.0e-16); against the host twin 5.3e-16."""
    eng = _engine_all_rn(P=16, n0=120, rn=False)
    nf = 8
    eng.prepare_likelihood(components=nf, timing_model="spin")
    eng.prepare_correlated_likelihood(components=nf, orfs=("curn",), timing_model="spin")
    R = 12
    rows = eng.generate(R)
    grid, _ = eng.theta_grid(gwb_log10_A=[-15.0, -14.4, -13.8], gwb_gamma=[3.0, 13. / 3.])
    G = 6
    got = eng.correlated_log_likelihood(rows, grid)["lnl_ratio"][:, 0, :]
    tie = eng.log_likelihood(rows, grid)["lnl"] - eng.log_likelihood(rows, {"gwb_log10_A": np.array([-30.0])})["lnl"]
    # the scales and delta of both sides on the host
    h = rows.cpu().numpy()
    cref, cscale = ost.clnl_from_rows(eng._clnl["plan"], h, grid["gwb_log10_A"], grid["gwb_gamma"], with_scale=True)
    calt = ost.clnl_from_rows(eng._clnl["plan"], h, grid["gwb_log10_A"], grid["gwb_gamma"], form="solve")
    lp = eng._lnl["plan"]
    b = ost.matched_prior(G, lp.s, nf=nf, T=lp.T, gw_log10_A=grid["gwb_log10_A"], gw_gamma=grid["gwb_gamma"])
    lref, _ = ost.lnl_from_rows(lp, h, b)
    lalt, _ = ost.lnl_from_rows(lp, h, b, form="solve")
    lscale = np.abs(lref) + (ost.lnl_quad(lp, h) / lp.s[None, :])[:, :, None]
    delta = max(float(np.max(np.abs(calt - cref) / cscale)), float(np.max(np.abs(lalt - lref) / lscale)))
    scale = np.maximum(cscale[:, 0, :], lscale.sum(axis=1))
    err = float(np.max(np.abs((got - tie).cpu().numpy()) / scale))
    err_host = float(np.max(np.abs(got.cpu().numpy() - cref[:, 0, :]) / cscale[:, 0, :]))
    print(f"curn tie: delta {delta:.3e}, device ratio against device ln L difference {err:.3e}, against the host twin {err_host:.3e}")
    assert err < _bound(delta) and err_host < _bound(delta)


@pytest.mark.parametrize("no_correlations", [False, True])
def test_discrimination(no_correlations):
    """16 pulsars, 0.1 us white noise, a GWB of log10_A = -14, R = 256, n_f = 5: Delta = Lambda_hd - Lambda_curn at the injected (A, gamma)
    is positive for a Hellings-Downs injection and negative for an uncorrelated one, by more than 5 standard errors of the mean.
    Measured: Hellings-Downs injection mean Delta = +10.17 +- 0.33 (30.6 standard errors), uncorrelated injection -11.07 +- 0.32 (34.7)."""
    from pta_replicator_amd.engine import ReplicaEngine
    eng = ReplicaEngine(_psrs(16, 200, 21, step=0, sessions=False, err_us=0.1), seed=8)
    eng.td_warmup = False
    eng.set_white_noise(efac=1.0)
    eng.set_gwb(-14.0, 13. / 3., no_correlations=no_correlations)
    eng.prepare()
    eng.prepare_correlated_likelihood(components=5, orfs=("hd", "curn"))
    R = 256
    lam = eng.generate_correlated_lnl(R, {})["lnl_ratio"][:, :, 0].cpu().numpy()
    d = lam[:, 0] - lam[:, 1]
    mean, se = float(d.mean()), float(d.std(ddof=1) / np.sqrt(R))
    print(f"no_correlations={no_correlations}: mean Delta = {mean:.3f} +- {se:.3f} ({mean / se:.1f} standard errors); mean Lambda_hd {lam[:, 0].mean():.2f}, "
          f"Lambda_curn {lam[:, 1].mean():.2f}")
    assert np.all(np.isfinite(lam))
    if no_correlations:
        assert mean < -5 * se
    else:
        assert mean > 5 * se
