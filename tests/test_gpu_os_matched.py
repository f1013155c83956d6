"""Optimal statistic under per-realisation noise parameters on the MI355X: pta_os_matched_solve / pta_os_matched_pairs /
pta_os_matched_prior against NumPy, the engine against the host evaluation (optimal_statistic.matched_from_rows), the configured
theta against the fixed-noise path, bit-identity across chunks / offsets / batches, the calibration of the null SNR over a prior,
the headline array and the refusals.

Calibrated bound: max(1e-12, 8 delta), delta = the disagreement of two independent CPU fp64 evaluations of the same quantity (the
Cholesky form against the np.linalg.solve form of matched_solve).  The device orders its K-long sums differently from both, which the
factor 8 covers; an algebra or indexing error is many orders of magnitude larger.  Every such test checks delta < 1e-8 itself.
At 68 x 5000 delta also takes the disagreement of the host evaluation with a dense OS of three of the pulsars: the two host forms
share one projection q = V r, and at 5000 TOAs its rounding, amplified by the subtraction in X, is the larger part of the error."""
import ctypes
import time

import numpy as np
import pytest
import torch

from pta_replicator_amd import optimal_statistic as ost
from test_gpu_os import _engine as _engine_all_rn, _psrs

pytestmark = pytest.mark.gpu


def _nrel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


def _bound(delta):
    assert delta < 1e-8, f"the inputs are too ill-conditioned for this check: delta = {delta:.3e}"
    return max(1e-12, 8 * delta)


def _unpack(Zp, C):
    """[..., C (C + 1) / 2] packed lower triangles -> symmetric [..., C, C]"""
    i, j = np.tril_indices(C)
    Z = np.zeros(Zp.shape[:-1] + (C, C))
    Z[..., i, j] = Zp
    Z[..., j, i] = Zp
    return Z


def _pack(Z):
    i, j = np.tril_indices(Z.shape[-1])
    return np.ascontiguousarray(Z[..., i, j])


def _q_blocked(q, blk):
    """q [R, P, K] -> the layout pta_os_project leaves when called once per block of blk rows of V: [R, sum_blocks P * cb]"""
    R, P, K = q.shape
    return np.concatenate([q[:, :, k0:k0 + blk].reshape(R, -1) for k0 in range(0, K, blk)], axis=1)


# ---------------------------------------------------------------- kernels ---------------------------------------------------
@pytest.mark.parametrize("R", [1, 17, 1000])
@pytest.mark.parametrize("K,C", [(2, 2), (29, 2), (29, 28), (88, 2), (88, 28), (88, 64), (128, 2), (128, 28), (128, 64)])
def test_matched_solve_vs_numpy(K, C, R):
    from pta_replicator_amd import _lib, device as dv
    P = 2
    rng = np.random.default_rng(K * 100000 + C * 1000 + R)
    A = np.zeros((P, K, K))
    for a in range(P):                               # SPD with eigenvalues over five decades
        Q = np.linalg.qr(rng.normal(size=(K, K)))[0]
        A[a] = (Q * 10.0 ** rng.uniform(-2, 3, K)) @ Q.T
        A[a] = 0.5 * (A[a] + A[a].T)
    b = rng.uniform(0, 3, (R, P, K)) * (rng.uniform(size=(R, P, K)) > 0.2)     # a fifth of the prior variances are exactly zero
    b[0, 0, :] = 0.0                                 # and one whole problem has none: Mc = I
    q = rng.normal(size=(R, P, K))
    S, s = rng.uniform(0.5, 2.0, C), rng.uniform(0.5, 2.0, P)
    blk = 64 if R == 17 else K                       # the blocked q layout of the engine, and the plain one
    qd = dv.f64(_q_blocked(q, blk))
    X, Z = dv.zeros((R, P, C)), dv.zeros((R, P, C * (C + 1) // 2))
    dA, db, dS, ds = dv.f64(A), dv.f64(b), dv.f64(S), dv.f64(s)
    _lib.call("pta_os_matched_solve", dv.ptr(dA), P, K, C, R, dv.ptr(db), dv.ptr(qd), P * K, blk, dv.ptr(dS), dv.ptr(ds), dv.ptr(X), dv.ptr(Z),
              dv.stream_ptr())
    Xr, Zr = ost.matched_solve(A[None], b, q, S, s[None, :])
    Xs, Zs = ost.matched_solve(A[None], b, q, S, s[None, :], form="solve")
    delta = max(_nrel(Xs, Xr), _nrel(Zs, Zr))
    eX, eZ = _nrel(X.cpu().numpy(), Xr), _nrel(_unpack(Z.cpu().numpy(), C), Zr)
    print(f"K={K} C={C} R={R}: delta {delta:.3e}, device X {eX:.3e} Z {eZ:.3e}")
    assert max(eX, eZ) < _bound(delta)
    if R >= 17:   # a problem's result does not depend on the batch it is computed in
        X2, Z2 = dv.zeros((3, P, C)), dv.zeros((3, P, C * (C + 1) // 2))
        q2, b2 = dv.f64(_q_blocked(q[13:16], blk)), dv.f64(b[13:16])
        _lib.call("pta_os_matched_solve", dv.ptr(dA), P, K, C, 3, dv.ptr(b2), dv.ptr(q2), P * K, blk, dv.ptr(dS), dv.ptr(ds), dv.ptr(X2), dv.ptr(Z2),
                  dv.stream_ptr())
        assert torch.equal(X2, X[13:16]) and torch.equal(Z2, Z[13:16])


def test_matched_solve_refuses_large_k():
    from pta_replicator_amd import _lib, device as dv
    x = dv.zeros((1,))
    for K, C in ((129, 28), (88, 65), (20, 28), (0, 0)):
        with pytest.raises(_lib.PtaError, match="pta_os_matched_solve"):
            _lib.call("pta_os_matched_solve", dv.ptr(x), 2, K, C, 1, dv.ptr(x), dv.ptr(x), 2 * K, 64, dv.ptr(x), dv.ptr(x), dv.ptr(x), dv.ptr(x),
                      dv.stream_ptr())


@pytest.mark.parametrize("n_orf", [1, 3])
@pytest.mark.parametrize("with_pairs", [False, True])
def test_matched_pairs_vs_numpy(with_pairs, n_orf):
    """fp64 dot products of lengths C and C^2 and sums over the pairs, in another order than NumPy's: 1e-12 of the largest entry
    (the bound tests/test_gpu_os.py holds pta_os_pairs to)"""
    from pta_replicator_amd import _lib, device as dv
    P, C, R = 23, 28, 37
    rng = np.random.default_rng(4 + n_orf)
    X = rng.normal(size=(R, P, C))
    B = rng.normal(size=(R, P, C, C))
    Z = B @ np.swapaxes(B, -1, -2) / C               # positive semi-definite: tr(Z_a Z_b) > 0
    ia, ib = np.triu_indices(P, 1)
    npairs = len(ia)
    G = rng.normal(size=(n_orf, npairs))
    dX, dZ, dG, dG2 = dv.f64(X), dv.f64(_pack(Z)), dv.f64(G), dv.f64(G ** 2)
    pa, pb = dv.i32(ia), dv.i32(ib)
    A2, sg = dv.zeros((R, n_orf + 1)), dv.zeros((R, n_orf))
    rho = dv.zeros((R, npairs)) if with_pairs else None
    sp = dv.zeros((R, npairs)) if with_pairs else None
    _lib.call("pta_os_matched_pairs", dv.ptr(dX), dv.ptr(dZ), P, C, R, dv.ptr(pa), dv.ptr(pb), npairs, dv.ptr(dG), dv.ptr(dG2), n_orf, dv.ptr(A2),
              n_orf + 1, dv.ptr(sg), n_orf, dv.ptr(rho), dv.ptr(sp), npairs if with_pairs else 0, dv.stream_ptr())
    num = np.einsum("rpc,rpc->rp", X[:, ia], X[:, ib])
    den = np.einsum("rpij,rpij->rp", Z[:, ia], Z[:, ib])
    norm = den @ (G ** 2).T

    def rel(a, ref):
        return float(np.max(np.abs(a - ref)) / np.max(np.abs(ref)))
    errs = {"A2": rel(A2.cpu().numpy()[:, :n_orf], (num @ G.T) / norm), "sigma": rel(sg.cpu().numpy(), norm ** -0.5)}
    assert np.all(A2.cpu().numpy()[:, n_orf] == 0)    # nothing written past n_orf
    if with_pairs:
        errs.update(rho=rel(rho.cpu().numpy(), num / den), sigma_pair=rel(sp.cpu().numpy(), den ** -0.5))
    print(errs)
    assert max(errs.values()) < 1e-12
    # realisation r alone gives the same bits
    A2b, sgb = dv.zeros((1, n_orf)), dv.zeros((1, n_orf))
    _lib.call("pta_os_matched_pairs", ctypes.c_void_p(dX.data_ptr() + 8 * 5 * P * C), ctypes.c_void_p(dZ.data_ptr() + 8 * 5 * P * (C * (C + 1) // 2)), P,
              C, 1, dv.ptr(pa), dv.ptr(pb), npairs, dv.ptr(dG), dv.ptr(dG2), n_orf, dv.ptr(A2b), n_orf, dv.ptr(sgb), n_orf, None, None, 0,
              dv.stream_ptr())
    assert torch.equal(A2b[0], A2[5, :n_orf]) and torch.equal(sgb[0], sg[5])


# ---------------------------------------------------------------- engines -----------------------------------------------------
RN_A = [-14.0, -13.6, None, -13.9, -14.3, -13.7]
RN_G = [3.0, 3.4, None, 4.1, 2.6, 3.8]


def _engine(gw=-14.4, seed=77, P=6):
    """6 ragged pulsars with ECORR sessions; pulsar 2 is configured without red noise"""
    from pta_replicator_amd.engine import ReplicaEngine
    eng = ReplicaEngine(_psrs(P, 150, 11), seed=seed)
    eng.td_warmup = False
    fl = [["A", "B"]] * P
    eng.set_white_noise(efac=[np.array([1.1, 0.9])] * P, log10_equad=[np.array([-6.5, -6.8])] * P, flags=fl)
    eng.set_jitter(log10_ecorr=[np.array([-6.6, -6.9])] * P, flags=fl, coarsegrain=0.1)
    eng.set_red_noise(RN_A[:P], RN_G[:P], components=20)
    if gw is not None:
        eng.set_gwb(gw, 13. / 3.)
    eng.prepare()
    return eng


def _host(eng, rows, theta, form="cholesky"):
    """the host evaluation of the engine's matched OS: its MatchedPlan, b from theta by matched_prior with the engine's tables"""
    m = eng._os["matched"]
    mp = m["plan"]
    R, P = rows.shape[0], eng.P

    def get(k):
        v = theta.get(k)
        return None if v is None else (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v, dtype=np.float64))
    lA, g = get("rn_log10_A"), get("rn_gamma")
    conf_A = np.array([np.nan if x is None else x for x in eng._rn["A"]])
    conf_g = np.array([np.nan if x is None else x for x in eng._rn["g"]])
    if lA is not None or g is not None:
        lA = np.broadcast_to(conf_A, (R, P)).copy() if lA is None else lA.copy()
        g = np.broadcast_to(conf_g, (R, P)).copy() if g is None else g.copy()
        lA[:, np.isnan(conf_A)] = np.nan
    gl = gg = None
    if m["gw"] is not None:
        gl = get("gwb_log10_A") if "gwb_log10_A" in theta else np.full(R, m["gw"][0])
        gg = get("gwb_gamma") if "gwb_gamma" in theta else np.full(R, m["gw"][1])
    b = ost.matched_prior(R, mp.s, np.stack(eng.rn_freqs), np.array([t.max() - t.min() for t in eng.tdb_s]), eng.rn_amp ** 2, lA, g, mp.nf, mp.T,
                          gl, gg)
    return ost.matched_from_rows(mp, rows.cpu().numpy(), b, form=form)


KEYS = ("A2", "sigma", "snr", "rho", "sigma_pair")


def _compare(res, ref, alt, what, delta_floor=0.0):
    delta = max([delta_floor] + [_nrel(alt[k], ref[k]) for k in KEYS])
    errs = {k: _nrel(res[k].cpu().numpy(), ref[k]) for k in KEYS}
    print(f"{what}: delta {delta:.3e}, device", {k: f"{v:.3e}" for k, v in errs.items()})
    assert max(errs.values()) < _bound(delta), errs
    return delta


@pytest.mark.parametrize("model", ["spin", "astrometric"])
def test_engine_matched_vs_host(model):
    eng = _engine()
    eng.prepare_optimal_statistic(components=10, timing_model=model, matched=True)
    R, P = 24, eng.P
    rng = np.random.default_rng(3)
    lA = rng.uniform(-15.0, -13.2, (R, P))
    lA[::5] = np.nan                                  # whole realisations, and single pulsars, "as configured"
    lA[1::4, 3] = np.nan
    g = np.where(np.isnan(lA), np.nan, rng.uniform(2, 6, (R, P)))
    thetas = {
        "rn+gw amplitude": {"rn_log10_A": lA, "rn_gamma": g, "gwb_log10_A": rng.uniform(-15, -14, R)},
        "gw only, own index": {"gwb_log10_A": torch.as_tensor(rng.uniform(-15, -14, R)), "gwb_gamma": rng.uniform(3, 5.5, R)},
        "rn index only": {"rn_gamma": rng.uniform(2, 5, (R, P))},
    }
    for what, theta in thetas.items():
        rows = eng.generate(R, r0=5, theta=theta)
        res = eng.optimal_statistic(rows, pairs=True, theta=theta)
        assert res["sigma"].shape == (R, 3) and res["sigma_pair"].shape == (R, P * (P - 1) // 2) and res["names"] == ["hd", "monopole", "dipole"]
        assert res["pairs"].shape == (P * (P - 1) // 2, 2) and res["zeta"].shape == (P * (P - 1) // 2,)
        _compare(res, _host(eng, rows, theta), _host(eng, rows, theta, form="solve"), f"{model}, {what}")
    # the caller's own residuals, and cw_* keys ignored
    rows = torch.as_tensor(rng.normal(0, 1e-6, (5, eng.n_toa)), device=rows.device)
    theta = {"rn_log10_A": lA[:5], "rn_gamma": g[:5], "cw_log10_mc": np.full(5, 9.0)}
    _compare(eng.optimal_statistic(rows, pairs=True, theta=theta), _host(eng, rows, theta), _host(eng, rows, theta, form="solve"), "own residuals")


def test_engine_matched_gwb_auto_off_and_no_red_noise():
    eng = _engine()
    eng.prepare_optimal_statistic(components=8, gwb_auto=False, matched=True)
    R = 6
    theta = {"rn_log10_A": np.full((R, eng.P), -13.8), "rn_gamma": np.full((R, eng.P), 3.3)}
    rows = eng.generate(R, theta=theta)
    _compare(eng.optimal_statistic(rows, pairs=True, theta=theta), _host(eng, rows, theta), _host(eng, rows, theta, form="solve"), "gwb_auto=False")
    # an engine without any red noise: K = C, theta holds the GWB alone
    from pta_replicator_amd.engine import ReplicaEngine
    eng = ReplicaEngine(_psrs(4, 100, 5), seed=3)
    eng.td_warmup = False
    eng.set_white_noise(efac=1.0)
    eng.set_gwb(-14.2, 13. / 3.)
    eng.prepare()
    eng.prepare_optimal_statistic(components=6, matched=True)
    m = eng._os["matched"]
    assert m["K_rn"] == 0 and m["K"] == 12
    theta = {"gwb_log10_A": np.linspace(-15, -14, R)}
    rows = eng.generate(R, theta=theta)
    res = eng.optimal_statistic(rows, pairs=True, theta=theta)
    ref = ost.matched_from_rows(m["plan"], rows.cpu().numpy(),
                                ost.matched_prior(R, m["plan"].s, nf=6, T=m["plan"].T, gw_log10_A=theta["gwb_log10_A"], gw_gamma=np.full(R, 13. / 3.)))
    alt = ost.matched_from_rows(m["plan"], rows.cpu().numpy(),
                                ost.matched_prior(R, m["plan"].s, nf=6, T=m["plan"].T, gw_log10_A=theta["gwb_log10_A"], gw_gamma=np.full(R, 13. / 3.)),
                                form="solve")
    _compare(res, ref, alt, "no red noise")


@pytest.mark.parametrize("gwb_auto", [None, False])
def test_configured_theta_reproduces_fixed_path(gwb_auto):
    eng = _engine()
    eng.prepare_optimal_statistic(components=12, gwb_auto=gwb_auto, matched=True)
    R, P = 20, eng.P
    rows = eng.generate(R)
    fixed = eng.optimal_statistic(rows, pairs=True)
    theta = {"rn_log10_A": np.array([[-14.0 if a is None else a for a in RN_A]] * R), "rn_gamma": np.array([[3.0 if x is None else x for x in RN_G]] * R)}
    if gwb_auto is None:
        theta.update(gwb_log10_A=np.full(R, -14.4), gwb_gamma=np.full(R, 13. / 3.))
    res = eng.optimal_statistic(rows, pairs=True, theta=theta)
    errs = {k: _nrel(res[k].cpu().numpy(), fixed[k].cpu().numpy()) for k in ("A2", "snr", "rho")}
    sig = max(_nrel(res["sigma"][r].cpu().numpy(), fixed["sigma"].cpu().numpy()) for r in range(R))
    sigp = max(_nrel(res["sigma_pair"][r].cpu().numpy(), fixed["sigma_pair"].cpu().numpy()) for r in range(R))
    print(f"gwb_auto={gwb_auto}: configured theta against the fixed path", errs, "sigma rows", sig, "sigma_pair rows", sigp)
    assert max(errs.values()) < 1e-9 and sig < 1e-9 and sigp < 1e-9
    # the default calls are today's: no theta -> the fixed-noise tensors, sigma [n_orf]
    assert fixed["sigma"].shape == (3,) and torch.equal(eng.optimal_statistic(rows)["A2"], fixed["A2"])
    # "as configured" through NaN amplitudes is the same model
    nan = {"rn_log10_A": np.full((R, P), np.nan), "rn_gamma": np.full((R, P), np.nan)}
    res2 = eng.optimal_statistic(rows, theta=nan)
    assert _nrel(res2["A2"].cpu().numpy(), fixed["A2"].cpu().numpy()) < 1e-9


# ---------------------------------------------------------------- bit-identity ------------------------------------------------
def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in KEYS if k in a)


def test_generate_os_matched_bit_identical():
    eng = _engine()
    eng.set_hyper_prior(gwb_log10_A=(-15.0, -14.0), gwb_gamma=(3.5, 5.0), rn_log10_A=(-14.8, -13.3), rn_gamma=(2.0, 5.0))
    eng.prepare_optimal_statistic(components=14, matched=True)
    R = 300
    theta = eng.sample_theta(R)
    ref = eng.optimal_statistic(eng.generate(R, theta=theta), pairs=True, theta=theta)
    assert bool(torch.isfinite(ref["snr"]).all())
    for chunk in (7, 256, R):
        assert _same(eng.generate_os(R, theta=theta, matched=True, chunk=chunk, pairs=True), ref), chunk
    sub_theta = {k: v[123:173] for k, v in theta.items()}
    sub = eng.generate_os(50, r0=123, theta=sub_theta, matched=True, chunk=16, pairs=True)
    assert all(torch.equal(sub[k], ref[k][123:173]) for k in KEYS)
    # a realisation recomputed inside a different batch (of generate and of the OS) is the same numbers
    th9 = {k: v[200:209] for k, v in theta.items()}
    again = eng.optimal_statistic(eng.generate(9, r0=200, theta=th9), pairs=True, theta=th9)
    assert all(torch.equal(again[k], ref[k][200:209]) for k in KEYS)
    # a small workspace cuts the chunks of both entry points; the numbers stay
    keep = eng.workspace_bytes
    try:
        eng.workspace_bytes = 40 * 8 * (eng.n_toa + eng.P * (2 * eng._os["matched"]["K"] + 28 + 406))
        assert _same(eng.generate_os(R, theta=theta, matched=True, pairs=True), ref)
        assert _same(eng.optimal_statistic(eng.generate(R, theta=theta), pairs=True, theta=theta), ref)
    finally:
        eng.workspace_bytes = keep
    # and the fixed-noise path is what it was: matched preparation changes nothing in it
    fixed = eng.generate_os(64, theta={k: v[:64] for k, v in theta.items()})
    eng2 = _engine()
    eng2.prepare_optimal_statistic(components=14)
    assert torch.equal(eng2.generate_os(64, theta={k: v[:64] for k, v in theta.items()})["A2"], fixed["A2"]) and fixed["sigma"].shape == (3,)


# ---------------------------------------------------------------- statistics --------------------------------------------------
def test_null_snr_is_calibrated_over_a_prior():
    """The array of test_exact_null_is_unit_variance, no GWB, red noise drawn per realisation from rn_log10_A ~ U(-15, -12.5),
    rn_gamma ~ U(2, 6).  Evaluated under each realisation's own theta the model is the data covariance: every ORF's SNR has zero
    mean and unit variance (that test's bounds).  The fixed-noise statistic of the same realisations is not calibrated (std > 2)."""
    eng = _engine_all_rn(P=16, n0=120, gw=None, psr_seed=3)
    eng.set_hyper_prior(rn_log10_A=(-15, -12.5), rn_gamma=(2, 6))
    eng.prepare_optimal_statistic(components=14, gwb_auto=False, matched=True)
    R = 4096
    theta = eng.sample_theta(R)
    snr = eng.generate_os(R, theta=theta, matched=True, chunk=1024)["snr"].cpu().numpy()
    fixed = eng.generate_os(R, theta=theta, chunk=1024)["snr"].cpu().numpy()
    m, s = snr.mean(axis=0), snr.std(axis=0)
    print("matched null SNR mean", m, "std", s)
    print("fixed-noise null SNR mean", fixed.mean(axis=0), "std", fixed.std(axis=0))
    assert np.all(np.isfinite(snr))
    assert np.all(np.abs(m) < 5 / np.sqrt(R)), m
    assert np.all((s > 0.94) & (s < 1.06)), s
    assert np.all(fixed.std(axis=0) > 2), fixed.std(axis=0)


def test_headline_size_matched_vs_host():
    import bench
    from pta_replicator_amd.engine import ReplicaEngine
    psrs, noise = bench.headline_array()
    eng = bench.configure_engine(ReplicaEngine(psrs, seed=5), noise)
    eng.td_warmup = False
    eng.prepare()
    t0 = time.perf_counter()
    eng.prepare_optimal_statistic()
    t1 = time.perf_counter()
    eng.prepare_optimal_statistic(matched=True)
    t2 = time.perf_counter()
    print(f"host preparation at 68 x 5000: fixed {t1 - t0:.2f} s, with matched=True {t2 - t1:.2f} s")
    assert eng._os["matched"]["K"] == 88 and eng._os["C"] == 28
    eng.set_hyper_prior(gwb_log10_A=(-15.0, -14.3), gwb_gamma=(3.5, 5.0), rn_log10_A=(-15.5, -13.5), rn_gamma=(2.0, 5.0))
    R = 16
    theta = eng.sample_theta(R)
    rows = eng.generate(R, theta=theta)
    res = eng.optimal_statistic(rows, pairs=True, theta=theta)
    ref = _host(eng, rows, theta)
    # delta at this size comes from a dense OS of three of the pulsars.  The two host forms share one q = V r, so their disagreement
    # does not hold the rounding of the 5000-term projection, which the subtraction in X amplifies and which the device, with its own
    # projection, does not share with the host; the dense OS never forms q.
    delta = _dense_delta(eng, rows.cpu().numpy(), theta, ref, (0, 1, 2))
    _compare(res, ref, _host(eng, rows, theta, form="solve"), "headline 68 x 5000", delta_floor=delta)


def _dense_delta(eng, rows, theta, ref, which, model="spin"):
    """disagreement of the host reduced-rank evaluation `ref` with a dense NumPy OS on the pulsars `which`: C_a(theta_r) assembled
    explicitly from the engine's configuration, np.linalg.solve, the timing model projected out; X and Z of those pulsars and rho,
    sigma_pair of the pairs among them, norm-wise"""
    from oracle import pta_oracle as po
    from pta_replicator_amd.simulate import timing_design_matrix
    m = eng._os["matched"]
    mp = m["plan"]
    R, P, nf, gamma = rows.shape[0], eng.P, mp.nf, m["gw"][1]
    toas = [x * 86400.0 for x in eng.mjd]
    T = max(t.max() for t in toas) - min(t.min() for t in toas)
    th = {k: v.cpu().numpy() for k, v in theta.items()}
    X, Z = np.zeros((R, len(which), 2 * nf)), np.zeros((R, len(which), 2 * nf, 2 * nf))
    for i, a in enumerate(which):
        t = toas[a]
        F, freqs = po.fourier_design_matrix(t, nmodes=nf, Tspan=T)
        S = (1 / (365.25 * 86400)) ** (gamma - 3) * freqs ** (-gamma) / (12 * np.pi ** 2 * T)
        sig2 = (eng.efacvec[a] * eng.sigma_s[a]) ** 2 + (eng.efacvec[a] * eng.equadvec[a]) ** 2
        ep = np.asarray(po.quantize(eng.mjd[a], dt=0.1)[0])
        C0 = np.diag(sig2) + (ep[:, None] == ep[None, :]) * (np.asarray(eng.ecorrvec[a])[ep] ** 2)[:, None]
        tdb = eng.tdb_s[a]
        Frn, fr = po.fourier_design_matrix(tdb, nmodes=eng._rn["components"], Tspan=tdb.max() - tdb.min())
        M = timing_design_matrix(t, model=model)[0]
        for r in range(R):
            lA, g = th["rn_log10_A"][r, a], th["rn_gamma"][r, a]
            if np.isnan(lA):
                lA, g = eng._rn["A"][a], eng._rn["g"][a]
            C = C0.copy()
            if lA is not None:
                C += (Frn * po.red_noise_prior(fr, lA, g, tdb.max() - tdb.min())) @ Frn.T
            Sr = (1 / (365.25 * 86400)) ** (th["gwb_gamma"][r] - 3) * freqs ** (-th["gwb_gamma"][r]) / (12 * np.pi ** 2 * T)
            C += 10 ** (2 * th["gwb_log10_A"][r]) * (F * Sr) @ F.T
            B = np.concatenate([F, rows[r, eng.off[a]:eng.off[a + 1], None], M], axis=1)
            CiB = np.linalg.solve(C, B)
            G = B.T @ CiB
            k = 2 * nf + 1
            Pr = G[:k, :k] - G[:k, k:] @ np.linalg.solve(G[k:, k:], G[k:, :k])      # [F | r]^T P [F | r]
            X[r, i] = np.sqrt(S) * Pr[:2 * nf, 2 * nf]
            Z[r, i] = np.sqrt(S)[:, None] * Pr[:2 * nf, :2 * nf] * np.sqrt(S)[None, :]
    w = list(which)
    errs = {"X": _nrel(ref["X"][:, w], X), "Z": _nrel(ref["Z"][:, w], Z)}
    ia, ib = np.triu_indices(len(w), 1)
    num = np.einsum("rpc,rpc->rp", X[:, ia], X[:, ib])
    den = np.einsum("rpij,rpij->rp", Z[:, ia], Z[:, ib])
    pidx = [int(np.flatnonzero((mp.pair_a == w[x]) & (mp.pair_b == w[y]))[0]) for x, y in zip(ia, ib)]
    errs["rho"] = _nrel(ref["rho"][:, pidx], num / den)
    errs["sigma_pair"] = _nrel(ref["sigma_pair"][:, pidx], den ** -0.5)
    print(f"host reduced-rank against dense on pulsars {w}:", {k: f"{v:.3e}" for k, v in errs.items()})
    return max(errs.values())


# ---------------------------------------------------------------- refusals ----------------------------------------------------
def test_refusals():
    eng = _engine(P=3)
    R = 4
    rows = eng.generate(R)
    theta = {"rn_log10_A": np.full((R, 3), -14.0), "rn_gamma": np.full((R, 3), 3.0)}
    eng.prepare_optimal_statistic(components=4)
    with pytest.raises(ValueError, match="matched=True"):
        eng.optimal_statistic(rows, theta=theta)
    with pytest.raises(ValueError, match="matched=True"):
        eng.generate_os(R, theta=theta, matched=True)
    eng.prepare_optimal_statistic(components=4, gwb_auto=False, matched=True)
    with pytest.raises(ValueError, match="needs theta"):
        eng.generate_os(R, matched=True)
    with pytest.raises(ValueError, match="without the GWB auto-term"):
        eng.optimal_statistic(rows, theta={"gwb_log10_A": np.full(R, -14.0)})
    with pytest.raises(ValueError, match="TD mode"):
        eng.generate_os(R, theta=theta, td=True, matched=True)
    for bad, msg in (({"rn_amp": np.zeros((R, 3))}, "unknown"), ({"rn_log10_A": np.zeros((R + 1, 3))}, "shape"),
                     ({**theta, "rn_log10_A": np.full((R, 3), np.inf)}, "infinite"), ({**theta, "rn_gamma": np.full((R, 3), np.inf)}, "non-finite")):
        with pytest.raises(ValueError, match=msg):
            eng.optimal_statistic(rows, theta=bad)
        with pytest.raises(ValueError, match=msg):
            eng.generate_os(R, theta=bad, matched=True)
    with pytest.raises(ValueError, match="rows must be"):
        eng.optimal_statistic(rows[:, :-1], theta=theta)
    eng.set_red_noise([-14.0] * 3, [3.0] * 3, components=60)         # 120 + 2 * 14 columns
    with pytest.raises(ValueError, match="exceeds the kernel limit"):
        eng.prepare_optimal_statistic(matched=True)
    eng = _engine(P=3)
    eng.prepare_optimal_statistic(components=4, matched=True)
    eng.set_gwb(-15.0, 13. / 3.)      # re-configured: the prepared OS is stale
    with pytest.raises(ValueError, match="re-configured"):
        eng.optimal_statistic(rows, theta=theta)
    with pytest.raises(ValueError, match="re-configured"):
        eng.generate_os(R, theta=theta, matched=True)
