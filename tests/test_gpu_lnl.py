"""Marginalised log-likelihood on a theta grid on the MI355X: pta_lnl_quad and pta_lnl_factor / pta_lnl_apply / pta_lnl_reduce against
NumPy, the engine against the host evaluation (optimal_statistic.lnl_from_rows) and, at 68 x 5000, against a dense likelihood of three
pulsars, bit-identity across chunks / offsets / batches, the chi-square calibration of the quadratic form and the recovery of an
injected red-noise amplitude.

Calibrated bound (the convention of tests/test_gpu_os_matched.py): every |d ln L| is taken relative to scale = |ln L| + r^T P0' r / s
(the two terms of the reduced-rank form cancel when red noise is strong) and held to max(1e-12, 8 delta), delta = the disagreement, on
the same scale, of two independent CPU fp64 evaluations (the Cholesky form against the np.linalg.solve / slogdet form of lnl_solve).
Every such test checks delta < 1e-8 itself.  At 68 x 5000 delta also takes the disagreement of the host evaluation with a dense
likelihood of three of the pulsars: the two host forms share one projection q = V r and one r^T P0' r.

Measured on one MI355X (worst |d ln L| / scale, device against host): kernels 1.7e-15 (K = 2 .. 128; pta_lnl_quad 5.9e-16 of r0), engines
with 16 pulsars 4.5e-15 with a timing model and 1.6e-13 without (delta 6.2e-14), 68 x 5000 1.1e-14 (host against dense there: 5.7e-13);
pta_lnl_apply with 2, 3 and 16 grid points per workgroup 1.6e-15 (delta 9.7e-16), with KT = 3, 4, 5, 7 blocks 1.4e-16 (the shapes of
tests/launch_cases.py, which the plan query holds to those instances)."""
import ctypes

import numpy as np
import pytest
import torch

import launch_cases as lc
from pta_replicator_amd import optimal_statistic as ost
from test_gpu_os import _engine as _engine_all_rn, _psrs
from test_lnl_host import NF, _array, _M, _q_blocked, _rn_basis, _rows

pytestmark = pytest.mark.gpu


def _bound(delta):
    assert delta < 1e-8, f"the inputs are too ill-conditioned for this check: delta = {delta:.3e}"
    return max(1e-12, 8 * delta)


# ---------------------------------------------------------------- kernels ---------------------------------------------------
@pytest.mark.parametrize("model", ["spin", None])
@pytest.mark.parametrize("with_ecorr", [True, False])
def test_lnl_quad_vs_numpy(with_ecorr, model):
    """ragged pulsars whose ECORR epochs are not contiguous in TOA order (the array of tests/test_lnl_host.py), and no ECORR at all;
    the timing-model rows in a blocked q whose block boundary they straddle.  Bound: 1e-12 of r^T P0' r (= 1e-12 scale, in units of s)."""
    from pta_replicator_amd import _lib, device as dv
    arr = _array()
    plan = ost.prepare_lnl([p["t"] for p in arr], [p["sigma2"] for p in arr], components=NF, epoch_of=[p["epoch_of"] for p in arr] if with_ecorr else None,
                           ecorr=[p["ecorr"] for p in arr] if with_ecorr else None, F_rn=[_rn_basis(p)[0] for p in arr], M=_M(arr, model))
    R, P, K, m = 37, plan.P, plan.K, plan.m
    rows = _rows(arr, plan, R, 5)
    n_toa = rows.shape[1]
    Vt = plan.Vt()
    q = np.stack([rows[:, plan.off[a]:plan.off[a + 1]] @ Vt[:, plan.off[a]:plan.off[a + 1]].T for a in range(P)], axis=1)
    ref = ost.lnl_quad(plan, rows)
    psr_ep, ep_ptr, ep_idx, ep_g = plan.epochs()
    d_rows = dv.zeros((R, n_toa + 5))                   # a row stride wider than the rows
    d_rows[:, :n_toa] = dv.f64(rows)
    d_off, d_dinv = dv.i32(plan.off), dv.f64(plan.dinv)
    d_Ht = dv.f64(plan.Ht_all()) if m else None
    ep = [dv.i32(psr_ep), dv.i32(ep_ptr), dv.i32(ep_idx), dv.f64(ep_g)] if with_ecorr else [None] * 4
    for blk in (16, 64):
        qd = dv.f64(_q_blocked(q, blk))
        out = dv.zeros((R, P))
        _lib.call("pta_lnl_quad", dv.ptr(d_rows), d_rows.stride(0), R, dv.ptr(d_off), P, dv.ptr(d_dinv), *[dv.ptr(x) for x in ep], dv.ptr(qd),
                  qd.shape[1], blk, K, m, dv.ptr(d_Ht), n_toa, dv.ptr(out), dv.stream_ptr())
        err = float(np.max(np.abs(out.cpu().numpy() - ref) / np.abs(ref)))
        print(f"ecorr={with_ecorr} model={model} q_block={blk}: worst |d r0| / r0 {err:.3e}")
        assert err < 1e-12
    # a realisation's value does not depend on the batch it is computed in
    sub = dv.zeros((3, P))
    _lib.call("pta_lnl_quad", ctypes.c_void_p(d_rows.data_ptr() + 8 * 11 * d_rows.stride(0)), d_rows.stride(0), 3, dv.ptr(d_off), P, dv.ptr(d_dinv),
              *[dv.ptr(x) for x in ep], ctypes.c_void_p(qd.data_ptr() + 8 * 11 * qd.shape[1]), qd.shape[1], 64, K, m, dv.ptr(d_Ht), n_toa, dv.ptr(sub), dv.stream_ptr())
    assert torch.equal(sub, out[11:14])


def _problem(K, R, G, P=2, m=3):
    rng = np.random.default_rng(K * 100000 + R * 100 + G)
    A = np.zeros((P, K, K))
    for a in range(P):                               # SPD with eigenvalues over five decades
        Q = np.linalg.qr(rng.normal(size=(K, K)))[0]
        A[a] = (Q * 10.0 ** rng.uniform(-2, 3, K)) @ Q.T
        A[a] = 0.5 * (A[a] + A[a].T)
    b = rng.uniform(0, 3, (G, P, K)) * (rng.uniform(size=(G, P, K)) > 0.2)     # a fifth of the prior variances are exactly zero
    b[0, 0, :] = 0.0                                 # and one whole problem has none: Mc = I
    q = rng.normal(size=(R, P, K + m))               # the timing-model rows are carried along and never read
    s, c = rng.uniform(0.5, 2.0, P), rng.normal(0, 100.0, P)
    r0 = np.einsum("rpk,rpk->rp", q[:, :, :K], q[:, :, :K]) * rng.uniform(1.0, 3.0, (R, P)) * 50.0
    return A, b, q, r0, s, c


def _device_lnl(A, b, q, r0, s, c, blk, C=2):
    from pta_replicator_amd import _lib, device as dv
    G, P, K = b.shape
    R, Kt = q.shape[0], q.shape[2]
    dA, db, dq, dr0, ds, dc = dv.f64(A), dv.f64(b), dv.f64(_q_blocked(q, blk)), dv.f64(r0), dv.f64(s), dv.f64(c)
    Lt, logdet, lp, tot = dv.zeros((G, P, K, K)), dv.zeros((G, P)), dv.zeros((G, P, R)), dv.zeros((G, R))
    st = dv.stream_ptr()
    _lib.call("pta_lnl_factor", dv.ptr(dA), P, K, C, G, dv.ptr(db), dv.ptr(Lt), dv.ptr(logdet), st)
    _lib.call("pta_lnl_apply", dv.ptr(Lt), dv.ptr(logdet), dv.ptr(db), P, K, C, G, dv.ptr(dq), P * Kt, blk, Kt, R, dv.ptr(dr0), dv.ptr(ds), dv.ptr(dc), dv.ptr(lp),
              P * R, R, st)
    _lib.call("pta_lnl_reduce", dv.ptr(lp), P * R, R, P, G, R, dv.ptr(tot), R, st)
    return Lt, logdet, lp, tot


@pytest.mark.parametrize("G", [1, 5, 64])
@pytest.mark.parametrize("R", [1, 17, 1000])
@pytest.mark.parametrize("K", lc.LNL_K_FIRST)
def test_factor_apply_vs_numpy(K, R, G):
    A, b, q, r0, s, c = _problem(K, R, G)
    P = A.shape[0]
    blk = 64 if R == 17 else K + 3                   # the blocked q layout of the engine, and the plain one
    Lt, logdet, lp, tot = _device_lnl(A, b, q, r0, s, c, blk)
    ref = np.stack([ost.lnl_solve(A[a], b[:, a], q[:, a, :K], r0[:, a], s[a], c[a]) for a in range(P)], axis=1)                   # [R, P, G]
    alt = np.stack([ost.lnl_solve(A[a], b[:, a], q[:, a, :K], r0[:, a], s[a], c[a], form="solve") for a in range(P)], axis=1)
    scale = np.abs(ref) + (r0 / s[None, :])[:, :, None]
    delta = float(np.max(np.abs(alt - ref) / scale))
    got = lp.permute(2, 1, 0).cpu().numpy()
    err = float(np.max(np.abs(got - ref) / scale))
    print(f"K={K} R={R} G={G}: delta {delta:.3e}, device {err:.3e}")
    assert np.all(np.isfinite(got)) and err < _bound(delta)
    # the operator is lower triangular with an exactly zero upper triangle, the identity where b = 0
    L = Lt.cpu().numpy().transpose(0, 1, 3, 2)       # L[g, a, i, k]
    assert np.all(np.triu(L, 1) == 0)
    assert np.array_equal(L[0, 0], np.eye(K)) and float(logdet[0, 0]) == 0.0          # b = 0: Mc = I
    # the fixed-order pulsar sum
    acc = torch.zeros_like(tot)
    for a in range(P):
        acc = acc + lp[:, a]
    assert torch.equal(acc, tot)
    if R >= 17 and G >= 5:   # a (realisation, grid point) value does not depend on the rows or grid points that share its launch
        sub = _device_lnl(A, b[2:5], q[13:16], r0[13:16], s, c, blk)
        assert torch.equal(sub[2], lp[2:5, :, 13:16]) and torch.equal(sub[3], tot[2:5, 13:16])


def _apply_vs_numpy(P, K, G, R, blk, what):
    """pta_lnl_factor / pta_lnl_apply / pta_lnl_reduce on _problem(K, R, G, P) under the file's bound; returns the inputs and the outputs"""
    inp = _problem(K, R, G, P=P)
    A, b, q, r0, s, c = inp
    out = _device_lnl(A, b, q, r0, s, c, blk)
    ref = np.stack([ost.lnl_solve(A[a], b[:, a], q[:, a, :K], r0[:, a], s[a], c[a]) for a in range(P)], axis=1)                   # [R, P, G]
    alt = np.stack([ost.lnl_solve(A[a], b[:, a], q[:, a, :K], r0[:, a], s[a], c[a], form="solve") for a in range(P)], axis=1)
    scale = np.abs(ref) + (r0 / s[None, :])[:, :, None]
    delta = float(np.max(np.abs(alt - ref) / scale))
    got = out[2].permute(2, 1, 0).cpu().numpy()
    err = float(np.max(np.abs(got - ref) / scale))
    print(f"{what} P={P} K={K} G={G} R={R}: delta {delta:.3e}, device {err:.3e}, error / bound {err / _bound(delta):.3f}")
    assert np.all(np.isfinite(got)) and err < _bound(delta)
    acc = torch.zeros_like(out[3])
    for a in range(P):                               # the fixed-order pulsar sum
        acc = acc + out[2][:, a]
    assert torch.equal(acc, out[3])
    return inp, out


@pytest.mark.parametrize("shape", lc.LNL_GROUPS, ids=lambda c: f"g_per{c['g_per']}")
def test_apply_several_grid_points_per_workgroup(shape):
    """g_per = 2, 3 and 16 grid points per workgroup of pta_lnl_apply (from G P cdiv(R, 128) >= 8192 on): the second and later trips of
    the kernel's loop over grid points, with their barrier and the restaging of the operator in LDS, and the short last group (1 of 3,
    3 of 16).  Value: the file's bound.  Bit-identity: a few grid points, those of the short last group among them, and a few
    realisations, the last of the partial tile among them, in a launch of their own with one grid point per workgroup (the plan query
    confirms both).  Measured on one MI355X: worst |d ln L| / scale 1.6e-15 (g_per = 16; delta 9.7e-16), error / bound 0.002."""
    P, K, G, R = (shape[k] for k in "PKGR")
    assert lc.plan("pta_lnl_apply", P, K, G, R)["g_per"] == shape["g_per"] > 1
    blk = 64 if R > 1 else K + 3                     # the blocked q layout of the engine, and the plain one
    (A, b, q, r0, s, c), (_, _, lp, tot) = _apply_vs_numpy(P, K, G, R, blk, f"g_per={shape['g_per']}")
    gi, ri = list(shape["sub_g"]), list(shape["sub_r"])
    assert lc.plan("pta_lnl_apply", P, K, len(gi), len(ri))["g_per"] == 1
    sub = _device_lnl(A, b[gi], q[ri], r0[ri], s, c, blk)
    assert torch.equal(sub[2], lp[gi][:, :, ri]) and torch.equal(sub[3], tot[gi][:, ri])


@pytest.mark.parametrize("K", lc.LNL_K_MORE)
def test_apply_every_block_count(K):
    """k_lnl_apply<KT> for KT = 3, 4, 5 and 7 (test_factor_apply_vs_numpy has 1, 2, 6, 8), with K a multiple of 16, one past it and
    neither.  Measured on one MI355X: worst |d ln L| / scale 1.4e-16 (delta 1.8e-16), error / bound 0.0001."""
    P, G, R = (lc.LNL_KT_SHAPE[k] for k in "PGR")
    assert lc.plan("pta_lnl_apply", P, K, G, R) == {"kt": (K + 15) // 16, "g_per": 1, "gz": G}
    (A, b, q, r0, s, c), (_, _, lp, tot) = _apply_vs_numpy(P, K, G, R, 64, f"kt={(K + 15) // 16}")
    sub = _device_lnl(A, b[2:5], q[13:16], r0[13:16], s, c, 64)
    assert torch.equal(sub[2], lp[2:5, :, 13:16]) and torch.equal(sub[3], tot[2:5, 13:16])


def test_lnl_kernels_refuse_bad_arguments():
    from pta_replicator_amd import _lib, device as dv
    x = dv.zeros((1,))
    for K, C in ((129, 28), (88, 89), (0, 0)):
        with pytest.raises(_lib.PtaError, match="pta_lnl_factor"):
            _lib.call("pta_lnl_factor", dv.ptr(x), 2, K, C, 1, dv.ptr(x), dv.ptr(x), dv.ptr(x), dv.stream_ptr())
        with pytest.raises(_lib.PtaError, match="pta_lnl_apply"):
            _lib.call("pta_lnl_apply", dv.ptr(x), dv.ptr(x), dv.ptr(x), 2, K, C, 1, dv.ptr(x), 2 * K, 64, K, 1, dv.ptr(x), dv.ptr(x), dv.ptr(x), dv.ptr(x), 2, 1,
                      dv.stream_ptr())
    with pytest.raises(_lib.PtaError, match="NULL"):
        _lib.call("pta_lnl_factor", None, 2, 8, 2, 1, dv.ptr(x), dv.ptr(x), dv.ptr(x), dv.stream_ptr())


# ---------------------------------------------------------------- engines -----------------------------------------------------
def _engine(P=16, gw=-14.4, seed=77, n0=120):
    """ragged pulsars with ECORR sessions; pulsar 2 is configured without red noise"""
    from pta_replicator_amd.engine import ReplicaEngine
    eng = ReplicaEngine(_psrs(P, n0, 11), seed=seed)
    eng.td_warmup = False
    fl = [["A", "B"]] * P
    eng.set_white_noise(efac=[np.array([1.1, 0.9])] * P, log10_equad=[np.array([-6.5, -6.8])] * P, flags=fl)
    eng.set_jitter(log10_ecorr=[np.array([-6.6, -6.9])] * P, flags=fl, coarsegrain=0.1)
    eng.set_red_noise([None if a == 2 else -14.0 + 0.05 * a for a in range(P)], [None if a == 2 else 3.0 + 0.2 * (a % 4) for a in range(P)], components=20)
    if gw is not None:
        eng.set_gwb(gw, 13. / 3.)
    eng.prepare()
    return eng


def _host_b(eng, grid, G):
    """prior variances of the grid by matched_prior with the engine's tables: keys not given as configured / as prepared"""
    st = eng._lnl
    plan = st["plan"]
    P = eng.P

    def get(k):
        v = grid.get(k)
        return None if v is None else (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v, dtype=np.float64))
    lA, g = get("rn_log10_A"), get("rn_gamma")
    rn = eng._rn is not None
    if rn:
        conf_A = np.array([np.nan if x is None else x for x in eng._rn["A"]])
        conf_g = np.array([np.nan if x is None else x for x in eng._rn["g"]])
        if lA is not None or g is not None:
            lA = np.broadcast_to(conf_A, (G, P)).copy() if lA is None else lA.copy()
            g = np.broadcast_to(conf_g, (G, P)).copy() if g is None else g.copy()
            lA[:, np.isnan(conf_A)] = np.nan
    gl = gg = None
    if st["gw"] is not None:
        gl = get("gwb_log10_A") if "gwb_log10_A" in grid else np.full(G, st["gw"][0])
        gg = get("gwb_gamma") if "gwb_gamma" in grid else np.full(G, st["gw"][1])
    if not rn:
        return ost.matched_prior(G, plan.s, nf=plan.nf, T=plan.T, gw_log10_A=gl, gw_gamma=gg)
    return ost.matched_prior(G, plan.s, np.stack(eng.rn_freqs), np.array([t.max() - t.min() for t in eng.tdb_s]), eng.rn_amp ** 2, lA, g, plan.nf, plan.T,
                             gl, gg)


def _compare(eng, rows, grid, G, what, delta_floor=0.0):
    res = eng.log_likelihood(rows, grid, per_pulsar=True)
    plan = eng._lnl["plan"]
    b = _host_b(eng, grid, G)
    h = rows.cpu().numpy()
    ref, tot = ost.lnl_from_rows(plan, h, b)
    alt, _ = ost.lnl_from_rows(plan, h, b, form="solve")
    scale = np.abs(ref) + (ost.lnl_quad(plan, h) / plan.s[None, :])[:, :, None]
    delta = max(delta_floor, float(np.max(np.abs(alt - ref) / scale)))
    R = h.shape[0]
    assert res["lnl"].shape == (R, G) and res["lnl_pulsar"].shape == (R, eng.P, G)
    got = res["lnl_pulsar"].cpu().numpy()
    err = float(np.max(np.abs(got - ref) / scale))
    err_tot = float(np.max(np.abs(res["lnl"].cpu().numpy() - tot) / scale.sum(axis=1)))
    print(f"{what}: delta {delta:.3e}, device per pulsar {err:.3e}, summed {err_tot:.3e}")
    assert np.all(np.isfinite(got)) and max(err, err_tot) < _bound(delta)
    return res, ref


@pytest.mark.parametrize("model", ["spin", "astrometric", None])
def test_engine_lnl_vs_host(model):
    eng = _engine()
    eng.prepare_likelihood(components=10, timing_model=model)
    st = eng._lnl
    assert st["K"] == 60 and st["C"] == 20 and st["Kt"] == 60 + st["m"] and (st["m"] == 3 if model == "spin" else st["m"] == 0 if model is None else st["m"] > 3)
    R, P, G = 24, eng.P, 7
    rng = np.random.default_rng(3)
    lA = rng.uniform(-15.0, -12.8, (G, P))
    lA[::3] = np.nan                                  # whole grid points, and single pulsars, "as configured"
    lA[1::4, 3] = np.nan
    g = np.where(np.isnan(lA), np.nan, rng.uniform(2, 6, (G, P)))
    rows = eng.generate(R, r0=5)
    grids = {
        "rn+gw amplitude": {"rn_log10_A": lA, "rn_gamma": g, "gwb_log10_A": rng.uniform(-15, -13.5, G)},
        "gw only, own index": {"gwb_log10_A": torch.as_tensor(rng.uniform(-15, -14, G)), "gwb_gamma": rng.uniform(3, 5.5, G)},
        "rn index only": {"rn_gamma": rng.uniform(2, 5, (G, P))},
    }
    for what, grid in grids.items():
        _compare(eng, rows, grid, G, f"{model}, {what}")
    # no key at all: one grid point, everything as configured; and the caller's own residuals
    own = torch.as_tensor(rng.normal(0, 1e-6, (5, eng.n_toa)), device=rows.device)
    res, ref = _compare(eng, own, {}, 1, f"{model}, own residuals, configured model")
    th, shape = eng.theta_grid(gwb_log10_A=np.linspace(-15, -14, 3), rn_gamma=[2.5, 4.5])
    assert shape == (3, 2)
    _compare(eng, own, th, 6, f"{model}, theta_grid")


def test_engine_lnl_single_pulsar_and_no_common_process():
    from pta_replicator_amd.engine import ReplicaEngine
    eng = ReplicaEngine(_psrs(1, 200, 5), seed=3)
    eng.td_warmup = False
    eng.set_white_noise(efac=1.0)
    eng.set_red_noise([-13.8], [3.5], components=15)
    eng.prepare()
    eng.prepare_likelihood(components=6)              # no GWB configured: the common-process columns carry no variance
    assert eng._lnl["gw"] is None and eng._lnl["K"] == 42
    rows = eng.generate(9)
    G = 5
    _compare(eng, rows, {"rn_log10_A": np.linspace(-15, -12.5, G)[:, None], "rn_gamma": np.linspace(2, 6, G)[:, None]}, G, "one pulsar")
    with pytest.raises(ValueError, match="without the GWB auto-term"):
        eng.log_likelihood(rows, {"gwb_log10_A": np.full(G, -14.0)})
    # no red noise at all: K = C, the grid holds the common process alone
    eng = ReplicaEngine(_psrs(4, 100, 5), seed=3)
    eng.td_warmup = False
    eng.set_white_noise(efac=1.0)
    eng.set_gwb(-14.2, 13. / 3.)
    eng.prepare()
    eng.prepare_likelihood(components=6, timing_model=None)
    assert eng._lnl["K_rn"] == 0 and eng._lnl["K"] == 12 and eng._lnl["m"] == 0
    rows = eng.generate(6)
    _compare(eng, rows, {"gwb_log10_A": np.linspace(-15, -13.5, G)}, G, "no red noise, no timing model")


def test_headline_size_vs_host_and_dense():
    import bench
    from pta_replicator_amd.engine import ReplicaEngine
    psrs, noise = bench.headline_array()
    eng = bench.configure_engine(ReplicaEngine(psrs, seed=5), noise)
    eng.td_warmup = False
    eng.prepare()
    eng.prepare_likelihood()
    assert eng._lnl["K"] == 88 and eng._lnl["C"] == 28
    R, G = 8, 4
    rng = np.random.default_rng(9)
    grid = {"gwb_log10_A": rng.uniform(-15.0, -14.3, G), "gwb_gamma": rng.uniform(3.5, 5.0, G), "rn_log10_A": rng.uniform(-15.5, -13.5, (G, eng.P)),
            "rn_gamma": rng.uniform(2.0, 5.0, (G, eng.P))}
    rows = eng.generate(R)
    plan = eng._lnl["plan"]
    b = _host_b(eng, grid, G)
    ref, _ = ost.lnl_from_rows(plan, rows.cpu().numpy(), b)
    delta = _dense_delta(eng, rows.cpu().numpy(), grid, ref, (0, 1, 2))
    _compare(eng, rows, grid, G, "headline 68 x 5000", delta_floor=delta)


def _dense_delta(eng, rows, grid, ref, which, model="spin"):
    """disagreement (on the scale |ln L| + r^T P0' r / s) of the host reduced-rank ln L `ref` [R, P, G] with a dense NumPy likelihood on
    the pulsars `which`: C_a(theta_g) assembled explicitly from the engine's configuration, Cholesky, the timing model marginalised"""
    from oracle import pta_oracle as po
    from pta_replicator_amd.simulate import timing_design_matrix
    st = eng._lnl
    plan = st["plan"]
    nf = plan.nf
    toas = [x * 86400.0 for x in eng.mjd]
    T = max(t.max() for t in toas) - min(t.min() for t in toas)
    G = ref.shape[2]
    r0 = ost.lnl_quad(plan, rows)
    worst = 0.0
    for a in which:
        t = toas[a]
        n = len(t)
        F, freqs = po.fourier_design_matrix(t, nmodes=nf, Tspan=T)
        sig2 = (eng.efacvec[a] * eng.sigma_s[a]) ** 2 + (eng.efacvec[a] * eng.equadvec[a]) ** 2
        ep = np.asarray(po.quantize(eng.mjd[a], dt=0.1)[0])
        C0 = np.diag(sig2) + (ep[:, None] == ep[None, :]) * (np.asarray(eng.ecorrvec[a])[ep] ** 2)[:, None]
        tdb = eng.tdb_s[a]
        Frn, fr = po.fourier_design_matrix(tdb, nmodes=eng._rn["components"], Tspan=tdb.max() - tdb.min())
        M = timing_design_matrix(t, model=model)[0]
        M = M / np.linalg.norm(M, axis=0)[None, :]
        r = rows[:, eng.off[a]:eng.off[a + 1]].T
        sc = float(np.mean(sig2))
        for g in range(G):
            C = C0 + (Frn * po.red_noise_prior(fr, grid["rn_log10_A"][g, a], grid["rn_gamma"][g, a], tdb.max() - tdb.min())) @ Frn.T
            Sg = (1 / (365.25 * 86400)) ** (grid["gwb_gamma"][g] - 3) * freqs ** (-grid["gwb_gamma"][g]) / (12 * np.pi ** 2 * T)
            C += 10 ** (2 * grid["gwb_log10_A"][g]) * (F * Sg) @ F.T
            L = np.linalg.cholesky(C / sc)
            Y = np.linalg.solve(L, np.concatenate([r, M], axis=1))
            y, Ym = Y[:, :r.shape[1]], Y[:, r.shape[1]:]
            Lb = np.linalg.cholesky(Ym.T @ Ym)
            z = np.linalg.solve(Lb, Ym.T @ y)
            m = M.shape[1]
            chi2 = (np.sum(y * y, axis=0) - np.sum(z * z, axis=0)) / sc
            logdet = 2 * np.sum(np.log(np.diag(L))) + n * np.log(sc) + 2 * np.sum(np.log(np.diag(Lb))) - m * np.log(sc)
            dense = -0.5 * (chi2 + logdet + (n - m) * np.log(2 * np.pi))
            # ln det(M^T C^-1 M) depends on the scaling of M's columns: the dense side normalises them, the plan does not
            M0 = timing_design_matrix(t, model=model)[0]
            dense = dense - np.sum(np.log(np.linalg.norm(M0, axis=0)))
            scale = np.abs(dense) + r0[:, a] / plan.s[a]
            worst = max(worst, float(np.max(np.abs(ref[:, a, g] - dense) / scale)))
    print(f"host reduced-rank against dense on pulsars {list(which)}: {worst:.3e}")
    return worst


# ---------------------------------------------------------------- bit-identity ------------------------------------------------
def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


def test_generate_lnl_bit_identical():
    eng = _engine(P=6)
    eng.prepare_likelihood(components=14)
    R = 300
    grid, shape = eng.theta_grid(gwb_log10_A=np.linspace(-15.2, -13.6, 5), rn_log10_A=[-14.5, -13.5], rn_gamma=[2.5, 3.5, 4.5])
    G = int(np.prod(shape))
    ref = eng.log_likelihood(eng.generate(R), grid, per_pulsar=True)
    assert ref["lnl"].shape == (R, G) and bool(torch.isfinite(ref["lnl"]).all())
    for chunk in (7, 256, R):
        assert _same(eng.generate_lnl(R, grid, chunk=chunk, per_pulsar=True), ref), chunk
    assert torch.equal(eng.generate_lnl(R, grid)["lnl"], ref["lnl"])
    sub = eng.generate_lnl(50, grid, r0=123, chunk=16, per_pulsar=True)
    assert torch.equal(sub["lnl"], ref["lnl"][123:173]) and torch.equal(sub["lnl_pulsar"], ref["lnl_pulsar"][123:173])
    # rows recomputed inside a different batch, grid points evaluated in a different grid: the same numbers
    again = eng.log_likelihood(eng.generate(9, r0=200), {k: v[11:17] for k, v in grid.items()}, per_pulsar=True)
    assert torch.equal(again["lnl"], ref["lnl"][200:209, 11:17]) and torch.equal(again["lnl_pulsar"], ref["lnl_pulsar"][200:209, :, 11:17])
    # lnl is the fixed-order pulsar sum of lnl_pulsar
    acc = torch.zeros_like(ref["lnl"])
    for a in range(eng.P):
        acc = acc + ref["lnl_pulsar"][:, a]
    assert torch.equal(acc, ref["lnl"])
    # a small workspace cuts the grid (3 points per chunk) and the realisations of both entry points; the numbers stay
    keep = eng.workspace_bytes
    try:
        K = eng._lnl["K"]
        eng.workspace_bytes = 6 * 8 * eng.P * (K * K + K + 1)
        assert eng._lnl_chunks(eng._lnl, R, G, False, True)[1] == 3 and eng._lnl_chunks(eng._lnl, R, G, False, True)[0] < R
        assert _same(eng.generate_lnl(R, grid, per_pulsar=True), ref)
        assert _same(eng.log_likelihood(eng.generate(R), grid, per_pulsar=True), ref)
        assert torch.equal(eng.generate_lnl(R, grid)["lnl"], ref["lnl"])
    finally:
        eng.workspace_bytes = keep
    # per-realisation theta of the generator, with the likelihood on the same grid
    eng.set_hyper_prior(rn_log10_A=(-14.8, -13.3), rn_gamma=(2.0, 5.0))
    eng.prepare_likelihood(components=14)
    theta = eng.sample_theta(64)
    ref2 = eng.log_likelihood(eng.generate(64, theta=theta), grid)
    assert torch.equal(eng.generate_lnl(64, grid, theta=theta, chunk=20)["lnl"], ref2["lnl"])


def test_generate_lnl_td_bit_identical():
    eng = _engine(P=6, gw=None)
    eng.prepare_td()
    eng.prepare_likelihood(components=6, gwb_auto=-14.5)
    R = 40
    grid, _ = eng.theta_grid(gwb_log10_A=[-15.0, -14.0], rn_gamma=[3.0, 4.0])
    ref = eng.log_likelihood(eng.generate_td(R), grid)
    for chunk in (7, R):
        assert torch.equal(eng.generate_lnl(R, grid, td=True, chunk=chunk)["lnl"], ref["lnl"])
    assert torch.equal(eng.generate_lnl(10, grid, r0=25, td=True, chunk=3)["lnl"], ref["lnl"][25:35])


# ---------------------------------------------------------------- statistics --------------------------------------------------
def test_quadratic_form_is_chi_square():
    """16 pulsars with WN + ECORR + red noise and no GWB: the engine's red noise is exactly the model, so at the configured values
    x = sum_a [-2 ln L_a - 2 sum ln L_kk - c_a] = sum_a r^T C_a^-1-marginalised r is chi-square with nu = sum (N_a - m) degrees of
    freedom: mean nu, variance 2 nu.  Bounds: five standard errors of the sample mean (sqrt(2 nu / R)) and of the sample variance
    (2 nu sqrt(2 / R), the Gaussian limit of a chi-square with nu in the thousands)."""
    eng = _engine_all_rn(P=16, n0=120, gw=None, psr_seed=3)
    eng.prepare_likelihood(components=14, gwb_auto=False)
    R = 4096
    res = eng.generate_lnl(R, {}, chunk=1024, per_pulsar=True)
    st = eng._lnl
    plan = st["plan"]
    b = _host_b(eng, {}, 1)[0]
    logdet = np.array([np.linalg.slogdet(np.eye(plan.K) + np.sqrt(b[a])[:, None] * plan.A[a] * np.sqrt(b[a])[None, :])[1] for a in range(eng.P)])
    lp = res["lnl_pulsar"].cpu().numpy()[:, :, 0]
    x = np.sum(-2.0 * lp - logdet[None, :] - plan.c[None, :], axis=1)
    nu = int(np.sum(plan.counts - plan.m))
    mean, var = float(np.mean(x)) / nu, float(np.var(x)) / (2 * nu)
    print(f"nu = {nu}: mean(x) / nu = {mean:.5f} (bound {5 * np.sqrt(2 / (nu * R)):.5f}), var(x) / 2 nu = {var:.4f} (bound {5 * np.sqrt(2 / R):.4f})")
    assert abs(mean - 1) <= 5 * np.sqrt(2 / (nu * R))
    assert abs(var - 1) <= 5 * np.sqrt(2 / R)


def test_recovers_an_injected_red_noise_amplitude():
    """rows generated with rn_log10_A = -12.8 on every pulsar (configured: -14.0 .. -13.5); per pulsar, the arg-max of ln L_a over a
    rn_log10_A axis of step 0.2 (the indices as configured, the truth on the axis), averaged over the realisations, lies within one step
    of the truth, on the device and in the CPU oracle on the same rows, and more than two steps from the configured value.  Step: the
    maximum-likelihood ln A^2 of n informative coefficients scatters by sqrt(2 / n), i.e. 0.217 sqrt(2 / n) dex in log10 A: 0.1 dex
    even if only 10 of the 40 coefficients stand above the white noise, 0.01 dex in the mean of 128 realisations, and the bias of the
    estimator is of the same order as its scatter per realisation at most: half a step of room."""
    eng = _engine_all_rn(P=6, n0=150, gw=None)
    eng.prepare_likelihood(components=8, gwb_auto=False)
    R, truth, step = 128, -12.8, 0.2
    rows = eng.generate(R, theta={"rn_log10_A": np.full((R, eng.P), truth)})
    axis = truth + step * np.arange(-6, 6)
    grid, shape = eng.theta_grid(rn_log10_A=axis)
    res = eng.log_likelihood(rows, grid, per_pulsar=True)
    best = axis[res["lnl_pulsar"].argmax(dim=2).cpu().numpy()].mean(axis=0)           # [P]
    ref, _ = ost.lnl_from_rows(eng._lnl["plan"], rows.cpu().numpy(), _host_b(eng, grid, len(axis)))
    best_cpu = axis[ref.argmax(axis=2)].mean(axis=0)
    conf = np.array(eng._rn["A"], dtype=np.float64)
    print("mean arg-max per pulsar: device", best, "CPU oracle", best_cpu, "configured", conf)
    assert np.all(np.abs(best_cpu - truth) < step) and np.all(np.abs(best - truth) < step)
    assert np.all(np.abs(best - conf) > 2 * step)
    # the full likelihood peaks there too
    assert abs(axis[res["lnl"].argmax(dim=1).cpu().numpy()].mean() - truth) < step


# ---------------------------------------------------------------- refusals ----------------------------------------------------
def test_refusals():
    eng = _engine(P=3)
    R, G = 4, 2
    rows = eng.generate(R)
    grid = {"rn_log10_A": np.full((G, 3), -14.0), "rn_gamma": np.full((G, 3), 3.0)}
    with pytest.raises(ValueError, match="not prepared"):
        eng.log_likelihood(rows, grid)
    eng.prepare_likelihood(components=4, gwb_auto=False)
    with pytest.raises(ValueError, match="without the GWB auto-term"):
        eng.log_likelihood(rows, {"gwb_log10_A": np.full(G, -14.0)})
    with pytest.raises(ValueError, match="cw_"):
        eng.log_likelihood(rows, dict(grid, cw_log10_mc=np.full(G, 9.0)))
    with pytest.raises(ValueError, match="TD mode"):
        eng.generate_lnl(R, grid, theta={"rn_log10_A": np.full((R, 3), -14.0)}, td=True)
    for bad, msg in (({"rn_amp": np.zeros((G, 3))}, "unknown"), ({"rn_log10_A": np.zeros((G, 2))}, "shape"),
                     ({**grid, "rn_log10_A": np.full((G, 3), np.inf)}, "infinite"), ({**grid, "rn_gamma": np.full((G, 3), np.inf)}, "non-finite")):
        with pytest.raises(ValueError, match=msg):
            eng.log_likelihood(rows, bad)
        with pytest.raises(ValueError, match=msg):
            eng.generate_lnl(R, bad)
    with pytest.raises(ValueError, match="rows must be"):
        eng.log_likelihood(rows[:, :-1], grid)
    with pytest.raises(ValueError, match="rows must be"):
        eng.log_likelihood(rows.cpu(), grid)
    eng.set_red_noise([-14.0] * 3, [3.0] * 3, components=60)         # 120 + 2 * 14 columns
    with pytest.raises(ValueError, match="exceeds the kernel limit"):
        eng.prepare_likelihood()
    eng = _engine(P=3)
    eng.prepare_likelihood(components=4)
    eng.set_gwb(-15.0, 13. / 3.)      # re-configured: the prepared likelihood is stale
    with pytest.raises(ValueError, match="re-prepared since"):
        eng.log_likelihood(rows, grid)
    with pytest.raises(ValueError, match="re-prepared since"):
        eng.generate_lnl(R, grid)
