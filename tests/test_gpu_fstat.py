"""Continuous-wave F-statistics on the MI355X: pta_fstat_project / pta_fstat_fp / pta_fstat_fe against NumPy, the engine's Fp / Fe
against a dense NumPy evaluation of the same residuals, bit-identity of generate_f_statistic across chunks / offsets / modes, the
exact null distribution, the identity and the recovery of a source injected by set_cw, and the refusals."""
import ctypes

import numpy as np
import pytest
import torch

import launch_cases as lc
from oracle import pta_oracle as po
from test_gpu_os import _engine, _psrs

pytestmark = pytest.mark.gpu

FREQS = np.array([5.1e-9, 1.21e-8, 2.33e-8, 4.57e-8])
SKY = (np.array([-0.71, -0.2, 0.05, 0.44, 0.83]), np.array([0.3, 1.9, 3.3, 4.4, 5.8]))


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(np.asarray(b))))


# ---------------------------------------------------------------- kernels ---------------------------------------------------
@pytest.mark.parametrize("C", [2, 30, 64, 130, 512])
@pytest.mark.parametrize("R", [1, 5, 17, 1000])
def test_fstat_project_vs_numpy(C, R):
    from pta_replicator_amd import _lib, device as dv
    counts = np.array([1, 15, 17, 64, 65, 130, 301, 16, 257])      # 301: a multiple of no tile size; 1: shorter than one MFMA step
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    N, P = int(off[-1]), len(counts)
    rng = np.random.default_rng(C * 1000 + R)
    W = rng.normal(size=(C, N))
    ld_rows = N + 3                                   # a row stride wider than the row, odd
    rows = rng.normal(size=(R, ld_rows))
    dW, drows, doff = dv.f64(W), dv.f64(rows), dv.i32(off)
    Q = dv.zeros((R, P * C + 2))
    _lib.call("pta_fstat_project", dv.ptr(dW), N, C, dv.ptr(doff), P, dv.ptr(drows), ld_rows, R, dv.ptr(Q), P * C + 2, dv.stream_ptr())
    got = Q.cpu().numpy()
    ref = np.stack([rows[:, off[a]:off[a + 1]] @ W[:, off[a]:off[a + 1]].T for a in range(P)], axis=1).reshape(R, P * C)
    scale = np.stack([np.abs(rows[:, off[a]:off[a + 1]]) @ np.abs(W[:, off[a]:off[a + 1]]).T for a in range(P)], axis=1).reshape(R, P * C)
    err = np.max(np.abs(got[:, :P * C] - ref) / scale)
    print(f"pta_fstat_project C={C} R={R}: max error / sum |w||r| = {err:.2e}")
    assert err < 1e-12
    assert np.all(got[:, P * C:] == 0)                # nothing written past P * C
    if R >= 17:   # a realisation's Q does not depend on the batch or the row slot it is computed in
        Q2 = dv.zeros((3, P * C))
        _lib.call("pta_fstat_project", dv.ptr(dW), N, C, dv.ptr(doff), P, ctypes.c_void_p(drows.data_ptr() + 8 * 13 * ld_rows), ld_rows, 3,
                  dv.ptr(Q2), P * C, dv.stream_ptr())
        assert np.array_equal(Q2.cpu().numpy(), got[13:16, :P * C])


@pytest.mark.parametrize("P, C", lc.FSTAT_PROJECT_LARGE)
def test_fstat_project_large_launch_tiles(P, C):
    """launches large enough for the wider tiles (128 x 128, 64 x 128, 128 x 64, 128 x 32 at R = 1000: the tile follows the number of
    workgroups, pta_fstat_kernels.hip), and the same realisations in a launch of 3, which takes the smallest: bit for bit the same"""
    from pta_replicator_amd import _lib, device as dv
    R = lc.FSTAT_PROJECT_R
    tile = lc.plan("pta_fstat_project", C, P, R)
    assert (tile["bm"], tile["bn"]) == lc.FSTAT_PROJECT_TILES[P, C] and lc.plan("pta_fstat_project", C, P, 3)["bm"] == 64
    rng = np.random.default_rng(P * 1000 + C)
    counts = rng.integers(1, 41, P)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    N = int(off[-1])
    W, rows = rng.normal(size=(C, N)), rng.normal(size=(R, N))
    dW, drows, doff = dv.f64(W), dv.f64(rows), dv.i32(off)
    Q = dv.zeros((R, P * C))
    _lib.call("pta_fstat_project", dv.ptr(dW), N, C, dv.ptr(doff), P, dv.ptr(drows), N, R, dv.ptr(Q), P * C, dv.stream_ptr())
    got = Q.cpu().numpy().reshape(R, P, C)
    for a in range(P):
        ref = rows[:, off[a]:off[a + 1]] @ W[:, off[a]:off[a + 1]].T
        scale = np.abs(rows[:, off[a]:off[a + 1]]) @ np.abs(W[:, off[a]:off[a + 1]]).T
        assert np.max(np.abs(got[:, a] - ref) / scale) < 1e-12
    Q2 = dv.zeros((3, P * C))
    _lib.call("pta_fstat_project", dv.ptr(dW), N, C, dv.ptr(doff), P, ctypes.c_void_p(drows.data_ptr() + 8 * 997 * N), N, 3, dv.ptr(Q2), P * C,
              dv.stream_ptr())
    assert np.array_equal(Q2.cpu().numpy().reshape(3, P, C), got[997:])


def _fe_operands(P, J, S, R, seed):
    rng = np.random.default_rng(seed)
    Q = rng.normal(size=(R, P, 2 * J))
    phi = rng.normal(size=(P, S, 2))
    A = rng.normal(size=(J, S, 4, 4))
    Minv = A @ np.swapaxes(A, -1, -2) + np.eye(4)
    B = rng.normal(size=(P, J, 2, 2))
    Ginv = B @ np.swapaxes(B, -1, -2) + np.eye(2)
    return Q, phi, Minv, Ginv


def test_fstat_fp_vs_numpy():
    from pta_replicator_amd import _lib, device as dv, f_statistic as fst
    P, J, S, R = 23, 11, 3, 37
    Q, _, _, Ginv = _fe_operands(P, J, S, R, 2)
    packed = np.stack([Ginv[..., 0, 0], Ginv[..., 0, 1], Ginv[..., 1, 1]], axis=-1)
    dQ, dG = dv.f64(Q.reshape(R, -1)), dv.f64(packed)
    fp = dv.zeros((R, J + 1))
    _lib.call("pta_fstat_fp", dv.ptr(dQ), P * 2 * J, P, J, R, dv.ptr(dG), dv.ptr(fp), J + 1, dv.stream_ptr())
    got = fp.cpu().numpy()
    assert _rel(got[:, :J], fst.fp_from_Q(Ginv, Q)) < 1e-12
    assert np.all(got[:, J] == 0)


@pytest.mark.parametrize("P,J,S,R", [(23, 11, 100, 37), (68, 8, 64, 9), (2, 1, 1, 1), (5, 17, 130, 300),
                                     (4, 8, 64, 8), (128, 9, 65, 5)])   # one full MFMA step / frequency block / sky tile; PMAX, one past each
def test_fstat_fe_vs_numpy_both_modes(P, J, S, R):
    from pta_replicator_amd import _lib, device as dv, f_statistic as fst
    Q, phi, Minv, _ = _fe_operands(P, J, S, R, P + J)
    dQ, dphi, dM = dv.f64(Q.reshape(R, -1)), dv.f64(phi), dv.f64(Minv[..., fst.TRI_I, fst.TRI_J])
    fe = dv.zeros((R, J * S + 1))
    s = dv.stream_ptr()
    _lib.call("pta_fstat_fe", dv.ptr(dQ), P * 2 * J, P, J, R, dv.ptr(dphi), S, dv.ptr(dM), dv.ptr(fe), J * S + 1, None, 0, None, 0, None, None, s)
    got = fe.cpu().numpy()
    ref = fst.fe_from_Q(phi, Minv, Q)
    err = _rel(got[:, :J * S].reshape(R, J, S), ref)
    print(f"pta_fstat_fe P={P} J={J} S={S} R={R}: rel = {err:.2e}")
    assert err < 1e-12
    assert np.all(got[:, J * S] == 0)
    nt = int(_lib.lib.pta_fstat_fe_tiles(S))
    mx, arg = dv.zeros((R, J)), torch.full((R, J), -1, dtype=torch.int32, device=fe.device)
    pv, pa = dv.empty((R * J * nt,)), torch.empty((R * J * nt,), dtype=torch.int32, device=fe.device)
    _lib.call("pta_fstat_fe", dv.ptr(dQ), P * 2 * J, P, J, R, dv.ptr(dphi), S, dv.ptr(dM), None, 0, dv.ptr(mx), J, dv.ptr(arg), J, dv.ptr(pv), dv.ptr(pa), s)
    full = got[:, :J * S].reshape(R, J, S)
    assert np.array_equal(mx.cpu().numpy(), full.max(axis=2))            # bit for bit the map's maxima
    assert np.array_equal(arg.cpu().numpy(), full.argmax(axis=2))        # NumPy's argmax is the first = lowest index
    # a realisation's values do not depend on the batch it is computed in
    if R >= 9:
        fe2 = dv.zeros((4, J * S))
        _lib.call("pta_fstat_fe", ctypes.c_void_p(dQ.data_ptr() + 8 * 5 * P * 2 * J), P * 2 * J, P, J, 4, dv.ptr(dphi), S, dv.ptr(dM), dv.ptr(fe2), J * S,
                  None, 0, None, 0, None, None, s)
        assert np.array_equal(fe2.cpu().numpy(), got[5:9, :J * S])


def _fe_launch(dQ, ld_q, P, J, R, dphi, S, dM):
    """(Fe [R, J S], maxima [R, J], argmaxima [R, J]) of pta_fstat_fe in its two output modes"""
    from pta_replicator_amd import _lib, device as dv
    s = dv.stream_ptr()
    fe = dv.zeros((R, J * S))
    _lib.call("pta_fstat_fe", dQ, ld_q, P, J, R, dv.ptr(dphi), S, dv.ptr(dM), dv.ptr(fe), J * S, None, 0, None, 0, None, None, s)
    nt = int(_lib.lib.pta_fstat_fe_tiles(S))
    mx, arg = dv.zeros((R, J)), torch.full((R, J), -1, dtype=torch.int32, device=fe.device)
    pv, pa = dv.empty((R * J * nt,)), torch.empty((R * J * nt,), dtype=torch.int32, device=fe.device)
    _lib.call("pta_fstat_fe", dQ, ld_q, P, J, R, dv.ptr(dphi), S, dv.ptr(dM), None, 0, dv.ptr(mx), J, dv.ptr(arg), J, dv.ptr(pv), dv.ptr(pa), s)
    return fe, mx, arg


def _fe_case(P, J, S, R, windows, what, ref_rows=None):
    """both modes against fe_from_Q (the file's 1e-12; of the realisations ref_rows where the host evaluation of all would take many
    seconds) and the maxima against the map bit for bit; then the realisations of each window (first, count) in a launch of their
    own, which one workgroup walks: bit for bit the large launch's, in both modes"""
    from pta_replicator_amd import device as dv, f_statistic as fst
    Q, phi, Minv, _ = _fe_operands(P, J, S, R, P + J + S)
    dQ, dphi, dM = dv.f64(Q.reshape(R, -1)), dv.f64(phi), dv.f64(Minv[..., fst.TRI_I, fst.TRI_J])
    fe, mx, arg = _fe_launch(dv.ptr(dQ), P * 2 * J, P, J, R, dphi, S, dM)
    full = fe.cpu().numpy().reshape(R, J, S)
    rr = np.arange(R) if ref_rows is None else np.asarray(ref_rows)
    err = _rel(full[rr], fst.fe_from_Q(phi, Minv, Q[rr]))
    print(f"pta_fstat_fe {what} P={P} J={J} S={S} R={R}: rel = {err:.2e}, error / bound {err / 1e-12:.4f}")
    assert err < 1e-12
    assert np.array_equal(mx.cpu().numpy(), full.max(axis=2))            # bit for bit the map's maxima
    assert np.array_equal(arg.cpu().numpy(), full.argmax(axis=2))        # NumPy's argmax is the first = lowest index
    for lo, n in windows:
        assert lc.plan("pta_fstat_fe", P, J, n, S)["ngz"] == 1
        fe2, mx2, arg2 = _fe_launch(dv.row_ptr(dQ, lo), P * 2 * J, P, J, n, dphi, S, dM)
        assert torch.equal(fe2, fe[lo:lo + n]) and torch.equal(mx2, mx[lo:lo + n]) and torch.equal(arg2, arg[lo:lo + n]), (lo, n)


@pytest.mark.parametrize("shape", lc.SKY_CHUNK["pta_fstat_fe"], ids=lambda c: f"rchunk{c['rchunk']}")
def test_fstat_fe_realisation_chunks(shape):
    """rchunk, the realisations one workgroup of k_sky_stat walks: 9 (a sky grid of more than 512 workgroups: the chunk is no multiple
    of the 8 realisations that share a scan of the maxima, so the flush ends a chunk part-way), 8, and all of 7 realisations in one
    workgroup.  Measured on one MI355X: worst relative error 4.8e-16, error / bound 0.0005."""
    P, J, S, R = (shape[k] for k in "PJSR")
    assert lc.plan("pta_fstat_fe", P, J, R, S)["rchunk"] == shape["rchunk"]
    ref_rows = None
    if R * J * S > 1 << 22:   # the host map of 13 M cells takes 5 s: the first two, a middle and the last two chunks whole, and every 7th
        c = shape["rchunk"]   # realisation (7 is coprime to the chunk and to the scan: every slot of both is met)
        ref_rows = sorted(set(range(2 * c)) | set(range(16 * c, 17 * c)) | set(range((R - 1) // c * c - c, R)) | set(range(0, R, 7)))
    _fe_case(P, J, S, R, shape["windows"], f"rchunk={shape['rchunk']}", ref_rows)


@pytest.mark.parametrize("P", lc.SKY_KS_P)
def test_fstat_fe_every_pulsar_step_count(P):
    """k_sky_stat<fe_stat, KS, mode> for every KS = ceil(P / 4) = 1 .. 32 in both modes (the other tests reach six of them), full steps
    (P = 4 k) and steps of one pulsar (P = 4 k + 1).  Measured on one MI355X: worst relative error 8.9e-16, error / bound 0.0009."""
    J, S, R = (lc.SKY_KS_SHAPE[k] for k in "JSR")
    assert lc.plan("pta_fstat_fe", P, J, R, S)["ks"] == (P + 3) // 4
    _fe_case(P, J, S, R, ((R - 1, 1),), f"ks={(P + 3) // 4}")


def test_fstat_fe_ties_take_the_lowest_index():
    """identical sky points give identical values: the argmax is the first of them, inside a 16-point group, across groups and
    across workgroup tiles"""
    from pta_replicator_amd import _lib, device as dv, f_statistic as fst
    P, J, S, R = 6, 3, 200, 4
    Q, phi, Minv, _ = _fe_operands(P, J, S, R, 9)
    phi[:, :, :] = phi[:, :1, :]
    Minv[:, :, :, :] = Minv[:, :1, :, :]
    dQ, dphi, dM = dv.f64(Q.reshape(R, -1)), dv.f64(phi), dv.f64(Minv[..., fst.TRI_I, fst.TRI_J])
    nt = int(_lib.lib.pta_fstat_fe_tiles(S))
    mx, arg = dv.zeros((R, J)), torch.full((R, J), -1, dtype=torch.int32, device=dQ.device)
    pv, pa = dv.empty((R * J * nt,)), torch.empty((R * J * nt,), dtype=torch.int32, device=dQ.device)
    _lib.call("pta_fstat_fe", dv.ptr(dQ), P * 2 * J, P, J, R, dv.ptr(dphi), S, dv.ptr(dM), None, 0, dv.ptr(mx), J, dv.ptr(arg), J, dv.ptr(pv), dv.ptr(pa),
              dv.stream_ptr())
    assert np.all(arg.cpu().numpy() == 0)
    assert _rel(mx.cpu().numpy(), fst.fe_from_Q(phi, Minv, Q)[:, :, 0]) < 1e-12


# ---------------------------------------------------------------- engines -----------------------------------------------------
def _dense_projectors(eng, model, amp2, nf=14, gamma=13. / 3.):
    """P_a^-1 [N_a, N_a] per pulsar through dense NumPy: C_a assembled explicitly from the engine's configuration, np.linalg.solve,
    the timing model projected out (tests/test_gpu_os.py::_dense_os's covariance)"""
    from pta_replicator_amd.simulate import timing_design_matrix
    toas = [m * 86400.0 for m in eng.mjd]
    T = max(t.max() for t in toas) - min(t.min() for t in toas)
    out = []
    for a in range(eng.P):
        t = toas[a]
        n = len(t)
        sig2 = (eng.efacvec[a] * eng.sigma_s[a]) ** 2 + (eng.efacvec[a] * eng.equadvec[a]) ** 2
        C = np.diag(sig2)
        ep, ne, first, _ = po.quantize(eng.mjd[a], dt=0.1)
        ep = np.asarray(ep)
        C += (ep[:, None] == ep[None, :]) * (np.asarray(eng.ecorrvec[a])[ep] ** 2)[:, None]
        if eng._rn is not None:
            tdb = eng.tdb_s[a]
            Frn, fr = po.fourier_design_matrix(tdb, nmodes=eng._rn["components"], Tspan=tdb.max() - tdb.min())
            C += (Frn * po.red_noise_prior(fr, eng._rn["A"][a], eng._rn["g"][a], tdb.max() - tdb.min())) @ Frn.T
        if amp2:
            F, freqs = po.fourier_design_matrix(t, nmodes=nf, Tspan=T)
            S = (1 / (365.25 * 86400)) ** (gamma - 3) * freqs ** (-gamma) / (12 * np.pi ** 2 * T)
            C += amp2 * (F * S) @ F.T
        Ci = np.linalg.solve(C, np.eye(n))
        if model is not None:
            M = timing_design_matrix(t, model=model)[0]
            CiM = Ci @ M
            Ci = Ci - CiM @ np.linalg.solve(M.T @ CiM, CiM.T)
        out.append(0.5 * (Ci + Ci.T))
    return out


def _phat(eng):
    out = []
    for p in eng.psrs:
        ra, dec = p.loc["RAJ"] * np.pi / 12, p.loc["DECJ"] * np.pi / 180
        out.append([np.cos(dec) * np.cos(ra), np.cos(dec) * np.sin(ra), np.sin(dec)])
    return np.array(out)


def _antenna(phat, cos_t, phi):
    th = np.arccos(cos_t)
    m = np.array([np.sin(phi), -np.cos(phi), 0.0])
    n = np.array([-np.cos(th) * np.cos(phi), -np.cos(th) * np.sin(phi), np.sin(th)])
    om = np.array([-np.sin(th) * np.cos(phi), -np.sin(th) * np.sin(phi), -np.cos(th)])
    d = 1 + om @ phat
    return np.array([0.5 * ((m @ phat) ** 2 - (n @ phat) ** 2) / d, (m @ phat) * (n @ phat) / d])


def _dense_fstat(eng, Pinv, rows, freqs, sky):
    """(Fp [R, J], Fe [R, J, S]) pulsar by pulsar, frequency by frequency, sky point by sky point"""
    P, J, S, R = eng.P, len(freqs), len(sky[0]), rows.shape[0]
    phat = _phat(eng)
    fp, fe = np.zeros((R, J)), np.zeros((R, J, S))
    for j, f in enumerate(freqs):
        q, G = [], []
        for a in range(P):
            t = eng.mjd[a] * 86400.0
            E = np.stack([np.sin(2 * np.pi * f * t), np.cos(2 * np.pi * f * t)], axis=1)
            q.append(rows[:, eng.off[a]:eng.off[a + 1]] @ (Pinv[a] @ E))
            G.append(E.T @ Pinv[a] @ E)
            fp[:, j] += 0.5 * np.einsum("rk,kl,rl->r", q[a], np.linalg.inv(G[a]), q[a])
        for s in range(S):
            N, M = np.zeros((R, 4)), np.zeros((4, 4))
            for a in range(P):
                ph = _antenna(phat[a], sky[0][s], sky[1][s])
                N += np.kron(ph[None, :], q[a])
                M += np.kron(np.outer(ph, ph), G[a])
            fe[:, j, s] = 0.5 * np.einsum("ru,ru->r", N, np.linalg.solve(M, N.T).T)
    return fp, fe


@pytest.mark.parametrize("model", ["spin", "astrometric"])
def test_engine_fstat_vs_dense_numpy(model):
    eng = _engine()
    assert eng.prepare_f_statistic(FREQS, sky=SKY, timing_model=model) is eng
    rows = eng.generate(24, r0=5)
    res = eng.f_statistic(rows)
    fp, fe = _dense_fstat(eng, _dense_projectors(eng, model, 10 ** (2 * -14.4)), rows.cpu().numpy(), FREQS, SKY)
    print(f"{model}: Fp rel = {_rel(res['fp'].cpu().numpy(), fp):.2e}, Fe rel = {_rel(res['fe'].cpu().numpy(), fe):.2e}")
    assert res["fp"].shape == (24, 4) and res["fe"].shape == (24, 4, 5)
    assert np.array_equal(res["freqs"].cpu().numpy(), FREQS)
    assert _rel(res["fp"].cpu().numpy(), fp) < 1e-10
    assert _rel(res["fe"].cpu().numpy(), fe) < 1e-10
    mx = eng.f_statistic(rows, sky_max=True)
    assert set(mx) == {"fp", "freqs", "fe_max", "fe_arg"} and mx["fe_arg"].dtype == torch.int32
    assert torch.equal(mx["fp"], res["fp"])
    assert np.array_equal(mx["fe_arg"].cpu().numpy(), fe.argmax(axis=2))


def test_engine_fstat_gwb_auto_off_and_fp_only():
    eng = _engine()
    eng.prepare_f_statistic(FREQS, gwb_auto=False, timing_model=None)
    rows = eng.generate(6)
    res = eng.f_statistic(rows)
    assert set(res) == {"fp", "freqs"}
    fp, _ = _dense_fstat(eng, _dense_projectors(eng, None, 0.0), rows.cpu().numpy(), FREQS, (SKY[0][:1], SKY[1][:1]))
    assert _rel(res["fp"].cpu().numpy(), fp) < 1e-10
    eng.prepare_f_statistic(FREQS, gwb_auto=-14.0, components=8)
    fp, _ = _dense_fstat(eng, _dense_projectors(eng, "spin", 1e-28, nf=8), rows.cpu().numpy(), FREQS, (SKY[0][:1], SKY[1][:1]))
    assert _rel(eng.f_statistic(rows)["fp"].cpu().numpy(), fp) < 1e-10


def test_headline_size_vs_host_plan():
    import bench
    from pta_replicator_amd import f_statistic as fst
    from pta_replicator_amd.engine import ReplicaEngine
    psrs, noise = bench.headline_array()
    eng = bench.configure_engine(ReplicaEngine(psrs, seed=5), noise)
    eng.td_warmup = False
    eng.prepare()
    rng = np.random.default_rng(2)
    freqs = np.geomspace(4e-9, 2e-7, 24)
    sky = (rng.uniform(-1, 1, 40), rng.uniform(0, 2 * np.pi, 40))
    eng.prepare_f_statistic(freqs, sky=sky)
    rows = eng.generate(64)
    res = eng.f_statistic(rows)
    fp, fe = fst.fstat_from_rows(eng._fs["plan"], rows.cpu().numpy())
    print(f"headline: Fp rel = {_rel(res['fp'].cpu().numpy(), fp):.2e}, Fe rel = {_rel(res['fe'].cpu().numpy(), fe):.2e}")
    assert _rel(res["fp"].cpu().numpy(), fp) < 1e-11
    assert _rel(res["fe"].cpu().numpy(), fe) < 1e-11
    mx = eng.f_statistic(rows, sky_max=True)
    assert torch.equal(mx["fe_max"], res["fe"].max(dim=2).values)


# ---------------------------------------------------------------- bit-identity ------------------------------------------------
def _same(a, b):
    return set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


def test_generate_f_statistic_bit_identical_to_f_statistic_of_generate():
    eng = _engine()
    eng.prepare_f_statistic(FREQS, sky=SKY)
    R = 300
    ref = eng.f_statistic(eng.generate(R))
    for chunk in (7, 256, R):
        assert _same(eng.generate_f_statistic(R, chunk=chunk), ref), chunk
    sub = eng.generate_f_statistic(50, r0=123, chunk=16)
    assert torch.equal(sub["fp"], ref["fp"][123:173]) and torch.equal(sub["fe"], ref["fe"][123:173])
    # from a different batch of generate(): realisation r is the same numbers wherever it is computed
    assert torch.equal(eng.f_statistic(eng.generate(9, r0=200))["fe"], ref["fe"][200:209])
    # the sky_max values are the full map's maxima, bit for bit, whatever the chunk
    refmax = eng.f_statistic(eng.generate(R), sky_max=True)
    assert torch.equal(refmax["fe_max"], ref["fe"].max(dim=2).values)
    assert np.array_equal(refmax["fe_arg"].cpu().numpy(), ref["fe"].cpu().numpy().argmax(axis=2))
    for chunk in (7, R):
        assert _same(eng.generate_f_statistic(R, chunk=chunk, sky_max=True), refmax), chunk
    # a workspace that holds Q of 11 realisations only: f_statistic cuts the rows, the values stay
    keep = eng.workspace_bytes
    eng.workspace_bytes = max(8 * 2 * len(FREQS) * eng.n_toa, 11 * 8 * eng.P * 2 * len(FREQS))
    try:
        assert eng._sky_chunk(eng._fs, R, False, False) < R
        assert _same(eng.f_statistic(eng.generate(R)), ref)
    finally:
        eng.workspace_bytes = keep


def test_generate_f_statistic_td_bit_identical():
    eng = _engine(gw=None)
    eng.prepare_td()
    eng.prepare_f_statistic(FREQS, sky=SKY)
    R = 40
    ref = eng.f_statistic(eng.generate_td(R))
    for chunk in (7, R):
        assert _same(eng.generate_f_statistic(R, td=True, chunk=chunk), ref)
    assert torch.equal(eng.generate_f_statistic(10, r0=25, td=True, chunk=3)["fe"], ref["fe"][25:35])


def test_generate_f_statistic_theta_bit_identical():
    eng = _engine()
    eng.set_cw(psrTerm=False, evolve=False)
    eng.set_hyper_prior(gwb_log10_A=(-15.0, -14.0), rn_log10_A=(-14.5, -13.5))
    eng.set_cw_prior(log10_mc=(8.5, 9.5), log10_fgw=(-8.3, -7.5), log10_h=(-14.5, -13.5))
    eng.prepare_f_statistic(FREQS, sky=SKY)
    R = 70
    theta = eng.sample_theta(R)
    assert any(k.startswith("cw_") for k in theta)
    ref = eng.f_statistic(eng.generate(R, theta=theta))
    for chunk in (7, R):
        assert _same(eng.generate_f_statistic(R, theta=theta, chunk=chunk), ref)
    rows, th = eng.generate_sampled(R)
    assert torch.equal(eng.f_statistic(rows)["fe"], ref["fe"])
    # CW keys alone in TD mode
    eng2 = _engine(gw=None)
    eng2.set_cw(psrTerm=False, evolve=False)
    eng2.prepare_td()
    eng2.prepare_f_statistic(FREQS, sky=SKY)
    cw = {k: v for k, v in theta.items() if k.startswith("cw_")}
    rows = eng2.generate_td(R)
    eng2._cw_apply(eng2._theta_parts(cw, R, td=True)[1], R, rows)
    assert _same(eng2.generate_f_statistic(R, theta=cw, td=True, chunk=16), eng2.f_statistic(rows))


# ---------------------------------------------------------------- statistics --------------------------------------------------
NULL_FREQS = np.array([4.3e-9, 6.9e-9, 1.07e-8, 1.61e-8, 2.29e-8, 3.05e-8, 4.21e-8, 5.83e-8])
NULL_SKY = (np.array([-0.9, -0.65, -0.4, -0.2, -0.05, 0.1, 0.25, 0.4, 0.55, 0.7, 0.85, 0.97]),
            np.array([0.2, 3.9, 1.1, 5.6, 2.4, 0.7, 4.6, 3.1, 1.8, 6.0, 2.9, 5.0]))


def _null_engine():
    """16 pulsars, white noise + ECORR + red noise and no GWB: the statistic's noise model is the data covariance"""
    return _engine(P=16, n0=120, gw=None, psr_seed=3)


def test_exact_null_moments():
    """the chi^2 moments of Fp (2 P degrees of freedom) and Fe (4) with their sampling errors; the observed ranges are printed"""
    eng = _null_engine()
    eng.prepare_f_statistic(NULL_FREQS, sky=NULL_SKY)
    R, P = 4096, eng.P
    res = eng.generate_f_statistic(R, chunk=1024)
    fp, fe = res["fp"].cpu().numpy(), res["fe"].cpu().numpy()
    assert fp.shape == (R, 8) and fe.shape == (R, 8, 12)
    m, v = fp.mean(axis=0), fp.var(axis=0, ddof=1)
    print("null Fp mean - P in", (m - P).min(), (m - P).max(), "of +-", 5 * np.sqrt(P / R), "; var / P - 1 in", (v / P - 1).min(), (v / P - 1).max(),
          "of +-", 5 * np.sqrt(2 / (R - 1) + 12 / (2 * P * R)))
    m2, v2 = fe.mean(axis=0), fe.var(axis=0, ddof=1)
    print("null Fe mean - 2 in", (m2 - 2).min(), (m2 - 2).max(), "of +-", 5 * np.sqrt(2 / R), "; var / 2 - 1 in", (v2 / 2 - 1).min(), (v2 / 2 - 1).max(),
          "of +-", 5 * np.sqrt(2 / (R - 1) + 3 / R))
    assert np.all(np.abs(m - P) < 5 * np.sqrt(P / R)), m
    assert np.all(np.abs(v / P - 1) < 5 * np.sqrt(2 / (R - 1) + 12 / (2 * P * R))), v
    assert np.all(np.abs(m2 - 2) < 5 * np.sqrt(2 / R)), m2
    assert np.all(np.abs(v2 / 2 - 1) < 5 * np.sqrt(2 / (R - 1) + 3 / R)), v2


JS, SS = 5, 7     # the grid point of the injected source


def _source_theta(R, log10_h, vary):
    rng = np.random.default_rng(17)

    def col(lo, hi):
        return rng.uniform(lo, hi, R) if vary else np.full(R, rng.uniform(lo, hi))
    return {"cw_cos_gwtheta": np.full(R, NULL_SKY[0][SS]), "cw_gwphi": np.full(R, NULL_SKY[1][SS]), "cw_log10_mc": np.full(R, 9.0),
            "cw_log10_fgw": np.full(R, np.log10(NULL_FREQS[JS])), "cw_phase0": col(0, 2 * np.pi), "cw_psi": col(0, np.pi),
            "cw_cos_inc": col(-1, 1), "cw_log10_h": np.full(R, log10_h) + (rng.uniform(-0.3, 0.3, R) if vary else 0.0)}


def _rho2(eng, Pinv, cw):
    """rho^2 [R] and its per-pulsar parts [R, P] of noiseless rows cw [R, n_toa]"""
    parts = np.stack([np.einsum("ri,ij,rj->r", cw[:, eng.off[a]:eng.off[a + 1]], Pinv[a], cw[:, eng.off[a]:eng.off[a + 1]]) for a in range(eng.P)], axis=1)
    return parts.sum(axis=1), parts


def test_source_identity():
    """a monochromatic earth-term source of set_cw at grid point (j*, s*), any psi / inclination / phase / strain: the noiseless term
    lies in the span of phi_a(s*) (x) E_aj*, so Fe[r, j*, s*] = rho_r^2 / 2 and no grid point exceeds it - the statistic's antenna
    patterns and time convention are the injector's"""
    eng = _null_engine()
    eng.set_cw(psrTerm=False, evolve=False)
    eng.prepare_f_statistic(NULL_FREQS, sky=NULL_SKY)
    R = 12
    theta = _source_theta(R, -14.0, vary=True)
    cw = eng.generate_per_signal(R, theta=theta)["cw"]
    res = eng.f_statistic(cw)
    rho2, _ = _rho2(eng, _dense_projectors(eng, "spin", 0.0), cw.cpu().numpy())
    fe = res["fe"].cpu().numpy()
    err = np.max(np.abs(fe[:, JS, SS] - 0.5 * rho2) / (0.5 * rho2))
    print(f"source identity: max |Fe - rho^2 / 2| / (rho^2 / 2) = {err:.2e}; rho^2 in {rho2.min():.3g} .. {rho2.max():.3g}")
    assert err < 1e-9
    for r in range(R):
        assert np.unravel_index(np.argmax(fe[r]), fe[r].shape) == (JS, SS), r
    mx = eng.f_statistic(cw, sky_max=True)
    assert np.all(mx["fe_arg"].cpu().numpy()[:, JS] == SS)


def test_source_recovery_in_noise():
    eng = _null_engine()
    eng.set_cw(psrTerm=False, evolve=False)
    eng.prepare_f_statistic(NULL_FREQS, sky=NULL_SKY)
    Pinv = _dense_projectors(eng, "spin", 0.0)
    # the strain that gives rho^2 = 50: the term is linear in h
    probe = _source_theta(1, -14.0, vary=False)
    r0, _ = _rho2(eng, Pinv, eng.generate_per_signal(1, theta=probe)["cw"].cpu().numpy())
    log10_h = -14.0 + 0.5 * np.log10(50.0 / r0[0])
    R, P = 2048, eng.P
    theta = _source_theta(R, log10_h, vary=False)
    rho2, parts = _rho2(eng, Pinv, eng.generate_per_signal(1, theta=_source_theta(1, log10_h, vary=False))["cw"].cpu().numpy())
    rho2 = float(rho2[0])
    assert abs(rho2 - 50.0) < 1e-6 * 50
    res = eng.generate_f_statistic(R, theta=theta, chunk=512)
    fe2, fp2 = 2 * res["fe"][:, JS, SS].cpu().numpy(), 2 * res["fp"][:, JS].cpu().numpy()
    print(f"source in noise: mean 2Fe = {fe2.mean():.3f} (4 + rho^2 = {4 + rho2:.3f} +- {5 * np.sqrt(2 * (4 + 2 * rho2) / R):.3f}), "
          f"mean 2Fp = {fp2.mean():.3f} (2P + rho^2 = {2 * P + rho2:.3f} +- {5 * np.sqrt(2 * (2 * P + 2 * rho2) / R):.3f})")
    assert abs(fe2.mean() - (4 + rho2)) < 5 * np.sqrt(2 * (4 + 2 * rho2) / R)
    # 2 Fp ~ chi^2(2 P; sum_a rho_a^2): variance 2 (2 P + 2 sum rho_a^2)
    assert abs(fp2.mean() - (2 * P + parts.sum())) < 5 * np.sqrt(2 * (2 * P + 2 * parts.sum()) / R)


# ---------------------------------------------------------------- refusals ----------------------------------------------------
def test_refusals():
    from pta_replicator_amd import device as dv
    from pta_replicator_amd.engine import ReplicaEngine
    eng = _engine(P=3, n0=60)
    rows = eng.generate(4)
    with pytest.raises(ValueError, match="not prepared"):
        eng.f_statistic(rows)
    with pytest.raises(ValueError, match="not prepared"):
        eng.generate_f_statistic(4)
    with pytest.raises(ValueError, match="freqs"):
        eng.prepare_f_statistic([1e-8, -1e-8])
    with pytest.raises(ValueError, match="freqs"):
        eng.prepare_f_statistic([1e-8, np.nan])
    with pytest.raises(ValueError, match=r"\|cos_gwtheta\| > 1"):
        eng.prepare_f_statistic(FREQS, sky=(np.array([1.5]), np.array([0.0])))
    with pytest.raises(ValueError, match="timing_model"):
        eng.prepare_f_statistic(FREQS, timing_model="binary")
    with pytest.raises(ValueError, match="singular"):
        eng.prepare_f_statistic([1e-8, 1.0 / (365.25 * 86400.0)], timing_model="astrometric")
    assert getattr(eng, "_fs", None) is None
    keep = eng.workspace_bytes
    eng.workspace_bytes = 2 * len(FREQS) * eng.n_toa * 8 - 1
    with pytest.raises(ValueError, match="workspace_bytes"):
        eng.prepare_f_statistic(FREQS)
    eng.workspace_bytes = keep
    eng.prepare_f_statistic(FREQS)                   # Fp only
    with pytest.raises(ValueError, match="sky_max=True needs a sky grid"):
        eng.f_statistic(rows, sky_max=True)
    with pytest.raises(ValueError, match="sky_max=True needs a sky grid"):
        eng.generate_f_statistic(4, sky_max=True)
    with pytest.raises(ValueError, match="rows must be"):
        eng.f_statistic(rows[:, :-1])
    with pytest.raises(ValueError, match="rows must be"):
        eng.f_statistic(rows[0])
    with pytest.raises(ValueError, match="stride"):
        eng.f_statistic(dv.empty((eng.n_toa, 4)).T)
    with pytest.raises(ValueError, match="float64 device"):
        eng.f_statistic(rows.cpu())
    with pytest.raises(ValueError, match="float64 device"):
        eng.f_statistic(rows.float())
    with pytest.raises(ValueError, match="must be >= 1"):
        eng.generate_f_statistic(0)
    eng.set_gwb(-15.0, 13. / 3.)      # re-configured: the prepared statistic is stale
    with pytest.raises(ValueError, match="re-configured"):
        eng.f_statistic(rows)
    with pytest.raises(ValueError, match="re-configured"):
        eng.generate_f_statistic(4)
    # one pulsar: Fp works, Fe is refused
    one = ReplicaEngine(_psrs(1, 80, 5), seed=1)
    one.td_warmup = False
    one.set_white_noise(efac=1.0)
    with pytest.raises(ValueError, match="at least two pulsars"):
        one.prepare_f_statistic(FREQS, sky=SKY)
    fp = one.prepare_f_statistic(FREQS).f_statistic(one.generate(3))["fp"]
    assert fp.shape == (3, 4) and bool(torch.all(fp > 0))
    # no white noise
    bare = ReplicaEngine(_psrs(2, 50, 1), seed=1)
    bare.td_warmup = False
    bare.set_red_noise([-14.0, -14.0], [3.0, 3.0], components=5)
    with pytest.raises(ValueError, match="measurement noise"):
        bare.prepare_f_statistic(FREQS)
