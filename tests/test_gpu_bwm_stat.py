"""The burst-with-memory matched filter on the device: pta_bwm_stat against NumPy on random operands, the engine against the dense
NumPy of tests/test_bwm_statistic_host.py, bit-identity across chunks / offsets / output modes / TD mode, the noiseless identity and
recovery of an injected burst, the null moments, and the refusals."""
import ctypes

import numpy as np
import pytest
import torch

import launch_cases as lc
from test_bwm_statistic_host import SKY, T0_MJD, dense_bwm, rel
from test_gpu_fstat import _dense_projectors, _phat
from test_gpu_os import _engine, _psrs

pytestmark = pytest.mark.gpu


def _operands(P, J, S, R, seed):
    rng = np.random.default_rng(seed)
    C = J + (J & 1)
    Q = rng.normal(size=(R, P, C))          # the pad column holds numbers too: the kernel must not read it
    phi = rng.normal(size=(P, S, 2))
    A = rng.normal(size=(J, S, 2, 2))
    Minv = A @ np.swapaxes(A, -1, -2) + np.eye(2)
    return Q, phi, Minv, C


def _packed(Minv):
    return np.stack([Minv[..., 0, 0], Minv[..., 0, 1], Minv[..., 1, 1]], axis=-1)


@pytest.mark.parametrize("P,J,S,R", [(23, 11, 100, 37), (68, 8, 64, 9), (2, 1, 1, 1), (5, 17, 130, 300),
                                     (4, 16, 64, 4), (128, 17, 65, 5)])   # one full MFMA step / epoch block / sky tile; PMAX, one past each
def test_bwm_stat_vs_numpy_all_modes(P, J, S, R):
    from pta_replicator_amd import _lib, bwm_statistic as bst, device as dv
    Q, phi, Minv, C = _operands(P, J, S, R, P + J)
    dQ, dphi, dM = dv.f64(Q.reshape(R, -1)), dv.f64(phi), dv.f64(_packed(Minv))
    s = dv.stream_ptr()
    ref_f, ref_a = bst.bwm_from_Q(phi, Minv, Q[:, :, :J])
    # the map alone, with a pad cell behind every row
    fb = dv.zeros((R, J * S + 1))
    _lib.call("pta_bwm_stat", dv.ptr(dQ), P * C, P, C, J, R, dv.ptr(dphi), S, dv.ptr(dM), dv.ptr(fb), J * S + 1, None, 0, None, 0, None, 0, None, None, s)
    got = fb.cpu().numpy()
    err = rel(got[:, :J * S].reshape(R, J, S), ref_f)
    assert np.all(got[:, J * S] == 0)
    # the map with the amplitudes
    fb2, amp = dv.zeros((R, J * S)), dv.zeros((R, 2 * J * S + 2))
    _lib.call("pta_bwm_stat", dv.ptr(dQ), P * C, P, C, J, R, dv.ptr(dphi), S, dv.ptr(dM), dv.ptr(fb2), J * S, dv.ptr(amp), 2 * J * S + 2, None, 0, None, 0,
              None, None, s)
    ga = amp.cpu().numpy()
    err_a = rel(ga[:, :2 * J * S].reshape(R, J, S, 2), ref_a)
    print(f"pta_bwm_stat P={P} J={J} S={S} R={R}: Fb rel = {err:.2e}, A rel = {err_a:.2e}")
    assert err < 1e-12 and err_a < 1e-12
    assert np.array_equal(fb2.cpu().numpy(), got[:, :J * S]) and np.all(ga[:, 2 * J * S:] == 0)
    # the maxima: bit for bit the map's own
    nt = int(_lib.lib.pta_fstat_fe_tiles(S))
    mx, arg = dv.zeros((R, J)), torch.full((R, J), -1, dtype=torch.int32, device=fb.device)
    pv, pa = dv.empty((R * J * nt,)), torch.empty((R * J * nt,), dtype=torch.int32, device=fb.device)
    _lib.call("pta_bwm_stat", dv.ptr(dQ), P * C, P, C, J, R, dv.ptr(dphi), S, dv.ptr(dM), None, 0, None, 0, dv.ptr(mx), J, dv.ptr(arg), J, dv.ptr(pv),
              dv.ptr(pa), s)
    full = got[:, :J * S].reshape(R, J, S)
    assert np.array_equal(mx.cpu().numpy(), full.max(axis=2))
    assert np.array_equal(arg.cpu().numpy(), full.argmax(axis=2))        # NumPy's argmax is the first = lowest index
    # a realisation's values do not depend on the batch it is computed in
    if R >= 9:
        fb3 = dv.zeros((4, J * S))
        _lib.call("pta_bwm_stat", ctypes.c_void_p(dQ.data_ptr() + 8 * 5 * P * C), P * C, P, C, J, 4, dv.ptr(dphi), S, dv.ptr(dM), dv.ptr(fb3), J * S, None, 0,
                  None, 0, None, 0, None, None, s)
        assert np.array_equal(fb3.cpu().numpy(), got[5:9, :J * S])


def _bwm_launch(dQ, P, C, J, R, dphi, S, dM):
    """(Fb [R, J S], amplitudes [R, 2 J S], maxima [R, J], argmaxima [R, J]) of pta_bwm_stat: the map with the amplitudes, and the maxima"""
    from pta_replicator_amd import _lib, device as dv
    s = dv.stream_ptr()
    fb, amp = dv.zeros((R, J * S)), dv.zeros((R, 2 * J * S))
    _lib.call("pta_bwm_stat", dQ, P * C, P, C, J, R, dv.ptr(dphi), S, dv.ptr(dM), dv.ptr(fb), J * S, dv.ptr(amp), 2 * J * S, None, 0, None, 0, None, None, s)
    nt = int(_lib.lib.pta_fstat_fe_tiles(S))
    mx, arg = dv.zeros((R, J)), torch.full((R, J), -1, dtype=torch.int32, device=fb.device)
    pv, pa = dv.empty((R * J * nt,)), torch.empty((R * J * nt,), dtype=torch.int32, device=fb.device)
    _lib.call("pta_bwm_stat", dQ, P * C, P, C, J, R, dv.ptr(dphi), S, dv.ptr(dM), None, 0, None, 0, dv.ptr(mx), J, dv.ptr(arg), J, dv.ptr(pv), dv.ptr(pa), s)
    return fb, amp, mx, arg


def _bwm_case(P, J, S, R, windows, what):
    """the map, the amplitudes and the maxima against bwm_from_Q (the file's 1e-12; the maxima against the map bit for bit); then the
    realisations of each window (first, count) in a launch of their own, which one workgroup walks: bit for bit the large launch's"""
    from pta_replicator_amd import bwm_statistic as bst, device as dv
    Q, phi, Minv, C = _operands(P, J, S, R, P + J + S)
    dQ, dphi, dM = dv.f64(Q.reshape(R, -1)), dv.f64(phi), dv.f64(_packed(Minv))
    ref_f, ref_a = bst.bwm_from_Q(phi, Minv, Q[:, :, :J])
    fb, amp, mx, arg = _bwm_launch(dv.ptr(dQ), P, C, J, R, dphi, S, dM)
    full = fb.cpu().numpy().reshape(R, J, S)
    err, err_a = rel(full, ref_f), rel(amp.cpu().numpy().reshape(R, J, S, 2), ref_a)
    print(f"pta_bwm_stat {what} P={P} J={J} S={S} R={R}: Fb rel = {err:.2e}, A rel = {err_a:.2e}, error / bound {max(err, err_a) / 1e-12:.4f}")
    assert err < 1e-12 and err_a < 1e-12
    assert np.array_equal(mx.cpu().numpy(), full.max(axis=2))
    assert np.array_equal(arg.cpu().numpy(), full.argmax(axis=2))        # NumPy's argmax is the first = lowest index
    for lo, n in windows:
        assert lc.plan("pta_bwm_stat", P, J, n, S)["ngz"] == 1
        sub = _bwm_launch(dv.row_ptr(dQ, lo), P, C, J, n, dphi, S, dM)
        assert all(torch.equal(x, y[lo:lo + n]) for x, y in zip(sub, (fb, amp, mx, arg))), (lo, n)


@pytest.mark.parametrize("shape", lc.SKY_CHUNK["pta_bwm_stat"], ids=lambda c: f"rchunk{c['rchunk']}")
def test_bwm_stat_realisation_chunks(shape):
    """rchunk, the realisations one workgroup of k_sky_stat walks: 9 (a sky grid of more than 512 workgroups: the chunk is no multiple
    of the 4 realisations that share a scan of the maxima, so the flush ends a chunk part-way), 8, and all of 7 realisations in one
    workgroup.  Measured on one MI355X: worst relative error 4.0e-16 (Fb), 2.3e-16 (A), error / bound 0.0004."""
    P, J, S, R = (shape[k] for k in "PJSR")
    assert lc.plan("pta_bwm_stat", P, J, R, S)["rchunk"] == shape["rchunk"]
    _bwm_case(P, J, S, R, shape["windows"], f"rchunk={shape['rchunk']}")


@pytest.mark.parametrize("P", lc.SKY_KS_P)
def test_bwm_stat_every_pulsar_step_count(P):
    """k_sky_stat<bwm_stat, KS, mode> for every KS = ceil(P / 4) = 1 .. 32 in both modes (the other tests reach six of them), full steps
    (P = 4 k) and steps of one pulsar (P = 4 k + 1).  Measured on one MI355X: worst relative error 9.4e-16 (Fb), 6.8e-16 (A), error / bound 0.0009."""
    J, S, R = (lc.SKY_KS_SHAPE[k] for k in "JSR")
    assert lc.plan("pta_bwm_stat", P, J, R, S)["ks"] == (P + 3) // 4
    _bwm_case(P, J, S, R, ((R - 1, 1),), f"ks={(P + 3) // 4}")


def test_bwm_stat_ties_take_the_lowest_index():
    """identical sky points give identical values: the argmax is the first of them, inside a 16-point group, across groups and
    across workgroup tiles"""
    from pta_replicator_amd import _lib, bwm_statistic as bst, device as dv
    P, J, S, R = 6, 3, 200, 5
    Q, phi, Minv, C = _operands(P, J, S, R, 9)
    phi[:, :, :] = phi[:, :1, :]
    Minv[:, :, :, :] = Minv[:, :1, :, :]
    dQ, dphi, dM = dv.f64(Q.reshape(R, -1)), dv.f64(phi), dv.f64(_packed(Minv))
    nt = int(_lib.lib.pta_fstat_fe_tiles(S))
    mx, arg = dv.zeros((R, J)), torch.full((R, J), -1, dtype=torch.int32, device=dQ.device)
    pv, pa = dv.empty((R * J * nt,)), torch.empty((R * J * nt,), dtype=torch.int32, device=dQ.device)
    _lib.call("pta_bwm_stat", dv.ptr(dQ), P * C, P, C, J, R, dv.ptr(dphi), S, dv.ptr(dM), None, 0, None, 0, dv.ptr(mx), J, dv.ptr(arg), J, dv.ptr(pv),
              dv.ptr(pa), dv.stream_ptr())
    assert np.all(arg.cpu().numpy() == 0)
    assert rel(mx.cpu().numpy(), bst.bwm_from_Q(phi, Minv, Q[:, :, :J])[0][:, :, 0]) < 1e-12


# ---------------------------------------------------------------- engines -----------------------------------------------------
def _toas(eng):
    return [m * 86400.0 for m in eng.mjd]


def test_engine_bwm_statistic_vs_dense_numpy():
    eng = _engine()
    assert eng.prepare_bwm_statistic(T0_MJD, SKY) is eng
    plan = eng._bs["plan"]
    sens = (plan.g > 0).sum(axis=0)
    print("sensitive pulsars per epoch:", sens)
    assert np.all(sens >= 2)
    rows = eng.generate(24, r0=5)
    res = eng.bwm_statistic(rows, amplitudes=True)
    assert set(res) == {"fb", "amp", "t0_mjd"} and res["fb"].shape == (24, 4, 5) and res["amp"].shape == (24, 4, 5, 2)
    assert np.array_equal(res["t0_mjd"].cpu().numpy(), T0_MJD)
    Pinv = _dense_projectors(eng, "spin", 10 ** (2 * -14.4))
    _, _, _, fb, amp = dense_bwm(Pinv, _toas(eng), _phat(eng), T0_MJD * 86400.0, SKY, rows.cpu().numpy())
    e_f, e_a = rel(res["fb"].cpu().numpy(), fb), rel(res["amp"].cpu().numpy(), amp)
    print(f"engine against dense NumPy: Fb rel = {e_f:.2e}, A rel = {e_a:.2e}")
    assert e_f < 1e-9 and e_a < 1e-9
    only = eng.bwm_statistic(rows)
    assert set(only) == {"fb", "t0_mjd"} and torch.equal(only["fb"], res["fb"])
    mx = eng.bwm_statistic(rows, sky_max=True)
    assert set(mx) == {"fb_max", "fb_arg", "t0_mjd"} and mx["fb_arg"].dtype == torch.int32
    assert torch.equal(mx["fb_max"], res["fb"].max(dim=2).values)
    assert np.array_equal(mx["fb_arg"].cpu().numpy(), res["fb"].cpu().numpy().argmax(axis=2))


def _theta(R, seed=3):
    rng = np.random.default_rng(seed)
    return {"bwm_log10_h": rng.uniform(-14.5, -13, R), "bwm_cos_gwtheta": rng.uniform(-1, 1, R), "bwm_gwphi": rng.uniform(0, 2 * np.pi, R),
            "bwm_psi": rng.uniform(0, np.pi, R), "bwm_t0_mjd": rng.uniform(53500, 57000, R)}


def test_generate_bwm_statistic_bit_identical():
    """chunks 1, 7, R; r0 offsets; sky_max against the map's own maximum; theta; TD mode"""
    R = 19
    eng = _engine().set_bwm()
    eng.prepare_bwm_statistic(T0_MJD, SKY)
    th = _theta(R)
    for theta in (None, th):
        ref = eng.bwm_statistic(eng.generate(R, r0=6, theta=theta), amplitudes=True)
        for chunk in (1, 7, R):
            got = eng.generate_bwm_statistic(R, r0=6, theta=theta, chunk=chunk, amplitudes=True)
            assert torch.equal(got["fb"], ref["fb"]) and torch.equal(got["amp"], ref["amp"]), chunk
        part = eng.generate_bwm_statistic(5, r0=6 + 8, theta=None if theta is None else {k: v[8:13] for k, v in theta.items()}, chunk=3)
        assert torch.equal(part["fb"], ref["fb"][8:13])
        mx = eng.generate_bwm_statistic(R, r0=6, theta=theta, chunk=7, sky_max=True)
        assert torch.equal(mx["fb_max"], ref["fb"].max(dim=2).values)
        assert np.array_equal(mx["fb_arg"].cpu().numpy(), ref["fb"].cpu().numpy().argmax(axis=2))
    ref_td = eng.bwm_statistic(eng.generate_td(R, r0=6, theta=th))
    assert torch.equal(eng.generate_bwm_statistic(R, r0=6, theta=th, td=True, chunk=7)["fb"], ref_td["fb"])
    ref_td0 = eng.bwm_statistic(eng.generate_td(R, r0=6))
    assert torch.equal(eng.generate_bwm_statistic(R, r0=6, td=True, chunk=R)["fb"], ref_td0["fb"])


JS, SS = 2, 3     # the grid point of the injected burst


def test_injected_burst_identity_and_recovery():
    """a burst of set_bwm injected through theta at grid point (j*, s*), any strain / polarisation: on its noiseless term Fb[r, j*, s*]
    = rho_r^2 / 2 against the dense rho^2, A = (h cos 2psi, h sin 2psi), and the map's maximum sits at that cell - the statistic's
    antenna patterns, epoch and time convention are the injector's.  Bound: ten times the 2.1e-11 the host test measured for the
    same identity (tests/test_bwm_statistic_host.py); measured here: Fb 2.1e-12, A 7.8e-16."""
    eng = _engine().set_bwm()
    eng.prepare_bwm_statistic(T0_MJD, SKY)
    R = 12
    rng = np.random.default_rng(17)
    th = {"bwm_log10_h": rng.uniform(-15, -13, R), "bwm_cos_gwtheta": np.full(R, SKY[0][SS]), "bwm_gwphi": np.full(R, SKY[1][SS]),
          "bwm_psi": rng.uniform(0, np.pi, R), "bwm_t0_mjd": np.full(R, T0_MJD[JS])}
    term = eng.generate_per_signal(R, theta=th)["bwm"]
    res = eng.bwm_statistic(term, amplitudes=True)
    Pinv = _dense_projectors(eng, "spin", 10 ** (2 * -14.4))
    x = term.cpu().numpy()
    rho2 = sum(np.einsum("ri,ij,rj->r", x[:, eng.off[a]:eng.off[a + 1]], Pinv[a], x[:, eng.off[a]:eng.off[a + 1]]) for a in range(eng.P))
    fb, amp = res["fb"].cpu().numpy(), res["amp"].cpu().numpy()
    h = 10 ** th["bwm_log10_h"]
    want = np.stack([h * np.cos(2 * th["bwm_psi"]), h * np.sin(2 * th["bwm_psi"])], axis=1)
    e_f = np.max(np.abs(fb[:, JS, SS] / (0.5 * rho2) - 1))
    e_a = np.max(np.abs(amp[:, JS, SS] - want) / h[:, None])
    print(f"identity: |Fb / (rho^2 / 2) - 1| <= {e_f:.2e}, |A - (h cos 2psi, h sin 2psi)| / h <= {e_a:.2e}; rho^2 in {rho2.min():.3g} .. {rho2.max():.3g}")
    assert e_f <= 2.1e-10 and e_a <= 2.1e-10
    for r in range(R):
        assert np.unravel_index(np.argmax(fb[r]), fb[r].shape) == (JS, SS), r
    mx = eng.bwm_statistic(term, sky_max=True)
    assert np.all(mx["fb_arg"].cpu().numpy()[:, JS] == SS)


def test_exact_null_moments():
    """no GWB, so the statistic's noise model is the data covariance: 2 Fb ~ chi^2(2) in every cell.  |mean - 2| < 5 * 2 / sqrt(R) and
    |var - 4| < 5 sqrt(128 / R) (the fourth central moment of chi^2(2) is 144: var of the sample variance = (144 - 16) / R); seeded."""
    eng = _engine(gw=None)
    eng.prepare_bwm_statistic(T0_MJD, SKY)
    R = 4096
    f2 = 2 * eng.generate_bwm_statistic(R, chunk=1024)["fb"].cpu().numpy()
    assert f2.shape == (R, 4, 5)
    m, v = f2.mean(axis=0), f2.var(axis=0, ddof=1)
    print("null 2Fb: mean - 2 in", (m - 2).min(), (m - 2).max(), "of +-", 5 * 2 / np.sqrt(R), "; var - 4 in", (v - 4).min(), (v - 4).max(), "of +-",
          5 * np.sqrt(128 / R))
    assert np.all(np.abs(m - 2) < 5 * 2 / np.sqrt(R)), m
    assert np.all(np.abs(v - 4) < 5 * np.sqrt(128 / R)), v


def test_refusals():
    from pta_replicator_amd import _lib
    from pta_replicator_amd.engine import ReplicaEngine
    eng = _engine(P=3, n0=60)
    rows = eng.generate(4)
    with pytest.raises(ValueError, match="not prepared"):
        eng.bwm_statistic(rows)
    with pytest.raises(ValueError, match="not prepared"):
        eng.generate_bwm_statistic(4)
    with pytest.raises(ValueError, match="mandatory"):
        eng.prepare_bwm_statistic(T0_MJD, None)
    with pytest.raises(ValueError, match=r"\|cos_gwtheta\| > 1"):
        eng.prepare_bwm_statistic(T0_MJD, (np.array([1.5]), np.array([0.0])))
    with pytest.raises(ValueError, match="finite"):
        eng.prepare_bwm_statistic([54000.0, np.nan], SKY)
    with pytest.raises(ValueError, match="timing_model"):
        eng.prepare_bwm_statistic(T0_MJD, SKY, timing_model="binary")
    with pytest.raises(ValueError, match=f"at most {_lib.FSTAT_CMAX - 1}"):
        eng.prepare_bwm_statistic(np.linspace(53500, 57000, _lib.FSTAT_CMAX), SKY)
    with pytest.raises(ValueError, match=r"singular at epoch 1 \(MJD 57600"):
        eng.prepare_bwm_statistic([55000.0, 57600.0], SKY)
    assert getattr(eng, "_bs", None) is None
    big = ReplicaEngine(_psrs(_lib.FSTAT_PMAX + 1, 6, 2, step=0), seed=1)     # refused before anything is prepared
    with pytest.raises(ValueError, match=f"at most {_lib.FSTAT_PMAX} pulsars"):
        big.prepare_bwm_statistic(T0_MJD, SKY)
    assert not big._prepared
    eng.prepare_bwm_statistic(T0_MJD[1:3], SKY)           # (two of these three short pulsars start after MJD 53100)
    for call in (lambda: eng.bwm_statistic(rows, sky_max=True, amplitudes=True), lambda: eng.generate_bwm_statistic(4, sky_max=True, amplitudes=True)):
        with pytest.raises(ValueError, match="amplitudes=True needs the full map"):
            call()
    with pytest.raises(ValueError, match="float64 device tensor"):
        eng.bwm_statistic(rows.cpu())
    with pytest.raises(ValueError, match="rows must be"):
        eng.bwm_statistic(rows[:, :-1])
    with pytest.raises(ValueError, match="R=0"):
        eng.generate_bwm_statistic(0)
    with pytest.raises(ValueError, match="set_bwm"):
        eng.generate_bwm_statistic(4, theta={"bwm_log10_h": np.zeros(4), "bwm_cos_gwtheta": np.zeros(4), "bwm_gwphi": np.zeros(4), "bwm_psi": np.zeros(4),
                                             "bwm_t0_mjd": np.full(4, 55000.0)})
    eng.prepare()                                     # a prepare() after it: the operands describe the previous plan
    with pytest.raises(ValueError, match="re-configured or re-prepared"):
        eng.bwm_statistic(rows)
    with pytest.raises(ValueError, match="re-configured or re-prepared"):
        eng.generate_bwm_statistic(4)
