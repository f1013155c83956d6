"""Cross-correlation optimal statistic on the MI355X: pta_os_project / pta_os_pairs against NumPy, the engine's OS against a dense
NumPy OS of the same residuals, bit-identity of generate_os across chunks / offsets / modes, the exact null distribution, signal
recovery and the refusals."""
import ctypes

import numpy as np
import pytest
import torch

import launch_cases as lc
from oracle import pta_oracle as po

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(np.asarray(b))))


# ---------------------------------------------------------------- kernels ---------------------------------------------------
@pytest.mark.parametrize("C", [2, 28, 64])
@pytest.mark.parametrize("R", [1, 5, 17, 1000])
def test_os_project_vs_numpy(C, R):
    from pta_replicator_amd import _lib, device as dv
    counts = np.array([1, 15, 17, 64, 65, 130, 301, 16])
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    N, P = int(off[-1]), len(counts)
    rng = np.random.default_rng(C * 1000 + R)
    W = rng.normal(size=(C, N))
    ld_rows = N + 3                                   # a row stride wider than the row, odd
    rows = rng.normal(size=(R, ld_rows))
    dW, drows, doff = dv.f64(W), dv.f64(rows), dv.i32(off)
    Y = dv.zeros((R, P * C + 2))
    _lib.call("pta_os_project", dv.ptr(dW), N, C, dv.ptr(doff), P, dv.ptr(drows), ld_rows, R, dv.ptr(Y), P * C + 2, dv.stream_ptr())
    got = Y.cpu().numpy()
    ref = np.stack([rows[:, off[a]:off[a + 1]] @ W[:, off[a]:off[a + 1]].T for a in range(P)], axis=1).reshape(R, P * C)
    scale = np.stack([np.abs(rows[:, off[a]:off[a + 1]]) @ np.abs(W[:, off[a]:off[a + 1]]).T for a in range(P)], axis=1).reshape(R, P * C)
    assert np.max(np.abs(got[:, :P * C] - ref) / scale) < 1e-12
    assert np.all(got[:, P * C:] == 0)                # nothing written past P * C
    if R >= 17:   # a realisation's Y does not depend on the batch it is computed in
        Y2 = dv.zeros((3, P * C))
        _lib.call("pta_os_project", dv.ptr(dW), N, C, dv.ptr(doff), P, ctypes.c_void_p(drows.data_ptr() + 8 * 13 * ld_rows), ld_rows, 3,
                  dv.ptr(Y2), P * C, dv.stream_ptr())
        assert np.array_equal(Y2.cpu().numpy(), got[13:16, :P * C])


_OS_LARGE = {}


def _os_large():
    """the 1024 ragged pulsars of tests/launch_cases.py at the largest R and C of its cases, on the host and on the device, with the
    long-double reference and sum |w||r| of every (realisation, pulsar, column): made once, every case reads a corner of it"""
    if not _OS_LARGE:
        from pta_replicator_amd import device as dv
        counts = lc.os_counts()
        off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        N, P, Rm, Cm = int(off[-1]), len(counts), max(lc.OS_R), max(lc.OS_C)
        rng = np.random.default_rng(1024)
        ld_rows = (N + 3) | 1                             # a row stride wider than the row, odd
        W, rows = rng.normal(size=(Cm, N)), rng.normal(size=(Rm, ld_rows))
        ref, scale = np.empty((Rm, P, Cm), dtype=np.longdouble), np.empty((Rm, P, Cm))
        Wl, rl = W.astype(np.longdouble), rows.astype(np.longdouble)
        for a in range(P):
            ref[:, a] = rl[:, off[a]:off[a + 1]] @ Wl[:, off[a]:off[a + 1]].T
            scale[:, a] = np.abs(rows[:, off[a]:off[a + 1]]) @ np.abs(W[:, off[a]:off[a + 1]]).T
        _OS_LARGE.update(counts=counts, off=off, N=N, P=P, ld_rows=ld_rows, ref=ref, scale=scale, dW=dv.f64(W), drows=dv.f64(rows), doff=dv.i32(off))
    return _OS_LARGE


@pytest.mark.parametrize("C", lc.OS_C)
@pytest.mark.parametrize("R", lc.OS_R)
def test_os_project_two_tiles_per_wave(C, R):
    """k_os_project<CT, 2>, which the launcher takes from cdiv(R, 128) * P >= 1024 on: 1024 ragged pulsars of 1 .. 40 TOAs, five of
    65 .. 301 (the prefetch of the next K chunk with two tiles in flight).  Value: the device result is one fp64 FMA chain over the n
    TOAs of the pulsar, so |got - ref| <= (n + 2) 2^-53 sum |w||r| against the long-double reference.  Bit-identity: the first and the
    last realisations again, over a window of 8 pulsars, in launches that take one tile per wave (the plan query confirms both).
    Measured on one MI355X: worst error / bound 0.51 (12 cases; 0.32 at C = 2, R = 1)."""
    from pta_replicator_amd import _lib, device as dv
    d = _os_large()
    P, N, ld_rows = d["P"], d["N"], d["ld_rows"]
    assert lc.plan("pta_os_project", C, P, R) == {"rw": 2, "ct": (C + 15) // 16, "grid_x": (R + 127) // 128}
    ld_y = P * C + 2
    Y = dv.zeros((R, ld_y))
    _lib.call("pta_os_project", dv.ptr(d["dW"]), N, C, dv.ptr(d["doff"]), P, dv.ptr(d["drows"]), ld_rows, R, dv.ptr(Y), ld_y, dv.stream_ptr())
    got = Y.cpu().numpy()
    bound = (d["counts"] + 2.0)[None, :, None] * 2.0 ** -53 * d["scale"][:R, :, :C]
    ratio = float(np.max(np.abs(got[:, :P * C].reshape(R, P, C) - d["ref"][:R, :, :C]) / bound))
    print(f"pta_os_project rw=2 C={C} R={R}: worst error / ((n + 2) 2^-53 sum |w||r|) = {ratio:.3f}")
    assert ratio <= 1.0
    assert np.all(got[:, P * C:] == 0)                # nothing written past P * C
    a0, pw = lc.OS_WINDOW
    for lo, n in lc.os_windows(R):
        assert lc.plan("pta_os_project", C, pw, n)["rw"] == 1
        Y2 = dv.zeros((n, pw * C))
        _lib.call("pta_os_project", dv.ptr(d["dW"]), N, C, ctypes.c_void_p(d["doff"].data_ptr() + 4 * a0), pw, dv.row_ptr(d["drows"], lo), ld_rows, n,
                  dv.ptr(Y2), pw * C, dv.stream_ptr())
        assert torch.equal(Y2, Y[lo:lo + n, a0 * C:(a0 + pw) * C]), (lo, n)


@pytest.mark.parametrize("with_rho", [False, True])
def test_os_pairs_vs_numpy(with_rho):
    from pta_replicator_amd import _lib, device as dv
    P, C, R, n_orf = 23, 28, 37, 3
    rng = np.random.default_rng(4)
    Y = rng.normal(size=(R, P * C))
    ia, ib = np.triu_indices(P, 1)
    npairs = len(ia)
    wt = rng.normal(size=(n_orf, npairs))
    den = rng.uniform(0.5, 2.0, npairs)
    dY, dwt, dden = dv.f64(Y), dv.f64(wt), dv.f64(den)
    pa, pb = dv.i32(ia), dv.i32(ib)
    A2 = dv.zeros((R, n_orf))
    rho = dv.zeros((R, npairs)) if with_rho else None
    _lib.call("pta_os_pairs", dv.ptr(dY), P * C, P, C, R, dv.ptr(pa), dv.ptr(pb), npairs, dv.ptr(dwt), n_orf, dv.ptr(A2), n_orf,
              dv.ptr(dden) if with_rho else None, dv.ptr(rho) if with_rho else None, npairs if with_rho else 0, dv.stream_ptr())
    y = Y.reshape(R, P, C)
    num = np.einsum("rpc,rpc->rp", y[:, ia], y[:, ib])
    assert _rel(A2.cpu().numpy(), num @ wt.T) < 1e-12
    if with_rho:
        assert _rel(rho.cpu().numpy(), num / den) < 1e-12


# ---------------------------------------------------------------- engines -----------------------------------------------------
def _psrs(P, n0, seed, step=37, sessions=True, err_us=0.5):
    from pta_replicator_amd.simulate import ArrayTOAs, SimulatedPulsar, make_ideal
    rng = np.random.default_rng(seed)
    out = []
    for a in range(P):
        n = n0 + step * a
        if sessions:   # sessions of three TOAs within 0.05 d: ECORR epochs (0.1 d) hold several TOAs
            sess = np.sort(rng.uniform(53000, 57500, (n + 2) // 3))
            mjd = np.sort(np.repeat(sess, 3)[:n] + rng.uniform(0, 0.05, n))
        else:
            mjd = np.sort(rng.uniform(53000, 57500, n))
        which = rng.integers(0, 2, n)
        p = SimulatedPulsar(toas=ArrayTOAs(mjd, err_us, flags=[{"f": ("A", "B")[k]} for k in which]), name=f"J{a:04d}",
                            loc={"RAJ": float(rng.uniform(0, 24)), "DECJ": float(np.degrees(np.arcsin(rng.uniform(-1, 1))))})
        make_ideal(p)
        out.append(p)
    return out


def _engine(P=6, n0=150, seed=77, gw=-14.4, rn=True, psr_seed=11, no_correlations=False):
    from pta_replicator_amd.engine import ReplicaEngine
    eng = ReplicaEngine(_psrs(P, n0, psr_seed), seed=seed)
    eng.td_warmup = False
    fl = [["A", "B"]] * P
    eng.set_white_noise(efac=[np.array([1.1, 0.9])] * P, log10_equad=[np.array([-6.5, -6.8])] * P, flags=fl)
    eng.set_jitter(log10_ecorr=[np.array([-6.6, -6.9])] * P, flags=fl, coarsegrain=0.1)
    if rn:
        eng.set_red_noise([-14.0 + 0.1 * a for a in range(P)], [3.0 + 0.2 * (a % 4) for a in range(P)], components=20)
    if gw is not None:
        eng.set_gwb(gw, 13. / 3., no_correlations=no_correlations)
    eng.prepare()
    return eng


def _dense_os(eng, rows, nf, model, amp2, gamma=13. / 3.):
    """(A2 [R, 3], sigma [3], rho [R, n_pairs]) of rows [R, n_toa] through dense NumPy: C_a assembled explicitly from the engine's
    configuration, np.linalg.solve, the timing model projected out; ORFs hd, monopole, dipole"""
    from pta_replicator_amd.simulate import timing_design_matrix
    P = eng.P
    toas = [m * 86400.0 for m in eng.mjd]
    T = max(t.max() for t in toas) - min(t.min() for t in toas)
    Ys, Zs = [], []
    for a in range(P):
        t = toas[a]
        n = len(t)
        F, freqs = po.fourier_design_matrix(t, nmodes=nf, Tspan=T)
        S = (1 / (365.25 * 86400)) ** (gamma - 3) * freqs ** (-gamma) / (12 * np.pi ** 2 * T)
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
            C += amp2 * (F * S) @ F.T
        Ci = np.linalg.solve(C, np.eye(n))
        if model is not None:
            M = timing_design_matrix(t, model=model)[0]
            CiM = Ci @ M
            Ci = Ci - CiM @ np.linalg.solve(M.T @ CiM, CiM.T)
        W = np.sqrt(S)[:, None] * (F.T @ Ci)
        Ys.append(rows[:, eng.off[a]:eng.off[a + 1]] @ W.T)
        Zs.append(W @ F * np.sqrt(S)[None, :])
    ia, ib = np.triu_indices(P, 1)
    num = np.stack([np.sum(Ys[a] * Ys[b], axis=1) for a, b in zip(ia, ib)], axis=1)
    den = np.array([np.trace(Zs[a] @ Zs[b]) for a, b in zip(ia, ib)])
    pos = []
    for p in eng.psrs:
        ra, dec = p.loc["RAJ"] * np.pi / 12, p.loc["DECJ"] * np.pi / 180
        pos.append([np.cos(dec) * np.cos(ra), np.cos(dec) * np.sin(ra), np.sin(dec)])
    pos = np.array(pos)
    cz = np.sum(pos[ia] * pos[ib], axis=1)
    x = (1 - cz) / 2
    A2, sig = [], []
    for G in (0.5 - x / 4 + 1.5 * x * np.log(x), np.ones_like(cz), cz):
        A2.append(num @ G / np.sum(G ** 2 * den))
        sig.append(np.sum(G ** 2 * den) ** -0.5)
    return np.stack(A2, axis=1), np.array(sig), num / den


@pytest.mark.parametrize("model", ["spin", "astrometric"])
def test_engine_os_vs_dense_numpy(model):
    eng = _engine()
    nf = 10
    eng.prepare_optimal_statistic(components=nf, timing_model=model)
    rows = eng.generate(24, r0=5)
    res = eng.optimal_statistic(rows, pairs=True)
    A2d, sigd, rhod = _dense_os(eng, rows.cpu().numpy(), nf, model, 10 ** (2 * -14.4))
    assert res["names"] == ["hd", "monopole", "dipole"]
    assert _rel(res["A2"].cpu().numpy(), A2d) < 1e-10
    assert _rel(res["sigma"].cpu().numpy(), sigd) < 1e-10
    assert _rel(res["snr"].cpu().numpy(), A2d / sigd) < 1e-10
    assert _rel(res["rho"].cpu().numpy(), rhod) < 1e-10
    P = eng.P
    assert res["pairs"].shape == (P * (P - 1) // 2, 2) and res["zeta"].shape == (P * (P - 1) // 2,)


def test_engine_os_gwb_auto_off_and_explicit():
    eng = _engine()
    eng.prepare_optimal_statistic(components=8, gwb_auto=False)
    rows = eng.generate(6)
    a = eng.optimal_statistic(rows)["A2"].cpu().numpy()
    assert _rel(a, _dense_os(eng, rows.cpu().numpy(), 8, "spin", 0.0)[0]) < 1e-10
    eng.prepare_optimal_statistic(components=8, gwb_auto=-14.0, timing_model=None)
    b = eng.optimal_statistic(rows)["A2"].cpu().numpy()
    assert _rel(b, _dense_os(eng, rows.cpu().numpy(), 8, None, 1e-28)[0]) < 1e-10


def test_headline_size_vs_host_plan():
    import bench
    from pta_replicator_amd import optimal_statistic as ost
    from pta_replicator_amd.engine import ReplicaEngine
    psrs, noise = bench.headline_array()
    eng = bench.configure_engine(ReplicaEngine(psrs, seed=5), noise)
    eng.td_warmup = False
    eng.prepare()
    eng.prepare_optimal_statistic()
    rows = eng.generate(64)
    res = eng.optimal_statistic(rows, pairs=True)
    A2, snr, num = ost.os_from_rows(eng._os["plan"], rows.cpu().numpy())
    assert _rel(res["A2"].cpu().numpy(), A2) < 1e-11
    assert _rel(res["snr"].cpu().numpy(), snr) < 1e-11
    assert _rel(res["rho"].cpu().numpy(), num / eng._os["plan"].den) < 1e-11


# ---------------------------------------------------------------- bit-identity ------------------------------------------------
def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in ("A2", "snr") + (("rho",) if "rho" in a else ()))


def test_generate_os_bit_identical_to_optimal_statistic_of_generate():
    eng = _engine()
    eng.prepare_optimal_statistic(components=14)
    R = 300
    ref = eng.optimal_statistic(eng.generate(R), pairs=True)
    for chunk in (7, 256, R):
        assert _same(eng.generate_os(R, chunk=chunk, pairs=True), ref), chunk
    sub = eng.generate_os(50, r0=123, chunk=16, pairs=True)
    assert torch.equal(sub["A2"], ref["A2"][123:173]) and torch.equal(sub["rho"], ref["rho"][123:173])
    # and from a different batch of generate(): realisation r is the same numbers wherever it is computed
    assert torch.equal(eng.optimal_statistic(eng.generate(9, r0=200))["A2"], ref["A2"][200:209])


def test_generate_os_td_bit_identical():
    eng = _engine(gw=None)
    eng.prepare_td()
    eng.prepare_optimal_statistic(components=6)
    R = 40
    ref = eng.optimal_statistic(eng.generate_td(R))
    for chunk in (7, R):
        assert _same(eng.generate_os(R, td=True, chunk=chunk), ref)
    assert torch.equal(eng.generate_os(10, r0=25, td=True, chunk=3)["A2"], ref["A2"][25:35])


def test_generate_os_theta_bit_identical():
    eng = _engine()
    eng.set_hyper_prior(gwb_log10_A=(-15.0, -14.0), rn_log10_A=(-14.5, -13.5))
    eng.prepare_optimal_statistic(components=12)
    R = 70
    theta = eng.sample_theta(R)
    ref = eng.optimal_statistic(eng.generate(R, theta=theta))
    for chunk in (7, R):
        assert _same(eng.generate_os(R, theta=theta, chunk=chunk), ref)
    rows, th = eng.generate_sampled(R)
    assert torch.equal(eng.optimal_statistic(rows)["A2"], ref["A2"])


# ---------------------------------------------------------------- statistics --------------------------------------------------
def test_exact_null_is_unit_variance():
    """WN + ECORR + RN and no GW term in the model: the model is the data covariance, so every ORF's SNR has zero mean, unit variance"""
    eng = _engine(P=16, n0=120, gw=None, psr_seed=3)
    eng.prepare_optimal_statistic(components=14, gwb_auto=False)
    R = 4096
    snr = eng.generate_os(R, chunk=1024)["snr"].cpu().numpy()
    m, s = snr.mean(axis=0), snr.std(axis=0)
    print("null SNR mean", m, "std", s)
    assert np.all(np.abs(m) < 5 / np.sqrt(R)), m
    assert np.all((s > 0.94) & (s < 1.06)), s


def _signal_engine(no_correlations):
    from pta_replicator_amd.engine import ReplicaEngine
    eng = ReplicaEngine(_psrs(16, 200, 21, step=0, sessions=False, err_us=0.1), seed=8)   # 0.1 us white noise
    eng.td_warmup = False
    eng.set_white_noise(efac=1.0)
    eng.set_gwb(-14.0, 13. / 3., no_correlations=no_correlations)
    eng.prepare()
    eng.prepare_optimal_statistic(components=14)
    return eng


@pytest.mark.parametrize("no_correlations", [False, True])
def test_signal_recovery(no_correlations):
    eng = _signal_engine(no_correlations)
    R = 2048
    A2 = eng.generate_os(R)["A2"][:, 0].cpu().numpy()
    ratio, err = A2.mean() / 1e-28, A2.std() / np.sqrt(R)
    print(f"no_correlations={no_correlations}: mean A2_HD / A^2 = {ratio:.4f} +- {err / 1e-28:.4f}")
    if no_correlations:
        assert abs(A2.mean()) < 5 * err
    else:
        assert 0.7 < ratio < 1.3


# ---------------------------------------------------------------- refusals ----------------------------------------------------
def test_refusals():
    from pta_replicator_amd import device as dv
    eng = _engine(P=3, n0=60)
    rows = eng.generate(4)
    with pytest.raises(ValueError, match="not prepared"):
        eng.optimal_statistic(rows)
    with pytest.raises(ValueError, match="not prepared"):
        eng.generate_os(4)
    for bad in (0, 33, 2.5, True):
        with pytest.raises(ValueError, match="components"):
            eng.prepare_optimal_statistic(components=bad)
    with pytest.raises(ValueError, match="unknown ORF"):
        eng.prepare_optimal_statistic(orfs=("hd", "quadrupole"))
    eng.prepare_optimal_statistic(components=4)
    with pytest.raises(ValueError, match="rows must be"):
        eng.optimal_statistic(rows[:, :-1])
    with pytest.raises(ValueError, match="rows must be"):
        eng.optimal_statistic(rows[0])
    with pytest.raises(ValueError, match="stride"):
        eng.optimal_statistic(dv.empty((eng.n_toa, 4)).T)
    with pytest.raises(ValueError, match="float64 device"):
        eng.optimal_statistic(rows.cpu())
    with pytest.raises(ValueError, match="float64 device"):
        eng.optimal_statistic(rows.float())
    eng.set_gwb(-15.0, 13. / 3.)      # re-configured: the prepared OS is stale
    with pytest.raises(ValueError, match="re-configured"):
        eng.optimal_statistic(rows)


def test_refuses_singular_timing_model():
    from pta_replicator_amd.engine import ReplicaEngine
    from pta_replicator_amd.simulate import ArrayTOAs, SimulatedPulsar, make_ideal
    psrs = _psrs(2, 50, 1)
    p = SimulatedPulsar(toas=ArrayTOAs(np.array([54000.0, 55000.0]), 0.5, flags=[{"f": "A"}] * 2), name="J9999",
                        loc={"RAJ": 3.0, "DECJ": 10.0})
    make_ideal(p)
    eng = ReplicaEngine(psrs + [p], seed=1)
    eng.td_warmup = False
    eng.set_white_noise(efac=1.0)
    with pytest.raises(ValueError, match="singular"):
        eng.prepare_optimal_statistic(components=4)
    assert getattr(eng, "_os", None) is None
