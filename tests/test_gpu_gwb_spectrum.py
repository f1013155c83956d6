"""Per-realisation GWB spectrum in throughput mode (theta key gwb_log10_hc on an engine configured with a userSpec) on the MI355X:
against engines configured with the spectrum of realisation r, per signal, batching, prior draws against philox_ref, the amplitude
scaling, the matched optimal statistic and its per-frequency form against the host evaluation, and the refusals."""
import numpy as np
import pytest
import torch

from oracle import philox_ref
from pta_replicator_amd import optimal_statistic as ost
from test_gpu_hyper import P, RN_A, RN_G, _psrs, _rms_rel

pytestmark = pytest.mark.gpu

YR = 365.25 * 86400.0
_PSRS = []


def _spec(M, seed=1):
    """userSpec [M, 2], nodes given unsorted and inside the frequency grid of the array (2.6e-10 .. 7.7e-7 Hz), so that the bins below
    the first and above the last node are clamped; hc near a gamma = 13/3 power law of amplitude 10^-14.4"""
    rng = np.random.default_rng(seed)
    nf = np.array([1e-7, 2e-9]) if M == 2 else (10 ** np.linspace(-9, np.log10(2e-7), M))[rng.permutation(M)]
    assert not np.all(np.diff(nf) > 0)
    hc = 10 ** (-14.4 - (2. / 3.) * np.log10(nf * 3.16e7) + rng.uniform(-0.2, 0.2, M))
    return np.stack([nf, hc], axis=1)


def _engine(userSpec, seed=77, rn_A=RN_A, rn_g=RN_G, transform="auto", rng_fast=0, det=True, rn=True, wn=True):
    """the 6-pulsar ragged array of tests/test_gpu_hyper.py with a userSpec GWB"""
    from pta_replicator_amd.engine import ReplicaEngine
    if not _PSRS:
        _PSRS.extend(_psrs())
    eng = ReplicaEngine(_PSRS, seed=seed)
    eng.td_warmup = False
    fl = [["A", "B"]] * P
    if wn:
        eng.set_white_noise(efac=[np.array([1.1, 0.9])] * P, log10_equad=[np.array([-6.5, -6.8])] * P, flags=fl)
        eng.set_jitter(log10_ecorr=[np.array([-6.6, -6.9])] * P, flags=fl, coarsegrain=0.1)
    if rn:
        eng.set_red_noise(list(rn_A), list(rn_g), components=20)
    eng.set_gwb(-14.4, 13. / 3., userSpec=userSpec)
    if det:
        eng.add_delays([1e-7 * np.sin(m / 50.0) for m in eng.mjd])
    eng.gwb_transform = transform
    eng.rng_fast = rng_fast
    return eng


def _y(U, R, seed=5, width=0.7):
    """[R, M] node values around the configured column, columns in the order of U's rows"""
    return np.log10(U[:, 1])[None, :] + np.random.default_rng(seed).uniform(-width, width, (R, len(U)))


def _rn_theta(R, seed=5):
    rng = np.random.default_rng(seed)
    th = dict(rn_log10_A=rng.uniform(-15, -13, (R, P)), rn_gamma=rng.uniform(1, 5, (R, P)))
    th["rn_log10_A"][1, 3] = np.nan    # pulsar 3 as configured in realisation 1
    th["rn_gamma"][1, 3] = np.nan
    return th


def _fixed_rn(th, r):
    rn_A, rn_g = [], []
    for a in range(P):
        keep = RN_A[a] is None or np.isnan(th["rn_log10_A"][r, a])
        rn_A.append(RN_A[a] if keep else float(th["rn_log10_A"][r, a]))
        rn_g.append(RN_G[a] if keep else float(th["rn_gamma"][r, a]))
    return dict(rn_A=rn_A, rn_g=rn_g)


def _with_column(U, y_r):
    return np.stack([U[:, 0], 10.0 ** y_r], axis=1)


@pytest.mark.parametrize("transform,rng_fast,M,with_rn", [("auto", 0, 2, False), ("auto", 0, 7, False), ("gemm", 0, 2, False), ("gemm", 0, 7, False),
                                                          ("auto", 1, 2, False), ("auto", 1, 7, False), ("auto", 0, 7, True), ("gemm", 0, 2, True)])
def test_theta_equals_fixed_userspec_engine(transform, rng_fast, M, with_rn):
    """row r of generate(R, theta) against generate(1, r0 + r) of an engine prepared with userSpec = (freqs, 10**y_r): the two sides
    differ by the interpolation's rounding alone (1e-12, the bound of test_theta_equals_fixed_parameter_engine)"""
    R, r0 = 6, 1000
    U = _spec(M)
    th = {"gwb_log10_hc": _y(U, R)}
    if with_rn:
        th.update(_rn_theta(R))
    eng = _engine(U, transform=transform, rng_fast=rng_fast).prepare()
    assert eng.use_czt == (transform == "auto")
    f = eng.grid["f"]
    assert f[1] < U[:, 0].min() and f[-1] > U[:, 0].max()       # both clamps are in play
    out = eng.generate(R, r0=r0, theta=th).cpu().numpy()
    base = eng.generate(R, r0=r0).cpu().numpy()
    for r in range(R):
        cfg = _fixed_rn(th, r) if with_rn else {}
        ref = _engine(_with_column(U, th["gwb_log10_hc"][r]), transform=transform, rng_fast=rng_fast, **cfg).prepare().generate(1, r0=r0 + r)
        err = _rms_rel(out[r], ref.cpu().numpy()[0])
        print(f"{transform} rng_fast={rng_fast} M={M} rn={with_rn} r={r}: {err:.3e}")
        assert err < 1e-12, (r, err)
        assert _rms_rel(out[r], base[r]) > 1e-6   # theta did change the realisation


def test_theta_per_signal():
    R, r0, M = 6, 300, 7
    U = _spec(M, seed=2)
    y = _y(U, R, seed=9)
    eng = _engine(U).prepare()
    th = {"gwb_log10_hc": torch.as_tensor(y, device="cuda")}          # a device tensor, like the other keys
    sig = {k: v.cpu().numpy() for k, v in eng.generate_per_signal(R, r0=r0, theta=th).items()}
    fixed = {k: v.cpu().numpy() for k, v in _engine(U).prepare().generate_per_signal(R, r0=r0).items()}
    for k in ("wn", "ecorr", "det", "rn"):
        assert np.array_equal(sig[k], fixed[k]), k
    for r in range(R):
        ref = {k: v.cpu().numpy()[0] for k, v in _engine(_with_column(U, y[r])).prepare().generate_per_signal(1, r0=r0 + r).items()}
        for k in ("wn", "ecorr", "det"):
            assert np.array_equal(sig[k][r], ref[k]), (k, r)
        assert _rms_rel(sig["gwb"][r], ref["gwb"]) < 1e-12, r
        assert _rms_rel(sig["gwb"][r], fixed["gwb"][r]) > 1e-6
    parts = sig["rn"] + sig["gwb"] + sig["wn"] + sig["ecorr"] + sig["det"]
    assert _rms_rel(parts, sig["total"]) < 1e-13


@pytest.mark.parametrize("transform", ["auto", "gemm"])
def test_theta_equal_to_the_configured_column(transform):
    R = 8
    U = _spec(7)
    eng = _engine(U, transform=transform).prepare()
    a = eng.generate(R, r0=7, theta={"gwb_log10_hc": np.tile(np.log10(U[:, 1]), (R, 1))}).cpu().numpy()
    b = eng.generate(R, r0=7).cpu().numpy()
    for r in range(R):
        assert _rms_rel(a[r], b[r]) < 1e-13, r


def test_batches_do_not_change_a_realisation():
    R, r0, M = 40, 90, 7
    U = _spec(M)
    y = _y(U, R, seed=4)
    eng = _engine(U).prepare()
    rng = np.random.default_rng(8)
    th = {"gwb_log10_hc": y, "rn_log10_A": rng.uniform(-15, -13, (R, P)), "rn_gamma": rng.uniform(2, 5, (R, P))}
    assert eng.max_batch(hyper=True) > R
    whole = eng.generate(R, r0=r0, theta=th).clone()
    per_real = 8 * P * (eng.K + 2 * eng.plan.gw_npts) + 8 * eng.grid["Nf"]
    eng.workspace_bytes = 16 * per_real
    assert eng.max_batch(hyper=True) == 16
    cut = eng.generate(R, r0=r0, theta=th)
    assert torch.equal(cut, whole)
    one = eng.generate(1, r0=r0 + 23, theta={k: v[23:24] for k, v in th.items()})
    assert torch.equal(one[0], whole[23])


def test_sampled_spectrum_keyed_by_realisation():
    from pta_replicator_amd.engine import STREAM_HYPER, stream_id
    M, r0 = 7, 40
    U = _spec(M)
    eng = _engine(U).prepare()
    plan = eng.plan
    lo = np.log10(U[:, 1]) - np.linspace(0.2, 0.8, M)
    hi = np.log10(U[:, 1]) + np.linspace(0.5, 0.1, M)
    hi[4] = lo[4]                                       # a degenerate box returns lo exactly
    rn_box = np.array([[-15, -13.5], [-14, -13], [-16, -14], [-15, -14], [-14.5, -13], [-15, -13]])
    eng.set_hyper_prior(gwb_log10_hc=np.stack([lo, hi], axis=1), rn_log10_A=rn_box)
    a, tha = eng.generate_sampled(7, r0=r0)
    b, thb = eng.generate_sampled(1, r0=r0 + 3)
    assert eng.plan is plan
    assert torch.equal(a[3], b[0])
    assert set(tha) == {"gwb_log10_hc", "rn_log10_A"} and tha["gwb_log10_hc"].shape == (7, M)
    for k in tha:
        assert np.array_equal(tha[k][3].cpu().numpy(), thb[k][0].cpu().numpy(), equal_nan=True), k
    lab = tha["gwb_log10_hc"].cpu().numpy()
    for r in range(7):
        _, u2 = philox_ref.uniform_pairs(eng.seed, r0 + r, stream_id(STREAM_HYPER, 1), M)
        want = lo + (hi - lo) * u2
        assert np.all(np.abs(lab[r] - want) <= np.spacing(np.abs(want))), r
        assert np.all(lab[r] >= lo) and np.all(lab[r] <= hi) and lab[r, 4] == lo[4]
    # the labels of stream (7, 0) are those drawn without the new key
    eng.set_hyper_prior(rn_log10_A=rn_box)
    thc = eng.sample_theta(7, r0=r0)
    assert set(thc) == {"rn_log10_A"}
    assert np.array_equal(thc["rn_log10_A"].cpu().numpy(), tha["rn_log10_A"].cpu().numpy(), equal_nan=True)
    # the sampled realisations are generate(theta) with the returned labels
    again = eng.generate(7, r0=r0, theta={k: v.cpu().numpy() for k, v in tha.items()})
    assert torch.equal(again, a)
    # the spectrum alone
    eng.set_hyper_prior(gwb_log10_hc=(-15.5, -14.0))
    c, thd = eng.generate_sampled(5, r0=r0)
    assert set(thd) == {"gwb_log10_hc"} and torch.equal(eng.generate(5, r0=r0, theta=thd), c)
    d = thd["gwb_log10_hc"].cpu().numpy()
    assert np.all(d >= -15.5) and np.all(d < -14.0) and len(np.unique(d)) == d.size


def test_gwb_spectrum_scaling():
    """GWB only, every node shifted by c_r ~ U(-1, 1) over 4096 realisations: log(mean square) against c_r ln 10 has slope 2 (within
    0.05, the bound of test_gwb_amplitude_scaling at the same R)"""
    R = 4096
    U = _spec(7)
    eng = _engine(U, rn=False, wn=False, det=False)
    c = np.random.default_rng(12).uniform(-1, 1, R)
    out = eng.generate(R, theta={"gwb_log10_hc": np.log10(U[:, 1])[None, :] + c[:, None]})
    ms = torch.mean(out ** 2, dim=1).cpu().numpy()
    slope = np.polyfit(c * np.log(10.0), np.log(ms), 1)[0]
    print(f"slope {slope:.4f}")
    assert abs(slope - 2.0) < 0.05, slope


# ---------------------------------------------------------------- matched statistics ------------------------------------------
def _nrel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


def _bound(delta):
    """the calibrated bound of tests/test_gpu_os_matched.py: delta = the Cholesky form against the solve form on the host"""
    assert delta < 1e-8, f"the inputs are too ill-conditioned for this check: delta = {delta:.3e}"
    return max(1e-12, 8 * delta)


def _host_b(eng, R, theta, U):
    m = eng._os["matched"]
    mp = m["plan"]
    lA, g = theta["rn_log10_A"].copy(), theta["rn_gamma"].copy()
    lA[:, [a for a in range(P) if RN_A[a] is None]] = np.nan
    return ost.matched_prior(R, mp.s, np.stack(eng.rn_freqs), np.array([t.max() - t.min() for t in eng.tdb_s]), eng.rn_amp ** 2, lA, g, mp.nf, mp.T,
                             gw_log10_hc=theta["gwb_log10_hc"], gw_nodes=U[:, 0])


OS_KEYS = ("A2", "sigma", "snr", "rho", "sigma_pair")
SP_KEYS = ("a2", "sigma", "snr", "phi", "phi_sigma")


@pytest.fixture(scope="module")
def matched():
    """one engine with the matched statistic prepared, R = 9 realisations with their own spectrum and red noise"""
    R, M = 9, 7
    U = _spec(M, seed=3)
    eng = _engine(U).prepare()
    eng.prepare_optimal_statistic(components=5, matched=True, gwb_auto=-14.4)
    mp = eng._os["matched"]["plan"]
    fk = np.arange(1, 6) / mp.T
    assert U[:, 0].min() < fk[0] and U[:, 0].max() > fk[-1]
    rng = np.random.default_rng(21)
    theta = {"gwb_log10_hc": _y(U, R, seed=6), "rn_log10_A": rng.uniform(-15, -13.2, (R, P)), "rn_gamma": rng.uniform(2, 6, (R, P))}
    rows = eng.generate(R, r0=5, theta=theta).clone()
    return dict(eng=eng, U=U, R=R, theta=theta, rows=rows, mp=mp)


def test_matched_statistic_vs_host(matched):
    eng, U, R, theta, rows, mp = (matched[k] for k in ("eng", "U", "R", "theta", "rows", "mp"))
    b = _host_b(eng, R, theta, U)
    ref = ost.matched_from_rows(mp, rows.cpu().numpy(), b)
    alt = ost.matched_from_rows(mp, rows.cpu().numpy(), b, form="solve")
    res = eng.optimal_statistic(rows, pairs=True, theta=theta)
    delta = max(_nrel(alt[k], ref[k]) for k in OS_KEYS)
    errs = {k: _nrel(res[k].cpu().numpy(), ref[k]) for k in OS_KEYS}
    print(f"matched OS: delta {delta:.3e}, device", {k: f"{v:.3e}" for k, v in errs.items()})
    assert max(errs.values()) < _bound(delta), errs
    # the spectrum is in the weights: the prepared auto-term alone gives another statistic
    plain = eng.optimal_statistic(rows, theta={k: theta[k] for k in ("rn_log10_A", "rn_gamma")})
    assert _nrel(plain["A2"].cpu().numpy(), ref["A2"]) > 1e-6
    # per frequency
    for mode in ost.SPECTRUM_MODES:
        sref = ost.matched_spectrum_from_XZ(mp, ref["X"], ref["Z"], mode)
        salt = ost.matched_spectrum_from_XZ(mp, alt["X"], alt["Z"], mode, form="solve")
        sres = eng.optimal_statistic_spectrum(rows, theta=theta, mode=mode)
        delta = max(_nrel(salt[k], sref[k]) for k in SP_KEYS)
        errs = {k: _nrel(sres[k].cpu().numpy(), sref[k]) for k in SP_KEYS}
        print(f"matched spectrum {mode}: delta {delta:.3e}, device", {k: f"{v:.3e}" for k, v in errs.items()})
        assert max(errs.values()) < _bound(delta), (mode, errs)


def test_matched_statistic_power_law_nodes(matched):
    """nodes on the power law (A_r, gamma_r) give the statistic of theta = {gwb_log10_A, gwb_gamma}"""
    eng, U, R, theta, rows, mp = (matched[k] for k in ("eng", "U", "R", "theta", "rows", "mp"))
    rng = np.random.default_rng(2)
    lA, g = rng.uniform(-15, -14, R), rng.uniform(3, 5.5, R)
    y = lA[:, None] + 0.5 * (3.0 - g[:, None]) * np.log10(U[:, 0] * YR)[None, :]
    rn = {k: theta[k] for k in ("rn_log10_A", "rn_gamma")}
    spec = eng.optimal_statistic(rows, pairs=True, theta=dict(rn, gwb_log10_hc=y))
    pl = eng.optimal_statistic(rows, pairs=True, theta=dict(rn, gwb_log10_A=lA, gwb_gamma=g))
    b = _host_b(eng, R, dict(rn, gwb_log10_hc=y), U)
    ref = ost.matched_from_rows(mp, rows.cpu().numpy(), b)
    alt = ost.matched_from_rows(mp, rows.cpu().numpy(), b, form="solve")
    delta = max(_nrel(alt[k], ref[k]) for k in OS_KEYS)
    errs = {k: _nrel(spec[k].cpu().numpy(), pl[k].cpu().numpy()) for k in OS_KEYS}
    print(f"power-law nodes: delta {delta:.3e}, spectrum against (A, gamma)", {k: f"{v:.3e}" for k, v in errs.items()})
    assert max(errs.values()) < _bound(delta), errs
    sp = eng.optimal_statistic_spectrum(rows, theta=dict(rn, gwb_log10_hc=y))
    sq = eng.optimal_statistic_spectrum(rows, theta=dict(rn, gwb_log10_A=lA, gwb_gamma=g))
    errs = {k: _nrel(sp[k].cpu().numpy(), sq[k].cpu().numpy()) for k in SP_KEYS}
    assert max(errs.values()) < _bound(delta), errs


def test_generate_os_matched_bit_identical(matched):
    eng, R, theta = matched["eng"], matched["R"], matched["theta"]
    ref = eng.optimal_statistic(eng.generate(R, r0=5, theta=theta), pairs=True, theta=theta)
    sref = eng.optimal_statistic_spectrum(eng.generate(R, r0=5, theta=theta), theta=theta)
    assert bool(torch.isfinite(ref["snr"]).all())
    for chunk in (4, R):
        res = eng.generate_os(R, r0=5, theta=theta, matched=True, chunk=chunk, pairs=True)
        assert all(torch.equal(res[k], ref[k]) for k in OS_KEYS), chunk
        sres = eng.generate_os_spectrum(R, r0=5, theta=theta, matched=True, chunk=chunk)
        assert all(torch.equal(sres[k], sref[k]) for k in SP_KEYS), chunk


def test_generation_step_of_the_other_statistics():
    """generate_os (fixed noise), generate_lnl and generate_f_statistic take the key through their generation step: the statistic of
    generate(R, theta), bit for bit, in chunks that do not divide R"""
    R, r0, M = 12, 4, 7
    U = _spec(M)
    eng = _engine(U).prepare()
    th = {"gwb_log10_hc": _y(U, R, seed=3)}
    rows = eng.generate(R, r0=r0, theta=th).clone()
    assert not torch.equal(rows, eng.generate(R, r0=r0))
    eng.prepare_optimal_statistic(components=5)
    assert torch.equal(eng.generate_os(R, r0=r0, theta=th, chunk=5)["A2"], eng.optimal_statistic(rows)["A2"])
    assert torch.equal(eng.generate_os_spectrum(R, r0=r0, theta=th, chunk=5)["a2"], eng.optimal_statistic_spectrum(rows)["a2"])
    eng.prepare_likelihood(components=5)
    grid, _ = eng.theta_grid(gwb_log10_A=np.linspace(-15.0, -14.0, 3))
    assert torch.equal(eng.generate_lnl(R, grid, r0=r0, theta=th, chunk=5)["lnl"], eng.log_likelihood(rows, grid)["lnl"])
    eng.prepare_f_statistic(np.array([5.1e-9, 1.21e-8]), sky=(np.array([-0.71, 0.44]), np.array([0.3, 4.4])))
    ref = eng.f_statistic(rows)
    res = eng.generate_f_statistic(R, r0=r0, theta=th, chunk=5)
    assert all(torch.equal(res[k], ref[k]) for k in ref if isinstance(ref[k], torch.Tensor))


def test_refusals_on_a_prepared_engine():
    R, M = 2, 7
    U = _spec(M)
    ok = np.tile(np.log10(U[:, 1]), (R, 1))
    eng = _engine(U).prepare()
    with pytest.raises(ValueError, match="TD mode"):
        eng.generate_td(R, theta={"gwb_log10_hc": ok})
    with pytest.raises(ValueError, match="shape"):
        eng.generate(R, theta={"gwb_log10_hc": torch.zeros((R, M + 1), dtype=torch.float64, device="cuda")})
    with pytest.raises(ValueError, match="non-finite"):
        eng.generate(R, theta={"gwb_log10_hc": torch.as_tensor(np.where(np.eye(R, M) > 0, np.nan, ok), device="cuda")})
    with pytest.raises(ValueError, match="userSpec"):
        eng.generate(R, theta={"gwb_log10_hc": ok, "gwb_log10_A": np.full(R, -14.0)})
    # without the GW auto-term the statistic has no column for the key to weight
    eng.prepare_optimal_statistic(components=3, matched=True, gwb_auto=False)
    with pytest.raises(ValueError, match="gwb_auto"):
        eng.optimal_statistic(eng.generate(R), theta={"gwb_log10_hc": ok})
    eng.gwb_mode = "grid"
    with pytest.raises(ValueError, match="grid"):
        eng.generate(R, theta={"gwb_log10_hc": ok})
    from test_gpu_hyper import _engine as _power_law_engine
    with pytest.raises(ValueError, match="userSpec"):
        _power_law_engine().prepare().generate(R, theta={"gwb_log10_hc": ok})
