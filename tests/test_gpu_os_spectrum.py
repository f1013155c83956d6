"""Per-frequency optimal statistic on the MI355X: pta_os_pairs_pf / pta_os_matched_pairs_pf against NumPy, the engine against the
host evaluation (optimal_statistic.spectrum_from_rows, matched_spectrum_from_XZ), the sum rule against the broadband statistic,
bit-identity of generate_os_spectrum across chunks / offsets / modes, the calibration of the exact null, recovery of a power-law and
of a turnover spectrum, and the refusals.

Calibrated bound of the matched kernel: max(1e-12, 8 delta), delta = the disagreement of two independent CPU fp64 evaluations of the
same quantity (spectrum_solve through the scaled Cholesky factor against np.linalg.solve / inv), the rule of
test_gpu_os_matched.test_matched_solve_vs_numpy."""
import ctypes
import types

import numpy as np
import pytest
import torch

from pta_replicator_amd import optimal_statistic as ost
from pta_replicator_amd import red_noise as rn
from test_gpu_os import _engine, _psrs, _signal_engine
from test_gpu_os_matched import _engine as _engine_matched, _host, _pack

pytestmark = pytest.mark.gpu

MODES = ost.SPECTRUM_MODES


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(np.asarray(b))))


def _nrel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


def _bound(delta):
    assert delta < 1e-8, f"the inputs are too ill-conditioned for this check: delta = {delta:.3e}"
    return max(1e-12, 8 * delta)


def _np(x):
    return x.cpu().numpy()


# ---------------------------------------------------------------- kernels ---------------------------------------------------
@pytest.mark.parametrize("C", [2, 28, 64])
@pytest.mark.parametrize("P", [2, 7])
def test_pairs_pf_vs_numpy(P, C):
    from pta_replicator_amd import _lib, device as dv
    nf = C // 2
    ia, ib = np.triu_indices(P, 1)
    npairs = len(ia)
    pa, pb = dv.i32(ia), dv.i32(ib)
    for R in (1, 17, 300):
        for n_orf in (1, 8):
            rng = np.random.default_rng(P * 100000 + C * 1000 + R * 10 + n_orf)
            Y = rng.normal(size=(R, P, C))
            G = rng.normal(size=(n_orf, npairs))
            ops = (rng.normal(size=(n_orf, nf, nf)), rng.uniform(0.5, 2.0, (n_orf, nf)))
            b = np.einsum("op,rpk->rok", G, ost.pair_numerators(Y, ia, ib))
            refs = (np.einsum("okj,roj->rok", ops[0], b), b * ops[1][None])
            dY, dG = dv.f64(Y), dv.f64(G)
            for mode in (0, 1):
                a2 = dv.zeros((R, n_orf * nf + 1))
                dop = dv.f64(ops[mode])
                _lib.call("pta_os_pairs_pf", dv.ptr(dY), P * C, P, C, R, dv.ptr(pa), dv.ptr(pb), npairs, dv.ptr(dG), n_orf, dv.ptr(dop), mode,
                          dv.ptr(a2), n_orf * nf + 1, dv.stream_ptr())
                got = _np(a2)
                err = _rel(got[:, :-1].reshape(R, n_orf, nf), refs[mode])
                assert err < 1e-12, (R, n_orf, mode, err)
                assert np.all(got[:, -1] == 0)                 # nothing written past n_orf * n_f
                if R >= 17:   # realisation 13 alone gives the same bits
                    one = dv.zeros((1, n_orf * nf))
                    _lib.call("pta_os_pairs_pf", ctypes.c_void_p(dY.data_ptr() + 8 * 13 * P * C), P * C, P, C, 1, dv.ptr(pa), dv.ptr(pb), npairs,
                              dv.ptr(dG), n_orf, dv.ptr(dop), mode, dv.ptr(one), n_orf * nf, dv.stream_ptr())
                    assert torch.equal(one[0], a2[13, :-1])


def test_pairs_pf_at_the_lds_limit():
    """P * C * 8 = 64 KiB of Y exactly: with b behind it the workgroup asks for more than 64 KiB of dynamic LDS"""
    from pta_replicator_amd import _lib, device as dv
    P, C, R, n_orf = 128, 64, 3, 8
    nf = C // 2
    ia, ib = np.triu_indices(P, 1)
    rng = np.random.default_rng(128)
    Y, G = rng.normal(size=(R, P, C)), rng.normal(size=(n_orf, len(ia)))
    ops = (rng.normal(size=(n_orf, nf, nf)), rng.uniform(0.5, 2.0, (n_orf, nf)))
    b = np.einsum("op,rpk->rok", G, ost.pair_numerators(Y, ia, ib))
    refs = (np.einsum("okj,roj->rok", ops[0], b), b * ops[1][None])
    dY, dG, pa, pb = dv.f64(Y), dv.f64(G), dv.i32(ia), dv.i32(ib)
    for mode in (0, 1):
        a2, dop = dv.zeros((R, n_orf * nf)), dv.f64(ops[mode])
        _lib.call("pta_os_pairs_pf", dv.ptr(dY), P * C, P, C, R, dv.ptr(pa), dv.ptr(pb), len(ia), dv.ptr(dG), n_orf, dv.ptr(dop), mode, dv.ptr(a2),
                  n_orf * nf, dv.stream_ptr())
        assert _rel(_np(a2).reshape(R, n_orf, nf), refs[mode]) < 1e-12


def _matched_inputs(P, C, R, n_orf, seed, zero_row=None):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(R, P, C))
    B = rng.normal(size=(R, P, C, C))
    Z = B @ np.swapaxes(B, -1, -2) / C               # positive definite
    ia, ib = np.triu_indices(P, 1)
    G = rng.normal(size=(n_orf, len(ia)))
    if zero_row is not None:
        G[zero_row] = 0.0
    return X, Z, types.SimpleNamespace(pair_a=ia.astype(np.int32), pair_b=ib.astype(np.int32), G=G)


def _matched_device(X, Z, plan, mode, fisher):
    from pta_replicator_amd import _lib, device as dv
    R, P, C = X.shape
    nf, n_orf, npairs = C // 2, plan.G.shape[0], len(plan.pair_a)
    dX, dZ, dG, dG2 = dv.f64(X), dv.f64(_pack(Z)), dv.f64(plan.G), dv.f64(plan.G ** 2)
    pa, pb = dv.i32(plan.pair_a), dv.i32(plan.pair_b)
    a2, sg = dv.zeros((R, n_orf * nf + 1)), dv.zeros((R, n_orf * nf))
    fi = dv.zeros((R, n_orf * nf * nf)) if fisher else None
    _lib.call("pta_os_matched_pairs_pf", dv.ptr(dX), dv.ptr(dZ), P, C, R, dv.ptr(pa), dv.ptr(pb), npairs, dv.ptr(dG), dv.ptr(dG2), n_orf,
              MODES.index(mode), dv.ptr(a2), n_orf * nf + 1, dv.ptr(sg), n_orf * nf, dv.ptr(fi), n_orf * nf * nf if fisher else 0, dv.stream_ptr())
    assert bool((a2[:, -1] == 0).all())                # nothing written past n_orf * n_f
    out = dict(a2=a2[:, :-1].reshape(R, n_orf, nf), sigma=sg.reshape(R, n_orf, nf), fisher=None if fi is None else fi.reshape(R, n_orf, nf, nf))
    if R >= 17:   # realisation 13 alone gives the same bits
        nz = C * (C + 1) // 2
        a2b, sgb = dv.zeros((1, n_orf * nf)), dv.zeros((1, n_orf * nf))
        _lib.call("pta_os_matched_pairs_pf", ctypes.c_void_p(dX.data_ptr() + 8 * 13 * P * C), ctypes.c_void_p(dZ.data_ptr() + 8 * 13 * P * nz), P, C, 1,
                  dv.ptr(pa), dv.ptr(pb), npairs, dv.ptr(dG), dv.ptr(dG2), n_orf, MODES.index(mode), dv.ptr(a2b), n_orf * nf, dv.ptr(sgb),
                  n_orf * nf, None, 0, dv.stream_ptr())
        assert _np(a2b[0]).tobytes() == _np(a2[13, :-1]).tobytes() and _np(sgb[0]).tobytes() == _np(sg[13]).tobytes()   # NaN included
    return out


@pytest.mark.parametrize("C", [2, 6, 28, 64])
@pytest.mark.parametrize("P", [2, 5, 9])
def test_matched_pairs_pf_vs_numpy(P, C):
    for R in (1, 17):
        for n_orf in (1, 3, 8):
            X, Z, plan = _matched_inputs(P, C, R, n_orf, P * 100000 + C * 1000 + R * 10 + n_orf)
            for mode in MODES:
                ref = ost.matched_spectrum_from_XZ(plan, X, Z, mode)
                alt = ost.matched_spectrum_from_XZ(plan, X, Z, mode, form="solve")
                delta = max(_nrel(alt[k], ref[k]) for k in ("a2", "sigma"))
                for fisher in (False, True):
                    got = _matched_device(X, Z, plan, mode, fisher)
                    errs = {k: _nrel(_np(got[k]), ref[k]) for k in ("a2", "sigma")}
                    if fisher:
                        assert _nrel(_np(got["fisher"]), ref["fisher"]) < 1e-12
                    assert max(errs.values()) < _bound(delta), (R, n_orf, mode, fisher, delta, errs)
            print(f"P={P} C={C} R={R} n_orf={n_orf}: delta {delta:.3e}, device", {k: f"{v:.3e}" for k, v in errs.items()})


@pytest.mark.parametrize("mode", MODES)
def test_matched_pairs_pf_zero_orf_row_is_nan(mode):
    X, Z, plan = _matched_inputs(5, 28, 17, 3, 99, zero_row=1)
    got = _matched_device(X, Z, plan, mode, True)
    ref = ost.matched_spectrum_from_XZ(plan, X, Z, mode)
    a2, sg = _np(got["a2"]), _np(got["sigma"])
    assert np.all(np.isnan(a2[:, 1])) and np.all(np.isnan(sg[:, 1])) and np.all(np.isnan(ref["a2"][:, 1]))
    assert np.all(_np(got["fisher"])[:, 1] == 0)
    keep = [0, 2]
    assert _nrel(a2[:, keep], ref["a2"][:, keep]) < 1e-10 and _nrel(sg[:, keep], ref["sigma"][:, keep]) < 1e-10


def test_kernel_refusals():
    from pta_replicator_amd import _lib, device as dv
    x = dv.zeros((8,))
    i = dv.i32(np.zeros(2))
    for P, C, n_orf, mode in ((2, 3, 1, 0), (2, 66, 1, 0), (2, 0, 1, 0), (2, 4, 9, 0), (2, 4, 1, 2), (1, 4, 1, 0), (200, 64, 1, 0)):
        with pytest.raises(_lib.PtaError, match="pta_os_pairs_pf"):
            _lib.call("pta_os_pairs_pf", dv.ptr(x), P * C, P, C, 1, dv.ptr(i), dv.ptr(i), 1, dv.ptr(x), n_orf, dv.ptr(x), mode, dv.ptr(x), 1024,
                      dv.stream_ptr())
        if P == 200:
            continue
        with pytest.raises(_lib.PtaError, match="pta_os_matched_pairs_pf"):
            _lib.call("pta_os_matched_pairs_pf", dv.ptr(x), dv.ptr(x), P, C, 1, dv.ptr(i), dv.ptr(i), 1, dv.ptr(x), dv.ptr(x), n_orf, mode, dv.ptr(x),
                      1024, dv.ptr(x), 1024, None, 0, dv.stream_ptr())
    with pytest.raises(_lib.PtaError, match="leading dimension"):
        _lib.call("pta_os_matched_pairs_pf", dv.ptr(x), dv.ptr(x), 2, 4, 1, dv.ptr(i), dv.ptr(i), 1, dv.ptr(x), dv.ptr(x), 1, 0, dv.ptr(x), 1, dv.ptr(x),
                  2, None, 0, dv.stream_ptr())
    with pytest.raises(_lib.PtaError, match="NULL"):
        _lib.call("pta_os_pairs_pf", dv.ptr(x), 8, 2, 4, 1, dv.ptr(i), dv.ptr(i), 1, dv.ptr(x), 1, None, 0, dv.ptr(x), 2, dv.stream_ptr())


# ---------------------------------------------------------------- engines -----------------------------------------------------
KEYS = ("a2", "sigma", "snr", "phi", "phi_sigma")


def _check_shapes(res, R, n_orf, nf, matched, fisher):
    lead = (R,) if matched else ()
    assert res["a2"].shape == res["snr"].shape == res["phi"].shape == res["phi_sigma"].shape == (R, n_orf, nf)
    assert res["sigma"].shape == lead + (n_orf, nf)
    assert res["freqs"].shape == (nf,) and len(res["names"]) == n_orf
    assert ("fisher" in res) == fisher
    if fisher:
        assert res["fisher"].shape == lead + (n_orf, nf, nf)


@pytest.mark.parametrize("mode", MODES)
def test_engine_spectrum_vs_host_fixed(mode):
    eng = _engine()
    nf = 10
    eng.prepare_optimal_statistic(components=nf, timing_model="astrometric")
    rows = eng.generate(24, r0=5)
    res = eng.optimal_statistic_spectrum(rows, mode=mode, fisher=True)
    _check_shapes(res, 24, 3, nf, False, True)
    plan = eng._os["plan"]
    ref = ost.spectrum_from_rows(plan, _np(rows), mode)
    errs = {k: _rel(_np(res[k]), ref[k]) for k in KEYS + ("fisher", "freqs")}
    print(mode, errs)
    assert max(errs.values()) < 1e-10, errs
    assert res["names"] == ["hd", "monopole", "dipole"]
    # sum rule: the Fisher-weighted mean of the bins is the broadband statistic
    F = res["fisher"]
    A2 = torch.einsum("okj,roj->ro", F, eng.optimal_statistic_spectrum(rows)["a2"]) / F.sum(dim=(1, 2))
    assert _rel(_np(A2), _np(eng.optimal_statistic(rows)["A2"])) < 1e-10
    assert "fisher" not in eng.optimal_statistic_spectrum(rows, mode=mode)


@pytest.mark.parametrize("mode", MODES)
def test_engine_spectrum_vs_host_matched(mode):
    """every pulsar with red noise, then the array whose pulsar 2 has none, with NaN rows ("as configured") and omitted keys"""
    rng = np.random.default_rng(3)
    for eng in (_engine(), _engine_matched()):
        nf, R, P = 10, 24, eng.P
        eng.prepare_optimal_statistic(components=nf, matched=True)
        lA = rng.uniform(-15.0, -13.2, (R, P))
        lA[::5] = np.nan
        lA[1::4, 3] = np.nan
        g = np.where(np.isnan(lA), np.nan, rng.uniform(2, 6, (R, P)))
        thetas = {"rn+gw amplitude": {"rn_log10_A": lA, "rn_gamma": g, "gwb_log10_A": rng.uniform(-15, -14, R)},
                  "gw only, own index": {"gwb_log10_A": torch.as_tensor(rng.uniform(-15, -14, R)), "gwb_gamma": rng.uniform(3, 5.5, R)},
                  "rn index only": {"rn_gamma": rng.uniform(2, 5, (R, P))}}
        mp = eng._os["matched"]["plan"]
        for what, theta in thetas.items():
            rows = eng.generate(R, r0=5, theta=theta)
            res = eng.optimal_statistic_spectrum(rows, theta=theta, mode=mode, fisher=True)
            _check_shapes(res, R, 3, nf, True, True)
            h = _host(eng, rows, theta)
            ref = ost.matched_spectrum_from_XZ(mp, h["X"], h["Z"], mode)
            errs = {k: _nrel(_np(res[k]), ref[k]) for k in KEYS + ("fisher", "freqs")}
            print(mode, what, {k: f"{v:.2e}" for k, v in errs.items()})
            assert max(errs.values()) < 1e-10, (what, errs)
            # sum rule against the broadband matched statistic of the same theta
            full = res if mode == "full" else eng.optimal_statistic_spectrum(rows, theta=theta, fisher=True)
            F = full["fisher"]
            A2 = torch.einsum("rokj,roj->ro", F, full["a2"]) / F.sum(dim=(2, 3))
            assert _rel(_np(A2), _np(eng.optimal_statistic(rows, theta=theta)["A2"])) < 1e-10


# ---------------------------------------------------------------- bit-identity ------------------------------------------------
def _same(a, b, sl=None):
    def cut(x):
        return x if sl is None or x.dim() < 3 else x[sl]
    return torch.equal(a["a2"], cut(b["a2"])) and torch.equal(a["sigma"], cut(b["sigma"]))


def test_generate_os_spectrum_bit_identical():
    eng = _engine()
    eng.set_hyper_prior(gwb_log10_A=(-15.0, -14.0), gwb_gamma=(3.5, 5.0), rn_log10_A=(-14.8, -13.3), rn_gamma=(2.0, 5.0))
    eng.prepare_optimal_statistic(components=14, matched=True)
    R = 300
    for mode in MODES:
        ref = eng.optimal_statistic_spectrum(eng.generate(R), mode=mode)
        for chunk in (7, 256, R):
            assert _same(eng.generate_os_spectrum(R, chunk=chunk, mode=mode), ref), (mode, chunk)
        assert _same(eng.generate_os_spectrum(50, r0=123, chunk=16, mode=mode), ref, slice(123, 173))
        assert torch.equal(eng.optimal_statistic_spectrum(eng.generate(9, r0=200), mode=mode)["a2"], ref["a2"][200:209])
    theta = eng.sample_theta(R)
    # theta for the generator alone: the fixed-noise statistic of realisations drawn under theta
    ref = eng.optimal_statistic_spectrum(eng.generate(R, theta=theta))
    for chunk in (7, 256, R):
        assert _same(eng.generate_os_spectrum(R, theta=theta, chunk=chunk), ref), chunk
    # theta + matched=True: F, and with it sigma, per realisation
    for mode in MODES:
        ref = eng.optimal_statistic_spectrum(eng.generate(R, theta=theta), theta=theta, mode=mode, fisher=True)
        assert ref["sigma"].shape == (R, 3, 14) and bool(torch.isfinite(ref["snr"]).all())
        for chunk in (7, 256, R):
            got = eng.generate_os_spectrum(R, theta=theta, matched=True, chunk=chunk, mode=mode, fisher=True)
            assert _same(got, ref) and torch.equal(got["fisher"], ref["fisher"]), (mode, chunk)
        sub = eng.generate_os_spectrum(50, r0=123, theta={k: v[123:173] for k, v in theta.items()}, matched=True, chunk=16, mode=mode)
        assert _same(sub, ref, slice(123, 173))


def test_generate_os_spectrum_td_bit_identical():
    eng = _engine(gw=None)
    eng.prepare_td()
    eng.prepare_optimal_statistic(components=6)
    R = 300
    ref = eng.optimal_statistic_spectrum(eng.generate_td(R))
    for chunk in (7, 256, R):
        assert _same(eng.generate_os_spectrum(R, td=True, chunk=chunk), ref), chunk
    assert _same(eng.generate_os_spectrum(50, r0=123, td=True, chunk=16), ref, slice(123, 173))


# ---------------------------------------------------------------- statistics --------------------------------------------------
def test_exact_null_is_unit_variance_per_bin():
    """the engine of test_gpu_os.test_exact_null_is_unit_variance: the model is the data covariance, so the SNR of every (ORF, bin)
    has zero mean and unit variance (that test's bounds)"""
    eng = _engine(P=16, n0=120, gw=None, psr_seed=3)
    eng.prepare_optimal_statistic(components=14, gwb_auto=False)
    R = 4096
    snr = _np(eng.generate_os_spectrum(R, chunk=1024)["snr"])
    m, s = snr.mean(axis=0), snr.std(axis=0)
    print("null SNR mean\n", m, "\nstd\n", s)
    assert np.all(np.abs(m) < 5 / np.sqrt(R)), m
    assert np.all((s > 0.94) & (s < 1.06)), s


def _phi_injected(eng, nf):
    """variance of one sin / cos coefficient of the configured GWB at the OS frequencies: hc(f)^2 / (12 pi^2 f^3 T)"""
    c = eng._gw
    T = eng._os["plan"].T
    f = np.arange(1, nf + 1) / T
    hc = rn.gwb_spectrum_hcf(f, c["A"], c["g"], c["turnover"], c["f0"], c["beta"], c["power"])
    return hc ** 2 / (12 * np.pi ** 2 * f ** 3 * T)


def test_power_law_recovery_per_bin():
    eng = _signal_engine(False)
    nf, R = 10, 2048
    eng.prepare_optimal_statistic(components=nf)
    res = eng.generate_os_spectrum(R)
    phi = _np(res["phi"])[:, 0]
    ratio, err = phi.mean(axis=0) / _phi_injected(eng, nf), phi.std(axis=0) / np.sqrt(R) / _phi_injected(eng, nf)
    print("power law: mean(phi_k) / phi_inj(f_k)", ratio, "+-", err)
    assert np.all((ratio > 0.7) & (ratio < 1.3)), ratio


def test_turnover_recovery_per_bin():
    """A turnover at f0 = 1e-8 under the power-law template: the broadband statistic reports a fraction of A^2, the per-frequency
    statistic follows the injected spectrum.  Bins 1 and 2 take power from below 1 / T (measured on the CPU: 1.80 +- 0.13 and
    1.20 +- 0.06 at R = 600); they are printed, not asserted."""
    from pta_replicator_amd.engine import ReplicaEngine
    eng = ReplicaEngine(_psrs(16, 200, 21, step=0, sessions=False, err_us=0.1), seed=8)
    eng.td_warmup = False
    eng.set_white_noise(efac=1.0)
    eng.set_gwb(-14.0, 13. / 3., turnover=True, f0=1e-8)
    eng.prepare()
    nf, R = 10, 2048
    eng.prepare_optimal_statistic(components=nf)
    phi = _np(eng.generate_os_spectrum(R)["phi"])[:, 0]
    inj = _phi_injected(eng, nf)
    ratio, err = phi.mean(axis=0) / inj, phi.std(axis=0) / np.sqrt(R) / inj
    A2 = _np(eng.generate_os(R)["A2"])[:, 0]
    print("turnover: mean(phi_k) / phi_inj(f_k)", ratio, "+-", err, f"(bins 1, 2 not asserted: {ratio[0]:.3f}, {ratio[1]:.3f})")
    print(f"turnover: broadband mean A2_HD / A^2 = {A2.mean() / 1e-28:.4f} +- {A2.std() / np.sqrt(R) / 1e-28:.4f}")
    assert np.all((ratio[2:] > 0.7) & (ratio[2:] < 1.3)), ratio
    assert A2.mean() / 1e-28 < 0.5


# ---------------------------------------------------------------- refusals ----------------------------------------------------
def test_refusals():
    eng = _engine_matched(P=3)
    R = 4
    rows = eng.generate(R)
    theta = {"rn_log10_A": np.full((R, 3), -14.0), "rn_gamma": np.full((R, 3), 3.0)}
    with pytest.raises(ValueError, match="not prepared"):
        eng.optimal_statistic_spectrum(rows)
    with pytest.raises(ValueError, match="not prepared"):
        eng.generate_os_spectrum(R)
    eng.prepare_optimal_statistic(components=4)
    for bad in ("wide", None, 0):
        with pytest.raises(ValueError, match="mode"):
            eng.optimal_statistic_spectrum(rows, mode=bad)
        with pytest.raises(ValueError, match="mode"):
            eng.generate_os_spectrum(R, mode=bad)
    with pytest.raises(ValueError, match="matched=True"):
        eng.optimal_statistic_spectrum(rows, theta=theta)
    with pytest.raises(ValueError, match="matched=True"):
        eng.generate_os_spectrum(R, theta=theta, matched=True)
    with pytest.raises(ValueError, match="rows must be"):
        eng.optimal_statistic_spectrum(rows[:, :-1])
    with pytest.raises(ValueError, match="float64 device"):
        eng.optimal_statistic_spectrum(rows.cpu())
    assert "spectrum" not in eng._os                    # nothing was prepared or launched by a refused call
    eng.prepare_optimal_statistic(components=4, gwb_auto=False, matched=True)
    with pytest.raises(ValueError, match="needs theta"):
        eng.generate_os_spectrum(R, matched=True)
    with pytest.raises(ValueError, match="without the GWB auto-term"):
        eng.optimal_statistic_spectrum(rows, theta={"gwb_log10_A": np.full(R, -14.0)})
    with pytest.raises(ValueError, match="shape"):
        eng.generate_os_spectrum(R, theta={"rn_log10_A": np.zeros((R + 1, 3))}, matched=True)
    eng.set_gwb(-15.0, 13. / 3.)      # re-configured: the prepared OS is stale
    with pytest.raises(ValueError, match="re-configured"):
        eng.optimal_statistic_spectrum(rows)
    with pytest.raises(ValueError, match="re-configured"):
        eng.generate_os_spectrum(R)
