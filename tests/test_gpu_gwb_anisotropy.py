"""Anisotropic GWB per realisation on the MI355X: pta_gwb_orf_factor and pta_gwb_mix_batched against NumPy, theta's gwb_clm end to
end (exact against the host factors, bit-identical across batches), its errors and sampled labels, and the joint spherical-harmonic
fit of the optimal statistic (against the host weights, and recovering an injected dipole).

The ORF reference is oracle.pta_oracle.correlated_basis + numpy.linalg.cholesky on the host; tests/golden/aniso_basis_p81_l4.npz holds
the oracle's basis of 81 positions up to l = 4 (scripts/gen_aniso_basis_golden.py; the basis of the first P positions up to lmax is a
sub-array).  Every test asserts that numpy.linalg.cholesky succeeds on the rows it calls good and raises on those it calls bad."""
import ctypes

import numpy as np
import pytest
import torch

import launch_cases as lc
from helpers import load
from oracle import pta_oracle as po

pytestmark = pytest.mark.gpu
C00 = np.sqrt(4.0 * np.pi)


def _host_factors(basis, clm, good):
    """[R, P, P] numpy.linalg.cholesky(2 sum_k clm[r, k] basis[k]) of the rows flagged good (zeros elsewhere); asserts the flags"""
    out = np.zeros((len(clm),) + basis.shape[1:])
    for r, c in enumerate(clm):
        orf = 2.0 * np.einsum("k,kab->ab", c, basis)
        if good[r]:
            out[r] = np.linalg.cholesky(orf)
        else:
            with pytest.raises(np.linalg.LinAlgError):
                np.linalg.cholesky(orf)
    return out


def _good_rows(rng, R, n):
    """c_00 = sqrt(4 pi), |c_lm| <= 1 for l >= 1: positive definite ORFs with condition numbers below 50 for these arrays"""
    return np.concatenate([np.full((R, 1), C00), rng.uniform(-1.0, 1.0, (R, n - 1))], axis=1)


def _bad_row(n):
    c = np.zeros(n)
    c[0] = C00
    if n > 1:
        c[2] = 8.0      # c_10 = 8: the power is negative over almost half the sky
    else:
        c[0] = -1.0
    return c


@pytest.fixture(scope="module")
def golden_basis():
    z = load("aniso_basis_p81_l4.npz")
    P = len(z["locs"])
    iu = np.triu_indices(P)
    B = np.zeros((z["tri"].shape[0], P, P))
    B[:, iu[0], iu[1]] = z["tri"]
    return B + np.triu(B, 1).transpose(0, 2, 1)


# ---------------------------------------------------------------- kernels ---------------------------------------------------
def _factor(basis, clm, ld):
    from pta_replicator_amd import _lib, device as dv
    n, P = basis.shape[0], basis.shape[1]
    R = len(clm)
    pad = np.full((R, ld), np.nan)
    pad[:, :n] = clm
    d_b, d_c = dv.f64(basis), dv.f64(pad)
    M = dv.f64(np.full((R, P, P), 7.0))
    info = dv.i32(np.full(R, -5))
    _lib.call("pta_gwb_orf_factor", dv.ptr(d_b), n, P, dv.ptr(d_c), ld, R, dv.ptr(M), dv.ptr(info), dv.stream_ptr())
    return M.cpu().numpy(), info.cpu().numpy()


@pytest.mark.parametrize("lmax", [0, 1, 4])
@pytest.mark.parametrize("P", [3, 16, 17, 68, 80, 81])      # 80 / 81: the last size of the LDS kernel and the first of the composed path
def test_orf_factor_vs_numpy(golden_basis, P, lmax):
    n, R = (lmax + 1) ** 2, 5
    basis = np.ascontiguousarray(golden_basis[:n, :P, :P])
    rng = np.random.default_rng(100 * P + lmax)
    clm = _good_rows(rng, R, n)
    ref = _host_factors(basis, clm, [True] * R)
    M, info = _factor(basis, clm, n + 3)
    assert np.all(info == 0), info
    err = max(np.max(np.abs(M[r] - ref[r])) / np.max(np.abs(ref[r])) for r in range(R))
    print(f"P={P} lmax={lmax}: factor vs numpy {err:.2e}")
    assert err < 1e-10
    iu = np.triu_indices(P, 1)
    assert np.all(M[:, iu[0], iu[1]] == 0.0)            # exactly zero: the mix reads the full square
    # one bad row among the five: flagged, all NaN, and the others unaffected bit for bit
    clm2 = clm.copy()
    clm2[2] = _bad_row(n)
    _host_factors(basis, clm2, [True, True, False, True, True])
    M2, info2 = _factor(basis, clm2, n + 3)
    assert 1 <= info2[2] <= P and np.all(info2[[0, 1, 3, 4]] == 0), info2
    assert np.all(np.isnan(M2[2]))
    assert np.array_equal(M2[[0, 1, 3, 4]], M[[0, 1, 3, 4]])


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("npts", [1, 63, 65, 600])
@pytest.mark.parametrize("P", [3, 17, 68, 80, 81])
def test_mix_batched_vs_numpy(P, npts, variant):
    from pta_replicator_amd import _lib, device as dv
    R, ldg, ld_m = 5, npts + 3, P * P + 5
    rng = np.random.default_rng(1000 * P + npts)
    M = rng.normal(size=(R, ld_m))
    G0 = rng.normal(size=(R, P, ldg))
    d_M, d_G0 = dv.f64(M), dv.f64(G0)
    G = dv.f64(np.full((R, P, ldg), np.nan))             # a NaN slab: what the kernel does not write stays NaN
    _lib.call("pta_gwb_mix_batched", dv.ptr(d_M), ld_m, P, dv.ptr(d_G0), R, npts, ldg, dv.ptr(G), variant, dv.stream_ptr())
    got = G.cpu().numpy()
    Mr = M[:, :P * P].reshape(R, P, P)
    ref = np.einsum("rab,rbj->raj", Mr, G0[:, :, :npts])
    scale = np.einsum("rab,rbj->raj", np.abs(Mr), np.abs(G0[:, :, :npts]))
    assert np.max(np.abs(got[:, :, :npts] - ref) / scale) < 1e-13
    assert np.all(np.isnan(got[:, :, npts:]))            # padding columns untouched
    if variant == 0:   # a realisation's product does not depend on the batch it is computed in
        G1 = dv.f64(np.full((2, P, ldg), np.nan))
        _lib.call("pta_gwb_mix_batched", ctypes.c_void_p(d_M.data_ptr() + 8 * 3 * ld_m), ld_m, P, ctypes.c_void_p(d_G0.data_ptr() + 8 * 3 * P * ldg),
                  2, npts, ldg, dv.ptr(G1), 0, dv.stream_ptr())
        assert np.array_equal(G1.cpu().numpy()[:, :, :npts], got[3:, :, :npts])


@pytest.mark.parametrize("P", lc.MIX_P)
def test_mix_batched_tiles_per_workgroup(P):
    """tpw, the 64-sample tiles one workgroup of k_gwb_mix_batched walks with its staged factor: 4 below 512 realisations (at 5 tiles the
    second workgroup takes tile 4 and leaves its loop at tile 5) and all 5 from 512 on, which no test had against a reference.
    Value: the device result is one fp64 FMA chain over the P pulsars, so |got - ref| <= (P + 2) 2^-53 sum |m||g0| against a long-double
    reference, taken for nine realisations spread over the batch; every realisation is held to twice that against the fp64 product
    of NumPy, whose own error has the same bound.  Bit-identity: R = 511 against the first 511 of R = 512, and the last realisations
    again in a launch of 3.  Measured on one MI355X: worst error / bound 0.38 (long double, P = 3; 0.06 at P = 80), 0.11 (fp64, all realisations)."""
    from pta_replicator_amd import _lib, device as dv
    npts, Rm = lc.MIX_NPTS, max(lc.MIX_R)
    ldg, ld_m = npts + 3, P * P + 5
    rng = np.random.default_rng(1000 * P + npts)
    M, G0 = rng.normal(size=(Rm, ld_m)), rng.normal(size=(Rm, P, ldg))
    Mr = M[:, :P * P].reshape(Rm, P, P)
    ref = Mr @ G0[:, :, :npts]
    scale = np.abs(Mr) @ np.abs(G0[:, :, :npts])
    pick = [0, 1, 127, 255, 256, 509, 510, 511, 300]
    ref_ld = np.stack([Mr[r].astype(np.longdouble) @ G0[r, :, :npts].astype(np.longdouble) for r in pick])
    d_M, d_G0 = dv.f64(M), dv.f64(G0)
    out = {}
    for R in lc.MIX_R:
        plan = lc.plan("pta_gwb_mix_batched", P, R, npts, 0)
        assert plan["tpw"] == (5 if R >= 512 else 4) and plan["grid_x"] == (1 if R >= 512 else 2)
        G = dv.f64(np.full((R, P, ldg), np.nan))             # a NaN slab: what the kernel does not write stays NaN
        _lib.call("pta_gwb_mix_batched", dv.ptr(d_M), ld_m, P, dv.ptr(d_G0), R, npts, ldg, dv.ptr(G), 0, dv.stream_ptr())
        got = G.cpu().numpy()
        sel = [i for i, r in enumerate(pick) if r < R]
        rr = [pick[i] for i in sel]
        r_ld = float(np.max(np.abs(got[rr, :, :npts] - ref_ld[sel]) / ((P + 2) * 2.0 ** -53 * scale[rr])))
        r_64 = float(np.max(np.abs(got[:, :, :npts] - ref[:R]) / (2 * (P + 2) * 2.0 ** -53 * scale[:R])))
        print(f"pta_gwb_mix_batched P={P} R={R} tpw={plan['tpw']}: worst error / bound {r_ld:.3f} (long double), {r_64:.3f} (fp64, all realisations)")
        assert r_ld <= 1.0 and r_64 <= 1.0
        assert np.all(np.isnan(got[:, :, npts:]))            # padding columns untouched
        out[R] = G
    assert torch.equal(out[511][:, :, :npts], out[512][:511, :, :npts])
    n = lc.MIX_SMALL_R
    assert lc.plan("pta_gwb_mix_batched", P, n, npts, 0)["tpw"] == 4
    G1 = dv.f64(np.full((n, P, ldg), np.nan))
    _lib.call("pta_gwb_mix_batched", dv.row_ptr(d_M, Rm - n), ld_m, P, dv.row_ptr(d_G0, Rm - n), n, npts, ldg, dv.ptr(G1), 0, dv.stream_ptr())
    assert torch.equal(G1[:, :, :npts], out[512][Rm - n:, :, :npts])


# ---------------------------------------------------------------- engines ----------------------------------------------------
def _psrs(P, n, seed, err_us=0.5, shared=False):
    from pta_replicator_amd.simulate import ArrayTOAs, SimulatedPulsar, make_ideal
    rng = np.random.default_rng(seed)
    common = np.sort(rng.uniform(53000, 57500, n))
    out = []
    for a in range(P):
        mjd = common if shared else np.sort(rng.uniform(53000, 57500, n))
        p = SimulatedPulsar(toas=ArrayTOAs(mjd.copy(), err_us), name=f"J{a:04d}",
                            loc={"RAJ": float(rng.uniform(0, 24)), "DECJ": float(np.degrees(np.arcsin(rng.uniform(-1, 1))))})
        make_ideal(p)
        out.append(p)
    return out


def _iso(lmax):
    return [C00] + [0.0] * ((lmax + 1) ** 2 - 1)


def _oracle_basis(eng, lmax):
    from pta_replicator_amd import red_noise as rn
    return np.array(po.correlated_basis(rn.pulsar_locations(eng.psrs), lmax))


def _engine(P=6, n=150, lmax=2, seed=77, psr_seed=11, rn=True):
    from pta_replicator_amd.engine import ReplicaEngine
    eng = ReplicaEngine(_psrs(P, n, psr_seed), seed=seed)
    eng.td_warmup = False
    eng.set_white_noise(efac=1.1, log10_equad=-6.6)
    if rn:
        eng.set_red_noise([-14.0 + 0.1 * a for a in range(P)], [3.0 + 0.2 * (a % 4) for a in range(P)], components=10)
    eng.set_gwb(-14.2, 13. / 3., clm=_iso(lmax), lmax=lmax)
    eng.prepare()
    return eng


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(np.asarray(b))))


def test_end_to_end_exact():
    """five pulsars on one TOA array: the GWB term of pulsar a is the same linear map of the mixed grid series for every a, so the
    anisotropic realisation is M_r M_iso^-1 times the isotropic one"""
    from pta_replicator_amd.engine import ReplicaEngine
    P, N, lmax, R, r0 = 5, 96, 2, 7, 3
    eng = ReplicaEngine(_psrs(P, N, 5, shared=True), seed=31)
    eng.td_warmup = False
    eng.set_gwb(-14.0, 13. / 3., clm=_iso(lmax), lmax=lmax)
    eng.prepare()
    basis = _oracle_basis(eng, lmax)
    rng = np.random.default_rng(9)
    clm = _good_rows(rng, R, 9)
    clm[0] = _iso(lmax)                                     # the configured sky
    Mr = _host_factors(basis, clm, [True] * R)
    Miso = Mr[0]
    X_iso = eng.generate_per_signal(R, r0=r0)["gwb"].cpu().numpy().reshape(R, P, N)
    out = eng.generate_per_signal(R, r0=r0, theta={"gwb_clm": clm})
    X = out["gwb"].cpu().numpy().reshape(R, P, N)
    assert torch.equal(out["gwb"], out["total"])
    ref = np.einsum("rab,rbn->ran", Mr @ np.linalg.inv(Miso)[None], X_iso)
    err = max(_rel(X[r], ref[r]) for r in range(R))
    print(f"X_aniso vs M_r M_iso^-1 X_iso: {err:.2e};  configured row vs fixed path: {_rel(X[0], X_iso[0]):.2e}")
    assert err < 1e-11
    assert _rel(X[0], X_iso[0]) < 1e-12
    assert _rel(X[1], X_iso[1]) > 1e-3                      # and the key does something
    # with the power-law keys on top: the same map of the rescaled isotropic realisation
    pl = {"gwb_log10_A": np.linspace(-14.5, -13.5, R), "gwb_gamma": np.linspace(3.0, 5.0, R)}
    Y_iso = eng.generate_per_signal(R, r0=r0, theta=pl)["gwb"].cpu().numpy().reshape(R, P, N)
    Y = eng.generate_per_signal(R, r0=r0, theta=dict(pl, gwb_clm=clm))["gwb"].cpu().numpy().reshape(R, P, N)
    assert max(_rel(Y[r], np.einsum("ab,bn->an", Mr[r] @ np.linalg.inv(Miso), Y_iso[r])) for r in range(R)) < 1e-11


@pytest.fixture(scope="module")
def eng6():
    eng = _engine()
    eng.prepare_optimal_statistic(components=6, anisotropy_lmax=2)
    return eng


def test_realisations_do_not_depend_on_the_batch(eng6):
    eng = eng6
    R, r0 = 40, 3
    rng = np.random.default_rng(12)
    theta = {"gwb_clm": _good_rows(rng, R, 9), "gwb_log10_A": rng.uniform(-14.5, -14.0, R), "rn_gamma": rng.uniform(2, 5, (R, eng.P))}
    _host_factors(_oracle_basis(eng, 2), theta["gwb_clm"], [True] * R)
    ref = eng.generate(R, r0=r0, theta=theta)
    parts = [eng.generate(n, r0=r0 + lo, theta={k: v[lo:lo + n] for k, v in theta.items()}) for lo, n in ((0, 13), (13, 27))]
    assert torch.equal(torch.cat(parts), ref)
    keep = eng.workspace_bytes
    try:
        eng.workspace_bytes = 1                              # max_batch() = 16: three batches
        assert eng.max_batch(hyper=True, clm=True) == 16
        assert torch.equal(eng.generate(R, r0=r0, theta=theta), ref)
    finally:
        eng.workspace_bytes = keep
    # generate_os = optimal_statistic(generate), the joint fit included, whatever the chunk
    want = eng.optimal_statistic(ref, pairs=True)
    assert want["a2clm"].shape == (R, 9) and want["clm_sigma"].shape == (9,) and want["clm_cov"].shape == (9, 9)
    for chunk in (7, R):
        got = eng.generate_os(R, r0=r0, theta=theta, chunk=chunk, pairs=True)
        for k in ("A2", "snr", "rho", "a2clm"):
            assert torch.equal(got[k], want[k]), (k, chunk)


def test_bad_sky_raises_and_sampled_labels(eng6):
    from pta_replicator_amd.engine import ReplicaEngine
    eng = eng6
    basis = _oracle_basis(eng, 2)
    R = 6
    clm = _good_rows(np.random.default_rng(3), R, 9)
    clm[4] = _bad_row(9)
    _host_factors(basis, clm, [True] * 4 + [False, True])
    with pytest.raises(np.linalg.LinAlgError, match="realisation 14"):
        eng.generate(R, r0=10, theta={"gwb_clm": clm})
    with pytest.raises(np.linalg.LinAlgError, match="positive definite"):
        eng.generate_os(R, theta={"gwb_clm": clm}, chunk=4)
    # ---- a wide box: NaN rows exactly where the sky is flagged, nothing raised
    R = 64
    eng.set_hyper_prior(gwb_clm=(-4.0, 4.0), gwb_log10_A=(-14.6, -14.0), rn_log10_A=(-14.5, -13.5), rn_gamma=(2, 5))
    rows, th = eng.generate_sampled(R, r0=5)
    info = th["gwb_orf_info"].cpu().numpy()
    c = th["gwb_clm"].cpu().numpy()
    assert th["gwb_clm"].shape == (R, 9) and np.all(c[:, 0] == C00) and np.all(np.abs(c[:, 1:]) <= 4.0)
    assert 0 < np.count_nonzero(info) < R, info
    _host_factors(basis, c, info == 0)
    nan = torch.isnan(rows).cpu().numpy()
    assert np.all(nan[info != 0]) and not np.any(nan[info == 0])
    # ---- labels are a function of (seed, r) alone
    th_a, th_b = eng.sample_theta(R, r0=5), eng.sample_theta(9, r0=20)
    for k in th:
        assert torch.equal(th_a[k], th[k]), k
        assert torch.equal(th_b[k], th[k][15:24]), k
    # ---- the sky's stream is its own: no other label moves, and with the configured sky drawn no residual does either
    eng.set_hyper_prior(gwb_log10_A=(-14.6, -14.0), rn_log10_A=(-14.5, -13.5), rn_gamma=(2, 5))
    rows0, th0 = eng.generate_sampled(R, r0=5)
    assert set(th0) == set(th) - {"gwb_clm", "gwb_orf_info"}
    for k in th0:
        assert torch.equal(th0[k], th[k]), k
    eng.set_hyper_prior(gwb_clm=(0.0, 0.0), gwb_log10_A=(-14.6, -14.0), rn_log10_A=(-14.5, -13.5), rn_gamma=(2, 5))
    rows1, th1 = eng.generate_sampled(R, r0=5)
    assert np.array_equal(th1["gwb_clm"].cpu().numpy(), np.tile(_iso(2), (R, 1))) and not th1["gwb_orf_info"].any()
    assert _rel(rows1.cpu().numpy(), rows0.cpu().numpy()) < 1e-12
    eng._prior = None


def test_joint_fit_on_the_device(eng6):
    """a2clm against the NumPy OS of the same rows with the host's joint weights: nine components, two pta_os_pairs slices"""
    from pta_replicator_amd import _lib, optimal_statistic as ost
    eng = eng6
    R = 33
    rows = eng.generate(R, r0=2)
    res = eng.optimal_statistic(rows)
    st = eng._os
    assert st["aniso"]["n_lm"] == 9 > _lib.OS_NORF
    _, _, num = ost.os_from_rows(st["plan"], rows.cpu().numpy())
    Wj, cov, sig = ost.joint_weights(eng.d_orf_basis.cpu().numpy()[:, st["plan"].pair_a, st["plan"].pair_b], st["plan"].den)
    assert np.array_equal(Wj, st["aniso"]["Wj_host"])
    err = _rel(res["a2clm"].cpu().numpy(), num @ Wj.T)
    print(f"a2clm vs host: {err:.2e}")
    assert err < 1e-10
    assert _rel(res["clm_cov"].cpu().numpy(), cov) < 1e-14 and _rel(res["clm_sigma"].cpu().numpy(), sig) < 1e-14
    # the basis the weights were built from is the oracle's
    assert _rel(eng.d_orf_basis.cpu().numpy(), _oracle_basis(eng, 2)) < 1e-10
    # every existing key is what the statistic without the joint fit returns
    keep = eng._os
    try:
        eng.prepare_optimal_statistic(components=6)
        plain = eng.optimal_statistic(rows, pairs=True)
        assert "a2clm" not in plain
    finally:
        eng._os = keep
    full = eng.optimal_statistic(rows, pairs=True)
    for k in ("A2", "snr", "sigma", "rho", "sigma_pair"):
        assert torch.equal(full[k], plain[k]), k
    # the matched statistic does not carry the joint fit
    with pytest.raises(ValueError, match="anisotropy_lmax"):
        eng.generate_os(4, theta={"gwb_log10_A": np.full(4, -14.0)}, matched=True)
    with pytest.raises(ValueError, match="anisotropy_lmax"):
        eng.optimal_statistic(rows, theta={"gwb_log10_A": np.full(R, -14.0)})


# ---------------------------------------------------------------- statistics --------------------------------------------------
def test_dipole_recovery():
    """16 pulsars, 200 TOAs, 0.1 us, GWB -14 (the signal engine of tests/test_gpu_os.py) with lmax = 1: inject c = (sqrt 4 pi, 0, 1, 0)
    into every realisation and recover c_1m / c_00 from the joint fit; 16 groups of 128 realisations give the standard error.

    Measured on the MI355X (q = mean over the groups +- standard error): dipole q_1m = (-0.099, 1.045, -0.051) +- (0.053, 0.056, 0.057),
    isotropic q_1m = (-0.100, 0.034, -0.049) +- (0.052, 0.051, 0.055)."""
    from pta_replicator_amd.engine import ReplicaEngine
    eng = ReplicaEngine(_psrs(16, 200, 21, err_us=0.1), seed=8)
    eng.td_warmup = False
    eng.set_white_noise(efac=1.0)
    eng.set_gwb(-14.0, 13. / 3., clm=_iso(1), lmax=1)
    eng.prepare()
    eng.prepare_optimal_statistic(components=14, anisotropy_lmax=1)
    R, groups = 2048, 16
    basis = _oracle_basis(eng, 1)
    inj = np.array([C00, 0.0, 1.0, 0.0])
    _host_factors(basis, inj[None], [True])

    def q_of(c):
        a2 = eng.generate_os(R, theta={"gwb_clm": np.tile(c, (R, 1))})["a2clm"].cpu().numpy().reshape(groups, R // groups, 4).mean(axis=1)
        q = a2 / a2[:, :1] * C00
        return q.mean(axis=0), q.std(axis=0, ddof=1) / np.sqrt(groups)
    q, se = q_of(inj)
    print("dipole   q =", q, "+-", se)
    assert np.all(np.abs(q[1:] - inj[1:]) < 5 * se[1:]), (q, se)
    assert q[2] > 5 * se[2]                                  # the injected dipole is detected: the test can fail
    q0, se0 = q_of(np.array(_iso(1)))
    print("isotropic q =", q0, "+-", se0)
    assert np.all(np.abs(q0[1:]) < 5 * se0[1:]), (q0, se0)
