"""Host side of the common red processes (no GPU): the constants across header, _lib and _cproc, the configuration and the ranks of the
ORF factors, theta's cp_* keys and their prior boxes, every refusal on a configured, unprepared engine, the device formulas compiled as
plain C++ (tests/cproc/cproc_host.cpp) - stream mapping against philox_ref, the coefficient sums and the harmonic rotation against
long-double evaluations - and the low-rank columns the fixed-noise statistics get."""
import os

import numpy as np
import pytest

import cproc_reference as cr
from oracle import philox_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 5
COUNTS = (40, 31, 57, 1, 64)


@pytest.fixture(scope="module")
def psrs():
    return cr.make_psrs(COUNTS)


def _engine(psrs, procs=(("monopole", 5, -14.0, 3.0), ("dipole", 3, -13.5, 2.0)), gwb=True):
    from pta_replicator_amd.engine import ReplicaEngine
    eng = ReplicaEngine(psrs, seed=5)
    eng.set_white_noise(efac=1.1, log10_equad=-6.5)
    n = len(psrs)
    eng.set_red_noise([-14.0, None, -13.5, -14.2, -14.1][:n], [3.0, None, 2.5, 4.0, 3.3][:n], components=10)
    if gwb:
        eng.set_gwb(-14.5, 13. / 3.)
    for orf, nf, lA, g in procs:
        eng.add_common_process(lA, g, orf=orf, components=nf)
    return eng


# ---------------------------------------------------------------- constants ------------------------------------------
def test_constants_agree():
    from pta_replicator_amd import _chrom, _cproc, _hyper, _lib, _wn_hyper, engine
    head = open(os.path.join(ROOT, "pta_replicator_amd", "csrc", "pta_cproc.h")).read()
    api = open(os.path.join(ROOT, "include", "pta_replicator_amd.h")).read()
    lib = cr.twin()
    assert "#define PTA_STREAM_CPROC 12u" in head
    assert lib.cp_stream_kind() == _cproc.STREAM_CPROC == engine.STREAM_CPROC == cr.STREAM_CPROC == 12
    taken_kinds = {engine.STREAM_GWB, engine.STREAM_RN, engine.STREAM_WN, engine.STREAM_ECORR, engine.STREAM_TD, engine.STREAM_TDGW,
                   engine.STREAM_HYPER, engine.STREAM_CW, engine.STREAM_BWM, engine.STREAM_CHROM, 11}
    assert taken_kinds == set(range(1, 12))   # 11: PTA_STREAM_POP
    assert f"#define PTA_CPROC_RG {_lib.CPROC_RG}\n" in head and lib.cp_rg() == _lib.CPROC_RG
    assert f"#define PTA_CPROC_MAX {_lib.CPROC_MAX} " in api and _lib.CPROC_MAX == _cproc.MAX == 4
    assert f"#define PTA_CPROC_KMAX {_lib.CPROC_KMAX} " in api and _lib.CPROC_KMAX == 64
    assert _cproc.KEYS == ("cp_log10_A", "cp_gamma")
    assert _cproc.FIELD == {"cp_log10_A": cr.FIELD_LOG10_A, "cp_gamma": cr.FIELD_GAMMA} == {"cp_log10_A": 8, "cp_gamma": 9}
    taken = {0, _hyper.SPEC_FIELD, _hyper.CLM_FIELD, *_wn_hyper.FIELD.values(), *_chrom.FIELD.values()}
    assert taken == set(range(8)) and not taken & set(_cproc.FIELD.values())
    assert not set(_cproc.KEYS) & set(_hyper.ALL_KEYS) and not set(_cproc.KEYS) & set(_chrom.KEYS)


# ---------------------------------------------------------------- configuration --------------------------------------
def test_configuration_and_ranks(psrs):
    """the ranks of B for the four names and a rank-2 array; B B^T = Gamma; the listing; the basis tables"""
    from pta_replicator_amd import _cproc
    from pta_replicator_amd import optimal_statistic as ost
    eng = _engine(psrs, procs=())
    assert eng.common_processes == [] and not eng._cproc
    user = cr.rank2_orf(P)
    for k, (orf, rank) in enumerate((("monopole", 1), ("dipole", 3), ("hd", P), (user, 2))):
        assert eng.add_common_process(-14.0 - k, 2.0 + k, orf=orf, components=3 + k) is eng
        p = eng._cproc[-1]
        assert p["B"].shape == (P, rank) and p["B"].flags["C_CONTIGUOUS"]
        assert np.allclose(p["B"] @ p["B"].T, p["Gamma"], atol=1e-13)
        assert np.array_equal(p["Gamma"], ost.orf_matrix(orf, eng._unit_vectors()))
    assert not eng._prepared
    listed = eng.common_processes
    assert [d["orf"] for d in listed] == ["monopole", "dipole", "hd", "array"] and [d["rank"] for d in listed] == [1, 3, P, 2]
    assert [d["components"] for d in listed] == [3, 4, 5, 6] and [d["log10_amplitude"] for d in listed] == [-14.0, -15.0, -16.0, -17.0]
    with pytest.raises(ValueError, match="at most 4 common processes"):
        eng.add_common_process(-14.0, 3.0)
    assert len(eng._cproc) == 4
    curn = _engine(psrs, procs=(("curn", 2, -14.0, 3.0),))
    assert curn._cproc[0]["B"].shape == (P, P) and curn.common_processes[0]["rank"] == P
    one = _engine(psrs[:1], procs=(("hd", 2, -14.0, 3.0), ("monopole", 2, -14.0, 3.0), ("dipole", 1, -14.0, 3.0)), gwb=False)
    assert [d["rank"] for d in one.common_processes] == [1, 1, 1]   # a single pulsar: every ORF is the number 1
    # the tables: T the array's span of mjd * 86400, K the widest process, amp zero beyond a process's columns
    t = _cproc.host_tables(eng._cproc, eng._cproc_toas())
    toas = np.concatenate(eng._cproc_toas())
    assert t["T"] == toas.max() - toas.min() and t["K"] == 12 and t["kp"] == [6, 8, 10, 12] and t["rho"] == [1, 3, P, 2]
    assert t["amp_host"].shape == (4, 12) and np.all(t["amp_host"][0, 6:] == 0) and np.all(t["amp_host"][0, :6] > 0)
    want = np.sqrt(cr.prior_phi(3, t["T"], -14.0, 2.0))
    assert np.all(np.abs(t["amp_host"][0, :6] - want) <= 4 * np.spacing(want))
    assert t["sc1_host"].shape == (eng.n_toa, 2) and t["sc1_host"].dtype == np.float64


def test_configuration_refusals(psrs):
    eng = _engine(psrs, procs=())
    bad_orf = np.eye(P)
    bad_orf[0, 1] = bad_orf[1, 0] = 2.0   # not positive semi-definite
    asym = np.eye(P)
    asym[0, 1] = 0.5
    for kw, msg in ((dict(components=0), "components"), (dict(components=33), "components"), (dict(components=2.5), "components"),
                    (dict(components=True), "components"), (dict(orf="quadrupole"), "unknown ORF"), (dict(orf=bad_orf), "not positive semi-definite"),
                    (dict(orf=asym), "symmetric"), (dict(orf=np.eye(P + 1)), "finite"), (dict(orf=np.zeros((P, P))), "rank 0")):
        with pytest.raises(ValueError, match=msg):
            eng.add_common_process(-14.0, 3.0, **kw)
    for lA, g in ((np.nan, 3.0), (-14.0, np.inf), ([-14.0, -13.0], 3.0), (None, 3.0)):
        with pytest.raises(ValueError, match="add_common_process"):
            eng.add_common_process(lA, g)
    assert not eng._cproc and not eng._prepared


# ---------------------------------------------------------------- theta and prior boxes -------------------------------
def test_theta_parts_and_validation(psrs):
    eng, plain = _engine(psrs), _engine(psrs, procs=())
    R, n = 3, 2
    th = dict(cp_log10_A=np.full((R, n), -13.5), cp_gamma=np.full((R, n), 3.0))
    hyper, det = eng._theta_parts(th, R)
    assert hyper is None and set(det) == set(th)
    both = dict(th, rn_log10_A=np.full((R, P), -14.0), wn_efac=np.ones((R, P)), gwb_gamma=np.full(R, 4.0))
    hyper, det = eng._theta_parts(both, R)
    assert set(hyper) == {"rn_log10_A", "gwb_gamma"} and set(det) == set(th) | {"wn_efac"}
    nan = dict(cp_log10_A=np.full((R, n), np.nan), cp_gamma=np.full((R, n), np.nan))   # all as configured: NaN indices are unused
    assert set(eng._theta_parts(nan, R)[1]) == set(th)
    assert set(eng._theta_parts({"cp_log10_A": th["cp_log10_A"]}, R)[1]) == {"cp_log10_A"}   # a key alone keeps the other parameter
    ok = np.full((R, n), -13.5)
    for bad, msg in (({"cp_log10_A": np.full((R, n + 1), -13.5)}, "shape"), ({"cp_gamma": np.full((R,), 3.0)}, "shape"),
                     ({"cp_log10_A": np.where(np.arange(n) == 1, np.inf, ok)}, "infinite values"),
                     ({"cp_log10_A": ok, "cp_gamma": np.where(np.arange(n) == 0, np.nan, 3.0 + 0 * ok)}, "non-finite values where the amplitude is sampled"),
                     ({"cp_gamma": np.where(np.arange(n) == 0, np.nan, 3.0 + 0 * ok)}, "non-finite values where the amplitude is sampled"),
                     ({"cp_log10_A": ok, "cp_gamma": np.full((R, n), np.inf)}, "non-finite"), ({"cp_log10_A": "x"}, "expected an array")):
        with pytest.raises(ValueError, match=msg):
            eng._theta_parts(bad, R)
    for call in (lambda: plain.generate(R, theta=th), lambda: plain.generate_per_signal(R, theta={"cp_gamma": th["cp_gamma"]}),
                 lambda: plain._theta_parts(th, R), lambda: plain.set_hyper_prior(cp_log10_A=(-15, -13))):
        with pytest.raises(ValueError, match="no common process is configured"):
            call()
    assert not eng._prepared and not plain._prepared


def test_prior_boxes(psrs):
    from pta_replicator_amd import _cproc
    eng = _engine(psrs)
    eng.set_hyper_prior(cp_log10_A=(-15, -13), cp_gamma=[[1, 2], [3, 4]])
    assert eng._prior is None and set(eng._cproc_prior) == set(_cproc.KEYS)
    assert np.array_equal(eng._cproc_prior["cp_log10_A"][0], [-15, -15]) and np.array_equal(eng._cproc_prior["cp_gamma"][1], [2, 4])
    for bad in (dict(cp_log10_A=(-13, -15)), dict(cp_gamma=np.zeros((3, 2))), dict(cp_gamma=(1.0, np.inf))):
        with pytest.raises(ValueError, match="set_hyper_prior"):
            eng.set_hyper_prior(**bad)
    eng.set_hyper_prior(gwb_log10_A=(-15, -14))
    assert eng._cproc_prior is None and eng._prior is not None
    lib = cr.twin()
    seed, r0, R, n = 0x0123456789ABCDEF, 77, 5, 4
    lo, hi = np.linspace(-15, -14, n), np.linspace(-13.5, -13, n)
    seen = []
    for key, field in _cproc.FIELD.items():
        unit, out = np.zeros(R * n), np.zeros(R * n)
        lib.cp_draw_field(seed, r0, R, n, field, cr._p(np.zeros(n)), cr._p(np.ones(n)), cr._p(unit))
        lib.cp_draw_field(seed, r0, R, n, field, cr._p(lo), cr._p(hi), cr._p(out))
        unit, out = unit.reshape(R, n), out.reshape(R, n)
        for r in range(R):
            _, u2 = philox_ref.uniform_pairs(seed, r0 + r, philox_ref.stream_id(7, field), n)
            assert np.array_equal(unit[r], np.asarray(u2, dtype=np.float64)), (key, r)
        assert np.all(out >= lo) and np.all(out <= hi)
        seen.append(unit)
    assert not np.array_equal(seen[0], seen[1])


# ---------------------------------------------------------------- refusals, before any launch -------------------------
def test_refusals_before_any_launch(psrs):
    """on a configured, unprepared engine: each is a ValueError that names the reason, and the engine is still unprepared"""
    eng, plain = _engine(psrs), _engine(psrs, procs=())
    R, n = 3, 2
    th = dict(cp_log10_A=np.full((R, n), -13.5), cp_gamma=np.full((R, n), 3.0))
    td = "common process.*no TD mode"
    for call in (lambda: eng.prepare_td(), lambda: eng.generate_td(R), lambda: eng.generate_os(R, td=True),
                 lambda: eng.generate_lnl(R, {"gwb_log10_A": np.array([-14.5])}, td=True), lambda: eng.generate_f_statistic(R, td=True),
                 lambda: eng.generate_bwm_statistic(R, td=True), lambda: eng.generate_correlated_lnl(R, {"gwb_log10_A": np.array([-14.5])}, td=True),
                 lambda: eng._theta_parts({"cw_log10_h": np.zeros(R)}, R, td=True)):
        with pytest.raises(ValueError, match=td):
            call()
    nm = "cannot be part of a statistic's noise model"
    for e in (eng, plain):
        with pytest.raises(ValueError, match=nm):
            e.optimal_statistic(None, theta=th)
        with pytest.raises(ValueError, match=nm):
            e.generate_os(R, theta=th, matched=True)
        with pytest.raises(ValueError, match=nm):
            e.log_likelihood(None, {"cp_log10_A": np.full((2, n), -13.5)})
        with pytest.raises(ValueError, match=nm):
            e.generate_lnl(R, {"cp_gamma": np.full((2, n), 3.0)})
    from pta_replicator_amd import _hyper
    from pta_replicator_amd.engine_clnl import check_grid_keys
    with pytest.raises(ValueError, match=nm):
        _hyper.check_theta_os(th, R, P, eng._rn, True)
    with pytest.raises(ValueError, match=r"grid\['cp_log10_A'\].*only \['gwb_log10_A', 'gwb_gamma'\] vary"):
        check_grid_keys({"cp_log10_A": np.array([-14.0])})
    with pytest.raises(ValueError, match=r"prepare_optimal_statistic\(matched=True\).*common process"):
        eng.prepare_optimal_statistic(matched=True)
    with pytest.raises(ValueError, match="prepare_likelihood.*common process"):
        eng.prepare_likelihood()
    assert not eng._prepared and not plain._prepared and eng._cproc_t is None


def test_list_api_refuses_before_drawing(psrs):
    from pta_replicator_amd.red_noise import add_common_process
    np.random.seed(9)
    state = np.random.get_state()[1].copy()
    for args, kw, msg in (((psrs, -14.0, 3.0), dict(orf="quadrupole"), "unknown ORF"), ((psrs, -14.0, 3.0), dict(components=33), "components"),
                          ((psrs[0], -14.0, 3.0), {}, "non-empty list"), (([], -14.0, 3.0), {}, "non-empty list"),
                          ((psrs, -14.0, 3.0), dict(Tspan=-1.0), "Tspan"), ((psrs, -14.0, 3.0), dict(orf=np.eye(P + 1)), "finite")):
        with pytest.raises(ValueError, match=msg):
            add_common_process(*args, **kw)
    assert np.array_equal(np.random.get_state()[1], state) and not any(p.added_signals for p in psrs)


# ---------------------------------------------------------------- device formulas on the host -------------------------
def test_stream_mapping_against_philox_ref():
    """deviate n = c rho + j of stream (12, p) is branch n & 1 of pair n >> 1, philox_ref's, to the bound the other streams' twins are
    held to; odd rho makes pairs straddle columns; a stream of its own per process"""
    seed, r = 0x0123456789ABCDEF, 2 ** 32 + 5
    for p, rho, kp in ((0, 1, 6), (1, 3, 4), (2, 5, 2), (3, 2, 64)):
        z = cr.twin_draws(seed, r, p, rho, kp)
        assert z.shape == (kp, rho) and np.max(np.abs(z - cr.draws(seed, r, p, rho, kp))) < 1e-13
    a, b = cr.twin_draws(seed, r, 0, 2, 4), cr.twin_draws(seed, r, 1, 2, 4)
    rn = np.empty(8)
    rn[0::2], rn[1::2] = philox_ref.normal_pairs(seed, r, philox_ref.stream_id(philox_ref.STREAM_RN, 0), 4)
    ch = np.empty(8)
    ch[0::2], ch[1::2] = philox_ref.normal_pairs(seed, r, philox_ref.stream_id(10, 0), 4)
    assert not np.array_equal(a, b) and np.max(np.abs(a.ravel() - rn)) > 1e-3 and np.max(np.abs(a.ravel() - ch)) > 1e-3


def test_coefficient_sums_against_long_double():
    """the twin of k_engine_cproc_coef: sum_j B z in ascending j with one fma per term is within gamma_rho sum_j |B z| of the long-double
    sum (rho roundings of partial sums that never exceed sum |B z|); a coefficient of n processes within u sum_p (rho_p + n) amp_p sum_j
    |B_p z_p| (one more rounding per process from the fma that joins it, n - 1 from the partial sums over the processes).  Configured
    amplitudes, NaN labels, labels; a process with fewer components leaves its upper columns to the others."""
    rng = np.random.default_rng(4)
    seed, r, Pn = 99, 7, 6
    lib = cr.twin()
    for rho in (1, 3, Pn):
        B, z = np.ascontiguousarray(rng.normal(size=(Pn, rho))), rng.normal(size=rho)
        val, mag = cr.mix_ld(B, z)
        got = np.array([lib.cp_mix(cr._p(np.ascontiguousarray(B[a])), cr._p(z), rho) for a in range(Pn)])
        assert np.all(np.abs(got.astype(cr.LD) - val) <= cr.gamma_n(rho) * mag)
    Bs = [np.ascontiguousarray(rng.normal(size=(Pn, rho))) for rho in (1, 3, Pn, 2)]
    kp, K, T = [6, 10, 4, 8], 10, 4.1e8
    conf = [(-14.0, 3.0), (-13.5, 2.0), (-14.2, 4.3), (-13.8, 1.1)]
    amp = np.zeros((4, K))
    for p, (lA, g) in enumerate(conf):
        amp[p, :kp[p]] = np.sqrt(cr.prior_phi(kp[p] // 2, T, lA, g))
    zs = [cr.twin_draws(seed, r, p, Bs[p].shape[1], kp[p]) for p in range(4)]

    def check(coef, amps, extra):
        for c in range(K):
            val, bound = np.zeros(Pn, dtype=cr.LD), np.zeros(Pn)
            for p in range(4):
                if c < kp[p]:
                    v, mag = cr.mix_ld(Bs[p], zs[p][c])
                    val += cr.LD(amps[p][c]) * v
                    bound += cr.U * (Bs[p].shape[1] + 4 + extra) * amps[p][c] * mag
            assert np.all(np.abs(coef[:, c].astype(cr.LD) - val) <= bound), c
    coef = cr.twin_coef(seed, r, Pn, K, kp, Bs, amp, T)
    check(coef, amp, 0)
    assert np.array_equal(coef, cr.twin_coef(seed, r, Pn, K, kp, Bs, amp, T, [np.nan] * 4, [np.nan] * 4))   # NaN = as configured, bit for bit
    lA, g = np.array([-13.1, np.nan, -14.4, -13.9]), np.array([2.2, np.nan, 3.9, 5.0])
    amp_th = amp.copy()
    for p in (0, 2, 3):
        amp_th[p, :kp[p]] = np.sqrt(cr.prior_phi(kp[p] // 2, T, lA[p], g[p]))
    # the twin's amplitude (two pows and a sqrt of libm) is within 8 ulp = 16 u of NumPy's: 16 more roundings' worth per process
    check(cr.twin_coef(seed, r, Pn, K, kp, Bs, amp, T, lA, g), amp_th, 16)
    # columns 8, 9 belong to process 1 alone: its term, one rounding
    for c in (8, 9):
        want = np.array([amp[1, c] * lib.cp_mix(cr._p(np.ascontiguousarray(Bs[1][a])), cr._p(np.ascontiguousarray(zs[1][c])), 3) for a in range(Pn)])
        assert np.array_equal(coef[:, c], want)


@pytest.mark.parametrize("nf", [1, 2, 14, 32])
def test_rotation_against_long_double(nf):
    """the twin of the add kernel's loop - harmonic k + 1 from harmonic k by rotation through the float64 (sin, cos)(2 pi x) that
    _cproc.sincos1 tabulates - against sum_c coef_c F_ic evaluated in long double from x = frac(t / T): |delta| <= 8 n_f u sum_c |coef_c|
    per element (cproc_reference.synth_ld), over spans of 3 - 20 yr at MJD 53000"""
    from pta_replicator_amd import _cproc
    rng = np.random.default_rng(nf)
    worst = 0.0
    for years in (3.0, 7.7, 12.5, 20.0):
        t = np.sort(rng.uniform(53000.0, 53000.0 + years * 365.25, 400)) * 86400.0
        T = t.max() - t.min()
        sc1 = _cproc.sincos1(t, T)
        assert np.all(np.abs(np.hypot(sc1[:, 0], sc1[:, 1]) - 1) < 4 * cr.U)
        for _ in range(3):
            coef = rng.normal(size=2 * nf) * 10.0 ** rng.uniform(-8, -5, 2 * nf)
            got = cr.twin_synth(coef, sc1)
            val, bound = cr.synth_ld(coef, t, T)
            ratio = float(np.max(np.abs(got.astype(cr.LD) - val) / bound))
            worst = max(worst, ratio)
            assert ratio <= 1.0, (years, ratio)
    print(f"n_f = {nf}: worst |delta| / bound = {worst:.3f}")


# ---------------------------------------------------------------- the fixed-noise statistics' columns ----------------
def test_low_rank_columns(psrs):
    """what the shared front hands to the plan builders: the array-wide basis and sum_p Gamma_p,aa phi_p per column, a process with fewer
    components contributing to its own columns only; they follow the red-noise columns"""
    from pta_replicator_amd import optimal_statistic as ost
    user = 2.5 * cr.rank2_orf(P)
    eng = _engine(psrs, procs=(("monopole", 5, -14.0, 3.0), (user, 3, -13.5, 2.0)))
    F, phi = eng._cproc_low_rank_host()
    toas = eng._cproc_toas()
    T = max(t.max() for t in toas) - min(t.min() for t in toas)
    for a in range(P):
        assert np.array_equal(F[a], ost.fourier_basis(toas[a], 5, T)) and F[a].shape == (COUNTS[a], 10)
        want = cr.prior_phi(5, T, -14.0, 3.0)
        want[:6] += user[a, a] * cr.prior_phi(3, T, -13.5, 2.0)
        assert np.all(np.abs(phi[a] - want) <= 8 * np.spacing(want))
    assert not eng._prepared
