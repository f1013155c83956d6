"""Host side of the chromatic Gaussian process (no GPU): the row weights against a long-double evaluation, the constants across
header, _lib and _chrom, the device formulas compiled as plain C++ (tests/chrom/chrom_host.cpp) - stream mapping and prior map against
philox_ref, the amplitude rule - every refusal on a configured, unprepared engine, and the low-rank columns the fixed-noise statistics
get against the reference module."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import chrom_reference as cr
from helpers import load, mjd_ld
from oracle import philox_ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
P = 4
CH_A, CH_G = [-13.5, None, -13.2, -14.0], [2.5, None, 3.5, 1.8]


@pytest.fixture(scope="module")
def ch(tmp_path_factory):
    out = tmp_path_factory.mktemp("chrom") / "libchromhost.so"
    src = os.path.join(HERE, "chrom", "chrom_host.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", str(out)])
    lib = ctypes.CDLL(str(out))
    i, u64, d, p = ctypes.c_int, ctypes.c_uint64, ctypes.c_double, ctypes.POINTER(ctypes.c_double)
    lib.ch_coef.argtypes = [u64, u64, i, i, p, p, p, i, d, d, p, p]
    lib.ch_draw_field.argtypes = [u64, u64, i, i, i, p, p, p]
    return lib


def _p(a):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _psrs(bands=(820.0, 1440.0)):
    from pta_replicator_amd.simulate import ArrayTOAs, SimulatedPulsar, make_ideal
    z = load("c3_mini.npz")
    psrs = []
    for i in range(P):
        mjd = mjd_ld(z, "", i)
        freqs = np.array([bands[k % len(bands)] for k in range(len(mjd))])
        p = SimulatedPulsar(toas=ArrayTOAs(mjd, z[f"err_us_{i}"], freqs_mhz=freqs), name=str(z["names"][i]),
                            loc={"RAJ": float(z["raj_hours"][i]), "DECJ": float(z["decj_deg"][i])})
        make_ideal(p)
        psrs.append(p)
    return psrs


def _engine(chrom=True, components=7, **kw):
    from pta_replicator_amd.engine import ReplicaEngine
    eng = ReplicaEngine(_psrs(), seed=5)
    eng.set_white_noise(efac=1.1, log10_equad=-6.5)
    eng.set_red_noise([-14.0, None, -13.5, -14.2], [3.0, None, 2.5, 4.0], components=10)
    eng.set_gwb(-14.5, 13. / 3.)
    if chrom:
        eng.set_chromatic_noise(list(CH_A), list(CH_G), components=components, **kw)
    return eng


# ---------------------------------------------------------------- weights --------------------------------------------
@pytest.mark.parametrize("index,ref", [(2.0, 1400.0), (4.0, 1400.0), (2.3, 1284.0), (-1.5, 800.0)])
def test_weights_against_long_double(index, ref):
    """w = fl(fl(nu_ref / nu) ** chi): the quotient is off by at most half an ulp, which the power multiplies by |chi|, and NumPy's **
    adds at most one ulp of its own: |w - exact| <= (|chi| / 2 + 1) 2^-52 w"""
    from pta_replicator_amd import _chrom
    rng = np.random.default_rng(3)
    nu = np.concatenate([rng.uniform(300.0, 3500.0, 4000), [ref, 327.0, 430.0, 820.0, 1440.0, 2300.0]])
    w = _chrom.weights(nu, index, ref)
    assert w.dtype == np.float64 and w.shape == nu.shape
    exact = cr.weights_longdouble(nu, index, ref)
    assert np.all(np.abs(w.astype(np.longdouble) - exact) <= (abs(index) / 2 + 1) * 2.0 ** -52 * exact)
    assert np.array_equal(w, cr.weights(nu, index, ref))
    assert w[4000] == 1.0   # a TOA at the reference frequency keeps weight one exactly


def test_weights_refuse_bad_frequencies_by_name():
    from pta_replicator_amd import _chrom
    for bad in (0.0, -1400.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="J1234.*TOA 2"):
            _chrom.weights(np.array([1400.0, 820.0, bad]), name="pulsar J1234")


def test_frequencies_come_from_freqs_mhz_then_get_freqs():
    from pta_replicator_amd import _chrom

    class Q:
        def __init__(self, v):
            self.value = v

        def to(self, unit):
            assert unit == "MHz"
            return self

    class Toas:
        def get_mjds(self):
            return Q(np.arange(5.0))

        def get_freqs(self):
            return Q(np.full(5, 430.0))

    class Psr:
        name, toas = "X", Toas()
    assert np.array_equal(_chrom.toa_freqs(Psr()), np.full(5, 430.0))
    Psr.toas.freqs_mhz = 1440.0
    assert np.array_equal(_chrom.toa_freqs(Psr()), np.full(5, 1440.0))


# ---------------------------------------------------------------- constants ------------------------------------------
def test_constants_agree(ch):
    from pta_replicator_amd import _chrom, _hyper, _lib, _wn_hyper, engine
    rng_h = open(os.path.join(ROOT, "pta_replicator_amd", "csrc", "pta_rng.h")).read()
    chrom_h = open(os.path.join(ROOT, "pta_replicator_amd", "csrc", "pta_chrom.h")).read()
    assert "#define PTA_STREAM_CHROM 10u" in rng_h
    assert ch.ch_stream_kind() == _chrom.STREAM_CHROM == engine.STREAM_CHROM == cr.STREAM_CHROM == 10
    assert f"#define PTA_CHROM_RG {_lib.CHROM_RG}\n" in chrom_h and ch.ch_rg() == _lib.CHROM_RG and _lib.CHROM_RG in (16, 32, 64)
    assert _chrom.KEYS == ("chrom_log10_A", "chrom_gamma")
    assert _chrom.FIELD == {"chrom_log10_A": cr.FIELD_LOG10_A, "chrom_gamma": cr.FIELD_GAMMA} == {"chrom_log10_A": 6, "chrom_gamma": 7}
    taken = {0, _hyper.SPEC_FIELD, _hyper.CLM_FIELD, *_wn_hyper.FIELD.values()}
    assert taken == {0, 1, 2, 3, 4, 5} and not taken & set(_chrom.FIELD.values())
    assert not set(_chrom.KEYS) & set(_hyper.ALL_KEYS)   # _hyper's key list stays as it is


# ---------------------------------------------------------------- device formulas on the host -------------------------
def test_coefficients_stream_mapping_and_amplitude_rule(ch):
    """coefficient c of pulsar a = amp(c) z_c with z_c = branch c & 1 of pair c >> 1 of stream (10, a), philox_ref's; amp the configured
    table without theta or at a NaN amplitude, else the prior of (log10_A, gamma) at the column's frequency"""
    seed, r, K = 0x0123456789ABCDEF, 2 ** 32 + 5, 14
    rng = np.random.default_rng(1)
    tdb = [np.sort(rng.uniform(53000, 57000, 50)) * 86400.0 for _ in range(P)]
    f = np.stack([cr.frequencies(t, K // 2)[0] for t in tdb])
    tspan = np.array([cr.frequencies(t, K // 2)[1] for t in tdb])
    amp = np.stack([np.sqrt(cr.prior(tdb[a], K // 2, -13.5 - 0.1 * a, 2.0 + a)) for a in range(P)])
    for a in range(P):
        z_ref = cr.draws(seed, r, a, K // 2)
        for theta, lA, g, want_amp in ((0, 0.0, 0.0, amp[a]), (1, np.nan, 3.0, amp[a]), (1, -14.2, 3.7, np.sqrt(cr.prior(tdb[a], K // 2, -14.2, 3.7)))):
            coef, z = np.zeros(K), np.zeros(K)
            ch.ch_coef(seed, r, a, K, _p(amp), _p(f), _p(tspan), theta, lA, g, _p(coef), _p(z))
            assert np.max(np.abs(z - z_ref)) < 1e-13          # the bound the other streams' twins are held to
            want = want_amp * z
            assert np.all(np.abs(coef - want) <= 8 * np.spacing(np.abs(want))), (a, theta)   # two pows and a sqrt against NumPy's
            if not theta or np.isnan(lA):
                assert np.array_equal(coef, want)
    z0, z1 = cr.draws(seed, r, 0, K // 2), cr.draws(seed, r, 1, K // 2)
    rn = np.empty(K)
    rn[0::2], rn[1::2] = philox_ref.normal_pairs(seed, r, philox_ref.stream_id(philox_ref.STREAM_RN, 0), K // 2)
    assert not np.array_equal(z0, z1) and not np.array_equal(z0, rn)   # a stream of its own, per pulsar


def test_prior_map_matches_philox_ref(ch):
    """label[r, a] = fma(hi_a - lo_a, u2, lo_a) of pair a of stream (7, 6) and (7, 7): the uniforms bit-equal to philox_ref's"""
    from pta_replicator_amd import _chrom
    seed, r0, R, n = 0x0123456789ABCDEF, 77, 5, 11
    lo, hi = np.linspace(-15, -14, n), np.linspace(-13.5, -13, n)
    seen = []
    for key, field in _chrom.FIELD.items():
        unit, out = np.zeros(R * n), np.zeros(R * n)
        ch.ch_draw_field(seed, r0, R, n, field, _p(np.zeros(n)), _p(np.ones(n)), _p(unit))
        ch.ch_draw_field(seed, r0, R, n, field, _p(lo), _p(hi), _p(out))
        unit, out = unit.reshape(R, n), out.reshape(R, n)
        for r in range(R):
            _, u2 = philox_ref.uniform_pairs(seed, r0 + r, philox_ref.stream_id(7, field), n)
            assert np.array_equal(unit[r], np.asarray(u2, dtype=np.float64)), (key, r)
        ref = cr.prior_labels(seed, r0, R, field, lo, hi)
        assert np.all(np.abs(out - ref) <= np.spacing(np.abs(ref))) and np.all(out >= lo) and np.all(out <= hi)
        seen.append(unit)
    assert not np.array_equal(seen[0], seen[1])
    for other in (3, 4, 5):   # and not the white-noise fields'
        u = np.zeros(R * n)
        ch.ch_draw_field(seed, r0, R, n, other, _p(np.zeros(n)), _p(np.ones(n)), _p(u))
        assert not np.array_equal(u.reshape(R, n), seen[0]) and not np.array_equal(u.reshape(R, n), seen[1])


# ---------------------------------------------------------------- configuration and theta ----------------------------
def test_configuration():
    from pta_replicator_amd import _chrom
    eng = _engine()
    assert eng._chrom == dict(A=CH_A, g=CH_G, components=7, index=2.0, ref=1400.0) and not eng._prepared
    lA, g = _chrom.configured(eng._chrom)
    assert np.array_equal(np.isnan(lA), [False, True, False, False]) and np.array_equal(np.isnan(g), np.isnan(lA))
    eng.set_chromatic_noise(-13.0, 3.0, components=1, index=4.0, ref_freq_mhz=1000.0)
    assert eng._chrom["A"] == [-13.0] * P and eng._chrom["index"] == 4.0 and eng._chrom["ref"] == 1000.0
    for kw in (dict(components=0), dict(components=2.5), dict(components=True), dict(index=np.nan), dict(ref_freq_mhz=0.0), dict(ref_freq_mhz=np.inf)):
        with pytest.raises(ValueError, match="set_chromatic_noise"):
            eng.set_chromatic_noise(-13.0, 3.0, **kw)
    with pytest.raises(ValueError, match="one entry per pulsar"):
        eng.set_chromatic_noise([-13.0, -14.0], 3.0)
    t = _engine()._chrom_host_tables()
    assert t["K"] == 14 and t["w"].shape == (eng.n_toa,) and np.all(t["amp_host"][1] == 0) and np.all(t["amp_host"][0] > 0)


def test_theta_parts_carries_the_keys_in_the_second_member():
    eng = _engine()
    R = 3
    th = dict(chrom_log10_A=np.full((R, P), -13.5), chrom_gamma=np.full((R, P), 3.0))
    hyper, det = eng._theta_parts(th, R)
    assert hyper is None and set(det) == set(th)
    both = dict(th, rn_log10_A=np.full((R, P), -14.0), wn_efac=np.ones((R, P)), gwb_gamma=np.full(R, 4.0))
    hyper, det = eng._theta_parts(both, R)
    assert set(hyper) == {"rn_log10_A", "gwb_gamma"} and set(det) == set(th) | {"wn_efac"}
    nan = dict(chrom_log10_A=np.full((R, P), np.nan), chrom_gamma=np.full((R, P), np.nan))   # all as configured: NaN indices are unused
    assert set(eng._theta_parts(nan, R)[1]) == set(th)
    assert set(eng._theta_parts({"chrom_gamma": np.array([[2.0, np.nan, 2.0, 2.0]] * R)}, R)[1]) == {"chrom_gamma"}   # NaN where no process


def test_theta_validation():
    eng = _engine()
    R = 3
    ok = np.full((R, P), -13.5)
    for th, msg in (({"chrom_log10_A": np.full((R, P + 1), -13.5)}, "shape"),
                    ({"chrom_gamma": np.full((R,), 3.0)}, "shape"),
                    ({"chrom_log10_A": np.where(np.arange(P) == 2, np.inf, ok)}, "infinite values"),
                    ({"chrom_log10_A": ok, "chrom_gamma": np.where(np.arange(P) == 0, np.nan, 3.0 + 0 * ok)}, "non-finite values where the amplitude is sampled"),
                    ({"chrom_gamma": np.where(np.arange(P) == 0, np.nan, 3.0 + 0 * ok)}, "non-finite values where the amplitude is sampled"),
                    ({"chrom_log10_A": ok, "chrom_gamma": np.full((R, P), np.inf)}, "non-finite"),
                    ({"chrom_log10_A": "x"}, "expected an array")):
        with pytest.raises(ValueError, match=msg):
            eng._theta_parts(th, R)


# ---------------------------------------------------------------- refusals, before any launch -------------------------
def test_refusals_before_any_launch():
    """on a configured, unprepared engine: each is a ValueError that names the reason, and the engine is still unprepared"""
    eng, plain = _engine(), _engine(chrom=False)
    R = 3
    th = dict(chrom_log10_A=np.full((R, P), -13.5), chrom_gamma=np.full((R, P), 3.0))
    td = "chromatic process.*no TD mode"
    for call in (lambda: eng.prepare_td(), lambda: eng.generate_td(R), lambda: eng.generate_os(R, td=True),
                 lambda: eng.generate_lnl(R, {"gwb_log10_A": np.array([-14.5])}, td=True), lambda: eng.generate_f_statistic(R, td=True),
                 lambda: eng.generate_bwm_statistic(R, td=True), lambda: eng._theta_parts({"cw_log10_h": np.zeros(R)}, R, td=True)):
        with pytest.raises(ValueError, match=td):
            call()
    for call in (lambda: plain.generate(R, theta=th), lambda: plain.generate_per_signal(R, theta={"chrom_gamma": th["chrom_gamma"]}),
                 lambda: plain._theta_parts(th, R)):
        with pytest.raises(ValueError, match="no chromatic process is configured"):
            call()
    with pytest.raises(ValueError, match="no chromatic process is configured"):
        plain.set_hyper_prior(chrom_log10_A=(-15, -13)).generate_sampled(R)
    nm = "cannot be part of a statistic's noise model"
    for e in (eng, plain):
        with pytest.raises(ValueError, match=nm):
            e.optimal_statistic(None, theta=th)
        with pytest.raises(ValueError, match=nm):
            e.generate_os(R, theta=th, matched=True)
        with pytest.raises(ValueError, match=nm):
            e.log_likelihood(None, {"chrom_log10_A": np.full((2, P), -13.5)})
        with pytest.raises(ValueError, match=nm):
            e.generate_lnl(R, {"chrom_gamma": np.full((2, P), 3.0)})
    from pta_replicator_amd import _hyper
    with pytest.raises(ValueError, match=nm):
        _hyper.check_theta_os(th, R, P, eng._rn, True)
    with pytest.raises(ValueError, match=r"prepare_optimal_statistic\(matched=True\).*chromatic process"):
        eng.prepare_optimal_statistic(matched=True)
    with pytest.raises(ValueError, match="prepare_likelihood.*chromatic process"):
        eng.prepare_likelihood()
    for bad in (dict(chrom_log10_A=(-13, -15)), dict(chrom_gamma=np.zeros((P + 1, 2))), dict(chrom_gamma=(1.0, np.inf))):
        with pytest.raises(ValueError, match="set_hyper_prior"):
            eng.set_hyper_prior(**bad)
    assert not eng._prepared and not plain._prepared and eng._chrom_t is None


def test_list_api_refuses_bad_frequencies_before_drawing():
    import re
    from pta_replicator_amd.red_noise import add_chromatic_noise
    psrs = _psrs()
    psrs[2].toas.freqs_mhz[3] = -820.0
    np.random.seed(9)
    state = np.random.get_state()[1].copy()
    with pytest.raises(ValueError, match=re.escape(str(psrs[2].name))):
        add_chromatic_noise(psrs[2], -13.5, 3.0, seed=4)
    with pytest.raises(ValueError, match=re.escape(str(psrs[2].name))):
        add_chromatic_noise(psrs, -13.5, 3.0)
    with pytest.raises(ValueError, match="add_chromatic_noise"):
        add_chromatic_noise(psrs[0], -13.5, 3.0, ref_freq_mhz=-1.0)
    assert np.array_equal(np.random.get_state()[1], state) and not any(p.added_signals for p in psrs)


# ---------------------------------------------------------------- the fixed-noise statistics' columns ----------------
def test_low_rank_columns_against_the_reference_module():
    """what the shared front hands to the plan builders for the chromatic process: w . F_chrom and phi_chrom, per pulsar"""
    eng = _engine(components=7)
    F, phi = eng._chrom_low_rank_host()
    assert len(F) == len(phi) == P
    for a in range(P):
        tdb = eng.tdb_s[a]
        want = cr.weights(eng.psrs[a].toas.freqs_mhz)[:, None] * cr.basis(tdb, 7)
        assert F[a].shape == (len(tdb), 14) and np.array_equal(F[a], want)
        if CH_A[a] is None:
            assert np.all(phi[a] == 0)
        else:
            want = cr.prior(tdb, 7, CH_A[a], CH_G[a])
            assert np.all(np.abs(phi[a] - want) <= 4 * np.spacing(want))
    assert not eng._prepared
