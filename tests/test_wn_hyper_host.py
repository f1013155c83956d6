"""CPU checks of the per-realisation white noise: the __host__ __device__ formulas of csrc/pta_wn_hyper.h compiled with g++
(tests/wn_hyper/wn_hyper_host.cpp) against NumPy and a long-double evaluation, the prior map of fields 3 - 5 against philox_ref, and
the groups, refusals and prior validation on an engine that is configured but not prepared (no GPU needed: every refusal happens
before anything is launched)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from helpers import load, mjd_ld
from oracle import philox_ref

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def wh(tmp_path_factory):
    out = tmp_path_factory.mktemp("wn_hyper") / "libwnhyperhost.so"
    src = os.path.join(HERE, "wn_hyper", "wn_hyper_host.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", str(out)])
    lib = ctypes.CDLL(str(out))
    i, u64, p = ctypes.c_int, ctypes.c_uint64, ctypes.POINTER(ctypes.c_double)
    lib.wh_amplitudes.argtypes = [i, p, p, p, p, i, p, p]
    lib.wh_ecorr.argtypes = [i, p, p, p]
    lib.wh_element.argtypes = [i, p, i, p, p, p, p, p, i, p, p, p]
    lib.wh_draw_field.argtypes = [u64, u64, i, i, i, p, p, p]
    return lib


def _p(a):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _ulps(got, want):
    return np.abs(got - want) / np.spacing(np.abs(want))


def _amplitudes(wh, efac, l10, efac_conf, equad_conf, tnequad):
    ea, eb = np.full(len(efac), np.nan), np.full(len(efac), np.nan)
    wh.wh_amplitudes(len(efac), _p(efac), _p(l10), _p(efac_conf), _p(equad_conf), int(tnequad), _p(ea), _p(eb))
    return ea, eb


def test_constants_agree():
    from pta_replicator_amd import _lib, _wn_hyper
    header = open(os.path.join(os.path.dirname(HERE), "include", "pta_replicator_amd.h")).read()
    assert "#define PTA_WN_HYPER_GMAX 16" in header
    assert _wn_hyper.GMAX == _lib.WN_HYPER_GMAX == 16
    assert _wn_hyper.KEYS == ("wn_efac", "wn_log10_equad", "wn_log10_ecorr")
    assert _wn_hyper.FIELD == {"wn_efac": 3, "wn_log10_equad": 4, "wn_log10_ecorr": 5}


def test_amplitudes_against_numpy(wh):
    """ea = efac exactly; eb = efac 10^x (or 10^x with tnequad) and ec = 10^x with 10^x within 4 ulp of NumPy's 10 ** x (one more
    rounding for the product)"""
    assert wh.wh_gmax() == 16
    rng = np.random.default_rng(1)
    n = 4000
    efac, l10 = rng.uniform(0.1, 5.0, n), rng.uniform(-9.0, -4.0, n)
    conf = np.full(n, 123.0)
    for tnequad in (False, True):
        ea, eb = _amplitudes(wh, efac, l10, conf, conf, tnequad)
        assert np.array_equal(ea, efac)
        p10 = 10 ** l10
        if tnequad:
            assert _ulps(eb, p10).max() <= 4
        else:
            # eb = fl(efac * p) with p within 4 ulp of p10: within 4 ulp + the two roundings of either product
            assert _ulps(eb, efac * p10).max() <= 4 + 2
            assert np.all(np.abs(eb / efac - p10) <= 5 * np.spacing(p10))
    ec = np.full(n, np.nan)
    wh.wh_ecorr(n, _p(l10), _p(conf), _p(ec))
    assert _ulps(ec, 10 ** l10).max() <= 4


def test_nan_rule_and_tnequad(wh):
    """a NaN label takes the configured value - efac as given, equad / ecorr in seconds as prepare() computed them - bit for bit, per
    parameter; tnequad decides whether efac multiplies equad"""
    nan = np.nan
    efac = np.array([nan, 1.7, nan, 1.7])
    l10 = np.array([nan, nan, -6.0, -6.0])
    efac_conf, equad_conf = np.full(4, 1.1), np.full(4, 10 ** -6.5)
    ea, eb = _amplitudes(wh, efac, l10, efac_conf, equad_conf, False)
    assert np.array_equal(ea, [1.1, 1.7, 1.1, 1.7])
    assert eb[0] == 1.1 * 10 ** -6.5 and eb[1] == 1.7 * 10 ** -6.5          # the fixed engine's ev * qv
    assert abs(eb[2] - 1.1e-6) <= 4 * np.spacing(1.1e-6) and abs(eb[3] - 1.7e-6) <= 4 * np.spacing(1.7e-6)
    ea, eb = _amplitudes(wh, efac, l10, efac_conf, equad_conf, True)
    assert np.array_equal(ea, [1.1, 1.7, 1.1, 1.7])
    assert eb[0] == eb[1] == 10 ** -6.5 and eb[2] == eb[3] and abs(eb[2] - 1e-6) <= 4 * np.spacing(1e-6)
    # a group configured without EQUAD (0 s): none as configured, the label's when it has one
    ea, eb = _amplitudes(wh, np.array([nan, nan]), np.array([nan, -6.0]), np.full(2, 0.9), np.zeros(2), False)
    assert eb[0] == 0.0 and abs(eb[1] - 0.9e-6) <= 4 * np.spacing(0.9e-6)
    ec = np.full(2, nan)
    wh.wh_ecorr(2, _p(np.array([nan, -7.0])), _p(np.full(2, 10 ** -6.6)), _p(ec))
    assert ec[0] == 10 ** -6.6 and abs(ec[1] - 1e-7) <= 4 * np.spacing(1e-7)


def test_element_against_long_double(wh):
    """(o + (ea sigma z1 + eb z2)) + ec z_e: five roundings of the products and sums, each at most half an ulp of a partial result that
    the sum of the absolute terms bounds - |delta| <= 4 * 2^-53 * sum |terms| with room to spare; a term that is switched off is left out;
    o = 0 gives the terms alone"""
    rng = np.random.default_rng(2)
    n = 5000
    o = rng.normal(0, 1e-6, n)
    ea, sigma, z1, z2, ze = rng.uniform(0.5, 2, n), rng.uniform(1e-7, 1e-6, n), rng.normal(size=n), rng.normal(size=n), rng.normal(size=n)
    eb, ec = rng.uniform(1e-8, 1e-6, n), rng.uniform(1e-8, 1e-6, n)
    ld = np.longdouble
    for has_wn, has_ec in ((1, 1), (1, 0), (0, 1)):
        out = np.full(n, np.nan)
        wh.wh_element(n, _p(o), has_wn, _p(ea), _p(sigma), _p(z1), _p(eb), _p(z2), has_ec, _p(ec), _p(ze), _p(out))
        t = [o.astype(ld)]
        if has_wn:
            t += [ea.astype(ld) * sigma * z1, eb.astype(ld) * z2]
        if has_ec:
            t += [ec.astype(ld) * ze]
        ref, scale = sum(t), sum(np.abs(x) for x in t)
        assert np.all(np.abs(out - ref) <= 4 * 2.0 ** -53 * scale)
        # the order of the operations, bit for bit
        v = o.copy()
        if has_wn:
            v = v + ((ea * sigma) * z1 + eb * z2)
        if has_ec:
            v = v + ec * ze
        assert np.array_equal(out, v)
    out = np.full(n, np.nan)
    zero = np.zeros(n)
    wh.wh_element(n, _p(zero), 1, _p(ea), _p(sigma), _p(z1), _p(eb), _p(z2), 0, _p(ec), _p(ze), _p(out))
    assert np.array_equal(out, (ea * sigma) * z1 + eb * z2)
    two = np.full(n, np.nan)   # efac doubled with tnequad off doubles both amplitudes: the term doubles exactly
    wh.wh_element(n, _p(zero), 1, _p(2 * ea), _p(sigma), _p(z1), _p(2 * eb), _p(z2), 0, _p(ec), _p(ze), _p(two))
    assert np.array_equal(two, 2 * out)
    wh.wh_element(n, _p(zero), 1, _p(zero), _p(sigma), _p(z1), _p(zero), _p(z2), 1, _p(zero), _p(ze), _p(out))
    assert np.all(out == 0.0)   # a TOA in no group


def test_prior_map_matches_philox_ref(wh):
    """label[r, j] = fma(hi_j - lo_j, u2, lo_j) of pair j of stream (7, field), fields 3 - 5: the uniforms bit-equal to philox_ref's"""
    from pta_replicator_amd import _wn_hyper
    from pta_replicator_amd.engine import STREAM_HYPER, stream_id
    seed, r0, R, n = 0x0123456789ABCDEF, 77, 5, 11
    lo, hi = np.linspace(-8, -7, n), np.linspace(-6.5, -6, n)
    seen = []
    for key, field in _wn_hyper.FIELD.items():
        unit, out = np.zeros(R * n), np.zeros(R * n)
        wh.wh_draw_field(seed, r0, R, n, field, _p(np.zeros(n)), _p(np.ones(n)), _p(unit))
        wh.wh_draw_field(seed, r0, R, n, field, _p(lo), _p(hi), _p(out))
        unit, out = unit.reshape(R, n), out.reshape(R, n)
        for r in range(R):
            _, u2 = philox_ref.uniform_pairs(seed, r0 + r, stream_id(STREAM_HYPER, field), n)
            assert np.array_equal(unit[r], np.asarray(u2, dtype=np.float64)), (key, r)
            ref = lo + (hi - lo) * u2
            assert np.all(np.abs(out[r] - ref) <= np.spacing(np.abs(ref))) and np.all(out[r] >= lo) and np.all(out[r] <= hi)
        seen.append(unit)
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])


# ---------------------------------------------------------------- validation (no GPU) -------------------------------
P = 4
FLAGS = ("A", "B", "C")   # two backends, and a third flag that is in no group


def _engine(wn=True, ec=True, flags=True, ecorr_none=1, **kw):
    from pta_replicator_amd.engine import ReplicaEngine
    from pta_replicator_amd.simulate import ArrayTOAs, SimulatedPulsar, make_ideal
    z = load("c3_mini.npz")
    psrs = []
    for i in range(P):
        mjd = mjd_ld(z, "", i)
        p = SimulatedPulsar(toas=ArrayTOAs(mjd, z[f"err_us_{i}"], flags=[{"f": FLAGS[k % 3]} for k in range(len(mjd))]), name=str(z["names"][i]),
                            loc={"RAJ": float(z["raj_hours"][i]), "DECJ": float(z["decj_deg"][i])})
        make_ideal(p)
        psrs.append(p)
    eng = ReplicaEngine(psrs, seed=5)
    fl = [["A", "B"]] * P if flags else None
    if wn:
        if flags:
            eng.set_white_noise(efac=[np.array([1.1, 0.9])] * P, log10_equad=[np.array([-6.5, -6.8])] * P, flags=fl, **kw)
        else:
            eng.set_white_noise(efac=1.1, log10_equad=-6.5, **kw)
    if ec:
        l10 = [None if a == ecorr_none else (np.array([-6.6, -6.9]) if flags else -6.6) for a in range(P)]
        eng.set_jitter(log10_ecorr=l10, flags=fl)
    eng.set_red_noise([-14.0, None, -13.5, -14.2], [3.0, None, 2.5, 4.0], components=10)
    eng.set_gwb(-14.5, 13. / 3.)
    return eng


def test_group_lists():
    eng = _engine()
    assert eng.wn_groups == [(a, f) for a in range(P) for f in ("A", "B")]
    assert eng.ecorr_groups == [(a, f) for a in range(P) if a != 1 for f in ("A", "B")]
    eng = _engine(flags=False)
    assert eng.wn_groups == [(a, None) for a in range(P)]
    assert eng.ecorr_groups == [(a, None) for a in range(P) if a != 1]
    eng = _engine(wn=False, ec=False)
    assert eng.wn_groups == [] and eng.ecorr_groups == []
    assert not eng._prepared


def test_configured_values_and_toa_groups():
    from pta_replicator_amd import _wn_hyper
    eng = _engine()
    efac, equad = _wn_hyper.configured_wn(P, eng._wn)
    assert np.array_equal(efac, [1.1, 0.9] * P) and np.array_equal(equad, [10 ** -6.5, 10 ** -6.8] * P)
    assert np.array_equal(_wn_hyper.configured_ecorr(P, eng._ec), [10 ** -6.6, 10 ** -6.9] * (P - 1))
    assert np.array_equal(_wn_hyper.psr_offsets(P, eng.wn_groups), [0, 2, 4, 6, 8])
    assert np.array_equal(_wn_hyper.psr_offsets(P, eng.ecorr_groups), [0, 2, 2, 4, 6])
    flags = np.array(["A", "B", "C", "A", "C"])
    assert np.array_equal(_wn_hyper.toa_groups(eng.wn_groups, 2, flags), [4, 5, -1, 4, -1])      # "C" is in no group
    assert np.array_equal(_wn_hyper.toa_groups(eng.ecorr_groups, 2, flags), [2, 3, -1, 2, -1])
    assert np.array_equal(_wn_hyper.toa_groups(eng.ecorr_groups, 1, flags), [-1] * 5)            # the pulsar without ECORR
    assert np.array_equal(_wn_hyper.toa_groups(_engine(flags=False).wn_groups, 3, flags), [3] * 5)
    eng = _engine(flags=False)
    eng.set_white_noise(efac=1.1)     # no EQUAD configured: 0 s
    assert np.array_equal(_wn_hyper.configured_wn(P, eng._wn)[1], np.zeros(P))


def _theta(R, G_wn=2 * P, G_ec=2 * (P - 1)):
    return {"wn_efac": np.full((R, G_wn), 1.2), "wn_log10_equad": np.full((R, G_wn), -6.3), "wn_log10_ecorr": np.full((R, G_ec), -6.4)}


def test_theta_parts_carries_the_keys_in_the_second_member():
    from pta_replicator_amd import _bwm, _cw, _wn_hyper
    R = 3
    eng = _engine()
    th = _theta(R)
    th["wn_efac"][1, 2] = np.nan          # NaN = as configured
    hyper, det = eng._theta_parts(th, R)
    assert hyper is None and set(det) == set(_wn_hyper.KEYS)
    assert _wn_hyper.has_keys(det) and _wn_hyper.has_wn(det) and _wn_hyper.has_ecorr(det)
    assert not _cw.has_keys(det) and not _bwm.has_keys(det) and _cw.n_sources(det) == 0
    hyper, det = eng._theta_parts({"wn_log10_equad": th["wn_log10_equad"], "gwb_log10_A": np.full(R, -14.0)}, R)
    assert set(hyper) == {"gwb_log10_A"} and set(det) == {"wn_log10_equad"}
    assert _wn_hyper.has_wn(det) and not _wn_hyper.has_ecorr(det)
    assert eng._theta_parts({"gwb_log10_A": np.full(R, -14.0)}, R)[1] == {}
    assert not eng._prepared


def test_refusals_before_any_launch():
    import torch
    R = 3
    eng = _engine()
    ok = _theta(R)
    cases = [
        (dict(ok, wn_efac=np.ones((R, 2 * P + 1))), "shape"),
        (dict(ok, wn_efac=np.ones((R + 1, 2 * P))), "shape"),
        (dict(ok, wn_log10_equad=np.ones(R)), "shape"),
        (dict(ok, wn_log10_ecorr=np.ones((R, 2 * P))), "shape"),                 # the pulsar without ECORR has no group
        (dict(ok, wn_efac=torch.ones((R, 3), dtype=torch.float64)), "shape"),
        ({"wn_efac": np.where(np.arange(2 * P) == 3, np.inf, np.ones((R, 2 * P)))}, "infinite"),
        ({"wn_log10_equad": np.where(np.arange(2 * P) == 0, -np.inf, np.ones((R, 2 * P)))}, "infinite"),
        ({"wn_log10_ecorr": torch.full((R, 2 * (P - 1)), float("inf"), dtype=torch.float64)}, "infinite"),
    ]
    for theta, msg in cases:
        for call in (eng.generate, eng.generate_per_signal):
            with pytest.raises(ValueError, match=msg):
                call(R, theta=theta)
    # TD mode names the keys
    for theta in (ok, {"wn_log10_ecorr": ok["wn_log10_ecorr"]}):
        with pytest.raises(ValueError, match=r"TD mode.*wn_log10_ecorr"):
            eng.generate_td(R, theta=theta)
    # not configured
    with pytest.raises(ValueError, match=r"no white noise is configured \(set_white_noise\)"):
        _engine(wn=False).generate(R, theta={"wn_efac": ok["wn_efac"]})
    with pytest.raises(ValueError, match=r"no white noise is configured \(set_white_noise\)"):
        _engine(wn=False).generate(R, theta={"wn_log10_equad": ok["wn_log10_equad"]})
    with pytest.raises(ValueError, match=r"no ECORR is configured \(set_jitter\)"):
        _engine(ec=False).generate(R, theta={"wn_log10_ecorr": ok["wn_log10_ecorr"]})
    # wn_mode "single"
    single = _engine()
    single.wn_mode = "single"
    for k in ok:
        with pytest.raises(ValueError, match="wn_mode='reference'"):
            single.generate(R, theta={k: ok[k]})
    # more groups on one pulsar than the add kernel stages
    many = _engine()
    names = [f"b{j}" for j in range(17)]
    many.set_white_noise(efac=[np.ones(17)] * P, log10_equad=[np.full(17, -7.0)] * P, flags=[names] * P)
    with pytest.raises(ValueError, match="at most 16 per pulsar"):
        many.generate(R, theta={"wn_efac": np.ones((R, 17 * P))})
    # unknown keys are still _hyper's to name, with its message
    with pytest.raises(ValueError, match=r"unknown keys \['wn_equad'\]"):
        eng.generate(R, theta={"wn_equad": np.ones((R, 2 * P))})
    assert not eng._prepared and not single._prepared and not many._prepared


def test_noise_model_theta_refuses_the_keys_with_a_reason():
    """optimal_statistic(theta=), matched=True and the likelihood grids validate their noise model through _hyper.check_theta_os"""
    from pta_replicator_amd import _hyper
    R = 3
    eng = _engine()
    for k, v in _theta(R).items():
        with pytest.raises(ValueError, match=rf"\['{k}'\] cannot be part of a statistic's noise model.*hold the white noise fixed"):
            _hyper.check_theta_os({k: v, "rn_gamma": np.full((R, P), 3.0)}, R, P, eng._rn, True, gw=eng._gw)
        with pytest.raises(ValueError, match="hold the white noise fixed"):
            _hyper.check_theta_os({k: v}, R, P, eng._rn, True)          # the likelihood grid's call
    with pytest.raises(ValueError, match=r"unknown keys \['wn_equad'\]"):
        _hyper.check_theta_os({"wn_equad": np.ones((R, 2 * P))}, R, P, eng._rn, True)
    assert _hyper.ALL_KEYS == ("gwb_log10_A", "gwb_gamma", "rn_log10_A", "rn_gamma", "gwb_log10_hc", "gwb_clm")


def test_set_hyper_prior_validation():
    from pta_replicator_amd import _wn_hyper
    eng = _engine()
    G_wn, G_ec = 2 * P, 2 * (P - 1)
    with pytest.raises(ValueError, match=r"wn_efac must be \(lo, hi\) or \[8, 2\]"):
        eng.set_hyper_prior(wn_efac=(0.5, 1.0, 2.0))
    with pytest.raises(ValueError, match=r"wn_log10_ecorr must be \(lo, hi\) or \[6, 2\]"):
        eng.set_hyper_prior(wn_log10_ecorr=np.zeros((G_wn, 2)))
    with pytest.raises(ValueError, match="lo <= hi"):
        eng.set_hyper_prior(wn_log10_equad=(-6, -7))
    with pytest.raises(ValueError, match="lo <= hi"):
        eng.set_hyper_prior(wn_efac=(0.5, np.inf))
    with pytest.raises(ValueError, match="set_jitter"):
        _engine(ec=False).set_hyper_prior(wn_log10_ecorr=(-7, -6))
    with pytest.raises(ValueError, match="set_white_noise"):
        _engine(wn=False).set_hyper_prior(wn_efac=(0.5, 2))
    with pytest.raises(ValueError, match="no parameter given"):
        eng.set_hyper_prior()
    with pytest.raises(ValueError, match="no prior"):
        eng.generate_sampled(2)
    box = np.stack([np.linspace(-8, -7, G_ec), np.linspace(-6.5, -6, G_ec)], axis=1)
    assert eng.set_hyper_prior(wn_efac=(0.5, 2), wn_log10_ecorr=box) is eng
    assert eng._prior is None and set(eng._wn_prior) == {"wn_efac", "wn_log10_ecorr"}
    assert np.array_equal(eng._wn_prior["wn_efac"][0], np.full(G_wn, 0.5)) and np.array_equal(eng._wn_prior["wn_log10_ecorr"][1], box[:, 1])
    eng.set_hyper_prior(gwb_gamma=(3, 5), wn_log10_equad=(-7, -6))
    assert set(eng._prior) == {"gwb_gamma"} and set(eng._wn_prior) == {"wn_log10_equad"}
    eng.set_hyper_prior(gwb_gamma=(3, 5))
    assert eng._wn_prior is None
    # a prior whose keys the configuration cannot honour is refused by generate_sampled before anything is launched
    eng.set_hyper_prior(wn_efac=(0.5, 2))
    eng.wn_mode = "single"
    with pytest.raises(ValueError, match="wn_mode='reference'"):
        eng.generate_sampled(2)
    assert _wn_hyper.make_prior(G_wn, G_ec) == {}
    assert not eng._prepared
