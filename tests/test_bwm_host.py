"""CPU checks of the per-realisation burst with memory: the __host__ __device__ formulas of csrc/pta_bwm.h compiled with g++
(tests/bwm/bwm_host.cpp) against the reference's golden add_gw_memory output and a long-double evaluation of its expression, the
label draw map against philox_ref, and the validation of set_bwm / set_bwm_prior / theta on an engine that is configured but not
prepared (no GPU needed: every refusal happens before anything is launched)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from helpers import load, mjd_ld
from oracle import philox_ref

HERE = os.path.dirname(os.path.abspath(__file__))
# the golden burst (oracle/gen_golden.py: add_gw_memory(p, 3e-14, 0.7, 5.1, 0.9, 55500.0))
STRAIN, GWTHETA, GWPHI, POL, T0_MJD = 3e-14, 0.7, 5.1, 0.9, 55500.0
SRC = np.array([np.cos(GWTHETA), GWPHI, np.log10(STRAIN), POL, T0_MJD])


@pytest.fixture(scope="module")
def bh(tmp_path_factory):
    out = tmp_path_factory.mktemp("bwm") / "libbwmhost.so"
    src = os.path.join(HERE, "bwm", "bwm_host.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", str(out)])
    lib = ctypes.CDLL(str(out))
    d, i, u64, p = ctypes.c_double, ctypes.c_int, ctypes.c_uint64, ctypes.POINTER(ctypes.c_double)
    lib.bh_uniform.argtypes = [u64, u64, i, p, p, p]
    lib.bh_params.argtypes = [p, p, p, p]
    lib.bh_ramp.argtypes = [d, d, p, i, p]
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _golden_pulsars():
    """[(toa_s float64, phat)] of the three pulsars of transients.npz, TOAs as the engine holds them (float64 MJD * 86400)"""
    from pta_replicator_amd import _cw
    z = load("transients.npz")
    out = []
    for a in range(3):
        mjd = np.asarray(mjd_ld(z, "", a), dtype=np.float64)
        ra, dec = float(z["raj_hours"][a]) * np.pi / 12, float(z["decj_deg"][a]) * np.pi / 180
        out.append((mjd * 86400, np.ascontiguousarray(_cw.pulsar_vectors([(ra, dec)])[0]), ra, dec))
    return z, out


def _host_term(bh, src, phat, toa_s):
    coef, t0 = ctypes.c_double(), ctypes.c_double()
    bh.bh_params(_p(np.ascontiguousarray(src)), _p(phat), ctypes.byref(coef), ctypes.byref(t0))
    out = np.full(len(toa_s), np.nan)
    bh.bh_ramp(coef.value, t0.value, _p(np.ascontiguousarray(toa_s)), len(toa_s), _p(out))
    return out, coef.value, t0.value


def _relrms(dev, ref):
    return float(np.sqrt(np.mean((dev - ref) ** 2)) / np.sqrt(np.mean(ref ** 2)))


def _reference_ld(toa_s, ra, dec, strain, gwtheta, gwphi, pol, t0_mjd):
    """the reference's expression (deterministic.py:834-872) in long double"""
    ld = np.longdouble
    gwtheta, gwphi, pol = ld(gwtheta), ld(gwphi), ld(pol)
    ct, cp, st, sp = np.cos(gwtheta), np.cos(gwphi), np.sin(gwtheta), np.sin(gwphi)
    m = np.array([sp, -cp, ld(0)])
    n = np.array([-ct * cp, -ct * sp, st])
    om = np.array([-st * cp, -st * sp, -ct])
    ptheta, pphi = ld(np.pi / 2 - dec), ld(ra)
    phat = np.array([np.sin(ptheta) * np.cos(pphi), np.sin(ptheta) * np.sin(pphi), np.cos(ptheta)])
    fplus = ld(0.5) * (np.dot(m, phat) ** 2 - np.dot(n, phat) ** 2) / (1 + np.dot(om, phat))
    fcross = (np.dot(m, phat) * np.dot(n, phat)) / (1 + np.dot(om, phat))
    p = np.cos(2 * pol) * fplus + np.sin(2 * pol) * fcross
    t = np.asarray(toa_s, dtype=ld)
    t0 = ld(t0_mjd) * 86400
    return np.where(t < t0, ld(0), p * ld(strain) * (t - t0))


def test_stream_kind_and_columns(bh):
    from pta_replicator_amd import _bwm
    from pta_replicator_amd.engine import STREAM_BWM
    assert STREAM_BWM == 9 == bh.bh_stream_kind()
    assert _bwm.COLUMNS == ("cos_gwtheta", "gwphi", "log10_h", "psi", "t0_mjd")
    assert _bwm.KEYS == ("bwm_cos_gwtheta", "bwm_gwphi", "bwm_log10_h", "bwm_psi", "bwm_t0_mjd")


def test_term_matches_golden_add_gw_memory(bh):
    """coefficient x ramp of pta_bwm.h against the unmodified reference's add_gw_memory rows: 1e-10 relative RMS per pulsar (the
    project's parity bound), exactly 0 before the epoch."""
    z, psrs = _golden_pulsars()
    for a, (toa, phat, _, _) in enumerate(psrs):
        dev, _, t0 = _host_term(bh, SRC, phat, toa)
        before = toa < T0_MJD * 86400
        assert 0 < before.sum() < len(toa) and t0 == T0_MJD * 86400
        assert np.all(dev[before] == 0.0)
        err = _relrms(dev, z["gw_memory"][a])
        print(f"pulsar {a}: relative RMS deviation from the golden {err:.3g}")
        assert err <= 1e-10, (a, err)


def test_term_matches_long_double_reference(bh):
    """the same against a long-double evaluation of the reference's expression, with further bursts at the edges (cos = +-1, an
    epoch before / after every TOA, an epoch exactly on a TOA).  Measured: 3.8e-14 relative RMS at worst over the cases below, 1.3e-15 on
    the golden burst (the float64 inputs differ from the long-double ones: the cosine is handed over rounded, the strain goes through
    log10 and pow, the epoch is rounded to float64 seconds as the reference rounds it)."""
    _, psrs = _golden_pulsars()
    rng = np.random.default_rng(4)
    cases = [(STRAIN, GWTHETA, GWPHI, POL, T0_MJD), (1e-13, 0.0, 1.0, 0.3, 55000.0), (2e-15, np.pi, 2.0, 2.9, 55000.0)]
    cases += [(10 ** rng.uniform(-16, -12), np.arccos(rng.uniform(-1, 1)), rng.uniform(0, 2 * np.pi), rng.uniform(0, np.pi),
               rng.uniform(53500, 57000)) for _ in range(12)]
    worst = 0.0
    for h, th, ph, pol, t0 in cases:
        src = np.array([np.cos(th), ph, np.log10(h), pol, t0])
        for toa, phat, ra, dec in psrs:
            dev, _, _ = _host_term(bh, src, phat, toa)
            ref = _reference_ld(toa, ra, dec, h, th, ph, pol, t0)
            assert np.all(np.isfinite(dev)) and np.all(dev[toa < t0 * 86400] == 0.0)
            if np.any(ref != 0):
                worst = max(worst, float(np.sqrt(np.mean((dev - ref) ** 2) / np.mean(ref ** 2))))
    print(f"worst relative RMS deviation from the long-double reference: {worst:.3g}")
    assert worst <= 1e-10, worst
    # the edges of the signal definition: before every TOA (a ramp everywhere), after every TOA (0 everywhere), exactly on a TOA (0 there)
    toa, phat, _, _ = psrs[0]
    dev, coef, _ = _host_term(bh, np.array([SRC[0], SRC[1], SRC[2], SRC[3], 40000.0]), phat, toa)
    assert np.all(dev == coef * (toa - 40000.0 * 86400)) and np.all(dev != 0)
    dev, _, _ = _host_term(bh, np.array([SRC[0], SRC[1], SRC[2], SRC[3], 70000.0]), phat, toa)
    assert np.all(dev == 0.0)
    out = np.full(3, np.nan)
    bh.bh_ramp(2.0, toa[5], _p(np.ascontiguousarray(toa[4:7])), 3, _p(out))
    assert out[0] == 0.0 and out[1] == 0.0 and out[2] == 2.0 * (toa[6] - toa[5])


def test_uniform_map_matches_philox_ref(bh):
    """label[r, j] = fma(hi_j - lo_j, u2, lo_j) of pair j of stream (9, 0): the uniforms bit-equal to philox_ref's, the labels inside
    their boxes, a degenerate box giving its value."""
    from pta_replicator_amd import _bwm
    from pta_replicator_amd.engine import STREAM_BWM, stream_id
    seed, r0, R, n = 0x0123456789ABCDEF, 77, 9, _bwm.N_SRC
    unit = np.zeros(R * n)
    bh.bh_uniform(seed, r0, R, _p(np.zeros(n)), _p(np.ones(n)), _p(unit))
    unit = unit.reshape(R, n)
    prior = _bwm.make_prior(log10_h=(-15, -13), t0_mjd=(54000, 54000))
    lo, hi = _bwm.prior_bounds(prior)
    assert lo[0] == -1 and hi[0] == 1 and hi[1] == 2 * np.pi and hi[3] == np.pi and lo[2] == -15 and lo[4] == hi[4] == 54000
    out = np.zeros(R * n)
    bh.bh_uniform(seed, r0, R, _p(lo), _p(hi), _p(out))
    out = out.reshape(R, n)
    for r in range(R):
        _, u2 = philox_ref.uniform_pairs(seed, r0 + r, stream_id(STREAM_BWM, 0), n)
        assert np.array_equal(unit[r], np.asarray(u2, dtype=np.float64)), r     # fma(1, u2, 0) = u2
        ref = lo + (hi - lo) * u2
        assert np.all(np.abs(out[r] - ref) <= np.spacing(np.abs(ref))), r
        assert np.all(out[r] >= lo) and np.all(out[r] <= hi)
        assert out[r, 4] == 54000.0


# ---------------------------------------------------------------- validation (no GPU) -------------------------------
def _engine(bwm=True, cw=False):
    from pta_replicator_amd.engine import ReplicaEngine
    from pta_replicator_amd.simulate import ArrayTOAs, SimulatedPulsar, make_ideal
    z = load("c3_mini.npz")
    psrs = []
    for i in range(4):
        p = SimulatedPulsar(toas=ArrayTOAs(mjd_ld(z, "", i), z[f"err_us_{i}"]), name=str(z["names"][i]),
                            loc={"RAJ": float(z["raj_hours"][i]), "DECJ": float(z["decj_deg"][i])})
        make_ideal(p)
        psrs.append(p)
    eng = ReplicaEngine(psrs, seed=5)
    eng.set_white_noise(efac=1.1)
    eng.set_red_noise([-14.0, None, -13.5, -14.2], [3.0, None, 2.5, 4.0], components=10)
    eng.set_gwb(-14.5, 13. / 3.)
    if bwm:
        assert eng.set_bwm() is eng
    if cw:
        eng.set_cw()
    return eng


def _theta(R):
    return {"bwm_log10_h": np.full(R, -14.0), "bwm_cos_gwtheta": np.linspace(-1, 1, R), "bwm_gwphi": np.full(R, 1.0),
            "bwm_psi": np.full(R, 0.5), "bwm_t0_mjd": np.full(R, 55000.0)}


def test_bwm_theta_refusals_before_any_launch():
    import torch
    R = 3
    eng = _engine()
    ok = _theta(R)
    cases = [
        ({k: v for k, v in ok.items() if k != "bwm_gwphi"}, "bwm_gwphi"),
        ({"bwm_log10_h": ok["bwm_log10_h"]}, "missing"),
        (dict(ok, bwm_psi=np.zeros(R + 1)), "shape"),
        (dict(ok, bwm_t0_mjd=np.zeros((R, 1))), "shape"),
        (dict(ok, bwm_log10_h=torch.zeros(R + 2, dtype=torch.float64)), "shape"),
        (dict(ok, bwm_cos_gwtheta=np.array([0.0, 1.5, 0.0])), r"\|cos\|"),
        (dict(ok, bwm_cos_gwtheta=np.array([0.0, -1.0000001, 0.0])), r"\|cos\|"),
        (dict(ok, bwm_log10_h=np.array([-14.0, np.nan, -14.0])), "non-finite"),
        (dict(ok, bwm_t0_mjd=np.array([np.inf, 55000.0, 55000.0])), "non-finite"),
        (dict(ok, bwm_gwphi=torch.tensor([0.0, float("nan"), 0.0], dtype=torch.float64)), "non-finite"),
    ]
    for theta, msg in cases:
        for call in (eng.generate, eng.generate_per_signal, eng.generate_td):
            with pytest.raises(ValueError, match=msg):
                call(R, theta=theta)
    with pytest.raises(ValueError, match="shape"):
        eng.generate(R, theta=dict(ok, gwb_log10_A=np.zeros(R + 1)))
    with pytest.raises(ValueError, match=r"no per-realisation burst with memory configured \(set_bwm\)"):
        _engine(bwm=False).generate(R, theta=ok)
    with pytest.raises(ValueError, match=r"set_cw"):
        eng.generate(R, theta=dict(ok, cw_psi=np.zeros(R)))
    for extra in ({"rn_gamma": np.full((R, 4), 3.0)}, {"gwb_log10_A": np.full(R, -14.0)}):
        with pytest.raises(ValueError, match="TD mode"):
            eng.generate_td(R, theta=dict(ok, **extra))
    assert not eng._prepared


def test_theta_parts_keeps_its_pair_and_carries_the_burst_in_the_second_member():
    from pta_replicator_amd import _bwm, _cw
    R = 3
    eng = _engine(cw=True)
    hyper, det = eng._theta_parts(_theta(R), R)
    assert hyper is None and set(det) == set(_bwm.KEYS)
    assert _cw.n_sources(det) == 0 and not _cw.is_catalog(det) and not _cw.has_keys(det) and _bwm.has_keys(det)
    hyper, det = eng._theta_parts(dict(_theta(R), gwb_log10_A=np.full(R, -14.0)), R)
    assert set(hyper) == {"gwb_log10_A"} and set(det) == set(_bwm.KEYS)
    assert eng._theta_parts(None, R) == (None, {})
    hyper, det = eng._theta_parts(_theta(R), R, td=True)
    assert hyper is None and _bwm.has_keys(det)
    assert not eng._prepared


def test_set_bwm_prior_validation():
    eng = _engine(bwm=False)
    with pytest.raises(ValueError, match="log10_h is required"):
        eng.set_bwm_prior(t0_mjd=(54000, 56000))
    with pytest.raises(ValueError, match="t0_mjd is required"):
        eng.set_bwm_prior(log10_h=(-15, -13))
    with pytest.raises(ValueError, match=r"\[-1, 1\]"):
        eng.set_bwm_prior(log10_h=(-15, -13), t0_mjd=(54000, 56000), cos_gwtheta=(-2, 1))
    with pytest.raises(ValueError, match="lo <= hi"):
        eng.set_bwm_prior(log10_h=(-13, -15), t0_mjd=(54000, 56000))
    with pytest.raises(ValueError, match="lo <= hi"):
        eng.set_bwm_prior(log10_h=(-15, np.inf), t0_mjd=(54000, 56000))
    with pytest.raises(ValueError, match=r"\(lo, hi\)"):
        eng.set_bwm_prior(log10_h=(-15, -14, -13), t0_mjd=(54000, 56000))
    with pytest.raises(ValueError, match="no prior"):
        eng.generate_sampled(2)
    assert eng.set_bwm_prior(log10_h=(-15, -13), t0_mjd=(54000, 56000)) is eng
    with pytest.raises(ValueError, match=r"set_bwm"):
        eng.generate_sampled(2)
    assert not eng._prepared
