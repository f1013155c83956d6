"""CPU checks of per-realisation hyperparameters: the __host__ __device__ formulas of csrc/pta_hyper.h compiled with g++
(tests/hyper/hyper_host.cpp) against NumPy / the engine's own host formulas, and the theta validation of ReplicaEngine on an engine
that is configured but not prepared (no GPU needed: every refusal happens before anything is launched)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from helpers import load, mjd_ld
from oracle import philox_ref

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def hh(tmp_path_factory):
    out = tmp_path_factory.mktemp("hyper") / "libhyperhost.so"
    src = os.path.join(HERE, "hyper", "hyper_host.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", str(out)])
    lib = ctypes.CDLL(str(out))
    d, i, u64, p = ctypes.c_double, ctypes.c_int, ctypes.c_uint64, ctypes.POINTER(ctypes.c_double)
    lib.hh_hyper_uniform.argtypes = [u64, u64, i, i, p, p, p]
    lib.hh_gwb_hcf.argtypes = [p, i, d, d, i, d, d, d, p]
    lib.hh_rn_amp.argtypes = [p, i, d, d, d, p]
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def test_uniform_map_matches_philox_ref(hh):
    """theta[r, j] = lo_j + (hi_j - lo_j) u2 of pair j of stream (7, 0): within 1 ulp of NumPy's lo + (hi - lo) * u."""
    from pta_replicator_amd import _hyper
    from pta_replicator_amd.engine import STREAM_HYPER, stream_id
    assert STREAM_HYPER == 7
    seed, r0, R, P = 0x0123456789ABCDEF, 40, 9, 5
    n = _hyper.n_columns(P)
    rng = np.random.default_rng(3)
    lo = rng.uniform(-18, -11, n)
    hi = lo + rng.uniform(0, 6, n)
    hi[3] = lo[3]                                  # a degenerate box returns lo exactly
    out = np.zeros(R * n)
    hh.hh_hyper_uniform(seed, r0, R, n, _p(lo), _p(hi), _p(out))
    out = out.reshape(R, n)
    for r in range(R):
        _, u2 = philox_ref.uniform_pairs(seed, r0 + r, stream_id(STREAM_HYPER, 0), n)
        ref = lo + (hi - lo) * u2
        assert np.all(np.abs(out[r] - ref) <= np.spacing(np.abs(ref))), r
        assert np.all(out[r] >= lo) and np.all(out[r] <= hi)
        assert out[r, 3] == lo[3]


@pytest.mark.parametrize("turnover", [False, True])
def test_gwb_hcf_ratio_matches_host_spectrum(hh, turnover):
    """hcf(theta) / hcf0 of pta_gwb_spectrum_scale, and sqrt(C) it implies, against red_noise.gwb_spectrum over the prior range."""
    from pta_replicator_amd import red_noise as rn
    dur, howml = 4.8e8, 10
    f = np.arange(0, 1 / (2 * dur / 600), 1 / (dur * howml))
    f[0] = f[1]
    kw = dict(turnover=turnover, f0=2e-9, beta=1.5, power=2)
    A0, g0 = -14.6, 13. / 3.
    hcf0 = rn.gwb_spectrum_hcf(f, A0, g0, **kw)
    C0 = rn.gwb_spectrum(f, dur, howml, A0, g0, **kw)
    worst = 0.0
    for lA in np.linspace(-18, -11, 8):
        for g in np.linspace(0.5, 7, 7):
            dev = np.zeros_like(f)
            hh.hh_gwb_hcf(_p(f), len(f), lA, g, int(turnover), kw["f0"], kw["beta"], kw["power"], _p(dev))
            ref = rn.gwb_spectrum_hcf(f, lA, g, **kw)
            worst = max(worst, np.max(np.abs(dev / ref - 1)))
            # the scaled pre-chirp carries sqrt(C0) * scale: the spectrum of theta up to rounding
            sqrtC = np.sqrt(C0) * (dev / hcf0)
            assert np.max(np.abs(sqrtC / np.sqrt(rn.gwb_spectrum(f, dur, howml, lA, g, **kw)) - 1)) < 1e-14
    assert worst < 1e-14, worst


def test_rn_amplitude_matches_prior_formula(hh):
    """sqrt(prior) of pta_engine_rn_coef_hyper against the expression prepare() evaluates (red_noise.py:126)."""
    from pta_replicator_amd.constants import YEAR_IN_SEC
    tspan = 4.3e8
    f = 1.0 * np.arange(1, 31) / tspan
    worst = 0.0
    for lA in np.linspace(-18, -11, 8):
        for g in np.linspace(0.5, 7, 7):
            dev = np.zeros_like(f)
            hh.hh_rn_amp(_p(f), len(f), tspan, lA, g, _p(dev))
            fyr = 1 / YEAR_IN_SEC
            ref = np.sqrt((10 ** lA) ** 2 * (f / fyr) ** (-g) / (12 * np.pi ** 2 * tspan) * YEAR_IN_SEC ** 3)
            worst = max(worst, np.max(np.abs(dev / ref - 1)))
    assert worst < 1e-14, worst


# ---------------------------------------------------------------- validation (no GPU) -------------------------------
def _engine(gwb=True, rn=True, userSpec=None):
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
    if rn:
        eng.set_red_noise([-14.0, None, -13.5, -14.2], [3.0, None, 2.5, 4.0], components=10)
    if gwb:
        eng.set_gwb(-14.5, 13. / 3., userSpec=userSpec)
    return eng


def test_theta_refusals_before_any_launch():
    R = 3
    eng = _engine()
    ok = {"gwb_log10_A": np.full(R, -14.0), "gwb_gamma": np.full(R, 4.0), "rn_log10_A": np.full((R, 4), -14.0),
          "rn_gamma": np.full((R, 4), 3.0)}
    cases = [
        ({"gwb_log10_A": np.zeros(R + 1)}, "shape"),
        ({"rn_log10_A": np.zeros((R, 3))}, "shape"),
        ({"gwb_gamma": np.array([4.0, np.nan, 4.0])}, "non-finite"),
        ({"gwb_log10_A": np.array([-14.0, np.inf, -14.0])}, "non-finite"),
        ({"rn_log10_A": np.full((R, 4), np.inf)}, "infinite"),
        ({**ok, "rn_gamma": np.where(np.eye(R, 4) > 0, np.nan, 3.0)}, "non-finite"),
        ({"rn_gamma": np.full((R, 4), np.nan)}, "non-finite"),
        ({"gwb_amplitude": np.zeros(R)}, "unknown"),
    ]
    for theta, msg in cases:
        with pytest.raises(ValueError, match=msg):
            eng.generate(R, theta=theta)
        with pytest.raises(ValueError, match=msg):
            eng.generate_per_signal(R, theta=theta)
    assert not eng._prepared
    with pytest.raises(ValueError, match="dict"):
        eng.generate(R, theta=[1, 2])
    # NaN amplitude = "as configured": accepted, with the index left NaN there too (validation only; no launch here)
    from pta_replicator_amd import _hyper
    th = dict(ok, rn_log10_A=np.where(np.eye(R, 4) > 0, np.nan, -14.0), rn_gamma=np.where(np.eye(R, 4) > 0, np.nan, 3.0))
    assert set(_hyper.check_theta(th, R, 4, eng._gw, eng._rn, eng.gwb_mode)) == set(ok)
    # the configured-None pulsar's entries are ignored: a NaN index there is fine when only the index is sampled
    g = np.full((R, 4), 3.0)
    g[:, 1] = np.nan
    assert "rn_gamma" in _hyper.check_theta({"rn_gamma": g}, R, 4, eng._gw, eng._rn, eng.gwb_mode)


def test_theta_refused_by_configuration():
    R = 2
    gw = {"gwb_log10_A": np.full(R, -14.0)}
    rn = {"rn_gamma": np.full((R, 4), 3.0)}
    with pytest.raises(ValueError, match="no GWB"):
        _engine(gwb=False).generate(R, theta=gw)
    with pytest.raises(ValueError, match="no red noise"):
        _engine(rn=False).generate(R, theta=rn)
    spec = np.array([[1e-9, 1e-15], [1e-8, 1e-16], [1e-7, 1e-17]])
    with pytest.raises(ValueError, match="userSpec"):
        _engine(userSpec=spec).generate(R, theta=gw)
    eng = _engine()
    eng.gwb_mode = "grid"
    with pytest.raises(ValueError, match="grid"):
        eng.generate(R, theta=gw)
    with pytest.raises(ValueError, match="TD mode"):
        _engine().generate_td(R, theta=rn)
    eng = _engine(gwb=False)
    eng.set_hyper_prior(gwb_log10_A=(-15, -13))
    with pytest.raises(ValueError, match="no GWB"):
        eng.generate_sampled(R)
    with pytest.raises(ValueError, match="no prior"):
        _engine().generate_sampled(R)


def test_hyper_prior_boxes():
    from pta_replicator_amd import _hyper
    eng = _engine()
    with pytest.raises(ValueError, match="lo <= hi"):
        eng.set_hyper_prior(gwb_log10_A=(-13, -15))
    with pytest.raises(ValueError, match="finite"):
        eng.set_hyper_prior(rn_gamma=(0, np.inf))
    with pytest.raises(ValueError, match=r"\[4, 2\]"):
        eng.set_hyper_prior(rn_log10_A=np.zeros((3, 2)))
    with pytest.raises(ValueError, match="no parameter"):
        eng.set_hyper_prior()
    box = np.array([[-15, -13], [-16, -14], [-17, -12], [-14, -14]])
    eng.set_hyper_prior(gwb_gamma=(3, 5), rn_log10_A=box)
    lo, hi = _hyper.prior_bounds(eng._prior, 4)
    cols = _hyper.columns(4)
    assert lo[cols["gwb_gamma"][0]] == 3 and hi[cols["gwb_gamma"][0]] == 5
    assert np.array_equal(lo[slice(*cols["rn_log10_A"])], box[:, 0]) and np.array_equal(hi[slice(*cols["rn_log10_A"])], box[:, 1])
    assert np.all(lo[slice(*cols["gwb_log10_A"])] == 0) and np.all(lo[slice(*cols["rn_gamma"])] == 0)
    assert not eng._prepared   # a prior is no configuration change
