"""CPU checks of the per-realisation CW source: the __host__ __device__ formulas of csrc/pta_cw_hyper.h compiled with g++
(tests/cw/cw_host.cpp) against a long-double evaluation of the reference's waveform and against oracle.cgw_dt, the label draw map
against philox_ref, and the validation of set_cw / set_cw_prior / theta on an engine that is configured but not prepared (no GPU
needed: every refusal happens before anything is launched)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from cw_reference import cgw_kwargs, corner_sources, phi_rad, theta_of, wave_ld
from helpers import load, mjd_ld, relrms
from oracle import philox_ref
from oracle import pta_oracle as po

HERE = os.path.dirname(os.path.abspath(__file__))
TREF_MJD = 53000 * 86400.0


@pytest.fixture(scope="module")
def ch(tmp_path_factory):
    out = tmp_path_factory.mktemp("cw") / "libcwhost.so"
    src = os.path.join(HERE, "cw", "cw_host.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", str(out)])
    lib = ctypes.CDLL(str(out))
    d, i, u64, p = ctypes.c_double, ctypes.c_int, ctypes.c_uint64, ctypes.POINTER(ctypes.c_double)
    lib.ch_uniform.argtypes = [u64, u64, i, i, p, p, p]
    lib.ch_params.argtypes = [p, i, p, d, i, p]
    lib.ch_wave.argtypes = [p, p, i, d, i, i, p]
    lib.ch_constants.argtypes = [p]
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _phat(ra, dec):
    from pta_replicator_amd import _cw
    return np.ascontiguousarray(_cw.pulsar_vectors([(ra, dec)])[0])


def _host_wave(ch, src, amp_is_h, ra, dec, pdist, mode, psr_term, toa_s, tref):
    par = np.zeros(16)
    ch.ch_params(_p(np.ascontiguousarray(src, dtype=np.float64)), int(amp_is_h), _p(_phat(ra, dec)), pdist, mode, _p(par))
    out = np.zeros(len(toa_s))
    ch.ch_wave(_p(par), _p(np.ascontiguousarray(toa_s)), len(toa_s), tref, mode, int(psr_term), _p(out))
    return out, par


def _toas(n=2000):
    mjd = np.linspace(53000, 58478, n)
    return mjd, mjd * 86400


def _close(dev, ref, scale=None):
    """relative RMS deviation; `scale` = the RMS the error is measured against (default: that of ref)"""
    if not np.any(ref):
        return 0.0 if not np.any(dev) else np.inf
    if scale is None:
        return relrms(dev, ref)
    return float(np.sqrt(np.mean((dev - ref) ** 2)) / scale)


def _scale(ref, ref_earth):
    """the RMS of the larger of the two terms a pulsar-term residual is the difference of: where they nearly cancel (equal
    amplitudes, phases a multiple of pi apart) the rounding of a 1e5 rad pulsar-term phase is measured against the terms, not
    against what is left of them"""
    return max(np.sqrt(np.mean(ref ** 2)), np.sqrt(np.mean(ref_earth ** 2)), np.sqrt(np.mean((ref - ref_earth) ** 2)))


def test_constants_match_python(ch):
    from pta_replicator_amd.constants import KPC2S, MPC2S, SOLAR2S
    c = np.zeros(3)
    ch.ch_constants(_p(c))
    assert c[0] == SOLAR2S and c[1] == KPC2S and c[2] == MPC2S


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("psr_term", [True, False])
@pytest.mark.parametrize("tref", [0.0, TREF_MJD])
def test_waveform_matches_long_double_reference(ch, mode, psr_term, tref):
    """every mode, with and without the pulsar term, over the corners of the usual CW prior (cos = +-1 edges included)."""
    _, toa = _toas()
    src = corner_sources(16, seed=3)
    rng = np.random.default_rng(1)
    worst = 0.0
    for r in range(len(src)):
        ra, dec = rng.uniform(0, 2 * np.pi), np.arcsin(rng.uniform(-1, 1))
        dev, _ = _host_wave(ch, src[r], True, ra, dec, 1.2, mode, psr_term, toa, tref)
        ref = wave_ld(toa, ra, dec, src[r], True, 1.2, mode, psr_term, tref)
        scale = _scale(ref, wave_ld(toa, ra, dec, src[r], True, 1.2, mode, False, tref)) if psr_term else None
        assert np.all(np.isfinite(dev))
        worst = max(worst, _close(dev, ref, scale))
    assert worst <= 1e-10, worst


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("psr_term", [True, False])
def test_waveform_matches_reference_formula_where_conditioned(ch, mode, psr_term):
    """against oracle.cgw_dt (the reference's own fp64 expression) wherever Phi <= 1e5 rad (its cancellation stays below 2e-10)."""
    mjd, toa = _toas()
    src = corner_sources(64, seed=8)
    keep = phi_rad(src[:, 2], src[:, 3]) <= 1e5
    assert keep.sum() >= 8
    rng = np.random.default_rng(2)
    worst = 0.0
    for r in np.flatnonzero(keep):
        ra, dec = rng.uniform(0, 2 * np.pi), np.arcsin(rng.uniform(-1, 1))
        dev, _ = _host_wave(ch, src[r], True, ra, dec, 1.2, mode, psr_term, toa, TREF_MJD)
        with np.errstate(invalid="ignore"):
            ref = po.cgw_dt(mjd, np.pi / 2 - dec, ra, pdist=1.2, psrTerm=psr_term, evolve=mode == 0, phase_approx=mode == 1,
                            tref=TREF_MJD, **cgw_kwargs(src[r], True))
        ref = np.where(np.isnan(ref), 0.0, ref)
        worst = max(worst, _close(dev, ref))
    assert worst <= 2e-10, worst


def test_conditioned_form_beats_reference_formula_for_light_binaries(ch):
    """the reason for the conditioned form: at Phi ~ 7e9 rad the reference's fp64 expression is off by ~1e-6, this one is not."""
    mjd, toa = _toas()
    src = np.array([0.3, 1.0, 7.0, -9.0, -14.0, 0.5, 0.4, 0.2])
    ra, dec = 1.0, 0.3
    ref = wave_ld(toa, ra, dec, src, True, 1.2, 0, True, 0.0)
    dev, _ = _host_wave(ch, src, True, ra, dec, 1.2, 0, True, toa, 0.0)
    old = po.cgw_dt(mjd, np.pi / 2 - dec, ra, pdist=1.2, **cgw_kwargs(src, True))
    assert relrms(dev, ref) < 1e-10
    assert relrms(old, ref) > 1e-8


def test_strain_and_distance_give_the_same_scalars(ch):
    from pta_replicator_amd import _cw
    src = corner_sources(32, seed=4)
    phat = _phat(0.7, -0.2)
    for r in range(len(src)):
        a, b = np.zeros(16), np.zeros(16)
        sd = src[r].copy()
        sd[4] = _cw.log10_dist_from_h(src[r, 2], src[r, 3], src[r, 4])
        assert abs(_cw.log10_h_from_dist(sd[2], sd[3], sd[4]) - src[r, 4]) < 1e-13
        for mode in (0, 1, 2):
            ch.ch_params(_p(src[r]), 1, _p(phat), 1.1, mode, _p(a))
            ch.ch_params(_p(sd), 0, _p(phat), 1.1, mode, _p(b))
            assert np.allclose(a, b, rtol=1e-13, atol=0), (r, mode, np.max(np.abs(a / np.where(b == 0, 1, b) - 1)))


def test_uniform_map_matches_philox_ref(ch):
    """label[r, j] = lo_j + (hi_j - lo_j) u2 of pair j of stream (8, 0): within 1 ulp of NumPy's lo + (hi - lo) * u."""
    from pta_replicator_amd import _cw
    from pta_replicator_amd.engine import STREAM_CW, stream_id
    assert STREAM_CW == 8
    P = 5
    prior = _cw.make_prior(P, log10_mc=(7, 10), log10_fgw=(-9, -7), log10_h=(-16, -13), pdist=np.column_stack([np.full(P, 0.5), np.arange(1, P + 1)]))
    lo, hi = _cw.prior_bounds(prior, P)
    assert len(lo) == _cw.n_columns(P, True) == 8 + P
    assert lo[0] == -1 and hi[1] == 2 * np.pi and hi[6] == np.pi and lo[2] == 7 and hi[4] == -13
    seed, r0, R, n = 0x0123456789ABCDEF, 77, 9, len(lo)
    out = np.zeros(R * n)
    ch.ch_uniform(seed, r0, R, n, _p(lo), _p(hi), _p(out))
    out = out.reshape(R, n)
    for r in range(R):
        _, u2 = philox_ref.uniform_pairs(seed, r0 + r, stream_id(STREAM_CW, 0), n)
        ref = lo + (hi - lo) * u2
        assert np.all(np.abs(out[r] - ref) <= np.spacing(np.abs(ref))), r
        assert np.all(out[r] >= lo) and np.all(out[r] <= hi)


def test_merger_contributes_zero(ch):
    """a binary that merges mid-span: finite before the merger (long-double reference), 0 after, no NaN."""
    mjd, toa = _toas()
    src = np.array([0.1, 2.0, 10.0, -7.2, -14.0, 1.0, 0.3, -0.4])
    dev, par = _host_wave(ch, src, True, 0.4, 0.9, 1.0, 0, False, toa, TREF_MJD)
    merged = 1 - par[3] * (toa - TREF_MJD) <= 0
    assert 0 < merged.sum() < len(toa)
    assert np.all(dev[merged] == 0) and np.all(np.isfinite(dev))
    ref = wave_ld(toa, 0.4, 0.9, src, True, 1.0, 0, False, TREF_MJD)
    assert relrms(dev[~merged], ref[~merged]) < 1e-10


# ---------------------------------------------------------------- validation (no GPU) -------------------------------
def _engine(cw=True):
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
    if cw:
        eng.set_cw(tref=TREF_MJD, pdist=[1.0, 1.5, 0.8, 2.0])
    return eng


def test_cw_keys_stay_out_of_hyper_layout():
    from pta_replicator_amd import _cw, _hyper
    assert not set(_cw.KEYS) & set(_hyper.KEYS)
    assert _hyper.KEYS == ("gwb_log10_A", "gwb_gamma", "rn_log10_A", "rn_gamma") and _hyper.n_columns(4) == 10


def test_cw_theta_refusals_before_any_launch():
    R = 3
    eng = _engine()
    ok = theta_of(corner_sources(R), True)
    bad_cos = dict(ok, cw_cos_gwtheta=np.array([0.0, 1.5, 0.0]))
    bad_inc = dict(ok, cw_cos_inc=np.array([0.0, -1.0000001, 0.0]))
    nan = dict(ok, cw_log10_mc=np.array([8.0, np.nan, 8.0]))
    inf = dict(ok, cw_psi=np.array([np.inf, 0.0, 0.0]))
    both = dict(ok, cw_log10_dist=np.ones(R))
    none = {k: v for k, v in ok.items() if k != "cw_log10_h"}
    missing = {k: v for k, v in ok.items() if k != "cw_gwphi"}
    cases = [
        (dict(ok, cw_phase0=np.zeros(R + 1)), "shape"),
        (dict(ok, cw_pdist=np.ones((R, 3))), "shape"),
        (dict(ok, cw_pdist=np.where(np.eye(R, 4) > 0, 0.0, 1.0)), "pdist"),
        (bad_cos, r"\|cos\|"), (bad_inc, r"\|cos\|"), (nan, "non-finite"), (inf, "non-finite"),
        (both, "exactly one"), (none, "exactly one"), (missing, "cw_gwphi"),
        ({"cw_pdist": np.ones((R, 4))}, "missing"),
        (dict(ok, gwb_log10_A=np.zeros(R + 1)), "shape"),
    ]
    for theta, msg in cases:
        with pytest.raises(ValueError, match=msg):
            eng.generate(R, theta=theta)
        with pytest.raises(ValueError, match=msg):
            eng.generate_per_signal(R, theta=theta)
    for theta, msg in cases[:-1]:
        with pytest.raises(ValueError, match=msg):
            eng.generate_td(R, theta=theta)
    assert not eng._prepared
    with pytest.raises(ValueError, match=r"no per-realisation CW configured \(set_cw\)"):
        _engine(cw=False).generate(R, theta=ok)
    with pytest.raises(ValueError, match="TD mode"):
        eng.generate_td(R, theta=dict(ok, rn_gamma=np.full((R, 4), 3.0)))
    assert not eng._prepared


def test_set_cw_and_prior_validation():
    eng = _engine(cw=False)
    with pytest.raises(ValueError, match="pdist"):
        eng.set_cw(pdist=[1.0, 2.0])
    with pytest.raises(ValueError, match="pdist"):
        eng.set_cw(pdist=-1.0)
    with pytest.raises(ValueError, match="log10_mc"):
        eng.set_cw_prior(log10_fgw=(-9, -7), log10_h=(-16, -13))
    with pytest.raises(ValueError, match="exactly one"):
        eng.set_cw_prior(log10_mc=(7, 10), log10_fgw=(-9, -7))
    with pytest.raises(ValueError, match="exactly one"):
        eng.set_cw_prior(log10_mc=(7, 10), log10_fgw=(-9, -7), log10_h=(-16, -13), log10_dist=(1, 2))
    with pytest.raises(ValueError, match=r"\[-1, 1\]"):
        eng.set_cw_prior(log10_mc=(7, 10), log10_fgw=(-9, -7), log10_h=(-16, -13), cos_inc=(-2, 1))
    with pytest.raises(ValueError, match="lo <= hi"):
        eng.set_cw_prior(log10_mc=(10, 7), log10_fgw=(-9, -7), log10_h=(-16, -13))
    with pytest.raises(ValueError, match=r"\[4, 2\]"):
        eng.set_cw_prior(log10_mc=(7, 10), log10_fgw=(-9, -7), log10_h=(-16, -13), pdist=np.ones((3, 2)))
    with pytest.raises(ValueError, match="> 0"):
        eng.set_cw_prior(log10_mc=(7, 10), log10_fgw=(-9, -7), log10_h=(-16, -13), pdist=(0, 1))
    with pytest.raises(ValueError, match="no prior"):
        eng.generate_sampled(2)
    eng.set_cw_prior(log10_mc=(7, 10), log10_fgw=(-9, -7), log10_dist=(1, 3))
    with pytest.raises(ValueError, match=r"set_cw"):
        eng.generate_sampled(2)
    assert not eng._prepared
