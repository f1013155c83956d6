"""CPU checks of the per-realisation GWB spectrum (theta key gwb_log10_hc): the __host__ __device__ formulas of csrc/pta_hyper.h and
csrc/pta_os_matched.h compiled with g++ (tests/gwb_spectrum/gwb_spectrum_host.cpp) against red_noise.gwb_spectrum_hcf, philox_ref
and optimal_statistic.matched_prior, and the validation of the key on an engine that is configured but not prepared (no GPU needed:
every refusal happens before anything is launched)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import philox_ref
from test_hyper_host import _engine

HERE = os.path.dirname(os.path.abspath(__file__))
YR = 365.25 * 86400.0


@pytest.fixture(scope="module")
def gs(tmp_path_factory):
    out = tmp_path_factory.mktemp("gwb_spectrum") / "libgwbspectrumhost.so"
    src = os.path.join(HERE, "gwb_spectrum", "gwb_spectrum_host.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", str(out)])
    lib = ctypes.CDLL(str(out))
    d, i, u64 = ctypes.c_double, ctypes.c_int, ctypes.c_uint64
    p, pi = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    lib.gs_hcf_user.argtypes = [pi, p, p, i, i, i, p, p]
    lib.gs_gwb_hcf.argtypes = [p, i, d, d, p]
    lib.gs_draw_field.argtypes = [u64, u64, i, i, i, p, p, p]
    lib.gs_osm_gw_b_hc.argtypes = [i, i, i, d, pi, p, p, i, p, p, p]
    lib.gs_osm_gw_b.argtypes = [i, i, i, d, p, p, p, p]
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _pi(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def _grid():
    """the 600-point grid of test_hyper_host.py"""
    dur, howml = 4.8e8, 10
    f = np.arange(0, 1 / (2 * dur / 600), 1 / (dur * howml))
    f[0] = f[1]
    return f


def _hcf_user(gs, f, U, Y):
    """device-twin hc [R, n] of spectra Y [R, M] (log10 hc, columns as the rows of U) at frequencies f"""
    from pta_replicator_amd import _hyper
    order, xp = _hyper.spec_nodes(U)
    seg, dx, dxp = (np.ascontiguousarray(t) for t in _hyper.spec_tables(f, xp))
    assert seg.dtype == np.int32 and seg.min() >= 0 and seg.max() <= len(xp) - 1
    Ys = np.ascontiguousarray(np.asarray(Y, dtype=np.float64)[:, order])
    out = np.zeros((len(Ys), len(f)))
    gs.gs_hcf_user(_pi(seg), _p(dx), _p(dxp), len(f), len(xp), len(Ys), _p(Ys), _p(out))
    return out


def _nodes(M, f, rng, outside=False):
    """M node frequencies given unsorted, one exactly on a grid frequency.  The band of the nodes ends inside the grid, so the bins
    below the first and above the last node are clamped; outside=True: a node below f[1] and one above Nyquist instead, so every bin
    is interpolated"""
    nf = 10 ** rng.uniform(np.log10(f[30]), np.log10(f[-30]), M)
    nf[0], nf[-1] = (0.4 * f[1], 1.7 * f[-1]) if outside else (1.0000001 * f[20], 0.9999999 * f[-20])
    if M > 2:
        nf[M // 2] = f[137]
    return nf[rng.permutation(M)]


@pytest.mark.parametrize("outside", [False, True])
@pytest.mark.parametrize("M", [2, 7, 40])
def test_interpolation_twin_matches_reference_userspec(gs, M, outside):
    """pta_gwb_hcf_user against red_noise.gwb_spectrum_hcf(userSpec=) - the reference's interp1d + extrap1d.  Bound 1e-13 for
    |log10 hc| <= 20: a few ulp of a number of size 20 (3.6e-15) times ln 10."""
    from pta_replicator_amd import red_noise as rn
    f = _grid()
    assert len(f) == 3000
    rng = np.random.default_rng(100 + M)
    nf = _nodes(M, f, rng, outside)
    if M == 2:
        nf = np.sort(nf)[::-1]
    assert not np.all(np.diff(nf) > 0)                      # given unsorted
    assert (nf.min() < f[1] and nf.max() > f[-1]) if outside else (nf.min() > f[1] and nf.max() < f[-1])
    Y = rng.uniform(-20, 20, (5, M))
    Y[1] = rng.uniform(-16, -13, M)
    got = _hcf_user(gs, f, np.stack([nf, np.ones(M)], axis=1), Y)
    for r in range(len(Y)):
        ref = rn.gwb_spectrum_hcf(f, 0.0, 0.0, userSpec=np.stack([nf, 10.0 ** Y[r]], axis=1))
        err = np.max(np.abs(got[r] / ref - 1))
        assert err < 1e-13, (r, err)
        # both clamps and the node on a grid frequency
        lo, hi = np.argmin(nf), np.argmax(nf)
        if not outside:
            assert np.all(got[r, :21] == 10.0 ** Y[r, lo]) and np.all(got[r, -20:] == 10.0 ** Y[r, hi])
            assert got[r, 21] != got[r, 20] and got[r, -21] != got[r, -20]
        if M > 2:
            on = int(np.flatnonzero(nf == f[137])[0])
            assert got[r, 137] == 10.0 ** Y[r, on]


def test_interpolation_twin_at_the_population_floor(gs):
    """a node value of -100 (the population code's 1e-100 floor): finite, and accurate to 5e-13 (the bound above scaled by 5)"""
    from pta_replicator_amd import red_noise as rn
    f = _grid()
    rng = np.random.default_rng(7)
    M = 7
    nf = _nodes(M, f, rng)
    Y = rng.uniform(-16, -13, (2, M))
    Y[0, 2] = Y[1, 5] = -100.0
    got = _hcf_user(gs, f, np.stack([nf, np.ones(M)], axis=1), Y)
    assert np.all(np.isfinite(got)) and np.all(got > 0)
    for r in range(2):
        ref = rn.gwb_spectrum_hcf(f, 0.0, 0.0, userSpec=np.stack([nf, 10.0 ** Y[r]], axis=1))
        err = np.max(np.abs(got[r] / ref - 1))
        assert err < 5e-13, (r, err)


def test_power_law_nodes_reproduce_the_power_law(gs):
    """nodes lying on A (f / f1yr)^((3 - gamma) / 2) and covering the grid reproduce pta_gwb_hcf to 1e-13"""
    f = _grid()
    rng = np.random.default_rng(11)
    f1yr = 1 / 3.16e7
    for lA, g in ((-14.6, 13. / 3.), (-13.2, 2.0), (-15.5, 6.5)):
        nf = 10 ** np.linspace(np.log10(0.5 * f[1]), np.log10(2 * f[-1]), 9)[rng.permutation(9)]
        y = lA + 0.5 * (3.0 - g) * np.log10(nf / f1yr)
        got = _hcf_user(gs, f, np.stack([nf, np.ones(9)], axis=1), y[None])[0]
        ref = np.zeros_like(f)
        gs.gs_gwb_hcf(_p(f), len(f), lA, g, _p(ref))
        err = np.max(np.abs(got / ref - 1))
        assert err < 1e-13, (lA, g, err)


def test_prior_draws_of_field_one(gs):
    """pta_hyper_draw_field: field 1 = lo + (hi - lo) u2 of pair j of stream (7, 1) within 1 ulp; field 0 = pta_hyper_draw exactly"""
    from pta_replicator_amd import _hyper
    from pta_replicator_amd.engine import STREAM_HYPER, stream_id
    assert _hyper.SPEC_FIELD == 1 and _hyper.SPEC_KEY == "gwb_log10_hc"
    seed, r0, R, M = 0x0123456789ABCDEF, 40, 9, 14
    rng = np.random.default_rng(3)
    lo = rng.uniform(-18, -13, M)
    hi = lo + rng.uniform(0, 3, M)
    hi[3] = lo[3]
    out1, out0, base = np.zeros(R * M), np.zeros(R * M), np.zeros(R * M)
    gs.gs_draw_field(seed, r0, R, M, 1, _p(lo), _p(hi), _p(out1))
    gs.gs_draw_field(seed, r0, R, M, 0, _p(lo), _p(hi), _p(out0))
    gs.gs_draw_field(seed, r0, R, M, -1, _p(lo), _p(hi), _p(base))
    assert np.array_equal(out0, base)
    out1 = out1.reshape(R, M)
    assert not np.any(out1[:, :3] == out0.reshape(R, M)[:, :3])
    for r in range(R):
        _, u2 = philox_ref.uniform_pairs(seed, r0 + r, stream_id(STREAM_HYPER, 1), M)
        ref = lo + (hi - lo) * u2
        assert np.all(np.abs(out1[r] - ref) <= np.spacing(np.abs(ref))), r
        assert np.all(out1[r] >= lo) and np.all(out1[r] <= hi) and out1[r, 3] == lo[3]


def test_matched_prior_spectrum_columns(gs):
    """pta_osm_gw_b_hc against optimal_statistic.matched_prior(gw_log10_hc=, gw_nodes=) to 1e-14 (the bound of the existing twins),
    and for nodes on A (f yr)^((3 - gamma) / 2) against pta_osm_gw_b to 1e-13"""
    from pta_replicator_amd import _hyper
    from pta_replicator_amd import optimal_statistic as ost
    rng = np.random.default_rng(5)
    R, P, nf, T, M = 6, 4, 7, 4.4e8, 9
    s = rng.uniform(1e-13, 4e-13, P)
    fk = np.arange(1, nf + 1) / T
    nodes = 10 ** rng.uniform(np.log10(0.6 * fk[0]), np.log10(0.8 * fk[-1]), M)     # the last bins lie above the nodes: clamped
    nodes[2] = fk[3]
    Y = rng.uniform(-16, -13, (R, M))
    order, xp = _hyper.spec_nodes(np.stack([nodes, np.ones(M)], axis=1))
    seg, dx, dxp = (np.ascontiguousarray(t) for t in _hyper.spec_tables(fk, xp))
    Ys = np.ascontiguousarray(Y[:, order])
    b = np.zeros((R, P, 2 * nf))
    gs.gs_osm_gw_b_hc(R, P, nf, T, _pi(seg), _p(dx), _p(dxp), M, _p(Ys), _p(s), _p(b))
    ref = ost.matched_prior(R, s, nf=nf, T=T, gw_log10_hc=Y, gw_nodes=nodes)
    assert ref.shape == b.shape and np.all(ref > 0)
    assert np.max(np.abs(b / ref - 1)) < 1e-14
    # existing calls of matched_prior are what they were
    lA, g = rng.uniform(-15, -13.5, R), rng.uniform(2, 6, R)
    pl = ost.matched_prior(R, s, nf=nf, T=T, gw_log10_A=lA, gw_gamma=g)
    bp = np.zeros_like(b)
    gs.gs_osm_gw_b(R, P, nf, T, _p(lA), _p(g), _p(s), _p(bp))
    assert np.max(np.abs(bp / pl - 1)) < 1e-14
    # nodes on the power law of (A_r, gamma_r), covering the bins
    nodes = 10 ** np.linspace(np.log10(0.5 * fk[0]), np.log10(2 * fk[-1]), M)[rng.permutation(M)]
    Y = lA[:, None] + 0.5 * (3.0 - g[:, None]) * np.log10(nodes * YR)[None, :]
    order, xp = _hyper.spec_nodes(np.stack([nodes, np.ones(M)], axis=1))
    seg, dx, dxp = (np.ascontiguousarray(t) for t in _hyper.spec_tables(fk, xp))
    Ys = np.ascontiguousarray(Y[:, order])
    gs.gs_osm_gw_b_hc(R, P, nf, T, _pi(seg), _p(dx), _p(dxp), M, _p(Ys), _p(s), _p(b))
    assert np.max(np.abs(b / bp - 1)) < 1e-13
    with pytest.raises(ValueError, match="gw_nodes"):
        ost.matched_prior(R, s, nf=nf, T=T, gw_log10_hc=Y)


# ---------------------------------------------------------------- validation (no GPU) -------------------------------
SPEC = np.array([[1e-8, 1e-16], [1e-9, 1e-15], [1e-7, 1e-17]])    # given unsorted
M = len(SPEC)


def test_spectrum_refusals_before_any_launch():
    R = 3
    ok = np.full((R, M), -15.0)

    def both(eng, theta, msg):
        with pytest.raises(ValueError, match=msg):
            eng.generate(R, theta=theta)
        with pytest.raises(ValueError, match=msg):
            eng.generate_per_signal(R, theta=theta)
        assert not eng._prepared
    both(_engine(gwb=False), {"gwb_log10_hc": ok}, "no GWB")
    both(_engine(), {"gwb_log10_hc": ok}, "userSpec")
    eng = _engine(userSpec=SPEC)
    both(eng, {"gwb_log10_hc": ok, "gwb_log10_A": np.full(R, -14.0)}, "userSpec")
    both(eng, {"gwb_log10_hc": ok, "gwb_gamma": np.full(R, 4.0)}, "userSpec")
    both(eng, {"gwb_log10_hc": np.zeros((R, M + 1))}, "shape")
    both(eng, {"gwb_log10_hc": np.zeros((R + 1, M))}, "shape")
    both(eng, {"gwb_log10_hc": np.zeros(R)}, "shape")
    for bad in (np.nan, np.inf, -np.inf):
        y = ok.copy()
        y[1, 2] = bad
        both(eng, {"gwb_log10_hc": y}, "non-finite")
    eng.gwb_mode = "grid"
    both(eng, {"gwb_log10_hc": ok}, "grid")
    with pytest.raises(ValueError, match="TD mode"):
        _engine(userSpec=SPEC).generate_td(R, theta={"gwb_log10_hc": ok})
    both(_engine(userSpec=SPEC[:1]), {"gwb_log10_hc": ok[:, :1]}, "node")
    both(_engine(userSpec=np.array([[1e-9, 1e-15], [1e-8, 1e-16], [1e-9, 1e-17]])), {"gwb_log10_hc": ok}, "node")
    # accepted: NumPy arrays, with red-noise keys beside it; the validated dict keeps the caller's arrays
    from pta_replicator_amd import _hyper
    eng = _engine(userSpec=SPEC)
    th = _hyper.check_theta({"gwb_log10_hc": ok, "rn_gamma": np.full((R, 4), 3.0)}, R, 4, eng._gw, eng._rn, eng.gwb_mode)
    assert set(th) == {"gwb_log10_hc", "rn_gamma"} and th["gwb_log10_hc"] is ok
    # the existing surface keeps its values
    assert _hyper.KEYS == ("gwb_log10_A", "gwb_gamma", "rn_log10_A", "rn_gamma") and _hyper.n_columns(4) == 10
    assert "gwb_log10_hc" not in _hyper.columns(4)


def test_spectrum_in_the_noise_model_of_the_statistic():
    """check_theta_os: the key needs the GW auto-term and the engine's userSpec; the likelihood grid (no gw handed over) refuses it"""
    from pta_replicator_amd import _hyper
    R = 2
    ok = np.full((R, M), -15.0)
    eng = _engine(userSpec=SPEC)
    th = _hyper.check_theta_os({"gwb_log10_hc": ok, "cw_log10_mc": np.zeros(R)}, R, 4, eng._rn, True, gw=eng._gw)
    assert set(th) == {"gwb_log10_hc"}
    with pytest.raises(ValueError, match="gwb_auto"):
        _hyper.check_theta_os({"gwb_log10_hc": ok}, R, 4, eng._rn, False, gw=eng._gw)
    with pytest.raises(ValueError, match="userSpec"):
        _hyper.check_theta_os({"gwb_log10_hc": ok}, R, 4, eng._rn, True, gw=_engine()._gw)
    with pytest.raises(ValueError, match="userSpec"):
        _hyper.check_theta_os({"gwb_log10_hc": ok, "gwb_gamma": np.full(R, 4.0)}, R, 4, eng._rn, True, gw=eng._gw)
    with pytest.raises(ValueError, match="shape"):
        _hyper.check_theta_os({"gwb_log10_hc": ok[:, :2]}, R, 4, eng._rn, True, gw=eng._gw)
    with pytest.raises(ValueError, match="unknown"):
        _hyper.check_theta_os({"gwb_log10_hc": ok}, R, 4, eng._rn, True)


def test_spectrum_prior_boxes():
    from pta_replicator_amd import _hyper
    eng = _engine(userSpec=SPEC)
    with pytest.raises(ValueError, match="lo <= hi"):
        eng.set_hyper_prior(gwb_log10_hc=(-13, -15))
    with pytest.raises(ValueError, match="finite"):
        eng.set_hyper_prior(gwb_log10_hc=(-np.inf, -15))
    with pytest.raises(ValueError, match=r"\[3, 2\]"):
        eng.set_hyper_prior(gwb_log10_hc=np.zeros((4, 2)))
    with pytest.raises(ValueError, match="userSpec"):
        _engine().set_hyper_prior(gwb_log10_hc=(-16, -14))
    eng.set_hyper_prior(gwb_log10_hc=(-16, -14))
    lo, hi = _hyper.spec_bounds(eng._prior)
    assert np.array_equal(lo, np.full(M, -16.0)) and np.array_equal(hi, np.full(M, -14.0))
    box = np.array([[-16, -14], [-15.5, -15], [-17, -17]])
    eng.set_hyper_prior(gwb_log10_hc=box, rn_log10_A=(-15, -13))
    lo, hi = _hyper.spec_bounds(eng._prior)
    assert np.array_equal(lo, box[:, 0]) and np.array_equal(hi, box[:, 1])
    # the table of field 0 is what it is without the new key
    eng2 = _engine(userSpec=SPEC)
    eng2.set_hyper_prior(rn_log10_A=(-15, -13))
    for a, b in zip(_hyper.prior_bounds(eng._prior, 4), _hyper.prior_bounds(eng2._prior, 4)):
        assert np.array_equal(a, b) and len(a) == _hyper.n_columns(4)
    assert _hyper.spec_bounds(eng2._prior) is None
    assert not eng._prepared
    # a prior the configuration cannot honour is refused before anything is launched
    eng.gwb_mode = "grid"
    with pytest.raises(ValueError, match="grid"):
        eng.generate_sampled(2)
    assert not eng._prepared
