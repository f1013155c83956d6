"""CPU checks of the anisotropic GWB per realisation: the theta key gwb_clm through pta_replicator_amd._hyper and an engine that is
configured but not prepared (every refusal happens before anything is launched), the prior boxes, the joint spherical-harmonic
weights of the optimal statistic against numpy.linalg.lstsq, and the two new entry points of the C ABI.  No GPU."""
import re
import subprocess

import numpy as np
import pytest

from test_abi import declared

ANISO = ("pta_gwb_orf_factor", "pta_gwb_mix_batched")
PTA_E_ARG = -1
X = 4096   # a non-NULL stand-in: every call below is refused before a pointer is used
C00 = np.sqrt(4.0 * np.pi)


def _engine(P=4, lmax=1, gwb=True, **gw):
    from pta_replicator_amd.engine import ReplicaEngine
    from pta_replicator_amd.simulate import ArrayTOAs, SimulatedPulsar, make_ideal
    rng = np.random.default_rng(2)
    psrs = []
    for a in range(P):
        p = SimulatedPulsar(toas=ArrayTOAs(np.sort(rng.uniform(53000, 56000, 40 + a)), 0.5), name=f"J{a:04d}",
                            loc={"RAJ": float(rng.uniform(0, 24)), "DECJ": float(np.degrees(np.arcsin(rng.uniform(-1, 1))))})
        make_ideal(p)
        psrs.append(p)
    eng = ReplicaEngine(psrs, seed=5)
    eng.set_white_noise(efac=1.0)
    eng.set_red_noise(-14.0, 3.0, components=5)
    if gwb:
        n = (lmax + 1) ** 2
        eng.set_gwb(-14.5, 13. / 3., clm=[C00] + [0.0] * (n - 1), lmax=lmax, **gw)
    return eng


def _clm(R, n):
    c = np.zeros((R, n))
    c[:, 0] = C00
    return c


# ---------------------------------------------------------------- theta ------------------------------------------------------
def test_key_is_accepted_and_checked_before_any_launch():
    from pta_replicator_amd import _hyper
    R = 3
    eng = _engine(lmax=2)
    assert _hyper.n_lm(eng._gw) == 9
    th = _hyper.check_theta({"gwb_clm": _clm(R, 9), "gwb_log10_A": np.full(R, -14.0), "rn_gamma": np.full((R, 4), 3.0)}, R, 4, eng._gw, eng._rn,
                            eng.gwb_mode)
    assert set(th) == {"gwb_clm", "gwb_log10_A", "rn_gamma"}
    hyper, det = eng._theta_parts({"gwb_clm": _clm(R, 9), "gwb_orf_info": np.zeros(R, dtype=np.int32)}, R)   # the label of sampled theta is skipped
    assert set(hyper) == {"gwb_clm"} and det == {}
    bad = _clm(R, 9)
    bad[1, 4] = np.nan
    inf = _clm(R, 9)
    inf[2, 0] = np.inf
    for theta, msg in [({"gwb_clm": _clm(R, 4)}, "shape"), ({"gwb_clm": _clm(R + 1, 9)}, "shape"), ({"gwb_clm": np.zeros(9)}, "shape"),
                       ({"gwb_clm": bad}, "non-finite"), ({"gwb_clm": inf}, "non-finite")]:
        for call in (eng.generate, eng.generate_per_signal):
            with pytest.raises(ValueError, match=msg):
                call(R, theta=theta)
    assert not eng._prepared


def test_key_refused_by_configuration():
    R = 2
    th = {"gwb_clm": _clm(R, 4)}
    with pytest.raises(ValueError, match="no GWB"):
        _engine(gwb=False).generate(R, theta=th)
    eng = _engine()
    eng.set_gwb(-14.5, 13. / 3.)                       # lmax left at its default
    with pytest.raises(ValueError, match="lmax"):
        eng.generate(R, theta={"gwb_clm": _clm(R, 1)})
    with pytest.raises(ValueError, match="no_correlations"):
        _engine(no_correlations=True).generate(R, theta=th)
    eng = _engine()
    eng.gwb_mode = "grid"
    with pytest.raises(ValueError, match="grid"):
        eng.generate(R, theta=th)
    with pytest.raises(ValueError, match="TD mode"):
        _engine().generate_td(R, theta=th)
    with pytest.raises(ValueError, match="TD mode"):
        _engine()._theta_parts(th, R, td=True)                       # what generate_os(td=True) and its kin call first
    assert not eng._prepared


def test_likelihood_grid_keeps_refusing_the_key():
    from pta_replicator_amd import _hyper
    eng = _engine()
    with pytest.raises(ValueError, match="unknown"):
        _hyper.check_theta_os({"gwb_clm": _clm(3, 4)}, 3, 4, eng._rn, True)          # the grid's call: no gw
    # the matched noise model skips it, as it skips cw_*
    assert _hyper.check_theta_os({"gwb_clm": _clm(3, 4), "gwb_log10_A": np.full(3, -14.0)}, 3, 4, eng._rn, True, gw=eng._gw).keys() == {"gwb_log10_A"}


def test_prior_boxes():
    from pta_replicator_amd import _hyper
    eng = _engine(lmax=1)
    with pytest.raises(ValueError, match="lo <= hi"):
        eng.set_hyper_prior(gwb_clm=(1, -1))
    with pytest.raises(ValueError, match="finite"):
        eng.set_hyper_prior(gwb_clm=(0, np.inf))
    with pytest.raises(ValueError, match=r"\[3, 2\]"):
        eng.set_hyper_prior(gwb_clm=np.zeros((4, 2)))
    with pytest.raises(ValueError, match="lmax"):
        _engine(lmax=0).set_hyper_prior(gwb_clm=(-1, 1))
    with pytest.raises(ValueError, match="lmax"):
        _engine(no_correlations=True).set_hyper_prior(gwb_clm=(-1, 1))
    eng.set_hyper_prior(gwb_clm=[[-1, 1], [-0.5, 0.25], [0, 0]], gwb_log10_A=(-15, -14))
    lo, hi = _hyper.clm_bounds(eng._prior, eng._gw)
    assert np.array_equal(lo, [C00, -1, -0.5, 0]) and np.array_equal(hi, [C00, 1, 0.25, 0])     # c_00: the degenerate box of the configured value
    plo, phi = _hyper.prior_bounds(eng._prior, 4)                                                # the stream (7, 0) table does not grow
    assert len(plo) == _hyper.n_columns(4) and plo[0] == -15 and phi[0] == -14
    eng.set_hyper_prior(gwb_clm=(-1, 1))
    lo, hi = _hyper.clm_bounds(eng._prior, eng._gw)
    assert np.array_equal(lo[1:], [-1] * 3) and np.array_equal(hi[1:], [1] * 3)
    assert _hyper.clm_bounds({"gwb_gamma": (np.zeros(1), np.ones(1))}, eng._gw) is None
    assert _hyper.CLM_FIELD == 2 and _hyper.SPEC_FIELD == 1


# ---------------------------------------------------------------- joint weights ----------------------------------------------
def test_joint_weights_are_the_whitened_least_squares():
    from pta_replicator_amd import optimal_statistic as ost
    from oracle import pta_oracle as po
    rng = np.random.default_rng(7)
    P, lmax, R = 7, 1, 5
    locs = np.stack([rng.uniform(0, 2 * np.pi, P), np.arccos(rng.uniform(-1, 1, P))], axis=1)
    basis = np.array(po.correlated_basis(locs, lmax))
    ia, ib = np.triu_indices(P, 1)
    G = basis[:, ia, ib]                                             # [4, 21]
    den = rng.uniform(0.5, 2.0, len(ia))
    num = rng.normal(size=(R, len(ia)))
    Wj, cov, sigma = ost.joint_weights(G, den)
    ref = np.linalg.lstsq((G * np.sqrt(den)).T, (num / np.sqrt(den)).T, rcond=None)[0].T
    assert np.max(np.abs(num @ Wj.T - ref)) / np.max(np.abs(ref)) < 1e-10
    F = (G * den) @ G.T
    assert np.max(np.abs(cov - np.linalg.inv(F))) / np.max(np.abs(cov)) < 1e-10
    assert np.allclose(sigma, np.sqrt(np.diag(np.linalg.inv(F))), rtol=1e-10, atol=0)
    # the estimate is unbiased for the model E[num] = den * (x G)
    x = rng.normal(size=4)
    assert np.allclose((den * (x @ G)) @ Wj.T, x, rtol=0, atol=1e-10)


def test_joint_weights_refusals():
    from pta_replicator_amd import optimal_statistic as ost
    rng = np.random.default_rng(8)
    with pytest.raises(ValueError, match="pairs"):
        ost.joint_weights(rng.normal(size=(4, 3)), np.ones(3))        # P = 3 with lmax = 1
    G = rng.normal(size=(3, 10))
    G[2] = G[0] + G[1]                                                # collinear ORFs
    with pytest.raises(ValueError, match="singular"):
        ost.joint_weights(G, np.ones(10))
    eng = _engine(P=3)
    with pytest.raises(ValueError, match="pairs"):
        eng.prepare_optimal_statistic(components=4, anisotropy_lmax=1)
    for bad in (-1, 9, 1.5, True):
        with pytest.raises(ValueError, match="anisotropy_lmax"):
            eng.prepare_optimal_statistic(components=4, anisotropy_lmax=bad)
    with pytest.raises(ValueError, match="matched"):
        _engine(P=4).prepare_optimal_statistic(components=4, anisotropy_lmax=0, matched=True)
    assert not eng._prepared


def test_golden_basis_is_the_oracles():
    """tests/golden/aniso_basis_p81_l4.npz (scripts/gen_aniso_basis_golden.py), the reference of the GPU factor tests: a sample of its
    pairs re-derived from the oracle, bit for bit"""
    from helpers import load
    from oracle import pta_oracle as po
    z = load("aniso_basis_p81_l4.npz")
    locs, tri = z["locs"], z["tri"]
    P = len(locs)
    assert tri.shape == (25, P * (P + 1) // 2) and int(z["lmax"]) == 4 and np.all(np.isfinite(tri))
    iu = np.triu_indices(P)
    for a, b in [(0, 0), (0, 1), (2, 80), (16, 17), (67, 68), (80, 80), (33, 59)]:
        pair = np.array(po.correlated_basis(locs[[a, b]], 4))      # [25, 2, 2]
        at = np.flatnonzero((iu[0] == a) & (iu[1] == b))[0]
        assert np.array_equal(pair[:, 0, 1], tri[:, at]), (a, b)


# ---------------------------------------------------------------- C ABI ------------------------------------------------------
def test_symbols_are_declared_exported_and_bound():
    from pta_replicator_amd import _lib
    d = declared()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = set(re.findall(r" T (pta_\w+)", syms))
    for name in ANISO:
        assert name in d and name in exported and name in _lib.EXPORTS, name
        assert len(getattr(_lib.lib, name).argtypes) == d[name], name
    assert _lib.lib.pta_abi_version() == 8
    names = [f[0] for f in _lib.EngineHyper._fields_]
    assert names[-2:] == ["gw_mchol", "ld_gw_mchol"] and names[0] == "gw_scale"      # trailing members: the struct's old prefix keeps its layout
    assert _lib.EngineHyper().gw_mchol is None


def test_argument_errors_without_gpu():
    from pta_replicator_amd import _lib
    lib = _lib.lib

    def refused(rc, what):
        assert rc == PTA_E_ARG and what in _lib.last_error(), (rc, _lib.last_error())
    # ---- pta_gwb_orf_factor(basis, n_lm, P, clm, ld_clm, R, Mchol, info, stream)
    def factor(p=(X,) * 4, n_lm=4, P=5, ld=4, R=3):
        return lib.pta_gwb_orf_factor(p[0], n_lm, P, p[1], ld, R, p[2], p[3], None)
    for null in range(4):
        refused(factor(tuple(None if i == null else X for i in range(4))), "NULL")
    refused(factor(n_lm=0), "n_lm=0")
    refused(factor(n_lm=82, ld=82), "n_lm=82")
    refused(factor(P=0), "P=0")
    refused(factor(R=0), "R=0")
    refused(factor(ld=3), "ld_clm=3")
    # ---- pta_gwb_mix_batched(Mchol, ld_m, P, G0, R, npts, ldg, G, variant, stream)
    def mix(p=(X,) * 3, ld_m=25, P=5, R=3, npts=10, ldg=10):
        return lib.pta_gwb_mix_batched(p[0], ld_m, P, p[1], R, npts, ldg, p[2], 0, None)
    for null in range(3):
        refused(mix(tuple(None if i == null else X for i in range(3))), "NULL")
    refused(mix(ld_m=24), "ld_m=24")
    refused(mix(ldg=9), "ldg=9")
    refused(mix(P=0, ld_m=0), "P=0")
    refused(mix(R=0), "R=0")
    refused(mix(R=65536), "too large")
