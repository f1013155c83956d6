"""CPU checks of the catalogue of CW sources per realisation: the __host__ __device__ formulas of csrc/pta_cw_catalog.h compiled with
g++ (tests/cw_catalog/cw_catalog_host.cpp) - the folded non-evolving terms and the sum over the sources against a long-double
evaluation of the reference's waveform, the label draw of source s against philox_ref - and the validation of [R, S] theta, cw_count
and n_sources on an engine that is configured but not prepared (no GPU needed: every refusal happens before anything is launched)."""
import ctypes
import os
import subprocess
import types

import numpy as np
import pytest

from cw_reference import corner_sources, theta_of, wave_ld
from oracle import philox_ref
from test_cw_host import TREF_MJD, _engine, _p, _phat, _scale, _toas, ch  # noqa: F401  (ch: the single-source host library fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
L = np.longdouble
MERGING = np.array([0.1, 2.0, 10.0, -7.2, -14.0, 1.0, 0.3, -0.4])   # the source of test_strain_scaling_and_merger


@pytest.fixture(scope="module")
def cc(tmp_path_factory):
    out = tmp_path_factory.mktemp("cw_catalog") / "libcwcataloghost.so"
    src = os.path.join(HERE, "cw_catalog", "cw_catalog_host.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", str(out)])
    lib = ctypes.CDLL(str(out))
    d, i, u64, p = ctypes.c_double, ctypes.c_int, ctypes.c_uint64, ctypes.POINTER(ctypes.c_double)
    lib.cc_npar.argtypes = [i]
    lib.cc_uniform.argtypes = [u64, u64, i, i, p, p, p]
    lib.cc_params.argtypes = [p, i, i, p, d, i, i, p]
    lib.cc_sum.argtypes = [p, i, p, i, d, i, i, p]
    return lib


def _host_sum(cc, src, n, ra, dec, pdist, mode, psr_term, toa_s, tref):
    """the catalogue sum of the first n of the sources src [S, 8] for one pulsar, as the device forms it"""
    src = np.ascontiguousarray(src, dtype=np.float64)
    S = len(src)
    par = np.full(S * cc.cc_npar(mode), np.nan)
    cc.cc_params(_p(src), S, 1, _p(_phat(ra, dec)), pdist, mode, int(psr_term), _p(par))
    out = np.zeros(len(toa_s))
    cc.cc_sum(_p(par), n, _p(np.ascontiguousarray(toa_s)), len(toa_s), tref, mode, int(psr_term), _p(out))
    return out


def _ref(toa, ra, dec, src, pdist, mode, psr_term, tref):
    """(long-double reference of one source, the RMS its error is measured against: tests/test_cw_host.py)"""
    ref = wave_ld(toa, ra, dec, src, True, pdist, mode, psr_term, tref)
    if psr_term:
        return ref, _scale(ref, wave_ld(toa, ra, dec, src, True, pdist, mode, False, tref))
    return ref, float(np.sqrt(np.mean(ref ** 2)))


def _rms(x):
    return float(np.sqrt(np.mean(np.asarray(x, dtype=np.float64) ** 2)))


def _err(diff, scale):
    """RMS of diff over scale; a reference that is zero throughout (merged before the first TOA) demands exact zeros"""
    if scale == 0:
        return 0.0 if not np.any(diff) else np.inf
    return _rms(diff) / scale


def test_npar_is_what_the_headers_document(cc):
    from pta_replicator_amd import _lib
    assert [cc.cc_npar(m) for m in (0, 1, 2)] == [16, 8, 8] == list(_lib.CW_CATALOG_NPAR)
    header = open(os.path.join(HERE, "..", "include", "pta_replicator_amd.h")).read()
    assert "#define PTA_CW_CATALOG_NPAR_EVOLVE 16" in header and "#define PTA_CW_CATALOG_NPAR_FOLDED 8" in header


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("psr_term", [True, False])
@pytest.mark.parametrize("tref", [0.0, TREF_MJD])
def test_terms_match_long_double_reference(cc, mode, psr_term, tref):
    """per (source, pulsar): the evolving term and the FOLDED non-evolving ones over the corners of the usual CW prior, <= 1e-10 on the
    scale of tests/test_cw_host.py (the host bound of the unfolded form)."""
    _, toa = _toas()
    src = corner_sources(16, seed=3)
    rng = np.random.default_rng(1)
    worst = 0.0
    for r in range(len(src)):
        ra, dec = rng.uniform(0, 2 * np.pi), np.arcsin(rng.uniform(-1, 1))
        dev = _host_sum(cc, src[r:r + 1], 1, ra, dec, 1.2, mode, psr_term, toa, tref)
        ref, scale = _ref(toa, ra, dec, src[r], 1.2, mode, psr_term, tref)
        assert np.all(np.isfinite(dev))
        worst = max(worst, _err(dev - ref, scale))
    print(f"mode {mode} psr_term {psr_term} tref {tref}: worst {worst:.3g}")
    assert worst <= 1e-10, worst


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("psr_term", [True, False])
@pytest.mark.parametrize("S", [1, 2, 7])
def test_catalogue_sum_matches_long_double_sum(cc, mode, psr_term, S):
    """per pulsar: the sum over S sources against the long-double sum of the sources' references, <= 1e-10 sum_s scale_s (the
    per-source bound plus S eps of summation); the per-source errors are reported where it fails."""
    _, toa = _toas()
    allsrc = corner_sources(16, seed=3)
    rng = np.random.default_rng(7)
    worst = 0.0
    for k in range(4):
        src = allsrc[(np.arange(S) * 3 + k) % 16]
        ra, dec = rng.uniform(0, 2 * np.pi), np.arcsin(rng.uniform(-1, 1))
        dev = _host_sum(cc, src, S, ra, dec, 1.2, mode, psr_term, toa, TREF_MJD)
        refs = [_ref(toa, ra, dec, s, 1.2, mode, psr_term, TREF_MJD) for s in src]
        total = np.sum([r.astype(L) for r, _ in refs], axis=0)
        err = _err((dev.astype(L) - total).astype(np.float64), sum(sc for _, sc in refs))
        per_source = [_err(_host_sum(cc, src[s:s + 1], 1, ra, dec, 1.2, mode, psr_term, toa, TREF_MJD) - refs[s][0], refs[s][1])
                      for s in range(S)]
        assert err <= 1e-10, (k, err, per_source)
        worst = max(worst, err)
    print(f"mode {mode} psr_term {psr_term} S {S}: worst {worst:.3g}")


def test_count_cuts_the_sum_and_ignores_what_lies_past_it(cc):
    _, toa = _toas(200)
    src = corner_sources(7, seed=3)
    full = _host_sum(cc, src[:3], 3, 0.4, 0.9, 1.0, 2, True, toa, TREF_MJD)
    poisoned = src.copy()
    poisoned[3:] = np.nan
    assert np.array_equal(_host_sum(cc, poisoned, 3, 0.4, 0.9, 1.0, 2, True, toa, TREF_MJD), full)
    assert not np.any(_host_sum(cc, poisoned, 0, 0.4, 0.9, 1.0, 2, True, toa, TREF_MJD))


def test_one_merging_source_among_three(cc):
    """a binary that merges mid-span among S = 3: the sum is finite everywhere, and after that source's merger it is the sum of the
    other two (the merged source contributes exactly 0, per source)."""
    _, toa = _toas()
    others = corner_sources(16, seed=3)[[4, 6]]
    src = np.stack([others[0], MERGING, others[1]])
    ra, dec = 0.4, 0.9
    dev = _host_sum(cc, src, 3, ra, dec, 1.0, 0, False, toa, TREF_MJD)
    assert np.all(np.isfinite(dev))
    refs = [_ref(toa, ra, dec, s, 1.0, 0, False, TREF_MJD) for s in src]
    after = refs[1][0] == 0
    assert 0 < after.sum() < len(toa)
    two = refs[0][0].astype(L) + refs[2][0].astype(L)
    bound = 1e-10 * (refs[0][1] + refs[2][1])
    assert _rms((dev[after].astype(L) - two[after]).astype(np.float64)) <= bound
    assert np.array_equal(dev[after], _host_sum(cc, src[[0, 2]], 2, ra, dec, 1.0, 0, False, toa, TREF_MJD)[after])
    three = two + refs[1][0].astype(L)
    assert _rms((dev[~after].astype(L) - three[~after]).astype(np.float64)) <= 1e-10 * sum(sc for _, sc in refs)


def test_draw_map_matches_philox_ref(cc, ch):  # noqa: F811
    """label (r, s, j) = lo_j + (hi_j - lo_j) u2 of pair j of stream (8, s): within 1 ulp of NumPy's expression; source 0 is the
    single-source draw bit for bit."""
    from pta_replicator_amd import _cw
    from pta_replicator_amd.engine import STREAM_CW, stream_id
    P, S = 5, 6
    prior = _cw.make_prior(P, n_sources=S, log10_mc=(7, 10), log10_fgw=(-9, -7), log10_h=(-16, -13))
    assert prior["n_sources"] == S
    lo, hi = _cw.prior_bounds(prior, P)
    assert len(lo) == 8
    seed, r0, R = 0x0123456789ABCDEF, 77, 9
    out = np.zeros(R * S * 8)
    cc.cc_uniform(seed, r0, R, S, _p(lo), _p(hi), _p(out))
    out = out.reshape(R, S, 8)
    for r in range(R):
        for s in range(S):
            _, u2 = philox_ref.uniform_pairs(seed, r0 + r, stream_id(STREAM_CW, s), 8)
            ref = lo + (hi - lo) * u2
            assert np.all(np.abs(out[r, s] - ref) <= np.spacing(np.abs(ref))), (r, s)
            assert np.all(out[r, s] >= lo) and np.all(out[r, s] <= hi)
    single = np.zeros(R * 8)
    ch.ch_uniform(seed, r0, R, 8, _p(lo), _p(hi), _p(single))
    assert np.array_equal(out[:, 0, :], single.reshape(R, 8))
    assert not np.array_equal(out[:, 1, :], out[:, 0, :])


# ---------------------------------------------------------------- validation (no GPU) -------------------------------
def _catalogue(R, S, seed=0):
    """theta of R x S sources, every source key [R, S]"""
    src = corner_sources(R * S, seed=seed)
    return {k: v.reshape(R, S) for k, v in theta_of(src, True).items()}


def test_catalogue_theta_refusals_before_any_launch():
    R, S = 3, 4
    eng = _engine()
    ok = _catalogue(R, S)
    nan_live = dict(ok, cw_log10_mc=np.where(np.arange(S)[None, :] == 1, np.nan, ok["cw_log10_mc"]), cw_count=np.array([2, 4, 3]))
    cos_live = dict(ok, cw_cos_inc=np.where(np.arange(S)[None, :] == 0, 1.5, ok["cw_cos_inc"]), cw_count=np.array([1, 0, 1]))
    cases = [
        (dict(ok, cw_phase0=ok["cw_phase0"][:, 0]), r"mix the shapes \[R\] and \[R, S\]"),                       # mixed [R] / [R, S]
        ({k: (v[:, 0] if k != "cw_psi" else v) for k, v in ok.items()}, r"mix the shapes \[R\] and \[R, S\]"),
        (dict(ok, cw_phase0=ok["cw_phase0"][:, :3]), "shape"),                                                # unequal S
        (dict(ok, cw_log10_h=np.zeros((R + 1, S))), "shape"),
        (dict(ok, cw_count=np.array([0, 5, 1])), r"0 \.\. S = 4"),                                            # count out of range
        (dict(ok, cw_count=np.array([0, -1, 1])), r"0 \.\. S = 4"),
        (dict(ok, cw_count=np.array([1.0, 2.0, 3.0])), "integer"),                                            # non-integer
        (dict(ok, cw_count=np.array([True, False, True])), "integer"),
        (dict(ok, cw_count=np.array([1, 2])), "shape"),
        (nan_live, "non-finite"),                                                                             # NaN below the count
        (cos_live, r"\|cos\|"),
        (dict(ok, cw_pdist=np.ones((R, S + 1))), "shape"),                                                    # pdist stays [R, P]
        (dict(ok, cw_log10_mc=np.where(np.eye(R, S) > 0, np.inf, ok["cw_log10_mc"])), "non-finite"),
    ]
    single = theta_of(corner_sources(R), True)
    cases.append((dict(single, cw_count=np.array([1, 1, 1])), r"cw_count.*catalogue"))                       # count with [R] keys
    for theta, msg in cases:
        with pytest.raises(ValueError, match=msg):
            eng.generate(R, theta=theta)
        with pytest.raises(ValueError, match=msg):
            eng.generate_per_signal(R, theta=theta)
        with pytest.raises(ValueError, match=msg):
            eng.generate_td(R, theta=theta)
    assert not eng._prepared


def test_values_past_the_count_are_not_checked():
    from pta_replicator_amd import _cw
    R, S = 3, 4
    eng = _engine()
    ok = _catalogue(R, S)
    count = np.array([2, 0, 4])
    live = np.arange(S)[None, :] < count[:, None]
    th = {k: np.where(live, v, np.nan) for k, v in ok.items()}
    th["cw_cos_inc"] = np.where(live, ok["cw_cos_inc"], 7.0)
    th["cw_count"] = count
    out = _cw.check_theta(th, R, eng.P, eng._cw)
    assert set(out) == set(th) and _cw.n_sources(out) == S and _cw.is_catalog(out)
    import torch
    tt = {k: torch.as_tensor(v) for k, v in th.items()}
    assert set(_cw.check_theta(tt, R, eng.P, eng._cw)) == set(th)
    with pytest.raises(ValueError, match="non-finite"):
        _cw.check_theta(dict(tt, cw_count=torch.as_tensor([3, 0, 4])), R, eng.P, eng._cw)
    with pytest.raises(ValueError, match="integer"):
        _cw.check_theta(dict(tt, cw_count=torch.as_tensor([2.0, 0.0, 4.0])), R, eng.P, eng._cw)
    # S = 1 is a catalogue too; [R] keys are not
    one = _cw.check_theta(_catalogue(R, 1), R, eng.P, eng._cw)
    assert _cw.is_catalog(one) and _cw.n_sources(one) == 1
    single = _cw.check_theta(theta_of(corner_sources(R), True), R, eng.P, eng._cw)
    assert not _cw.is_catalog(single) and _cw.n_sources(single) == 1 and _cw.n_sources({}) == 0
    # a slice along axis 0 (what the chunked paths pass on) stays valid
    part = {k: v[1:3] for k, v in out.items()}
    assert set(_cw.check_theta(part, 2, eng.P, eng._cw)) == set(th)


def test_n_sources_validation_and_labels_layout():
    from pta_replicator_amd import _cw
    eng = _engine()
    box = dict(log10_mc=(7, 10), log10_fgw=(-9, -7), log10_h=(-16, -13))
    for bad in (0, -1, 1.5, True, "3", 1 << 25):
        with pytest.raises(ValueError, match="n_sources"):
            eng.set_cw_prior(n_sources=bad, **box)
    assert eng.set_cw_prior(**box)._cw_prior["n_sources"] is None
    assert eng.set_cw_prior(n_sources=1, **box)._cw_prior["n_sources"] == 1
    assert eng.set_cw_prior(n_sources=np.int64(5), **box)._cw_prior["n_sources"] == 5
    import torch
    prior = _cw.make_prior(4, n_sources=3, pdist=(0.5, 2.0), **box)
    table, catalog = torch.arange(2.0 * 12).reshape(2, 12), torch.arange(2.0 * 3 * 8).reshape(2, 3, 8)
    lab = _cw.labels(table, prior, 4, catalog)
    assert tuple(lab["cw_log10_h"].shape) == (2, 3) and torch.equal(lab["cw_log10_h"], catalog[:, :, 4])
    assert tuple(lab["cw_pdist"].shape) == (2, 4) and torch.equal(lab["cw_pdist"], table[:, 8:])
    assert tuple(_cw.labels(table, _cw.make_prior(4, **box), 4)["cw_psi"].shape) == (2,)
    assert not eng._prepared


def test_max_batch_counts_the_catalogue():
    """max_batch's byte budget on an engine whose plan is a stand-in (it reads rn_k, gw_npts, K and Nf of prepare() alone)."""
    eng = _engine()
    eng.plan, eng.K, eng.grid = types.SimpleNamespace(rn_k=20, gw_npts=400), 20, {"Nf": 2000}
    eng.workspace_bytes = 1 << 24
    P = eng.P
    today = int(max(16, min(65536, eng.workspace_bytes // (8 * P * (20 + 800) + 8 * 2000 + 8 * (P * 16 + 8 + P)))))
    assert eng.max_batch(hyper=True, cw=True) == eng.max_batch(hyper=True, cw=1) == today
    assert eng.max_batch(cw=True) == eng.max_batch(cw=1)
    assert eng.max_batch(hyper=True) > today and eng.max_batch(cw=False) == eng.max_batch(cw=0) == eng.max_batch()
    sizes = [eng.max_batch(hyper=True, cw=S) for S in (1, 2, 16, 128)]
    assert all(a > b for a, b in zip(sizes, sizes[1:])), sizes
    eng.workspace_bytes = 8 << 30
    assert eng.max_batch(cw=1 << 20) * P * (1 << 20) < 1 << 31   # one launch's index range
    with pytest.raises(ValueError, match="max_batch"):
        eng.max_batch(cw=-2)
