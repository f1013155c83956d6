"""A catalogue of CW sources per realisation (cw_* theta of shape [R, S], cw_count, set_cw_prior(n_sources=S)) on the MI355X: against
the long-double sum of the reference's waveform, against the single-source path of the same engine, the bit-for-bit identities
(composition with the other signals, batch independence, count = slice, count 0 = no CW), the composition with TD mode, the OS, ln L and
the F-statistic, the sampled labels against philox_ref, a merging source inside a catalogue, and the headline shape."""
import numpy as np
import pytest
import torch

from cw_reference import corner_sources, wave_ld
from oracle import philox_ref
from test_gpu_cw import MODES, P, TREF_MJD, _engine, _radec, _scale

pytestmark = pytest.mark.gpu

L = np.longdouble
SRC = ("cos_gwtheta", "gwphi", "log10_mc", "log10_fgw", "amp", "phase0", "psi", "cos_inc")
MERGING = np.array([0.1, 2.0, 10.0, -7.2, -14.0, 1.0, 0.3, -0.4])   # the source of test_strain_scaling_and_merger


def _theta(src, pdist=None, count=None):
    """the cw_* theta dict of a [R, S, 8] source array (strain amplitudes)"""
    th = {("cw_log10_h" if k == "amp" else "cw_" + k): np.ascontiguousarray(src[:, :, j]) for j, k in enumerate(SRC)}
    if pdist is not None:
        th["cw_pdist"] = np.asarray(pdist, dtype=np.float64)
    if count is not None:
        th["cw_count"] = np.asarray(count)
    return th


def _column(th, s):
    """source s of a catalogue theta as single-source theta ([R] keys)"""
    return {k: (v if k == "cw_pdist" else v[:, s].copy()) for k, v in th.items() if k != "cw_count"}


def _sources(R, S, seed):
    return corner_sources(R * S, seed=seed).reshape(R, S, 8)


def _mode(evolve, phase_approx):
    return 0 if evolve else (1 if phase_approx else 2)


def _ld_sum(toa, radec, srcs, pdist, mode, psr_term, tref):
    """(long-double sum of the sources' references, sum of the RMS scales their errors are measured against)"""
    total, scale = np.zeros(len(toa), dtype=L), 0.0
    for s in srcs:
        ref = wave_ld(toa, *radec, s, True, pdist, mode, psr_term, tref)
        scale += _scale(ref, wave_ld(toa, *radec, s, True, pdist, mode, False, tref)) if psr_term else float(np.sqrt(np.mean(ref ** 2)))
        total = total + ref.astype(L)
    return total, scale


def _rel(dev, total, scale):
    if scale == 0:
        return 0.0 if not np.any(dev) else np.inf
    return float(np.sqrt(np.mean(((dev.astype(L) - total).astype(np.float64)) ** 2)) / scale)


@pytest.mark.parametrize("evolve,phase_approx,psr_term", MODES)
def test_catalogue_matches_long_double_sum(evolve, phase_approx, psr_term):
    """R = 17 realisations (no multiple of a realisation group) x S = 7 sources on the ragged 6-pulsar array, ragged counts (0, 1 and 7
    among them, NaN past the count), cw_pdist [R, P]: per (r, a) against the long-double sum, <= 1e-9 sum_s scale_s."""
    R, S = 17, 7
    src = _sources(R, S, seed=5)
    rng = np.random.default_rng(6)
    pdist = rng.uniform(0.5, 2.0, (R, P))
    count = rng.integers(0, S + 1, R)
    count[:3] = [0, 1, 7]
    live = np.arange(S)[None, :] < count[:, None]
    tref = 0.0 if psr_term else TREF_MJD
    eng = _engine(noise=False, psrTerm=psr_term, evolve=evolve, phase_approx=phase_approx, tref=tref)
    given = np.where(live[:, :, None], src, np.nan)
    cw = eng.generate_per_signal(R, r0=3, theta=_theta(given, pdist, count))["cw"].cpu().numpy()
    assert np.all(np.isfinite(cw))
    mode, radec = _mode(evolve, phase_approx), _radec(eng)
    worst = 0.0
    for r in range(R):
        for a in range(P):
            dev = cw[r, eng.off[a]:eng.off[a + 1]]
            total, scale = _ld_sum(eng.mjd[a] * 86400, radec[a], src[r, :count[r]], pdist[r, a], mode, psr_term, tref)
            if count[r] == 0:
                assert not np.any(dev), (r, a)
            worst = max(worst, _rel(dev, total, scale))
    print(f"mode {mode} psr_term {psr_term}: worst {worst:.3g}")
    assert worst <= 1e-9, worst


@pytest.mark.parametrize("evolve,phase_approx,psr_term", MODES)
def test_catalogue_matches_single_source_path(evolve, phase_approx, psr_term):
    """a catalogue of S = 3 against the sum of three single-source generate_per_signal(...)["cw"] calls (the kernels this engine had
    before the catalogue), per (r, a) on sum_s scale_s.  Both are fp64 evaluations of the same quantity; the bound is 1e-12, and where
    the two differ by more - the folded non-evolving modes with the pulsar term, whose phase constants round 1e5 rad at another place
    than the unfolded form does - twice the larger of the two paths' own long-double errors on these inputs, each of which has to
    meet the device bound 1e-9.
    Measured on an MI355X (catalogue - single; own long-double errors catalogue, single): evolve 0 with and without the pulsar term;
    without the pulsar term 1.7e-15 (phase_approx, monochromatic); with it phase_approx 1.05e-12 (5.1e-12, 5.3e-12: bound 1.06e-11)
    and monochromatic 1.82e-12 (2.6e-12, 2.6e-12: bound 5.2e-12)."""
    R, S = 8, 3
    src = _sources(R, S, seed=12)
    tref = TREF_MJD
    eng = _engine(noise=False, psrTerm=psr_term, evolve=evolve, phase_approx=phase_approx, tref=tref, pdist=1.3)
    th = _theta(src)
    cat = eng.generate_per_signal(R, theta=th)["cw"].cpu().numpy()
    single = np.zeros_like(cat)
    for s in range(S):
        single = single + eng.generate_per_signal(R, theta=_column(th, s))["cw"].cpu().numpy()
    mode, radec = _mode(evolve, phase_approx), _radec(eng)
    worst = own_cat = own_single = 0.0
    for r in range(R):
        for a in range(P):
            sl = slice(eng.off[a], eng.off[a + 1])
            total, scale = _ld_sum(eng.mjd[a] * 86400, radec[a], src[r], 1.3, mode, psr_term, tref)
            worst = max(worst, float(np.sqrt(np.mean((cat[r, sl] - single[r, sl]) ** 2)) / scale))
            own_cat, own_single = max(own_cat, _rel(cat[r, sl], total, scale)), max(own_single, _rel(single[r, sl], total, scale))
    print(f"mode {mode} psr_term {psr_term}: catalogue - single {worst:.3g}, own errors: catalogue {own_cat:.3g}, single {own_single:.3g}")
    assert own_cat <= 1e-9 and own_single <= 1e-9, (own_cat, own_single)
    if mode == 0 or not psr_term:
        assert worst <= 1e-12, worst
    else:
        assert worst <= max(1e-12, 2 * max(own_cat, own_single)), (worst, own_cat, own_single)


def test_identities_bit_for_bit():
    R, S = 24, 5
    eng = _engine(tref=TREF_MJD)
    src = _sources(R, S, seed=9)
    th_cw = _theta(src)
    rng = np.random.default_rng(3)
    th_h = dict(gwb_log10_A=rng.uniform(-15, -13.5, R), rn_gamma=rng.uniform(1, 5, (R, P)))
    cw = eng.generate_per_signal(R, r0=100, theta=th_cw)["cw"].cpu().numpy()
    # the catalogue's sum is formed first and added once
    both = eng.generate(R, r0=100, theta={**th_h, **th_cw}).cpu().numpy()
    hyp = eng.generate(R, r0=100, theta=th_h).cpu().numpy()
    assert np.array_equal(both, hyp + cw)
    only = eng.generate(R, r0=100, theta=th_cw).cpu().numpy()
    base = eng.generate(R, r0=100).cpu().numpy()
    assert np.array_equal(only, base + cw)
    assert np.sqrt(np.mean((only - base) ** 2)) > 1e-6 * np.sqrt(np.mean(base ** 2))   # the CW term is there
    # any r0 / batch split: row r is the same
    sub = eng.generate(5, r0=107, theta={k: v[7:12] for k, v in th_cw.items()}).cpu().numpy()
    assert np.array_equal(sub, only[7:12])
    eng.workspace_bytes = 1 << 20
    assert eng.max_batch(hyper=True, cw=S) < R
    small = eng.generate(R, r0=100, theta={**th_h, **th_cw}).cpu().numpy()
    assert np.array_equal(small, both)
    eng.workspace_bytes = 8 << 30
    # per-signal total is the combined pass
    sig = eng.generate_per_signal(R, r0=100, theta={**th_h, **th_cw})
    assert np.array_equal(sig["total"].cpu().numpy(), both) and np.array_equal(sig["cw"].cpu().numpy(), cw)
    # cw_count = c is theta sliced to [:, :c], whatever lies past the count; count 0 is the row without CW keys
    count = np.repeat([0, 1, 3, 5], R // 4)
    junk = np.where((np.arange(S)[None, :] < count[:, None])[:, :, None], src, np.nan)
    junk[1::2][np.isnan(junk[1::2])] = 1e30
    counted = eng.generate(R, r0=100, theta=_theta(junk, count=count)).cpu().numpy()
    counted_t = eng.generate(R, r0=100, theta={k: torch.as_tensor(v, device="cuda") for k, v in _theta(junk, count=count).items()})
    assert np.array_equal(counted_t.cpu().numpy(), counted)
    for c in (0, 1, 3, 5):
        rows = np.flatnonzero(count == c)
        if c == 0:
            assert np.array_equal(counted[rows], base[rows])
            continue
        cut = eng.generate(len(rows), r0=100 + rows[0], theta=_theta(src[rows, :c])).cpu().numpy()
        assert np.array_equal(counted[rows], cut), c
    # S = 1 through the catalogue path: the single source, added once
    one = eng.generate(R, r0=100, theta=_theta(src[:, :1])).cpu().numpy()
    cw1 = eng.generate_per_signal(R, r0=100, theta=_theta(src[:, :1]))["cw"].cpu().numpy()
    assert np.array_equal(one, base + cw1)


def test_td_os_lnl_and_fstat_composition():
    R, S = 12, 3
    eng = _engine(tref=TREF_MJD)
    eng._gw = None   # TD mode without the GWB keeps the dense factors small
    eng.prepare()
    src = _sources(R, S, seed=4)
    count = np.array([3, 0, 1, 2] * 3)
    th_cw = _theta(src, count=count)
    cw = eng.generate_per_signal(R, r0=9, theta=th_cw)["cw"].cpu().numpy()
    td = eng.generate_td(R, r0=9, theta=th_cw).cpu().numpy()
    td0 = eng.generate_td(R, r0=9).cpu().numpy()
    assert np.array_equal(td, td0 + cw)
    with pytest.raises(ValueError, match="TD mode"):
        eng.generate_td(R, theta={**th_cw, "rn_gamma": np.full((R, P), 3.0)})
    eng.prepare_optimal_statistic()
    rows = eng.generate(R, r0=9, theta=th_cw)
    a = eng.optimal_statistic(rows)
    b = eng.generate_os(R, r0=9, theta=th_cw, chunk=5)
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert torch.equal(a[k], b[k]), k
    rows_td = eng.generate_td(R, r0=9, theta=th_cw)
    a = eng.optimal_statistic(rows_td)
    b = eng.generate_os(R, r0=9, theta=th_cw, td=True, chunk=5)
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert torch.equal(a[k], b[k]), k
    # ln L on a 2-point grid and the F-statistic (J = 2, no sky), chunks that cut the realisations
    eng.prepare_likelihood(components=6, gwb_auto=-14.5)
    grid, _ = eng.theta_grid(gwb_log10_A=[-15.0, -14.0])
    ref = eng.log_likelihood(eng.generate(R, r0=9, theta=th_cw), grid)
    assert torch.equal(eng.generate_lnl(R, grid, r0=9, theta=th_cw, chunk=5)["lnl"], ref["lnl"])
    eng.prepare_f_statistic([1.21e-8, 2.33e-8])
    ref = eng.f_statistic(eng.generate(R, r0=9, theta=th_cw))
    got = eng.generate_f_statistic(R, r0=9, theta=th_cw, chunk=5)
    assert all(torch.equal(got[k], ref[k]) for k in ref)


def test_sampled_labels_and_reproduction():
    from pta_replicator_amd import _cw
    from pta_replicator_amd.engine import STREAM_CW, stream_id
    S, R, r0 = 4, 6, 40
    eng = _engine(tref=TREF_MJD, pdist=1.0)
    eng.set_hyper_prior(gwb_log10_A=(-15, -13.5), rn_gamma=(1, 5))
    _, th0 = eng.generate_sampled(R, r0=r0)
    pd_box = np.column_stack([np.full(P, 0.5), np.linspace(1, 3, P)])
    box = dict(log10_mc=(7, 10), log10_fgw=(-9, -7), log10_h=(-16, -13), pdist=pd_box)
    eng.set_cw_prior(**box)
    _, th1 = eng.generate_sampled(R, r0=r0)                # one source, labels [R]
    eng.set_cw_prior(n_sources=S, **box)
    out, th = eng.generate_sampled(R, r0=r0)
    for k in th0:                                          # GWB / RN labels are unchanged by the CW prior
        assert np.array_equal(th0[k].cpu().numpy(), th[k].cpu().numpy(), equal_nan=True), k
    assert set(th) == set(th0) | set(_cw.SRC_KEYS) | {"cw_log10_h", "cw_pdist"}
    lo, hi = _cw.prior_bounds(eng._cw_prior, P)
    cols = _cw.columns(P)
    for k in [k for k in th if k.startswith("cw_")]:
        c0, c1 = cols[k]
        got = th[k].cpu().numpy()
        assert got.shape == ((R, P) if k == "cw_pdist" else (R, S)), k
        for r in range(R):
            for s in range(1 if k == "cw_pdist" else S):   # pdist: stream (CW, 0), pairs 8 .. 8 + P - 1
                _, u2 = philox_ref.uniform_pairs(eng.seed, r0 + r, stream_id(STREAM_CW, s), len(lo))
                want = (lo + (hi - lo) * u2)[c0:c1]
                mine = got[r] if k == "cw_pdist" else got[r, s:s + 1]
                assert np.all(np.abs(mine - want) <= np.spacing(np.abs(want))), (k, r, s)
                assert np.all(mine >= lo[c0:c1]) and np.all(mine <= hi[c0:c1])
        # source 0 is the single-source draw; pdist is the same table
        assert np.array_equal(got if k == "cw_pdist" else got[:, 0], th1[k].cpu().numpy()), k
    again = eng.generate(R, r0=r0, theta=th).cpu().numpy()
    assert np.array_equal(again, out.cpu().numpy())
    # labels of (seed, r, s) do not depend on R, r0 or S
    eng.set_cw_prior(n_sources=7, **box)
    th7 = eng.sample_theta(3, r0=r0 + 2)
    for k in _cw.SRC_KEYS + ("cw_log10_h",):
        assert torch.equal(th7[k][:, :S], th[k][2:5]), k
    assert torch.equal(th7["cw_pdist"], th["cw_pdist"][2:5])
    # a CW-only catalogue prior without a pdist box
    eng2 = _engine(tref=TREF_MJD)
    eng2.set_cw_prior(n_sources=2, log10_mc=(7, 10), log10_fgw=(-9, -7), log10_dist=(1, 3))
    a, tha = eng2.generate_sampled(7, r0=40)
    b, _ = eng2.generate_sampled(1, r0=43)
    assert np.array_equal(a[3].cpu().numpy(), b[0].cpu().numpy())
    assert set(tha) == set(_cw.SRC_KEYS) | {"cw_log10_dist"} and tuple(tha["cw_psi"].shape) == (7, 2)
    assert np.array_equal(eng2.generate(7, r0=40, theta=tha).cpu().numpy(), a.cpu().numpy())


def test_merger_inside_a_catalogue():
    """a binary that merges mid-span among S = 3: zeros from that source only, no NaN."""
    eng = _engine(noise=False, psrTerm=False, tref=TREF_MJD)
    others = corner_sources(16, seed=3)[[4, 6]]
    src = np.stack([others[0], MERGING, others[1]])[None]
    cw = eng.generate_per_signal(1, theta=_theta(src))["cw"].cpu().numpy()[0]
    two = eng.generate_per_signal(1, theta=_theta(src[:, [0, 2]]))["cw"].cpu().numpy()[0]
    assert np.all(np.isfinite(cw))
    radec = _radec(eng)
    zeros = 0
    for a in range(P):
        toa = eng.mjd[a] * 86400
        sl = slice(eng.off[a], eng.off[a + 1])
        after = wave_ld(toa, *radec[a], MERGING, True, 1.0, 0, False, TREF_MJD) == 0
        zeros += after.sum()
        assert np.array_equal(cw[sl][after], two[sl][after])
        assert np.all(cw[sl][~after] != two[sl][~after])
        total, scale = _ld_sum(toa[~after], radec[a], src[0], 1.0, 0, False, TREF_MJD)
        if (~after).any():
            assert _rel(cw[sl][~after], total, scale) <= 1e-9
        total, scale = _ld_sum(toa, radec[a], src[0, [0, 2]], 1.0, 0, False, TREF_MJD)
        assert _rel(two[sl], total, scale) <= 1e-9 and np.any(two[sl])
    assert 0 < zeros < eng.n_toa


def test_headline_sampled_catalogue_against_long_double():
    """68 x 5000 with 32 sampled catalogues of 8 sources: 2 realisations x 68 pulsars against the long-double sum (<= 1e-9 sum_s
    scale_s), and out == generate(32) + cw bit for bit on those rows."""
    from bench import configure_engine, headline_array
    from pta_replicator_amd._position import ra_dec
    from pta_replicator_amd.engine import ReplicaEngine
    psrs, noise = headline_array(68, 5000)
    eng = configure_engine(ReplicaEngine(psrs, seed=21), noise)
    eng.set_cw(tref=TREF_MJD, pdist=1.2)
    eng.set_cw_prior(log10_mc=(7, 10), log10_fgw=(-9, -7), log10_h=(-16, -13), n_sources=8)
    out, th = eng.generate_sampled(32)
    rows = np.array([5, 30])
    sub = {k: v[torch.as_tensor(rows, device=v.device)] for k, v in th.items()}
    cw = eng.generate_per_signal(len(rows), theta=sub)["cw"].cpu().numpy()
    base = eng.generate(32).cpu().numpy()[rows]
    assert np.array_equal(out.cpu().numpy()[rows], base + cw)
    sub = {k: v.cpu().numpy() for k, v in sub.items()}
    radec = [ra_dec(p) for p in eng.psrs]
    worst = 0.0
    for i in range(len(rows)):
        src = np.stack([sub["cw_log10_h" if k == "amp" else "cw_" + k][i] for k in SRC], axis=1)   # [S, 8]
        for a in range(68):
            total, scale = _ld_sum(eng.mjd[a] * 86400, radec[a], src, 1.2, 0, True, TREF_MJD)
            worst = max(worst, _rel(cw[i, eng.off[a]:eng.off[a + 1]], total, scale))
    print(f"headline catalogue: worst {worst:.3g}")
    assert worst <= 1e-9, worst
