"""One continuous-wave source per realisation (ReplicaEngine.set_cw + cw_* theta, set_cw_prior + generate_sampled) on the MI355X:
against a long-double evaluation of the reference's waveform, against oracle.cgw_dt and the fixed add_cgw path where the reference's
formula is well conditioned, bit-for-bit composition with the other signals (throughput, TD, OS), batch independence, the label draws
against philox_ref, and the physics (strain scaling, merger)."""
import numpy as np
import pytest
import torch

from cw_reference import cgw_kwargs, corner_sources, phi_rad, theta_of, wave_ld
from helpers import relrms
from oracle import philox_ref
from oracle import pta_oracle as po

pytestmark = pytest.mark.gpu

P = 6
TREF_MJD = 53000 * 86400.0
_PSRS = []


def _psrs():
    """a ragged array: unequal TOA counts"""
    from pta_replicator_amd.simulate import ArrayTOAs, SimulatedPulsar, make_ideal
    if not _PSRS:
        rng = np.random.default_rng(11)
        for a in range(P):
            n = 150 + 37 * a
            mjd = np.sort(rng.uniform(53000, 57500, n))
            p = SimulatedPulsar(toas=ArrayTOAs(mjd, 0.5), name=f"J{a:04d}",
                                loc={"RAJ": float(rng.uniform(0, 24)), "DECJ": float(np.degrees(np.arcsin(rng.uniform(-1, 1))))})
            make_ideal(p)
            _PSRS.append(p)
    return _PSRS


def _engine(seed=31, noise=True, **cw):
    from pta_replicator_amd.engine import ReplicaEngine
    eng = ReplicaEngine(_psrs(), seed=seed)
    eng.td_warmup = False
    if noise:
        eng.set_white_noise(efac=1.1, log10_equad=-6.5)
        eng.set_red_noise([-14.0, -13.6, None, -14.3, -13.9, -14.8], [3.0, 2.2, None, 4.1, 3.3, 1.5], components=20)
        eng.set_gwb(-14.4, 13. / 3.)
    if cw is not None:
        eng.set_cw(**cw)
    return eng


def _radec(eng):
    from pta_replicator_amd._position import ra_dec
    return [ra_dec(p) for p in eng.psrs]


def _scale(ref, ref_earth):
    """RMS of the larger of the two terms a pulsar-term residual is the difference of (tests/test_cw_host.py)"""
    return max(np.sqrt(np.mean(ref ** 2)), np.sqrt(np.mean(ref_earth ** 2)), np.sqrt(np.mean((ref - ref_earth) ** 2)))


def _err(dev, ref, scale=None):
    if not np.any(ref):
        return 0.0 if not np.any(dev) else np.inf
    return float(np.sqrt(np.mean((dev - ref) ** 2)) / (scale if scale is not None else np.sqrt(np.mean(ref ** 2))))


MODES = [(True, False, True), (True, False, False), (False, True, True), (False, True, False), (False, False, True), (False, False, False)]


@pytest.mark.parametrize("evolve,phase_approx,psr_term", MODES)
def test_cw_matches_long_double_reference(evolve, phase_approx, psr_term):
    """R = 64 explicit sources over log10 mc in [7, 10], log10 fgw in [-9, -7] on a ragged 6-pulsar array: per (r, a) against the
    long-double reference (<= 1e-9), against oracle.cgw_dt where Phi <= 1e5 rad (<= 2e-10)."""
    R = 64
    src = corner_sources(R, seed=5, amp_is_h=True)
    rng = np.random.default_rng(6)
    pdist = rng.uniform(0.5, 2.0, (R, P))
    tref = 0.0 if psr_term else TREF_MJD
    eng = _engine(noise=False, psrTerm=psr_term, evolve=evolve, phase_approx=phase_approx, tref=tref)
    half = theta_of(src, True, pdist)
    cw = eng.generate_per_signal(R, r0=3, theta=half)["cw"].cpu().numpy()
    assert np.all(np.isfinite(cw))
    mode = 0 if evolve else (1 if phase_approx else 2)
    radec = _radec(eng)
    worst_ld = worst_po = 0.0
    npo = 0
    for r in range(R):
        for a in range(P):
            ra, dec = radec[a]
            dev = cw[r, eng.off[a]:eng.off[a + 1]]
            toa = eng.mjd[a] * 86400
            ref = wave_ld(toa, ra, dec, src[r], True, pdist[r, a], mode, psr_term, tref)
            scale = _scale(ref, wave_ld(toa, ra, dec, src[r], True, pdist[r, a], mode, False, tref)) if psr_term else None
            worst_ld = max(worst_ld, _err(dev, ref, scale))
            if phi_rad(src[r, 2], src[r, 3]) <= 1e5:
                with np.errstate(invalid="ignore"):
                    ref = po.cgw_dt(eng.mjd[a], np.pi / 2 - dec, ra, pdist=pdist[r, a], psrTerm=psr_term, evolve=evolve,
                                    phase_approx=phase_approx, tref=tref, **cgw_kwargs(src[r], True))
                worst_po = max(worst_po, _err(dev, np.where(np.isnan(ref), 0.0, ref), scale))
                npo += 1
    assert npo >= 6 * P
    assert worst_ld <= 1e-9, worst_ld
    assert worst_po <= 2e-10, worst_po


@pytest.mark.parametrize("evolve,phase_approx", [(True, False), (False, True), (False, False)])
def test_cw_matches_fixed_add_cgw_path(evolve, phase_approx):
    """a well-conditioned source as theta against an engine with add_cgw(**source) (its 'det' entry): <= 2e-10."""
    src = corner_sources(8, seed=2, amp_is_h=False)
    src[:, 2], src[:, 3] = np.linspace(9.2, 9.8, 8), np.linspace(-8.0, -7.4, 8)
    assert np.all(phi_rad(src[:, 2], src[:, 3]) <= 1e5)
    eng = _engine(noise=False, evolve=evolve, phase_approx=phase_approx, tref=TREF_MJD, pdist=1.3)
    cw = eng.generate_per_signal(8, theta=theta_of(src, False))["cw"].cpu().numpy()
    for r in range(8):
        from pta_replicator_amd.engine import ReplicaEngine
        fx = ReplicaEngine(_psrs(), seed=1)
        fx.td_warmup = False
        fx.add_cgw(pdist=1.3, evolve=evolve, phase_approx=phase_approx, tref=TREF_MJD, **cgw_kwargs(src[r], False))
        det = fx.generate_per_signal(1)["det"].cpu().numpy()[0]
        for a in range(P):
            sl = slice(eng.off[a], eng.off[a + 1])
            assert relrms(cw[r, sl], det[sl]) <= 2e-10, (r, a, relrms(cw[r, sl], det[sl]))


def test_composition_bit_for_bit():
    R = 24
    eng = _engine(tref=TREF_MJD)
    src = corner_sources(R, seed=9)
    th_cw = theta_of(src, True)
    rng = np.random.default_rng(3)
    th_h = dict(gwb_log10_A=rng.uniform(-15, -13.5, R), rn_gamma=rng.uniform(1, 5, (R, P)))
    cw = eng.generate_per_signal(R, r0=100, theta=th_cw)["cw"].cpu().numpy()
    both = eng.generate(R, r0=100, theta={**th_h, **th_cw}).cpu().numpy()
    hyp = eng.generate(R, r0=100, theta=th_h).cpu().numpy()
    assert np.array_equal(both, hyp + cw)
    only = eng.generate(R, r0=100, theta=th_cw).cpu().numpy()
    base = eng.generate(R, r0=100).cpu().numpy()
    assert np.array_equal(only, base + cw)
    assert relrms(only, base) > 1e-6   # the CW term is there
    # any r0 / batch split: row r is the same
    sub = eng.generate(5, r0=107, theta={k: v[7:12] for k, v in th_cw.items()}).cpu().numpy()
    assert np.array_equal(sub, only[7:12])
    eng.workspace_bytes = 1 << 20
    small = eng.generate(R, r0=100, theta={**th_h, **th_cw}).cpu().numpy()
    assert eng.max_batch(hyper=True, cw=True) < R
    assert np.array_equal(small, both)
    eng.workspace_bytes = 8 << 30
    # per-signal total is the combined pass
    sig = eng.generate_per_signal(R, r0=100, theta={**th_h, **th_cw})
    assert np.array_equal(sig["total"].cpu().numpy(), both) and np.array_equal(sig["cw"].cpu().numpy(), cw)


def test_td_and_os_composition():
    R = 12
    eng = _engine(tref=TREF_MJD)
    eng._gw = None   # TD mode without the GWB keeps the dense factors small
    eng.prepare()
    src = corner_sources(R, seed=4)
    th_cw = theta_of(src, True)
    cw = eng.generate_per_signal(R, r0=9, theta=th_cw)["cw"].cpu().numpy()
    td = eng.generate_td(R, r0=9, theta=th_cw).cpu().numpy()
    td0 = eng.generate_td(R, r0=9).cpu().numpy()
    assert np.array_equal(td, td0 + cw)
    with pytest.raises(ValueError, match="TD mode"):
        eng.generate_td(R, theta={**th_cw, "rn_gamma": np.full((R, P), 3.0)})
    with pytest.raises(ValueError, match="TD mode"):
        eng.generate_td(R, theta={"rn_gamma": np.full((R, P), 3.0)})
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
    with pytest.raises(ValueError, match="TD mode"):
        eng.generate_os(R, theta={"rn_gamma": np.full((R, P), 3.0)}, td=True)


def test_sampled_labels_and_reproduction():
    from pta_replicator_amd import _cw
    from pta_replicator_amd.engine import STREAM_CW, stream_id
    eng = _engine(tref=TREF_MJD, pdist=1.0)
    eng.set_hyper_prior(gwb_log10_A=(-15, -13.5), rn_gamma=(1, 5))
    _, th0 = eng.generate_sampled(6, r0=40)
    pd_box = np.column_stack([np.full(P, 0.5), np.linspace(1, 3, P)])
    eng.set_cw_prior(log10_mc=(7, 10), log10_fgw=(-9, -7), log10_h=(-16, -13), pdist=pd_box)
    out, th = eng.generate_sampled(6, r0=40)
    # GWB / RN labels are unchanged by the CW prior
    for k in th0:
        assert np.array_equal(th0[k].cpu().numpy(), th[k].cpu().numpy(), equal_nan=True), k
    assert set(th) == set(th0) | set(_cw.SRC_KEYS) | {"cw_log10_h", "cw_pdist"}
    lo, hi = _cw.prior_bounds(eng._cw_prior, P)
    cols = _cw.columns(P)
    for r in range(6):
        _, u2 = philox_ref.uniform_pairs(eng.seed, 40 + r, stream_id(STREAM_CW, 0), len(lo))
        want = lo + (hi - lo) * u2
        for k in [k for k in th if k.startswith("cw_")]:
            c0, c1 = cols[k]
            got = np.atleast_1d(th[k][r].cpu().numpy())
            assert np.all(np.abs(got - want[c0:c1]) <= np.spacing(np.abs(want[c0:c1]))), (k, r)
            assert np.all(got >= lo[c0:c1]) and np.all(got <= hi[c0:c1])
    again = eng.generate(6, r0=40, theta=th).cpu().numpy()
    assert np.array_equal(again, out.cpu().numpy())
    # a CW-only prior: labels keyed by (seed, realisation)
    eng2 = _engine(tref=TREF_MJD)
    eng2.set_cw_prior(log10_mc=(7, 10), log10_fgw=(-9, -7), log10_dist=(1, 3))
    a, tha = eng2.generate_sampled(7, r0=40)
    b, thb = eng2.generate_sampled(1, r0=43)
    assert np.array_equal(a[3].cpu().numpy(), b[0].cpu().numpy())
    assert set(tha) == set(_cw.SRC_KEYS) | {"cw_log10_dist"}
    assert np.array_equal(eng2.generate(7, r0=40, theta=tha).cpu().numpy(), a.cpu().numpy())


def test_strain_scaling_and_merger():
    eng = _engine(noise=False, psrTerm=False, tref=TREF_MJD)
    src = corner_sources(4, seed=1)
    th = theta_of(src, True)
    a = eng.generate_per_signal(4, theta=th)["cw"].cpu().numpy()
    th2 = dict(th, cw_log10_h=th["cw_log10_h"] + 0.3)
    b = eng.generate_per_signal(4, theta=th2)["cw"].cpu().numpy()
    for r in range(4):
        assert np.any(a[r]) and relrms(b[r], a[r] * 10 ** 0.3) < 1e-14, r
    # a binary that merges mid-span: finite before the merger (long-double reference), zeros after, no NaN
    m = np.array([[0.1, 2.0, 10.0, -7.2, -14.0, 1.0, 0.3, -0.4]])
    cw = eng.generate_per_signal(1, theta=theta_of(m, True))["cw"].cpu().numpy()[0]
    assert np.all(np.isfinite(cw))
    radec = _radec(eng)
    zeros = 0
    for a_ in range(P):
        toa = eng.mjd[a_] * 86400
        dev = cw[eng.off[a_]:eng.off[a_ + 1]]
        ref = wave_ld(toa, *radec[a_], m[0], True, 1.0, 0, False, TREF_MJD)
        after = ref == 0
        zeros += after.sum()
        assert np.all(dev[after] == 0)
        assert _err(dev[~after], ref[~after]) < 1e-9
    assert 0 < zeros < eng.n_toa


def test_headline_sampled_against_long_double():
    """68 x 5000 with 1024 sampled sources: 16 realisations x 68 pulsars against the long-double reference (<= 1e-9)."""
    from bench import configure_engine, headline_array
    from pta_replicator_amd.engine import ReplicaEngine
    psrs, noise = headline_array(68, 5000)
    eng = configure_engine(ReplicaEngine(psrs, seed=21), noise)
    eng.set_cw(tref=TREF_MJD, pdist=1.2)
    eng.set_cw_prior(log10_mc=(7, 10), log10_fgw=(-9, -7), log10_h=(-16, -13))
    out, th = eng.generate_sampled(1024)
    rows = np.arange(0, 1024, 64)
    sub = {k: v[torch.as_tensor(rows, device=v.device)] for k, v in th.items()}
    cw = eng.generate_per_signal(len(rows), theta=sub)["cw"].cpu().numpy()
    base = eng.generate(1024).cpu().numpy()[rows]
    assert np.array_equal(out.cpu().numpy()[rows], base + cw)
    sub = {k: v.cpu().numpy() for k, v in sub.items()}
    from pta_replicator_amd._position import ra_dec
    radec = [ra_dec(p) for p in eng.psrs]
    worst = 0.0
    for i in range(len(rows)):
        src = np.array([sub[k][i] for k in ("cw_cos_gwtheta", "cw_gwphi", "cw_log10_mc", "cw_log10_fgw", "cw_log10_h", "cw_phase0",
                                            "cw_psi", "cw_cos_inc")])
        for a in range(68):
            toa = eng.mjd[a] * 86400
            ref = wave_ld(toa, *radec[a], src, True, 1.2, 0, True, TREF_MJD)
            scale = _scale(ref, wave_ld(toa, *radec[a], src, True, 1.2, 0, False, TREF_MJD))
            worst = max(worst, _err(cw[i, eng.off[a]:eng.off[a + 1]], ref, scale))
    assert worst <= 1e-9, worst
