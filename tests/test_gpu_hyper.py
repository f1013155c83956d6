"""Per-realisation GWB / red-noise hyperparameters in throughput mode (ReplicaEngine.generate(theta=...), generate_per_signal,
set_hyper_prior + generate_sampled) on the MI355X: against engines configured with theta_r, against the CPU oracle on the
dumped draws, prior draws against philox_ref, and the amplitude scaling of the GWB."""
import numpy as np
import pytest
import torch

from helpers import relrms
from oracle import philox_ref
from oracle import pta_oracle as po

pytestmark = pytest.mark.gpu

P = 6
RN_A = [-14.0, -13.6, None, -14.3, -13.9, -14.8]
RN_G = [3.0, 2.2, None, 4.1, 3.3, 1.5]
GW_A, GW_G = -14.4, 13. / 3.


def _rms_rel(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))


def _psrs(P=P, seed=11, n0=150):
    """a ragged array: unequal TOA counts, two backends per pulsar"""
    from pta_replicator_amd.simulate import ArrayTOAs, SimulatedPulsar, make_ideal
    rng = np.random.default_rng(seed)
    out = []
    for a in range(P):
        n = n0 + 37 * a
        mjd = np.sort(rng.uniform(53000, 57500, n))
        which = rng.integers(0, 2, n)
        p = SimulatedPulsar(toas=ArrayTOAs(mjd, 0.5, flags=[{"f": ("A", "B")[k]} for k in which]), name=f"J{a:04d}",
                            loc={"RAJ": float(rng.uniform(0, 24)), "DECJ": float(np.degrees(np.arcsin(rng.uniform(-1, 1))))})
        make_ideal(p)
        out.append(p)
    return out


_PSRS = []


def _engine(seed=77, rn_A=RN_A, rn_g=RN_G, gw_A=GW_A, gw_g=GW_G, transform="auto", rng_fast=0, det=True, rn=True, wn=True):
    from pta_replicator_amd.engine import ReplicaEngine
    if not _PSRS:
        _PSRS.extend(_psrs())
    eng = ReplicaEngine(_PSRS, seed=seed)
    eng.td_warmup = False
    fl = [["A", "B"]] * P
    if wn:
        eng.set_white_noise(efac=[np.array([1.1, 0.9])] * P, log10_equad=[np.array([-6.5, -6.8])] * P, flags=fl)
        eng.set_jitter(log10_ecorr=[np.array([-6.6, -6.9])] * P, flags=fl, coarsegrain=0.1)
    if rn:
        eng.set_red_noise(list(rn_A), list(rn_g), components=20)
    eng.set_gwb(gw_A, gw_g)
    if det:
        eng.add_delays([1e-7 * np.sin(m / 50.0) for m in eng.mjd])
    eng.gwb_transform = transform
    eng.rng_fast = rng_fast
    return eng


def _theta(R, seed=5):
    rng = np.random.default_rng(seed)
    th = dict(gwb_log10_A=rng.uniform(-15, -13.5, R), gwb_gamma=rng.uniform(3, 5, R),
              rn_log10_A=rng.uniform(-15, -13, (R, P)), rn_gamma=rng.uniform(1, 5, (R, P)))
    th["rn_log10_A"][1, 3] = np.nan    # pulsar 3 as configured in realisation 1
    th["rn_gamma"][1, 3] = np.nan
    return th


def _fixed_for(th, r):
    """configuration of an engine whose fixed parameters are theta_r"""
    rn_A, rn_g = [], []
    for a in range(P):
        if RN_A[a] is None:
            rn_A.append(None)
            rn_g.append(None)
        elif np.isnan(th["rn_log10_A"][r, a]):
            rn_A.append(RN_A[a])
            rn_g.append(RN_G[a])
        else:
            rn_A.append(float(th["rn_log10_A"][r, a]))
            rn_g.append(float(th["rn_gamma"][r, a]))
    return dict(rn_A=rn_A, rn_g=rn_g, gw_A=float(th["gwb_log10_A"][r]), gw_g=float(th["gwb_gamma"][r]))


@pytest.mark.parametrize("transform,rng_fast", [("auto", 0), ("gemm", 0), ("auto", 1), ("gemm", 1)])
def test_theta_equals_fixed_parameter_engine(transform, rng_fast):
    R, r0 = 6, 1000
    th = _theta(R)
    eng = _engine(transform=transform, rng_fast=rng_fast).prepare()
    assert eng.use_czt == (transform == "auto")
    out = eng.generate(R, r0=r0, theta=th).cpu().numpy()
    base = eng.generate(R, r0=r0).cpu().numpy()
    for r in range(R):
        ref = _engine(transform=transform, rng_fast=rng_fast, **_fixed_for(th, r)).prepare().generate(1, r0=r0 + r).cpu().numpy()[0]
        assert _rms_rel(out[r], ref) < 1e-12, (r, _rms_rel(out[r], ref))
        assert _rms_rel(out[r], base[r]) > 1e-6   # theta did change the realisation


def test_theta_per_signal():
    R, r0 = 6, 300
    th = _theta(R, seed=9)
    eng = _engine().prepare()
    sig = {k: v.cpu().numpy() for k, v in eng.generate_per_signal(R, r0=r0, theta=th).items()}
    fixed = {k: v.cpu().numpy() for k, v in _engine().prepare().generate_per_signal(R, r0=r0).items()}
    for k in ("wn", "ecorr", "det"):
        assert np.array_equal(sig[k], fixed[k]), k
    for r in range(R):
        ref = {k: v.cpu().numpy()[0] for k, v in _engine(**_fixed_for(th, r)).prepare().generate_per_signal(1, r0=r0 + r).items()}
        for k in ("rn", "gwb"):
            assert _rms_rel(sig[k][r], ref[k]) < 1e-12, (k, r)
    parts = sig["rn"] + sig["gwb"] + sig["wn"] + sig["ecorr"] + sig["det"]
    assert _rms_rel(parts, sig["total"]) < 1e-13


def test_sampled_theta_against_oracle_headline():
    """68 x 5000 headline array with GWB (A, gamma) and all red-noise (A, gamma) drawn on chip: two realisations re-derived by the
    CPU oracle from dump_draws and theta_r."""
    from bench import configure_engine, headline_array
    from helpers import oracle_realisation
    from pta_replicator_amd.engine import ReplicaEngine
    psrs, noise = headline_array(68, 5000)
    eng = configure_engine(ReplicaEngine(psrs, seed=21), noise)
    eng.set_hyper_prior(gwb_log10_A=(-15, -14), gwb_gamma=(3, 5), rn_log10_A=(-15, -13), rn_gamma=(1, 5))
    r0 = 500
    out, th = eng.generate_sampled(2, r0=r0)
    out = out.cpu().numpy()
    th = {k: v.cpu().numpy() for k, v in th.items()}
    for r in range(2):
        nz = dict(noise)
        nz["gw_log10_A"] = float(th["gwb_log10_A"][r])
        nz["rn_log10_A"] = [None if a is None else float(th["rn_log10_A"][r, i]) for i, a in enumerate(noise["rn_log10_A"])]
        nz["rn_gamma"] = [None if a is None else float(th["rn_gamma"][r, i]) for i, a in enumerate(noise["rn_log10_A"])]
        for i, a in enumerate(noise["rn_log10_A"]):
            assert (a is None) == np.isnan(th["rn_log10_A"][r, i])
        ref = oracle_realisation(po, psrs, nz, eng.dump_draws(r0 + r), gw_gamma=float(th["gwb_gamma"][r]))
        worst = max(relrms(out[r, eng.off[a]:eng.off[a + 1]], ref[a]) for a in range(68))
        assert worst < 1e-10, (r, worst)


def test_prior_draws_keyed_by_realisation():
    from pta_replicator_amd import _hyper
    from pta_replicator_amd.engine import STREAM_HYPER, stream_id
    eng = _engine().prepare()
    plan = eng.plan
    box = np.array([[-15, -13.5], [-14, -13], [-16, -14], [-15, -14], [-14.5, -13], [-15, -13]])
    eng.set_hyper_prior(gwb_log10_A=(-15, -13), gwb_gamma=(3, 5), rn_log10_A=box, rn_gamma=(1, 5))
    a, tha = eng.generate_sampled(7, r0=40)
    b, thb = eng.generate_sampled(1, r0=43)
    assert np.array_equal(a[3].cpu().numpy(), b[0].cpu().numpy())
    tha = {k: v.cpu().numpy() for k, v in tha.items()}
    thb = {k: v.cpu().numpy() for k, v in thb.items()}
    assert set(tha) == set(_hyper.KEYS)
    for k in tha:
        assert np.array_equal(tha[k][3], thb[k][0], equal_nan=True), k
    lo, hi = _hyper.prior_bounds(eng._prior, P)
    cols = _hyper.columns(P)
    for r in range(7):
        _, u2 = philox_ref.uniform_pairs(eng.seed, 40 + r, stream_id(STREAM_HYPER, 0), _hyper.n_columns(P))
        want = lo + (hi - lo) * u2
        for k, (c0, c1) in cols.items():
            got = np.atleast_1d(tha[k][r])
            w = want[c0:c1].copy()
            if k.startswith("rn_"):
                w[[i for i in range(P) if RN_A[i] is None]] = np.nan
            close = np.isnan(w) | (np.abs(got - w) <= np.spacing(np.abs(w)))
            assert np.all(close) and np.array_equal(np.isnan(got), np.isnan(w)), (k, r)
            fin = ~np.isnan(got)
            assert np.all(got[fin] >= lo[c0:c1][fin]) and np.all(got[fin] <= hi[c0:c1][fin])
    # the sampled realisations are generate(theta) with the returned labels
    again = eng.generate(7, r0=40, theta={k: torch.as_tensor(v) for k, v in tha.items()}).cpu().numpy()
    assert np.array_equal(again, a.cpu().numpy())
    # a new box for one parameter: that parameter and the residuals change, the other labels do not, and nothing is re-prepared
    eng.set_hyper_prior(gwb_log10_A=(-14, -13), gwb_gamma=(3, 5), rn_log10_A=box, rn_gamma=(1, 5))
    c, thc = eng.generate_sampled(7, r0=40)
    assert eng.plan is plan
    thc = {k: v.cpu().numpy() for k, v in thc.items()}
    assert not np.any(thc["gwb_log10_A"] == tha["gwb_log10_A"])
    for k in ("gwb_gamma", "rn_log10_A", "rn_gamma"):
        assert np.array_equal(thc[k], tha[k], equal_nan=True), k
    assert not np.array_equal(c.cpu().numpy(), a.cpu().numpy())


def test_gwb_amplitude_scaling():
    """GWB only, gamma fixed, log10_A ~ U(-15, -13) over 4096 realisations: log(mean square) against ln(A) has slope 2."""
    eng = _engine(rn=False, wn=False, det=False)
    eng.set_hyper_prior(gwb_log10_A=(-15, -13))
    out, th = eng.generate_sampled(4096)
    ms = torch.mean(out ** 2, dim=1).cpu().numpy()
    lnA = th["gwb_log10_A"].cpu().numpy() * np.log(10.0)
    slope = np.polyfit(lnA, np.log(ms), 1)[0]
    assert abs(slope - 2.0) < 0.05, slope


@pytest.mark.parametrize("transform", ["auto", "gemm"])
def test_theta_equal_to_base_model(transform):
    R = 8
    eng = _engine(transform=transform).prepare()
    th = dict(gwb_log10_A=np.full(R, GW_A), gwb_gamma=np.full(R, GW_G),
              rn_log10_A=np.array([[np.nan if a is None else a for a in RN_A]] * R),
              rn_gamma=np.array([[np.nan if g is None else g for g in RN_G]] * R))
    a = eng.generate(R, r0=7, theta=th).cpu().numpy()
    b = eng.generate(R, r0=7).cpu().numpy()
    for r in range(R):
        assert _rms_rel(a[r], b[r]) < 1e-13, r


def test_red_noise_theta_in_grid_mode():
    """gwb_mode='grid': red-noise theta is honoured (the GWB grid factor is built for the configured spectrum)."""
    R, r0 = 2, 60
    th = _theta(R, seed=2)
    rn_th = {k: th[k] for k in ("rn_log10_A", "rn_gamma")}
    eng = _engine().prepare()
    eng.gwb_mode = "grid"
    out = eng.generate(R, r0=r0, theta=rn_th).cpu().numpy()
    for r in range(R):
        cfg = _fixed_for(th, r)
        cfg.update(gw_A=GW_A, gw_g=GW_G)
        ref = _engine(**cfg).prepare()
        ref.gwb_mode = "grid"
        assert _rms_rel(out[r], ref.generate(1, r0=r0 + r).cpu().numpy()[0]) < 1e-12, r


def test_refusals_on_a_prepared_engine():
    eng = _engine().prepare()
    R = 2
    with pytest.raises(ValueError, match="TD mode"):
        eng.generate_td(R, theta={"rn_gamma": np.full((R, P), 3.0)})
    with pytest.raises(ValueError, match="shape"):
        eng.generate(R, theta={"gwb_log10_A": torch.zeros(R + 1, dtype=torch.float64, device="cuda")})
    with pytest.raises(ValueError, match="non-finite"):
        eng.generate(R, theta={"gwb_gamma": torch.tensor([4.0, float("nan")], dtype=torch.float64, device="cuda")})
    eng.gwb_mode = "grid"
    with pytest.raises(ValueError, match="grid"):
        eng.generate(R, theta={"gwb_log10_A": np.full(R, -14.0)})
    user = _engine()
    user.set_gwb(GW_A, GW_G, userSpec=np.array([[1e-9, 1e-15], [1e-8, 1e-16], [1e-7, 1e-17]]))
    with pytest.raises(ValueError, match="userSpec"):
        user.generate(R, theta={"gwb_log10_A": np.full(R, -14.0)})
