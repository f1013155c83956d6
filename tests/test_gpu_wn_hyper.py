"""Per-realisation white noise in throughput mode (theta's wn_efac / wn_log10_equad / wn_log10_ecorr per backend group) on the
MI355X: against engines configured with theta_r, against a NumPy evaluation of the dumped draws, the per-signal split, exact
scaling, TOAs in no group, placement independence, views, the prior draws against philox_ref, and through a statistic."""
import numpy as np
import pytest
import torch

from oracle import philox_ref

pytestmark = pytest.mark.gpu

P = 6
RN_A = [-14.0, -13.6, None, -14.3, -13.9, -14.8]
RN_G = [3.0, 2.2, None, 4.1, 3.3, 1.5]
GW_A, GW_G = -14.4, 13. / 3.
EFAC, L10_EQUAD, L10_ECORR = np.array([1.1, 0.9]), np.array([-6.5, -6.8]), np.array([-6.6, -6.9])
NO_ECORR = 2     # the pulsar with log10_ecorr = None
SHUFFLED = 4     # the pulsar whose TOAs are in shuffled order: 298 TOAs, its full tile spans ~298 epochs > 2 PTA_ENGINE_EPMAX
FLAGS = ("A", "B", "C")   # "C" is in no group
U = 2.0 ** -53


def _rms_rel(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))


def _psrs(seed=11, n0=150):
    """the ragged array of test_gpu_hyper.py (150 + 37 a TOAs: pulsar 5 has a full tile and a short one) with a third flag on a few
    TOAs, per-TOA errors, some TOAs sharing an epoch, and one pulsar in shuffled order"""
    from pta_replicator_amd.simulate import ArrayTOAs, SimulatedPulsar, make_ideal
    rng = np.random.default_rng(seed)
    out = []
    for a in range(P):
        n = n0 + 37 * a
        mjd = np.sort(rng.uniform(53000, 57500, n))
        mjd[1::12] = mjd[0::12][:len(mjd[1::12])] + 0.01     # a second TOA in some epochs
        which = rng.integers(0, 2, n)
        which[rng.choice(n, 9, replace=False)] = 2
        err = rng.uniform(0.2, 0.9, n)
        if a == SHUFFLED:
            order = rng.permutation(n)
            mjd, which, err = mjd[order], which[order], err[order]
        p = SimulatedPulsar(toas=ArrayTOAs(mjd, err, flags=[{"f": FLAGS[k]} for k in which]), name=f"J{a:04d}",
                            loc={"RAJ": float(rng.uniform(0, 24)), "DECJ": float(np.degrees(np.arcsin(rng.uniform(-1, 1))))})
        make_ideal(p)
        out.append(p)
    return out


_PSRS = []


def _engine(seed=77, efac=None, l10_equad=None, l10_ecorr=None, rn_A=RN_A, rn_g=RN_G, gw_A=GW_A, gw_g=GW_G, transform="auto", rng_fast=0,
            tnequad=False, backends=("A", "B")):
    """efac / l10_equad [P][2], l10_ecorr [P][2] (entry NO_ECORR ignored): the white noise of every (pulsar, backend); None = the base model.
    backends = FLAGS: the third flag is a group too (base model only)"""
    from pta_replicator_amd.engine import ReplicaEngine
    if not _PSRS:
        _PSRS.extend(_psrs())
    eng = ReplicaEngine(_PSRS, seed=seed)
    eng.td_warmup = False
    fl = [list(backends)] * P
    if len(backends) == 3:
        efac, l10_equad, l10_ecorr = ([np.append(x, x[0])] * P for x in (EFAC, L10_EQUAD, L10_ECORR))
    efac = [EFAC] * P if efac is None else [np.asarray(x) for x in efac]
    l10_equad = [L10_EQUAD] * P if l10_equad is None else [np.asarray(x) for x in l10_equad]
    l10_ecorr = [L10_ECORR] * P if l10_ecorr is None else [np.asarray(x) for x in l10_ecorr]
    l10_ecorr = [None if a == NO_ECORR else x for a, x in enumerate(l10_ecorr)]
    eng.set_white_noise(efac=efac, log10_equad=l10_equad, flags=fl, tnequad=tnequad)
    eng.set_jitter(log10_ecorr=l10_ecorr, flags=fl, coarsegrain=0.1)
    eng.set_red_noise(list(rn_A), list(rn_g), components=20)
    eng.set_gwb(gw_A, gw_g)
    eng.add_delays([1e-7 * np.sin(m / 50.0) for m in eng.mjd])
    eng.gwb_transform = transform
    eng.rng_fast = rng_fast
    return eng


G_WN, G_EC = 2 * P, 2 * (P - 1)


def _theta(R, seed=5):
    rng = np.random.default_rng(seed)
    th = dict(wn_efac=rng.uniform(0.5, 2.0, (R, G_WN)), wn_log10_equad=rng.uniform(-7.5, -6.0, (R, G_WN)),
              wn_log10_ecorr=rng.uniform(-7.5, -6.0, (R, G_EC)))
    th["wn_efac"][1, 3] = np.nan          # group (1, "B") as configured in realisation 1
    th["wn_log10_equad"][R - 1, 0] = np.nan
    th["wn_log10_equad"][1, 3] = np.nan
    th["wn_log10_ecorr"][0, 5] = np.nan
    return th


def _other_theta(R, seed=6):
    rng = np.random.default_rng(seed)
    return dict(gwb_log10_A=rng.uniform(-15, -13.5, R), gwb_gamma=rng.uniform(3, 5, R), rn_log10_A=rng.uniform(-15, -13, (R, P)),
                rn_gamma=rng.uniform(1, 5, (R, P)))


def _fixed_for(th, r):
    """configuration of an engine whose fixed parameters are theta_r (keys not given and NaN entries: the base model)"""
    def table(key, conf):
        if key not in th:
            return None
        row, out, g = th[key][r], [], 0
        for a in range(P):
            if key == "wn_log10_ecorr" and a == NO_ECORR:
                out.append(conf)
                continue
            v = row[g:g + 2]
            out.append(np.where(np.isnan(v), conf, v))
            g += 2
        return out
    cfg = dict(efac=table("wn_efac", EFAC), l10_equad=table("wn_log10_equad", L10_EQUAD), l10_ecorr=table("wn_log10_ecorr", L10_ECORR))
    if "gwb_log10_A" in th:
        cfg.update(gw_A=float(th["gwb_log10_A"][r]), gw_g=float(th["gwb_gamma"][r]),
                   rn_A=[None if RN_A[a] is None else float(th["rn_log10_A"][r, a]) for a in range(P)],
                   rn_g=[None if RN_A[a] is None else float(th["rn_gamma"][r, a]) for a in range(P)])
    return cfg


def test_groups_and_tile_table():
    """the group lists, and the host tile table: the shuffled pulsar's full tile takes the tile_epn == 0 path, the others stage"""
    from pta_replicator_amd import _lib
    eng = _engine().prepare()
    assert eng.wn_groups == [(a, f) for a in range(P) for f in ("A", "B")] and len(eng.wn_groups) == G_WN
    assert eng.ecorr_groups == [(a, f) for a in range(P) if a != NO_ECORR for f in ("A", "B")] and len(eng.ecorr_groups) == G_EC
    t_psr, _, t_count, _, t_epn = (x.cpu().numpy() for x in eng.d_tiles)
    assert list(t_count[t_psr == 5]) == [_lib.ENGINE_TILE, 335 - _lib.ENGINE_TILE]
    assert t_epn[(t_psr == SHUFFLED) & (t_count == _lib.ENGINE_TILE)][0] == 0
    assert np.all(t_epn[t_psr != SHUFFLED] > 0)


@pytest.mark.parametrize("transform,rng_fast", [("auto", 0), ("gemm", 0), ("auto", 1), ("gemm", 1)])
def test_theta_equals_fixed_parameter_engine(transform, rng_fast):
    """row r of generate(R, r0, theta) against generate(1, r0 + r) of an engine configured with theta_r's values: all three keys with
    NaN entries, and the same combined with GWB / red-noise keys"""
    R, r0 = 6, 1000
    eng = _engine(transform=transform, rng_fast=rng_fast).prepare()
    base = eng.generate(R, r0=r0).cpu().numpy()
    for th in (_theta(R), dict(_theta(R, seed=8), **_other_theta(R))):
        out = eng.generate(R, r0=r0, theta=th).cpu().numpy()
        for r in range(R if "gwb_log10_A" not in th else 2):
            ref = _engine(transform=transform, rng_fast=rng_fast, **_fixed_for(th, r)).prepare().generate(1, r0=r0 + r).cpu().numpy()[0]
            print(f"{transform} rng_fast={rng_fast} r={r}: vs fixed engine {_rms_rel(out[r], ref):.3g}, vs unchanged {_rms_rel(out[r], base[r]):.3g}")
            assert _rms_rel(out[r], ref) < 1e-12, (r, _rms_rel(out[r], ref))
            assert _rms_rel(out[r], base[r]) > 1e-6   # theta did change the realisation


@pytest.mark.parametrize("key", ["wn_efac", "wn_log10_equad", "wn_log10_ecorr"])
def test_each_key_alone(key):
    R, r0 = 3, 40
    th = {key: _theta(R)[key]}
    eng = _engine().prepare()
    out = eng.generate(R, r0=r0, theta=th).cpu().numpy()
    base = eng.generate(R, r0=r0).cpu().numpy()
    for r in range(R):
        ref = _engine(**_fixed_for(th, r)).prepare().generate(1, r0=r0 + r).cpu().numpy()[0]
        assert _rms_rel(out[r], ref) < 1e-12, (key, r, _rms_rel(out[r], ref))
        assert _rms_rel(out[r], base[r]) > 1e-6


def _host_terms(eng, th, r, r0):
    """(wn, sum |terms| of wn, ecorr, |term| of ecorr) [n_toa] of realisation r0 + r in NumPy from dump_draws, the configured vectors
    and theta_r"""
    d = eng.dump_draws(r0 + r)
    wn, wn_abs, ec, ec_abs = (np.zeros(eng.n_toa) for _ in range(4))
    tnequad = eng._wn["tnequad"]
    for a in range(P):
        sl = slice(eng.off[a], eng.off[a + 1])
        flags = eng._flag_array(a, "f")
        efac, equad = np.zeros(eng.counts[a]), np.zeros(eng.counts[a])
        for g, (b, f) in enumerate(eng.wn_groups):
            if b == a:
                e, q = th["wn_efac"][r, g], th["wn_log10_equad"][r, g]
                efac[flags == f] = EFAC[g % 2] if np.isnan(e) else e
                equad[flags == f] = 10 ** (L10_EQUAD[g % 2] if np.isnan(q) else q)
        z1, z2 = d["wn"][a]
        t1, t2 = (efac * eng.sigma_s[a]) * z1, (equad if tnequad else efac * equad) * z2
        wn[sl], wn_abs[sl] = t1 + t2, np.abs(t1) + np.abs(t2)
        if a == NO_ECORR:
            continue
        eflags = flags[eng.epoch_first[a]]
        ecorr = np.zeros(len(eflags))
        for g, (b, f) in enumerate(eng.ecorr_groups):
            if b == a:
                v = th["wn_log10_ecorr"][r, g]
                ecorr[eflags == f] = 10 ** (L10_ECORR[g % 2] if np.isnan(v) else v)
        term = (ecorr * d["ecorr"][a])[eng.epoch_of[a]]
        ec[sl], ec_abs[sl] = term, np.abs(term)
    return wn, wn_abs, ec, ec_abs


@pytest.fixture(scope="module")
def per_signal():
    """one generate_per_signal of the base engine with and without white-noise theta, shared by the tests below"""
    R, r0 = 6, 300
    th = _theta(R, seed=9)
    eng = _engine().prepare()
    sig = {k: v.cpu().numpy() for k, v in eng.generate_per_signal(R, r0=r0, theta=th).items()}
    fixed = {k: v.cpu().numpy() for k, v in eng.generate_per_signal(R, r0=r0).items()}
    return eng, th, R, r0, sig, fixed


def test_per_signal_against_host_reference(per_signal):
    """|delta| <= 16 * 2^-53 * sum |terms| per element: three products and two sums in fp64, fused or not, and 10^x of the device against
    NumPy's"""
    eng, th, R, r0, sig, _ = per_signal
    worst = [0.0, 0.0]
    for r in range(R):
        wn, wn_abs, ec, ec_abs = _host_terms(eng, th, r, r0)
        for j, (dev, ref, scale) in enumerate(((sig["wn"][r], wn, wn_abs), (sig["ecorr"][r], ec, ec_abs))):
            err = np.abs(dev - ref)
            nz = scale > 0
            worst[j] = max(worst[j], float(np.max(err[nz] / scale[nz])) / U)
            assert np.all(err <= 16 * U * scale), (r, j, float(np.max(err[nz] / scale[nz])) / U)
            assert np.all(dev[~nz] == 0.0)
    print(f"worst |delta| / sum|terms| in units of 2^-53: wn {worst[0]:.2f}, ecorr {worst[1]:.2f}")


def test_per_signal_split(per_signal):
    _, _, _, _, sig, fixed = per_signal
    for k in ("rn", "gwb", "det"):
        assert np.array_equal(sig[k], fixed[k]), k
    for k in ("wn", "ecorr"):
        assert not np.array_equal(sig[k], fixed[k]), k
    parts = sig["rn"] + sig["gwb"] + sig["wn"] + sig["ecorr"] + sig["det"]
    assert _rms_rel(parts, sig["total"]) < 1e-13


def test_zero_amplitude_toas(per_signal):
    """TOAs of flag "C" (in no group) and the epochs of the pulsar without ECORR get exactly 0"""
    eng, _, _, _, sig, _ = per_signal
    n_c = 0
    for a in range(P):
        flags = eng._flag_array(a, "f")
        sl = slice(eng.off[a], eng.off[a + 1])
        c = flags == "C"
        n_c += int(c.sum())
        assert np.all(sig["wn"][:, sl][:, c] == 0.0) and np.all(sig["wn"][:, sl][:, ~c] != 0.0)
        c_epoch = (flags[eng.epoch_first[a]] == "C")[eng.epoch_of[a]]    # an epoch's flag is its first TOA's
        if a == NO_ECORR:
            assert np.all(sig["ecorr"][:, sl] == 0.0)
        else:
            assert np.all(sig["ecorr"][:, sl][:, c_epoch] == 0.0) and np.all(sig["ecorr"][:, sl][:, ~c_epoch] != 0.0)
    assert n_c == 9 * P


def test_exact_scaling():
    """tnequad = False: both amplitudes carry efac, so doubling wn_efac doubles 'wn' exactly"""
    R, r0 = 4, 12
    th = _theta(R, seed=3)
    th["wn_efac"] = np.where(np.isnan(th["wn_efac"]), 1.25, th["wn_efac"])
    eng = _engine(tnequad=False).prepare()
    one = eng.generate_per_signal(R, r0=r0, theta=th)["wn"].cpu().numpy()
    two = eng.generate_per_signal(R, r0=r0, theta=dict(th, wn_efac=2 * th["wn_efac"]))["wn"].cpu().numpy()
    assert np.any(one != 0) and np.array_equal(two, 2 * one)


def test_tnequad_keeps_its_configured_meaning():
    R, r0 = 2, 5
    th = {k: np.where(np.isnan(v), -6.7 if "log10" in k else 1.3, v) for k, v in _theta(R, seed=4).items()}
    out = _engine(tnequad=True).prepare().generate(R, r0=r0, theta=th).cpu().numpy()
    for r in range(R):
        ref = _engine(tnequad=True, **_fixed_for(th, r)).prepare().generate(1, r0=r0 + r).cpu().numpy()[0]
        assert _rms_rel(out[r], ref) < 1e-12


def test_placement_independence_and_views():
    """R = 19 crosses a realisation group: a row is bit-identical in one call, in calls of 1, at another r0 slot, with workspace_bytes
    lowered to force several batches, and when out is a view starting at an odd column of a wider buffer with odd ld_out, whose other
    columns stay untouched"""
    R, r0 = 19, 70
    th = dict(_theta(R, seed=21), **{k: v for k, v in _other_theta(R).items() if k.startswith("rn_")})
    eng = _engine().prepare()
    full = eng.generate(R, r0=r0, theta=th).cpu().numpy()
    for r in (0, 7, 8, 18):
        one = eng.generate(1, r0=r0 + r, theta={k: v[r:r + 1] for k, v in th.items()}).cpu().numpy()[0]
        assert np.array_equal(one, full[r]), r
    part = eng.generate(R - 5, r0=r0 + 5, theta={k: v[5:] for k, v in th.items()}).cpu().numpy()
    assert np.array_equal(part, full[5:])
    small = _engine()
    small.workspace_bytes = 1
    small.prepare()
    assert small.max_batch(hyper=True) == 16 < R
    assert np.array_equal(small.generate(R, r0=r0, theta=th).cpu().numpy(), full)
    n = eng.n_toa
    assert n % 2 == 1
    wide = torch.full((R, n + 4), -7.0, dtype=torch.float64, device="cuda")
    assert wide.stride(0) % 2 == 1
    view = wide[:, 1:1 + n]
    assert eng.generate(R, r0=r0, out=view, theta=th) is view
    w = wide.cpu().numpy()
    assert np.array_equal(w[:, 1:1 + n], full)
    assert np.all(w[:, :1] == -7.0) and np.all(w[:, 1 + n:] == -7.0)


def test_prior():
    from pta_replicator_amd import _wn_hyper
    from pta_replicator_amd.engine import STREAM_HYPER, stream_id
    R, r0 = 7, 40
    hyper_box = dict(gwb_log10_A=(-15, -13), gwb_gamma=(3, 5), rn_log10_A=(-15, -13), rn_gamma=(1, 5))
    eng = _engine().prepare()
    plan = eng.plan
    eng.set_hyper_prior(**hyper_box)
    a, tha = eng.generate_sampled(R, r0=r0)
    ec_box = np.stack([np.linspace(-7.5, -7.0, G_EC), np.linspace(-6.5, -6.0, G_EC)], axis=1)
    boxes = dict(wn_efac=(0.5, 2.0), wn_log10_equad=(-7.5, -6.0), wn_log10_ecorr=ec_box)
    eng.set_hyper_prior(**hyper_box, **boxes)
    b, thb = eng.generate_sampled(R, r0=r0)
    assert eng.plan is plan
    assert set(thb) == set(tha) | set(_wn_hyper.KEYS)
    for k in tha:   # the other labels do not move
        assert np.array_equal(tha[k].cpu().numpy(), thb[k].cpu().numpy(), equal_nan=True), k
    assert not np.array_equal(a.cpu().numpy(), b.cpu().numpy())
    for k, n in (("wn_efac", G_WN), ("wn_log10_equad", G_WN), ("wn_log10_ecorr", G_EC)):
        lo, hi = (np.broadcast_to(np.asarray(boxes[k], dtype=float), (n, 2))[:, j] for j in (0, 1))
        got = thb[k].cpu().numpy()
        assert got.shape == (R, n)
        for r in range(R):
            _, u2 = philox_ref.uniform_pairs(eng.seed, r0 + r, stream_id(STREAM_HYPER, _wn_hyper.FIELD[k]), n)
            want = lo + (hi - lo) * u2
            assert np.all(np.abs(got[r] - want) <= np.spacing(np.abs(want))), (k, r)
            assert np.all(got[r] >= lo) and np.all(got[r] <= hi)
    # the sampled realisations are generate(theta) with the returned labels
    again = eng.generate(R, r0=r0, theta={k: torch.as_tensor(v.cpu().numpy()) for k, v in thb.items()}).cpu().numpy()
    assert np.array_equal(again, b.cpu().numpy())
    # keyed by realisation
    c, thc = eng.generate_sampled(1, r0=r0 + 3)
    assert np.array_equal(c[0].cpu().numpy(), b[3].cpu().numpy())
    # the boxes taken away again: everything is as it was; white-noise boxes alone: the fixed GWB / red noise with sampled white noise
    eng.set_hyper_prior(**hyper_box)
    a2, tha2 = eng.generate_sampled(R, r0=r0)
    assert set(tha2) == set(tha) and np.array_equal(a2.cpu().numpy(), a.cpu().numpy())
    eng.set_hyper_prior(**boxes)
    d, thd = eng.generate_sampled(R, r0=r0)
    assert set(thd) == set(_wn_hyper.KEYS)
    for k in thd:
        assert np.array_equal(thd[k].cpu().numpy(), thb[k].cpu().numpy()), k
    assert np.array_equal(d.cpu().numpy(), eng.generate(R, r0=r0, theta=thd).cpu().numpy())


def test_through_a_statistic():
    """(the optimal statistic needs a positive white-noise variance at every TOA, so here the third flag is a group too: three groups
    per pulsar, and every pulsar has ECORR groups but NO_ECORR)"""
    R, r0 = 5, 9
    rng = np.random.default_rng(13)
    th = dict(wn_efac=rng.uniform(0.5, 2.0, (R, 3 * P)), wn_log10_equad=rng.uniform(-7.5, -6.0, (R, 3 * P)),
              wn_log10_ecorr=rng.uniform(-7.5, -6.0, (R, 3 * (P - 1))))
    th["wn_efac"][2, 4] = np.nan
    eng = _engine(backends=FLAGS).prepare()
    assert len(eng.wn_groups) == 3 * P and len(eng.ecorr_groups) == 3 * (P - 1)
    eng.prepare_optimal_statistic(components=5, matched=True)
    direct = eng.optimal_statistic(eng.generate(R, r0=r0, theta=th))
    fused = eng.generate_os(R, r0=r0, theta=th, chunk=2)
    for k in ("A2", "snr"):
        assert np.array_equal(direct[k].cpu().numpy(), fused[k].cpu().numpy()), k
    plain = eng.generate_os(R, r0=r0)
    assert not np.array_equal(plain["A2"].cpu().numpy(), fused["A2"].cpu().numpy())
    with pytest.raises(ValueError, match="hold the white noise fixed"):
        eng.generate_os(R, r0=r0, theta=th, matched=True)
    with pytest.raises(ValueError, match="hold the white noise fixed"):
        eng.optimal_statistic(eng.generate(R, r0=r0), theta=th)
    with pytest.raises(ValueError, match="TD mode.*wn_efac"):
        eng.generate_td(R, r0=r0, theta=th)


def test_grid_mode():
    """gwb_mode "grid": the terms are added after pta_engine_synth there as well"""
    R, r0 = 3, 17
    th = _theta(R, seed=2)
    eng = _engine()
    eng.gwb_mode = "grid"
    out = eng.prepare().generate(R, r0=r0, theta=th).cpu().numpy()
    for r in range(R):
        ref = _engine(**_fixed_for(th, r))
        ref.gwb_mode = "grid"
        assert _rms_rel(out[r], ref.prepare().generate(1, r0=r0 + r).cpu().numpy()[0]) < 1e-12, r


def test_pulsars_as_groups_and_terms_configured_alone():
    """flags = None: the pulsar is its own group.  An engine with EFAC alone (no EQUAD, no ECORR configured) takes wn_log10_equad, which
    simply gives the group an EQUAD; an engine with ECORR alone (no set_white_noise) takes wn_log10_ecorr"""
    from pta_replicator_amd.engine import ReplicaEngine
    if not _PSRS:
        _PSRS.extend(_psrs())
    R, r0 = 3, 21
    rng = np.random.default_rng(17)

    def engine(efac=None, l10_equad=None, l10_ecorr=None):
        eng = ReplicaEngine(_PSRS, seed=3)
        eng.td_warmup = False
        if efac is not None:
            eng.set_white_noise(efac=list(efac), log10_equad=None if l10_equad is None else list(l10_equad))
        if l10_ecorr is not None:
            eng.set_jitter(log10_ecorr=list(l10_ecorr), coarsegrain=0.1)
        eng.set_gwb(GW_A, GW_G)
        return eng.prepare()
    base_efac = np.linspace(0.8, 1.3, P)
    eng = engine(efac=base_efac)
    assert eng.wn_groups == [(a, None) for a in range(P)] and eng.ecorr_groups == []
    th = {"wn_efac": rng.uniform(0.5, 2.0, (R, P)), "wn_log10_equad": rng.uniform(-7.0, -6.0, (R, P))}
    th["wn_efac"][0, 2] = np.nan
    out = eng.generate(R, r0=r0, theta=th).cpu().numpy()
    alone = eng.generate(R, r0=r0, theta={"wn_log10_equad": th["wn_log10_equad"]}).cpu().numpy()
    plain = eng.generate(R, r0=r0).cpu().numpy()
    for r in range(R):
        ef = np.where(np.isnan(th["wn_efac"][r]), base_efac, th["wn_efac"][r])
        ref = engine(efac=ef, l10_equad=th["wn_log10_equad"][r]).generate(1, r0=r0 + r).cpu().numpy()[0]
        assert _rms_rel(out[r], ref) < 1e-12, (r, _rms_rel(out[r], ref))
        ref = engine(efac=base_efac, l10_equad=th["wn_log10_equad"][r]).generate(1, r0=r0 + r).cpu().numpy()[0]
        assert _rms_rel(alone[r], ref) < 1e-12 and _rms_rel(alone[r], plain[r]) > 1e-6
    with pytest.raises(ValueError, match="set_jitter"):
        eng.generate(R, theta={"wn_log10_ecorr": np.zeros((R, P))})
    base_ecorr = np.linspace(-6.9, -6.4, P)
    eng = engine(l10_ecorr=base_ecorr)
    assert eng.wn_groups == [] and eng.ecorr_groups == [(a, None) for a in range(P)]
    th = {"wn_log10_ecorr": rng.uniform(-7.0, -6.0, (R, P))}
    th["wn_log10_ecorr"][1, 4] = np.nan
    out = eng.generate(R, r0=r0, theta=th).cpu().numpy()
    for r in range(R):
        ec = np.where(np.isnan(th["wn_log10_ecorr"][r]), base_ecorr, th["wn_log10_ecorr"][r])
        ref = engine(l10_ecorr=ec).generate(1, r0=r0 + r).cpu().numpy()[0]
        assert _rms_rel(out[r], ref) < 1e-12, (r, _rms_rel(out[r], ref))
    with pytest.raises(ValueError, match="set_white_noise"):
        eng.generate(R, theta={"wn_efac": np.ones((R, P))})
