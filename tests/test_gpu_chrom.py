"""The chromatic Gaussian process (set_chromatic_noise, theta's chrom_* keys, add_chromatic_noise) on the MI355X: against the NumPy
reference on philox_ref deviates, exact superposition on the engine without it, placement independence, the ties to the red noise at
one band and two, dump_draws / replay, the prior draws, and the fixed-noise statistics against host plans built from explicitly
concatenated columns."""
import numpy as np
import pytest
import torch

import chrom_reference as cr
from helpers import load, mjd_ld, relrms

pytestmark = pytest.mark.gpu

COUNTS = (37, 255, 256, 257, 298, 513)   # a short tile, one TOA short of a tile, a full tile, one past, shuffled, two tiles and one TOA
P = len(COUNTS)
SHUFFLED, NONE = 4, 2                      # the pulsar in shuffled TOA order; the pulsar without a chromatic process
BANDS = (820.0, 1440.0, 2300.0)            # two bands and a few TOAs at a third frequency
CH_A = [-13.2, -13.6, None, -13.9, -13.4, -14.1]
CH_G = [2.4, 3.1, None, 1.7, 3.8, 2.9]
RN_A = [-14.0, -13.6, -14.2, None, -13.9, -14.8]
RN_G = [3.0, 2.2, 3.5, None, 3.3, 1.5]
GW_A, GW_G = -14.4, 13. / 3.
TOL_SIG = 1e-11                            # the project's per-signal bound (tests/test_gpu_parity.py)


def _rg():
    from pta_replicator_amd import _lib
    return _lib.CHROM_RG


def _psrs(seed=11, one_band=None):
    from pta_replicator_amd.simulate import ArrayTOAs, SimulatedPulsar, make_ideal
    rng = np.random.default_rng(seed)
    out = []
    for a, n in enumerate(COUNTS):
        mjd = np.sort(rng.uniform(53000, 57500, n))
        mjd[1::12] = mjd[0::12][:len(mjd[1::12])] + 0.01     # a second TOA in some epochs
        band = rng.integers(0, 2, n)
        band[rng.choice(n, 5, replace=False)] = 2
        err = rng.uniform(0.2, 0.9, n)
        if a == SHUFFLED:
            order = rng.permutation(n)
            mjd, band, err = mjd[order], band[order], err[order]
        freqs = np.asarray(BANDS)[band] if one_band is None else np.full(n, one_band)
        p = SimulatedPulsar(toas=ArrayTOAs(mjd, err, flags=[{"f": "AB"[k & 1]} for k in band], freqs_mhz=freqs), name=f"J{a:04d}",
                            loc={"RAJ": float(rng.uniform(0, 24)), "DECJ": float(np.degrees(np.arcsin(rng.uniform(-1, 1))))})
        make_ideal(p)
        out.append(p)
    return out


_PSRS = {}


def _engine(chrom=True, components=30, seed=77, full=True, one_band=None, ch_A=CH_A, ch_g=CH_G):
    """white noise + ECORR + red noise + GWB (full) or white noise alone, with the chromatic process or without it"""
    from pta_replicator_amd.engine import ReplicaEngine
    if one_band not in _PSRS:
        _PSRS[one_band] = _psrs(one_band=one_band)
    eng = ReplicaEngine(_PSRS[one_band], seed=seed)
    eng.td_warmup = False
    eng.set_white_noise(efac=1.1, log10_equad=-6.6)
    if full:
        eng.set_jitter(log10_ecorr=-6.7, coarsegrain=0.1)
        eng.set_red_noise(list(RN_A), list(RN_G), components=20)
        eng.set_gwb(GW_A, GW_G)
    if chrom:
        eng.set_chromatic_noise(list(ch_A), list(ch_g), components=components)
    return eng


def _freqs(eng, a):
    return eng.psrs[a].toas.freqs_mhz


def _theta(R, seed=5):
    rng = np.random.default_rng(seed)
    th = dict(chrom_log10_A=rng.uniform(-14.5, -13.0, (R, P)), chrom_gamma=rng.uniform(1.0, 5.0, (R, P)))
    th["chrom_log10_A"][0, 1] = np.nan           # pulsar 1 as configured in realisation 0
    th["chrom_log10_A"][R - 1, :] = np.nan       # a whole row as configured
    th["chrom_gamma"][R - 1, 3] = np.nan
    return th


def _reference(eng, components, r0, R, th=None):
    """[R, n_toa] of the term through NumPy on philox_ref deviates; theta rows where given (NaN amplitude = as configured)"""
    ref = np.zeros((R, eng.n_toa))
    for r in range(R):
        for a in range(P):
            lA, g = CH_A[a], CH_G[a]
            if th is not None and lA is not None and not np.isnan(th["chrom_log10_A"][r, a]):
                lA, g = th["chrom_log10_A"][r, a], th["chrom_gamma"][r, a]
            z = cr.draws(eng.seed, r0 + r, a, components)
            ref[r, eng.off[a]:eng.off[a + 1]] = cr.term(eng.tdb_s[a], _freqs(eng, a), components, lA, g, z)
    return ref


def _check(eng, got, ref, what):
    worst = 0.0
    for r in range(got.shape[0]):
        for a in range(P):
            sl = slice(eng.off[a], eng.off[a + 1])
            if a == NONE:
                assert np.all(got[r, sl] == 0.0), (what, r)
            else:
                worst = max(worst, relrms(got[r, sl], ref[r, sl]))
    print(f"{what}: worst per-pulsar relative RMS deviation = {worst:.2e}")
    assert worst < TOL_SIG, (what, worst)


@pytest.mark.parametrize("components", [1, 7, 30])
def test_against_numpy(components):
    """K_c = 2, 14, 60 (fewer columns than one MFMA K-step, K_c mod 4 != 0, the default); R = 1, RG - 1, RG + 1, 2 RG + 1; the configured
    process, then theta rows with NaN entries; the pulsar without a process is exactly zero"""
    RG = _rg()
    eng = _engine(components=components, full=False).prepare()
    r0 = 3
    ref = _reference(eng, components, r0, 2 * RG + 1)
    for R in (1, RG - 1, RG + 1, 2 * RG + 1):
        sig = eng.generate_per_signal(R, r0=r0)
        assert set(sig) == {"total", "wn", "chrom"}
        _check(eng, sig["chrom"].cpu().numpy(), ref[:R], f"K_c={2 * components} R={R}")
    R = RG + 1
    th = _theta(R)
    got = eng.generate_per_signal(R, r0=r0, theta=th)["chrom"].cpu().numpy()
    _check(eng, got, _reference(eng, components, r0, R, th), f"K_c={2 * components} theta")
    last = eng.generate_per_signal(R, r0=r0)["chrom"].cpu().numpy()[R - 1]
    assert np.array_equal(got[R - 1], last)   # the all-NaN row is the configured process, bit for bit
    only_g = eng.generate_per_signal(2, r0=r0, theta={"chrom_gamma": th["chrom_gamma"][:2]})["chrom"].cpu().numpy()
    th_g = dict(chrom_log10_A=np.array([[np.nan if x is None else x for x in CH_A]] * 2), chrom_gamma=th["chrom_gamma"][:2])
    _check(eng, only_g, _reference(eng, components, r0, 2, th_g), "gamma alone")


def test_exact_superposition():
    """generate of the engine = generate of the engine without the process + the term, one fp64 add per element; every other
    per-signal entry is the one of the engine without it; with theta of both kinds too"""
    RG = _rg()
    R, r0 = 2 * RG + 1, 11
    with_c, without = _engine().prepare(), _engine(chrom=False).prepare()
    sig, sig0 = with_c.generate_per_signal(R, r0=r0), without.generate_per_signal(R, r0=r0)
    assert set(sig) == set(sig0) | {"chrom"}
    for k in sig0:
        if k != "total":
            assert torch.equal(sig[k], sig0[k]), k
    assert torch.equal(with_c.generate(R, r0=r0), without.generate(R, r0=r0) + sig["chrom"])
    assert torch.equal(sig["total"], sig0["total"] + sig["chrom"])
    assert float(sig["chrom"].abs().max()) > 0
    rng = np.random.default_rng(2)
    other = dict(rn_log10_A=rng.uniform(-15, -13, (R, P)), rn_gamma=rng.uniform(1, 5, (R, P)), gwb_log10_A=rng.uniform(-15, -14, R),
                 gwb_gamma=rng.uniform(3, 5, R), wn_efac=rng.uniform(0.5, 2.0, (R, P)))
    th = _theta(R)
    term = with_c.generate_per_signal(R, r0=r0, theta=th)["chrom"]
    assert torch.equal(with_c.generate(R, r0=r0, theta=dict(other, **th)), without.generate(R, r0=r0, theta=other) + term)
    # an engine without the call is what it was: the same rows as before set_chromatic_noise existed, and no term
    assert "chrom" not in sig0 and without._chrom_t is None


@pytest.mark.parametrize("gwb_mode,wn_mode", [("grid", "reference"), ("fourier", "single"), ("grid", "single")])
def test_other_generation_modes(gwb_mode, wn_mode):
    """the term depends on neither the GWB draw nor the white-noise draw: in gwb_mode "grid" and wn_mode "single" it is the term of the
    default modes, bit for bit, and superposes exactly on the engine without the process in the same mode"""
    RG = _rg()
    R, r0 = RG + 1, 9
    default = _engine().prepare().generate_per_signal(R, r0=r0)["chrom"]
    with_c, without = _engine(), _engine(chrom=False)
    for e in (with_c, without):
        e.gwb_mode, e.wn_mode = gwb_mode, wn_mode
        e.prepare()
    term = with_c.generate_per_signal(R, r0=r0)["chrom"]
    assert torch.equal(term, default)
    assert torch.equal(with_c.generate(R, r0=r0), without.generate(R, r0=r0) + term)


def test_placement_independence():
    """a row is the same bits in one call, in calls of one, at another r0 slot, in several batches, inside generate_os whatever the
    chunk, and when out is a view at an odd column of a wider buffer with odd ld_out, whose other columns stay untouched"""
    RG = _rg()
    R, r0 = 2 * RG + 3, 70
    th = _theta(R, seed=21)
    eng = _engine().prepare()
    full = eng.generate(R, r0=r0, theta=th)
    for r in (0, RG - 1, RG, R - 1):
        assert torch.equal(eng.generate(1, r0=r0 + r, theta={k: v[r:r + 1] for k, v in th.items()})[0], full[r]), r
    assert torch.equal(eng.generate(R - 5, r0=r0 + 5, theta={k: v[5:] for k, v in th.items()}), full[5:])
    small = _engine()
    small.workspace_bytes = 1
    small.prepare()
    assert small.max_batch() == 16 < R
    assert torch.equal(small.generate(R, r0=r0, theta=th), full)
    n = eng.n_toa
    for pad in (4, 5):   # even and odd ld_out: every row on an odd 8-byte slot, then rows alternating
        wide = torch.full((R, n + pad), -7.0, dtype=torch.float64, device="cuda")
        view = wide[:, 1:1 + n]
        assert eng.generate(R, r0=r0, out=view, theta=th) is view
        assert torch.equal(view, full)
        assert bool((wide[:, :1] == -7.0).all()) and bool((wide[:, 1 + n:] == -7.0).all())
        term = torch.full((R, n + pad), -7.0, dtype=torch.float64, device="cuda")
        eng._chrom_apply(eng._theta_parts(th, R)[1], R, r0, term[:, 1:1 + n], accumulate=False)
        assert torch.equal(term[:, 1:1 + n], eng.generate_per_signal(R, r0=r0, theta=th)["chrom"])
        assert bool((term[:, :1] == -7.0).all()) and bool((term[:, 1 + n:] == -7.0).all())
    eng.prepare_optimal_statistic(components=6)
    want = eng.optimal_statistic(full)["A2"]
    for chunk in (1, 7, RG + 1, R):
        assert torch.equal(eng.generate_os(R, r0=r0, theta=th, chunk=chunk)["A2"], want), chunk
    host = np.concatenate([x.copy() for _, x in eng.stream_to_host(R, chunk=RG + 1, r0=r0)])
    assert np.array_equal(host, eng.generate(R, r0=r0).cpu().numpy())


def test_tie_to_red_noise_one_band():
    """every TOA at nu_ref: the weights are 1.0 and the chromatic process is the red noise of the same spectrum on another stream -
    replay with the red-noise draws gives the red noise bit for bit, and so does the list API on the c1_small pulsars"""
    from pta_replicator_amd.engine import ReplicaEngine
    from pta_replicator_amd.red_noise import add_chromatic_noise, add_red_noise
    chrom = _engine(full=False, one_band=1400.0).prepare()
    red = ReplicaEngine(_PSRS[1400.0], seed=77)
    red.td_warmup = False
    red.set_white_noise(efac=1.1, log10_equad=-6.6)
    red.set_red_noise(list(CH_A), list(CH_G), components=30)
    red.prepare()
    assert np.all(chrom._chrom_t["w"] == 1.0)
    d_red = [red.dump_draws(r) for r in range(3)]
    d_chrom = [dict(wn=d["wn"], chrom=d["rn"]) for d in d_red]
    a, b = chrom.replay(d_chrom, per_signal=True), red.replay(d_red, per_signal=True)
    assert torch.equal(a["chrom"], b["rn"]) and torch.equal(a["total"], b["total"])
    assert float(a["chrom"].abs().max()) > 0
    z = load("c1_small.npz")

    def psrs():
        from pta_replicator_amd.simulate import ArrayTOAs, SimulatedPulsar, make_ideal
        out = []
        for i in range(3):
            p = SimulatedPulsar(toas=ArrayTOAs(mjd_ld(z, "raw_", i), z[f"raw_err_us_{i}"]), name=str(z["raw_names"][i]),
                                loc={"RAJ": float(z["raw_raj_hours"][i]), "DECJ": float(z["raw_decj_deg"][i])})
            make_ideal(p)
            out.append(p)
        return out
    one, two, lst_c, lst_r = psrs(), psrs(), psrs(), psrs()
    for i, (pc, pr) in enumerate(zip(one, two)):   # ArrayTOAs' default frequency is 1440 MHz
        add_chromatic_noise(pc, -13.5 + 0.1 * i, 3.0 + i, ref_freq_mhz=1440.0, seed=1234 + i)
        add_red_noise(pr, -13.5 + 0.1 * i, 3.0 + i, seed=1234 + i)
        got = np.asarray(pc.added_signals_time[f"{pc.name}_chromatic_noise"].value)
        assert np.array_equal(got, np.asarray(pr.added_signals_time[f"{pr.name}_red_noise"].value)) and np.any(got != 0)
        assert pc.added_signals[f"{pc.name}_chromatic_noise"] == {"amplitude": -13.5 + 0.1 * i, "spectral_index": 3.0 + i, "index": 2.0,
                                                                   "ref_freq_mhz": 1440.0}
        assert np.array_equal(np.asarray(pc.toas.get_mjds().value), np.asarray(pr.toas.get_mjds().value))
    add_chromatic_noise(lst_c, [-13.5, None, -13.3], [3.0, None, 5.0], ref_freq_mhz=1440.0, seed=[1234, 7, 1236])
    add_red_noise(lst_r, [-13.5, None, -13.3], [3.0, None, 5.0], seed=[1234, 7, 1236])
    for i in (0, 2):
        got = np.asarray(lst_c[i].added_signals_time[f"{lst_c[i].name}_chromatic_noise"].value)
        assert np.array_equal(got, np.asarray(lst_r[i].added_signals_time[f"{lst_r[i].name}_red_noise"].value))
        assert np.array_equal(got, np.asarray(one[i].added_signals_time[f"{one[i].name}_chromatic_noise"].value))
    assert f"{lst_c[1].name}_chromatic_noise" not in lst_c[1].added_signals


def test_tie_to_red_noise_two_bands():
    """the list API at two bands is w . the one-band result, to one rounding (the weights multiply the synthesised delay)"""
    from pta_replicator_amd.red_noise import add_chromatic_noise, add_red_noise
    two, one = _psrs(seed=3), _psrs(seed=3, one_band=1400.0)
    seeds = [100 + a for a in range(P)]
    add_chromatic_noise(two, CH_A, CH_G, components=7, seed=seeds)
    add_red_noise(one, CH_A, CH_G, components=7, seed=seeds)
    for a in range(P):
        if a == NONE:
            assert f"{two[a].name}_chromatic_noise" not in two[a].added_signals
            continue
        got = np.asarray(two[a].added_signals_time[f"{two[a].name}_chromatic_noise"].value)
        want = cr.weights(two[a].toas.freqs_mhz) * np.asarray(one[a].added_signals_time[f"{one[a].name}_red_noise"].value)
        assert np.all(np.abs(got - want) <= np.spacing(np.abs(want))) and np.any(got != 0), a
    bad = _psrs(seed=3)
    bad[1].toas.freqs_mhz[4] = 0.0
    with pytest.raises(ValueError, match="J0001"):
        add_chromatic_noise(bad, CH_A, CH_G, seed=seeds)
    assert not bad[0].added_signals   # refused before any pulsar was touched


def test_dump_draws_and_replay():
    """dump_draws has the chromatic deviates of stream (10, pulsar), the twin's to the bound the other streams are held to, and replay
    of the dumped draws reproduces generate to the bound of the existing replay tests; 'total' sums rn, chrom, gwb, wn, ecorr"""
    eng = _engine(components=7).prepare()
    out = eng.generate(4, r0=5).cpu().numpy()
    for r in (0, 3):
        d = eng.dump_draws(5 + r)
        assert set(d) == {"gwb", "rn", "wn", "ecorr", "chrom"} and len(d["chrom"]) == P
        for a in range(P):
            assert d["chrom"][a].shape == (14,) and np.max(np.abs(d["chrom"][a] - cr.draws(eng.seed, 5 + r, a, 7))) < 1e-13
        sig = eng.replay([d], per_signal=True)
        rep = sig["total"].cpu().numpy()[0]
        assert np.max(np.abs(out[r] - rep)) < 1e-12 * np.sqrt(np.mean(rep ** 2))
        assert torch.equal(sig["total"], (((sig["rn"] + sig["chrom"]) + sig["gwb"]) + sig["wn"]) + sig["ecorr"])
        ref = np.concatenate([cr.term(eng.tdb_s[a], _freqs(eng, a), 7, CH_A[a], CH_G[a], d["chrom"][a]) for a in range(P)])
        got = sig["chrom"].cpu().numpy()[0]
        for a in range(P):
            if a != NONE:
                assert relrms(got[eng.off[a]:eng.off[a + 1]], ref[eng.off[a]:eng.off[a + 1]]) < TOL_SIG


def test_generate_sampled():
    """labels = the philox_ref map of the boxes on stream (7, 6) and (7, 7), pair = pulsar; residuals = generate(theta = labels); the
    labels of every other key do not move when the chromatic boxes are added"""
    from pta_replicator_amd import _chrom
    R, r0 = 7, 40
    other = dict(gwb_log10_A=(-15, -13), gwb_gamma=(3, 5), rn_log10_A=(-15, -13), rn_gamma=(1, 5), wn_efac=(0.5, 2.0))
    eng = _engine().prepare()
    eng.set_hyper_prior(**other)
    a, tha = eng.generate_sampled(R, r0=r0)
    g_box = np.stack([np.linspace(1.0, 2.0, P), np.linspace(3.0, 5.0, P)], axis=1)
    boxes = dict(chrom_log10_A=(-14.5, -13.0), chrom_gamma=g_box)
    eng.set_hyper_prior(**other, **boxes)
    b, thb = eng.generate_sampled(R, r0=r0)
    assert set(thb) == set(tha) | set(_chrom.KEYS)
    for k in tha:
        assert np.array_equal(tha[k].cpu().numpy(), thb[k].cpu().numpy(), equal_nan=True), k
    assert not torch.equal(a, b)
    for k, field in (("chrom_log10_A", cr.FIELD_LOG10_A), ("chrom_gamma", cr.FIELD_GAMMA)):
        lo, hi = (np.broadcast_to(np.asarray(boxes[k], dtype=float), (P, 2))[:, j] for j in (0, 1))
        got, want = thb[k].cpu().numpy(), cr.prior_labels(eng.seed, r0, R, field, lo, hi)
        assert got.shape == (R, P) and np.all(np.isnan(got[:, NONE]))
        live = [x for x in range(P) if x != NONE]
        assert np.all(np.abs(got[:, live] - want[:, live]) <= np.spacing(np.abs(want[:, live]))), k
        assert np.all(got[:, live] >= lo[live]) and np.all(got[:, live] <= hi[live])
    again = eng.generate(R, r0=r0, theta={k: torch.as_tensor(v.cpu().numpy()) for k, v in thb.items()})
    assert torch.equal(again, b)
    c, _ = eng.generate_sampled(1, r0=r0 + 3)
    assert torch.equal(c[0], b[3])
    eng.set_hyper_prior(**boxes)   # chromatic boxes alone are a prior
    d, thd = eng.generate_sampled(R, r0=r0)
    assert set(thd) == set(_chrom.KEYS)
    for k in thd:
        assert np.array_equal(thd[k].cpu().numpy(), thb[k].cpu().numpy(), equal_nan=True), k
    assert torch.equal(d, eng.generate(R, r0=r0, theta=thd))


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def _host_noise_model(eng, components, model="spin"):
    """the operands of the host plan builders from the configuration alone, the low-rank columns concatenated explicitly: red noise
    (20 components), then the weighted chromatic columns"""
    from pta_replicator_amd._cw import pulsar_vectors
    from pta_replicator_amd._position import ra_dec
    from pta_replicator_amd.simulate import timing_design_matrix
    toas = [m * 86400.0 for m in eng.mjd]
    sigma2 = [(eng.efacvec[a] * eng.sigma_s[a]) ** 2 + (eng.efacvec[a] * eng.equadvec[a]) ** 2 for a in range(P)]
    F_low, phi_low = [], []
    for a in range(P):
        tdb = eng.tdb_s[a]
        F, phi = [cr.basis(tdb, 20)], [cr.prior(tdb, 20, RN_A[a], RN_G[a]) if RN_A[a] is not None else np.zeros(40)]
        F.append(cr.weights(_freqs(eng, a))[:, None] * cr.basis(tdb, components))
        phi.append(cr.prior(tdb, components, CH_A[a], CH_G[a]) if CH_A[a] is not None else np.zeros(2 * components))
        F_low.append(np.concatenate(F, axis=1))
        phi_low.append(np.concatenate(phi))
    M = [timing_design_matrix(t, model=model)[0] for t in toas]
    phat = pulsar_vectors([ra_dec(p) for p in eng.psrs])
    return toas, sigma2, F_low, phi_low, M, phat


def test_statistics_carry_the_process():
    """generate_os / generate_f_statistic / generate_bwm_statistic on the engine with the process agree with host plans built here from
    explicitly concatenated columns (the bounds of the existing engine tests of each statistic), and differ from the statistic
    prepared on the engine without the process"""
    from pta_replicator_amd import bwm_statistic as bst
    from pta_replicator_amd import f_statistic as fst
    from pta_replicator_amd import optimal_statistic as ost
    R, r0, comps = 12, 4, 7
    eng, eng0 = _engine(components=comps).prepare(), _engine(chrom=False).prepare()
    rows = eng.generate(R, r0=r0)
    toas, sigma2, F_low, phi_low, M, phat = _host_noise_model(eng, comps)
    pos = []
    for p in eng.psrs:
        ra, dec = p.loc["RAJ"] * np.pi / 12, p.loc["DECJ"] * np.pi / 180
        pos.append([np.cos(dec) * np.cos(ra), np.cos(dec) * np.sin(ra), np.sin(dec)])
    # ---- OS, with the GW auto-term of the configured GWB
    eng.prepare_optimal_statistic(components=8)
    res = eng.generate_os(R, r0=r0, pairs=True)
    plan = ost.prepare(toas, sigma2, np.array(pos), components=8, gamma=13. / 3., orfs=ost.ORF_NAMES, epoch_of=eng.epoch_of, ecorr=eng.ecorrvec,
                       F_rn=F_low, phi_rn=phi_low, gw_amp2=10.0 ** (2 * GW_A), M=M)
    A2, snr, num = ost.os_from_rows(plan, rows.cpu().numpy())
    e = (_rel(res["A2"].cpu().numpy(), A2), _rel(res["snr"].cpu().numpy(), snr), _rel(res["rho"].cpu().numpy(), num / plan.den))
    print("OS against the host plan: A2 %.2e snr %.2e rho %.2e" % e)
    assert max(e) < 1e-11
    eng0.prepare_optimal_statistic(components=8)
    assert _rel(eng0.optimal_statistic(rows)["A2"].cpu().numpy(), A2) > 1e-6
    # ---- F-statistics
    freqs = np.geomspace(4e-9, 2e-7, 4)
    rng = np.random.default_rng(2)
    sky = (rng.uniform(-1, 1, 5), rng.uniform(0, 2 * np.pi, 5))
    eng.prepare_f_statistic(freqs, sky=sky, gwb_auto=False)
    res = eng.generate_f_statistic(R, r0=r0)
    plan = fst.prepare(toas, sigma2, freqs, phat=phat, sky=sky, epoch_of=eng.epoch_of, ecorr=eng.ecorrvec, F_rn=F_low, phi_rn=phi_low, M=M)
    fp, fe = fst.fstat_from_rows(plan, rows.cpu().numpy())
    e = (_rel(res["fp"].cpu().numpy(), fp), _rel(res["fe"].cpu().numpy(), fe))
    print("F-statistics against the host plan: Fp %.2e Fe %.2e" % e)
    assert max(e) < 1e-11
    eng0.prepare_f_statistic(freqs, sky=sky, gwb_auto=False)
    assert _rel(eng0.f_statistic(rows)["fp"].cpu().numpy(), fp) > 1e-6
    # ---- BWM filter
    t0 = np.array([54000.0, 55000.0, 56000.0])
    eng.prepare_bwm_statistic(t0, sky, gwb_auto=False)
    res = eng.generate_bwm_statistic(R, r0=r0)
    plan = bst.prepare(toas, sigma2, t0 * 86400.0, phat, sky, epoch_of=eng.epoch_of, ecorr=eng.ecorrvec, F_rn=F_low, phi_rn=phi_low, M=M)
    fb = bst.bwm_from_rows(plan, rows.cpu().numpy())
    fb = fb[0] if isinstance(fb, tuple) else fb
    e = _rel(res["fb"].cpu().numpy(), fb)
    print("BWM filter against the host plan: Fb %.2e" % e)
    assert e < 1e-9
    eng0.prepare_bwm_statistic(t0, sky, gwb_auto=False)
    assert _rel(eng0.bwm_statistic(rows)["fb"].cpu().numpy(), fb) > 1e-6
