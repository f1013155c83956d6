"""CPU checks of the per-realisation chromatic events (set_chromatic_events): the __host__ __device__ formulas of
csrc/pta_chrom_event.h compiled with g++ (tests/chrom_event/chrom_event_host.cpp) against a long-double evaluation of the definition
within the rounding bound counted in chrom_event_reference.py, the NumPy evaluation and the list-API twin against the same reference,
the label draws against philox_ref, and the validation of the configuration, the prior and theta on an engine that is configured but
not prepared (no GPU needed: every refusal happens before anything is launched)."""
import re

import numpy as np
import pytest

import chrom_event_reference as cr
from chrom_event_reference import LD
from helpers import load, mjd_ld
from oracle import philox_ref


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return cr.build(tmp_path_factory.mktemp("chrom_event"))


def _toas(seed=1, n=400):
    rng = np.random.default_rng(seed)
    toa = np.sort(rng.uniform(53000, 57500, n)) * 86400.0
    return toa, cr.two_bands(rng, n)


def _lnu(freqs, ref=1400.0):
    from pta_replicator_amd import _chrom_event as ce
    return ce.log_freq_ratio(freqs, ref)


def _check(host, events, toa, freqs, what, ref_freq=1400.0):
    """every event alone and their sum in pulsar 0 against long double; returns the worst error in units of the bound"""
    tab = cr.tables(host, cr.src_rows(events))
    lnu = _lnu(freqs, ref_freq)
    worst = 0.0
    for sel in [slice(e, e + 1) for e in range(len(tab))] + [slice(None)]:
        got = cr.term_host(host, tab[sel], 0, toa, lnu)
        ref, bound = cr.term_ld(tab[sel], 0, toa, freqs, ref_freq)
        err = np.abs(got.astype(LD) - ref)
        assert np.all(err <= bound), (what, sel, float(np.max(err / np.where(bound > 0, bound, 1))))
        if np.any(bound > 0):
            worst = max(worst, float(np.max((err / np.where(bound > 0, bound, 1))[bound > 0])))
        assert np.all(got[bound == 0] == 0.0)
    for row in tab:   # the relative bound stays below 1e-12 wherever the reference is a normal number (X <= 800 there)
        ref, bound, X = cr.event_ld(row, toa, freqs, ref_freq)
        normal = np.abs(ref) >= LD(2) ** -1022
        if int(row[1]) == 3:
            assert np.all(bound <= LD(1e-12) * np.exp(LD(row[7]) + LD(row[8]) * np.log(LD(ref_freq) / freqs.astype(LD))))
        else:
            assert np.all((bound - LD(2) ** -1074)[normal] <= LD(1e-12) * np.abs(ref[normal])) and np.all(X[normal] <= 800)
    print(f"{what}: worst deviation in units of the bound {worst:.3g}")
    return worst


def test_stream_kind_columns_and_threshold(host):
    from pta_replicator_amd import _chrom_event as ce
    assert ce.STREAM_CE == 15 == host.ce_stream()
    assert ce.KEYS == ("ce_psr", "ce_kind", "ce_t0_mjd", "ce_log10_tau", "ce_log10_tau_pre", "ce_log10_a", "ce_sign", "ce_index", "ce_phase")
    assert ce.KINDS == ("decay", "cusp", "bump", "annual") and len(ce.TABLE) == 10 and ce.E_MAX == 128
    assert np.exp(host.ce_arg_zero()) == 0.0 and host.ce_arg_zero() < -1075 * np.log(2.0)   # exp < 2^-1075 rounds to 0


def test_term_against_long_double_random_events(host):
    """200 random events of every kind over the 4500-day span in two bands, chi from 0 to 6.4, each alone and summed"""
    toa, freqs = _toas()
    rng = np.random.default_rng(11)
    worst = 0.0
    for block in range(20):
        events = [{"kind": int(rng.integers(0, 4)) if block else k % 4, "t0_mjd": rng.uniform(52800, 57700), "log10_tau": rng.uniform(5.5, 8.0),
                   "log10_tau_pre": np.nan if rng.integers(0, 2) else rng.uniform(5.5, 7.5), "log10_a": rng.uniform(-8.0, -5.0),
                   "sign": rng.choice([-1.0, 1.0, -2.5, 0.3]), "index": rng.uniform(0, 6.4), "phase": rng.uniform(-1, 7)} for k in range(10)]
        worst = max(worst, _check(host, events, toa, freqs, f"random block {block}"))
    assert worst > 0


def test_term_edge_cases(host):
    """a decay and a cusp with a TOA exactly at t0; events before the first and after the last TOA (a decay after the last TOA is exactly
    0 everywhere); a tau so short that the envelope underflows to exactly 0; chi = 0, where the weight is exactly 1"""
    toa, freqs = _toas(seed=2)
    k = 137
    t0_on = toa[k] / 86400.0
    assert t0_on * 86400.0 == toa[k]                     # the epoch in seconds is this TOA
    lnu = _lnu(freqs)
    for kind in ("decay", "cusp"):
        ev = {"kind": kind, "t0_mjd": t0_on, "log10_tau": 6.8, "log10_tau_pre": 6.1, "log10_a": -6.0, "index": 2.0}
        _check(host, [ev], toa, freqs, f"{kind} with a TOA at t0")
        got = cr.term_host(host, cr.tables(host, cr.src_rows([ev])), 0, toa, lnu)
        peak = -np.exp(-6.0 * np.log(10.0) + 2.0 * lnu[k])
        # the t >= t0 side: the full amplitude, whatever tau_pre says (|exponent| < 20: two roundings of it and the exp's ulp, < 40 ulp)
        assert abs(got[k] - peak) <= 40 * np.spacing(abs(peak))
        assert np.all(got[:k] == 0) if kind == "decay" else np.all(got[:k] < 0)
    first, last = toa[0] / 86400.0, toa[-1] / 86400.0
    for kind in ("decay", "cusp", "bump"):
        _check(host, [{"kind": kind, "t0_mjd": first - 30, "log10_tau": 6.5, "log10_a": -6.0}], toa, freqs, f"{kind} before the first TOA")
        _check(host, [{"kind": kind, "t0_mjd": last + 30, "log10_tau": 6.5, "log10_a": -6.0}], toa, freqs, f"{kind} after the last TOA")
    late = cr.term_host(host, cr.tables(host, cr.src_rows([{"kind": "decay", "t0_mjd": last + 1e-3, "log10_tau": 7.0, "log10_a": -5.0}])), 0, toa, lnu)
    assert np.all(late == 0.0) and not np.any(np.signbit(late))
    # tau = 1000 s: the envelope is subnormal ~ 7.1e5 s after t0 and exactly 0 ~ 7.45e5 s after it
    short = [{"kind": kind, "t0_mjd": first, "log10_tau": 3.0, "log10_a": -6.0} for kind in ("decay", "cusp", "bump")]
    _check(host, short, toa, freqs, "tau = 1000 s")
    got = cr.term_host(host, cr.tables(host, cr.src_rows(short[:1])), 0, toa, lnu)
    assert got[0] != 0 and np.all(got[toa > toa[0] + 8e5] == 0.0)
    # chi = 0: the weight is exactly 1, the term is the same in both bands
    flat = [{"kind": kind, "t0_mjd": 55000.0, "log10_tau": 7.0, "log10_a": -6.5, "index": 0.0, "phase": 1.0} for kind in range(4)]
    _check(host, flat, toa, freqs, "chi = 0")
    tab = cr.tables(host, cr.src_rows(flat))
    assert np.array_equal(cr.term_host(host, tab, 0, toa, lnu), cr.term_host(host, tab, 0, toa, np.zeros(len(toa))))
    # another reference frequency, and a large amplitude (a positive exponent)
    _check(host, [{"kind": 0, "t0_mjd": 54000.0, "log10_tau": 7.5, "log10_a": 1.5, "index": 4.0, "sign": 1}], toa, freqs, "nu_ref = 700", 700.0)


def test_table_row(host):
    """the row pta_engine_chrom_event_params writes, against NumPy: t0 in seconds exact, the sign -1 / +1, a NaN tau_pre = tau"""
    src = cr.src_rows([{"psr": 3, "kind": "cusp", "t0_mjd": 55123.25, "log10_tau": 6.7, "log10_a": -6.2, "sign": -0.2, "index": 4.4, "phase": 1.3},
                       {"psr": 5, "kind": 1, "t0_mjd": 55123.25, "log10_tau": 6.7, "log10_tau_pre": 5.9, "log10_a": -6.2, "sign": 7.0}])
    tab = cr.tables(host, src)
    assert np.array_equal(tab[:, :3], [[3, 1, 55123.25 * 86400.0], [5, 1, 55123.25 * 86400.0]]) and np.array_equal(tab[:, 6], [-1.0, 1.0])
    tau = 10 ** 6.7
    want = np.array([[1 / tau, 1 / tau, -0.5 / tau ** 2, -1, -6.2 * np.log(10), 4.4, 1.3 / (2 * np.pi)],
                     [1 / tau, 1 / 10 ** 5.9, -0.5 / tau ** 2, 1, -6.2 * np.log(10), 2.0, 0.0]])
    assert np.all(np.abs(tab[:, 3:] - want) <= 1e-14 * np.abs(want))
    assert tab[0, 3] == tab[0, 4]


# ---------------------------------------------------------------- NumPy evaluation, the list API --------------------------------------
def _numpy_bound(row, toa, freqs, ref, X):
    """_chrom_event.term evaluates the definition as written in float64, u = 2^-53, a library function within one ulp = 2 u.  Amplitude:
    10^x (2 u), the weight's quotient (1 u) raised to chi (chi u + 2 u), two products (2 u), the exp (2 u): (9 + chi) u, taken as
    (16 + 2 chi) u; the reference's A = exp(ln A) takes the row's ln A = log10_a ln 10, a rounded constant and a rounded product: 2 |ln A| u.  The envelope's argument, kinds 0 / 1: t - t0 (1 u), tau = 10^x (2 u), the quotient (1 u), and on the reference's side the
    row's 1 / tau (2 u + 1 u): 7 |arg| u.  Kind 2: the same quotient squared (8 u) and the square's rounding (1 u), and the row's
    -1/2 / tau^2 (4 u + 1 u + 1 u): 15 |arg| u.  A subnormal result is rounded twice, the exp within an ulp there
    (one spacing, 2^-1074, scaled by an amplitude < 1 in this test) and the product (half a spacing): 2 * 2^-1074.  The annual sine's argument 2 pi t / YEAR ~ 2 pi 150 carries three
    roundings: 3 * 2 pi (t / YEAR) u absolute, + 2 for the phase's"""
    u = LD(2) ** -53
    chi, lna = abs(LD(row[8])), abs(LD(row[7]))
    if int(row[1]) == 3:
        amp = np.exp(LD(row[7]) + LD(row[8]) * np.log(LD(1400.0) / freqs.astype(LD)))
        return amp * ((16 + 2 * chi + 2 * lna) * np.abs(ref / amp) + 6 * np.pi * (toa / cr.YEAR + 2)) * u
    arg = X - (abs(LD(row[7])) + abs(LD(row[8]) * np.log(LD(1400.0) / freqs.astype(LD))))
    return (16 + 2 * chi + 2 * lna + (15 if int(row[1]) == 2 else 7) * np.where(X > 0, arg, 0)) * u * np.abs(ref) + LD(2) ** -1073


def test_numpy_term_and_list_api_against_the_reference(host):
    from pta_replicator_amd import _chrom_event as ce
    from pta_replicator_amd.deterministic import add_chromatic_event
    toa, freqs = _toas(seed=4, n=300)
    rng = np.random.default_rng(9)
    events = [{"kind": ce.KINDS[k % 4], "t0_mjd": rng.uniform(53500, 57000), "log10_tau": rng.uniform(6.0, 7.8),
               "log10_tau_pre": np.nan if k % 3 else rng.uniform(6.0, 7.0), "log10_a": rng.uniform(-7.5, -5.5), "sign": rng.choice([-1.0, 1.0]),
               "index": rng.uniform(0, 6.4), "phase": rng.uniform(0, 2 * np.pi)} for k in range(24)]
    tab = cr.tables(host, cr.src_rows(events))
    worst = 0.0
    for ev, row in zip(events, tab):
        got = ce.term(toa, freqs, [ev])
        ref, _, X = cr.event_ld(row, toa, freqs)
        lim = _numpy_bound(row, toa, freqs, ref, X)
        err = np.abs(got.astype(LD) - ref)
        worst = max(worst, float(np.max(err / lim)))
        assert np.all(err <= lim), (ev, float(np.max(err / lim)))
    print(f"_chrom_event.term: worst deviation in units of its bound {worst:.3g}")
    assert np.array_equal(ce.term(toa, freqs, events[:3]), (ce.term(toa, freqs, events[:1]) + ce.term(toa, freqs, events[1:2])) + ce.term(toa, freqs, events[2:3]))
    with pytest.raises(ValueError, match="tau0"):
        ce.term(toa, freqs, [dict(events[0], tau0=1.0)])
    # the list API records exactly the NumPy term on the pulsar's own TOAs and frequencies, on a pulsar and on a list
    psrs = cr.ragged_pulsars()[3:6]
    kw = dict(kind="cusp", log10_a=-6.1, t0_mjd=55200.0, log10_tau=6.9, log10_tau_pre=6.2, sign=-1, index=2.0)
    add_chromatic_event(psrs[0], **kw)
    add_chromatic_event(psrs[1:], "annual", -6.5, index=2.0, phase=0.7, signal_name="annual_dm")
    for p, name, row in ((psrs[0], "chromatic_event", dict(kw)), (psrs[1], "annual_dm", {"kind": 3, "log10_a": -6.5, "phase": 0.7}),
                         (psrs[2], "annual_dm", {"kind": 3, "log10_a": -6.5, "phase": 0.7})):
        rec = np.asarray(p.added_signals_time[f"{p.name}_{name}"].value, dtype=np.float64)
        t = np.asarray(p.toas.get_mjds().value * 86400, dtype=np.float64)
        assert rec.shape == t.shape and np.any(rec != 0)
    fresh = cr.ragged_pulsars()[3]
    want = ce.term(np.asarray(fresh.toas.get_mjds().value * 86400, dtype=np.float64), fresh.toas.freqs_mhz, [kw])
    assert np.array_equal(np.asarray(psrs[0].added_signals_time[f"{psrs[0].name}_chromatic_event"].value, dtype=np.float64), want)
    fresh = cr.ragged_pulsars()[5]
    want = ce.term(np.asarray(fresh.toas.get_mjds().value * 86400, dtype=np.float64), fresh.toas.freqs_mhz, [{"kind": "annual", "log10_a": -6.5, "phase": 0.7}])
    assert np.array_equal(np.asarray(psrs[2].added_signals_time[f"{psrs[2].name}_annual_dm"].value, dtype=np.float64), want)
    for bad, word in ((dict(kw, kind=4), "kind"), (dict(kw, t0_mjd=None), "t0_mjd"), (dict(kw, sign=0), "sign"), (dict(kw, ref_freq_mhz=0.0), "ref_freq_mhz")):
        with pytest.raises(ValueError, match=word):
            add_chromatic_event(cr.ragged_pulsars()[1], **bad)


# ---------------------------------------------------------------- the draws ---------------------------------------------------------
def test_uniform_maps_match_philox_ref(host):
    """column j of slot e = pair j of stream (15, e) through the slot's own box: the uniforms bit-equal to philox_ref's, a degenerate box
    its value exactly, the pulsar the floor of its draw inside 0 .. P-1"""
    from pta_replicator_amd import _chrom_event as ce
    from pta_replicator_amd.engine import stream_id
    seed, r0, R, E, P = 0x0123456789ABCDEF, 77, 6, 3, 7
    lo, hi = np.zeros((E, 9)), np.ones((E, 9))
    lo[:, 0], hi[:, 0] = 0.25, 0.75
    unit = cr.uniform(host, seed, r0, R, E, P, lo, hi)
    prior = ce.make_prior(E, P, kind=["decay", "cusp", "annual"], log10_a=[(-7.0, -6.0), -6.5, (-7.5, -6.5)], psr=[None, 4, None],
                          t0_mjd=[(54000.0, 56000.0), (55000.0, 55500.0), None], log10_tau=[(6.0, 7.5), (6.5, 7.0), None],
                          log10_tau_pre=[None, (6.0, 6.5), None], sign=[-1, "random", 1], index=[2.0, (1.0, 4.4), 2.0])
    assert list(prior["kind"]) == [0, 1, 3]
    plo, phi = ce.prior_bounds(prior)
    assert plo.shape == (E * 9,) and (plo[0], phi[0]) == (0, P) and (plo[9], phi[9]) == (4, 4) and (plo[9 + 6], phi[9 + 6]) == (-1, 1)
    assert (plo[18 + 2], phi[18 + 2], plo[18 + 3], phi[18 + 3]) == (0, 0, 0, 0) and (plo[8], phi[8]) == (0, 2 * np.pi)
    lab = cr.uniform(host, seed, r0, R, E, P, plo, phi)
    plo, phi = plo.reshape(E, 9), phi.reshape(E, 9)
    for r in range(R):
        for e in range(E):
            _, u2 = philox_ref.uniform_pairs(seed, r0 + r, stream_id(ce.STREAM_CE, e), 9)
            u2 = np.asarray(u2, dtype=np.float64)
            assert np.array_equal(unit[r, e, 1:], u2[1:]) and unit[r, e, 0] == 0.0, (r, e)      # fma(1, u2, 0) = u2
            ref = plo[e] + (phi[e] - plo[e]) * u2
            fin = np.isfinite(ref)
            fin[0] = False
            assert np.all(np.abs(lab[r, e] - ref)[fin] <= np.spacing(np.abs(ref[fin]))), (r, e)
            assert np.all(lab[r, e][fin] >= plo[e][fin]) and np.all(lab[r, e][fin] <= phi[e][fin])
            assert lab[r, e, 0] == (4 if e == 1 else min(np.floor(P * u2[0]), P - 1)) and 0 <= lab[r, e, 0] <= P - 1
            assert lab[r, e, 1] == prior["kind"][e] and lab[r, e, 7] == (lab[r, e, 7] if e == 1 else 2.0)
    assert np.all(np.isnan(lab[:, 0, 4])) and np.all(np.isnan(lab[:, 2, 4])) and np.all(np.isfinite(lab[:, 1, 4]))
    assert np.all(lab[:, 0, 6] == -1.0) and np.all(lab[:, 2, 6] == 1.0) and np.all(lab[:, 1, 5] == -6.5) and lab[:, 1, 6].std() > 0
    assert len(np.unique(lab[:, 0, 0])) > 2
    # a label row is a function of (seed, realisation, slot) alone
    assert np.array_equal(cr.uniform(host, seed, r0 + 2, 3, E, P, plo, phi), lab[2:5], equal_nan=True)
    assert np.array_equal(cr.uniform(host, seed, r0, R, 2, P, plo[:2], phi[:2]), lab[:, :2], equal_nan=True)


# ---------------------------------------------------------------- validation (no GPU) -----------------------------------------------
def _engine(n=2, freqs=True):
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
    if n:
        assert eng.set_chromatic_events(n) is eng
    return eng


def _theta(R, E):
    return {"ce_psr": np.zeros((R, E), dtype=np.int64), "ce_kind": np.zeros((R, E), dtype=np.int64), "ce_t0_mjd": np.full((R, E), 55000.0),
            "ce_log10_tau": np.full((R, E), 6.5), "ce_log10_a": np.full((R, E), -6.5)}


def test_theta_refusals_before_any_launch():
    import torch
    from pta_replicator_amd import _chrom_event as ce
    R, E = 3, 2
    eng = _engine(E)
    ok = _theta(R, E)

    def spoiled(key, value, fill=None):
        v = np.array(ok[key] if key in ok else np.full((R, E), fill), dtype=np.float64)
        v[1, 1] = value
        return dict(ok, **{key: v})
    cases = [
        (dict(ok, ce_amplitude=np.zeros((R, E))), "ce_amplitude"),
        ({k: v for k, v in ok.items() if k != "ce_log10_a"}, "ce_log10_a"),
        ({"ce_count": np.ones(R, dtype=np.int64)}, "missing"),
        (dict(ok, ce_t0_mjd=np.zeros(R)), "ce_t0_mjd"),
        (dict(ok, ce_index=np.zeros((R, E + 1))), "ce_index"),
        (spoiled("ce_psr", 4), "ce_psr"),
        (spoiled("ce_psr", -1), "ce_psr"),
        (spoiled("ce_psr", 1.5), "ce_psr"),
        (spoiled("ce_kind", 4), "ce_kind"),
        (dict(ok, ce_kind=[["decay", "dip"]] * R), "dip"),
        (spoiled("ce_sign", 0.0, -1.0), "ce_sign"),
        (spoiled("ce_log10_tau", np.nan), "ce_log10_tau"),
        (spoiled("ce_log10_a", np.inf), "ce_log10_a"),
        (spoiled("ce_phase", np.nan, 0.0), "ce_phase"),
        (spoiled("ce_index", np.nan, 2.0), "ce_index"),
        (spoiled("ce_log10_tau_pre", np.inf, np.nan), "ce_log10_tau_pre"),
        (dict(ok, ce_count=np.full(R, E + 1)), "ce_count"),
        (dict(ok, ce_count=np.ones(R)), "ce_count"),
        (dict(ok, ce_count=np.ones(R + 1, dtype=np.int64)), "ce_count"),
    ]
    for theta, word in cases:
        with pytest.raises(ValueError, match=word):
            eng._theta_parts(theta, R)
        with pytest.raises(ValueError, match=word):
            eng._theta_parts(theta, R, td=True)
    # names for kinds, a NaN tau_pre, torch tensors, entries at or past the count are not examined
    named = eng._theta_parts(dict(ok, ce_kind=np.array([["cusp", "bump"]] * R)), R)[1]["ce_kind"]
    assert np.array_equal(named, [[1, 2]] * R)
    good = dict(ok, ce_kind=[["decay", "annual"]] * R, ce_log10_tau_pre=np.full((R, E), np.nan), ce_sign=torch.full((R, E), 2.0, dtype=torch.float64))
    hyper, det = eng._theta_parts(good, R)
    assert hyper is None and set(det) == set(ce.KEYS) and np.array_equal(det["ce_kind"], [[0, 3]] * R)
    assert np.all(det["ce_index"] == 2.0) and np.all(det["ce_phase"] == 0.0) and ce.has_keys(det)
    past = dict(spoiled("ce_psr", 99), ce_count=np.array([2, 1, 0]))
    past["ce_log10_a"] = spoiled("ce_log10_a", np.nan)["ce_log10_a"]
    _, det = eng._theta_parts(past, R)
    assert "ce_count" in det
    _, det = eng._theta_parts(ok, R, td=True)     # TD mode takes the keys
    assert ce.has_keys(det)
    with pytest.raises(ValueError, match=r"ce_\*"):
        eng._theta_parts({"rn_gamma": np.zeros((R, 4))}, R, td=True)
    # keys without set_chromatic_events
    with pytest.raises(ValueError, match="set_chromatic_events"):
        _engine(0)._theta_parts(ok, R)
    with pytest.raises(ValueError, match="set_chromatic_events"):
        _engine(0).set_chromatic_event_prior("decay", -6.0, t0_mjd=55000.0, log10_tau=6.0)


def test_configuration_and_prior_validation():
    from pta_replicator_amd import _chrom_event as ce
    eng = _engine(0)
    for bad in (0, 129, -1, 2.5, True):
        with pytest.raises(ValueError, match=r"1 \.\. 128"):
            eng.set_chromatic_events(bad)
    for bad in (0.0, -1400.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="ref_freq_mhz"):
            eng.set_chromatic_events(1, ref_freq_mhz=bad)
    # a pulsar without radio frequencies, or with a bad one, is refused by name
    eng.psrs[2].toas.freqs_mhz[3] = -820.0
    with pytest.raises(ValueError, match=re.escape(eng.psrs[2].name)):
        eng.set_chromatic_events(1)

    class NoFreqs:
        def get_mjds(self):
            return eng.psrs[1].toas.get_mjds()
    eng = _engine(0)
    eng.psrs[1].toas = NoFreqs()
    with pytest.raises(ValueError, match=re.escape(eng.psrs[1].name)):
        eng.set_chromatic_events(1)
    eng = _engine(3)
    assert eng._ce == {"E": 3, "ref_freq_mhz": 1400.0}
    req = dict(t0_mjd=(54000.0, 56000.0), log10_tau=(6.0, 7.0))
    assert eng.set_chromatic_event_prior("decay", (-7.0, -6.0), **req) is eng
    assert list(eng._ce_prior["kind"]) == [0, 0, 0] and eng._ce_prior["lo"].shape == (3, 9)
    eng.set_chromatic_event_prior(["annual", 2, "cusp"], -6.5, t0_mjd=[None, 55000.0, 55000.0], log10_tau=[None, 6.0, 6.5])
    assert list(eng._ce_prior["kind"]) == [3, 2, 1]
    for kw, word in ((dict(kind="dip", log10_a=-6.0, **req), "dip"), (dict(kind=4, log10_a=-6.0, **req), "kind"),
                     (dict(kind=["decay", "cusp"], log10_a=-6.0, **req), "kind"), (dict(kind="decay", log10_a=None, **req), "log10_a"),
                     (dict(kind="decay", log10_a=-6.0, log10_tau=6.0), "t0_mjd"), (dict(kind="bump", log10_a=-6.0, t0_mjd=55000.0), "log10_tau"),
                     (dict(kind=["annual", "annual", "cusp"], log10_a=-6.0), "t0_mjd"),
                     (dict(kind="decay", log10_a=(-6.0, -7.0), **req), "log10_a"), (dict(kind="decay", log10_a=(-6.0, np.inf), **req), "log10_a"),
                     (dict(kind="decay", log10_a=-6.0, psr=4, **req), "psr"), (dict(kind="decay", log10_a=-6.0, psr=1.5, **req), "psr"),
                     (dict(kind="decay", log10_a=-6.0, psr=(0, 5), **req), "psr"), (dict(kind="decay", log10_a=-6.0, sign=0, **req), "sign"),
                     (dict(kind="decay", log10_a=-6.0, sign="both", **req), "sign"), (dict(kind="decay", log10_a=-6.0, index=[2.0, 2.0], **req), "index"),
                     (dict(kind="decay", log10_a=-6.0, phase=(0, 1, 2), **req), "phase")):
        with pytest.raises(ValueError, match=word):
            eng.set_chromatic_event_prior(**kw)
    assert ce.make_prior(1, 4, "annual", -6.0)["lo"][0, 4] != ce.make_prior(1, 4, "annual", -6.0)["lo"][0, 4]     # NaN: symmetric
    eng.set_chromatic_events(2)   # a prior made for another E is dropped with it
    assert eng._ce_prior is None
