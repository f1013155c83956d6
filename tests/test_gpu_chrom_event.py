"""Chromatic events per realisation on the device: pta_engine_chrom_event_add against the long-double reference on a ragged two-band
array with unaligned rows (the sparse skip included: untouched pulsars keep their bits), pta_engine_chrom_event_params against NumPy,
composition with generate / generate_per_signal / generate_td / a statistic and the other per-realisation keys, and the sampled
labels against the host twin's draws."""
import ctypes

import numpy as np
import pytest
import torch

import chrom_event_reference as cr
from chrom_event_reference import LD
from test_gpu_bwm import _sum_close, _theta as _bwm_theta
from test_gpu_os import _engine

pytestmark = pytest.mark.gpu

R, E = 19, 5                      # R: no multiple of the realisation group of the add kernel
QUIET = (1, 2)                    # pulsars that never hold an event
NEG0 = np.array([0x8000000000000000], dtype=np.uint64).view(np.float64)[0]
NAN_PAYLOAD = np.array([0x7FF8000000ABCDEF], dtype=np.uint64).view(np.float64)[0]


@pytest.fixture(scope="module")
def ragged2():
    """test_gpu_bwm's ragged array (593 TOAs, a 301-TOA pulsar of two tiles, partial tiles) in two radio bands, white noise only"""
    from pta_replicator_amd.engine import ReplicaEngine
    eng = ReplicaEngine(cr.ragged_pulsars(), seed=2)
    eng.td_warmup = False
    eng.set_white_noise(efac=1.0)
    eng.set_chromatic_events(E)
    eng.prepare()
    assert list(eng.counts) == cr.COUNTS and eng.plan.n_tiles == 8
    return eng


def _freqs(eng):
    return np.concatenate([p.toas.freqs_mhz for p in eng.psrs])


def _tables(eng, seed):
    """random table rows [R, E, 10] for the ragged engine and count [R] covering 0, 1 and E; no event in the pulsars QUIET; row 0 holds a
    decay and an annual term in the two-tile pulsar (the summation order), a decay after the last TOA and one with tau = 1000 s (exactly 0
    on all but a few TOAs); rows past a count are NaN (never read)"""
    rng = np.random.default_rng(seed)
    toa = np.concatenate([m * 86400 for m in eng.mjd])
    tau = 10 ** rng.uniform(6.0, 7.8, (R, E))
    pre = 10 ** rng.uniform(6.0, 7.0, (R, E))
    tab = np.stack([rng.choice([0, 3, 4, 5, 6], (R, E)).astype(np.float64), rng.integers(0, 4, (R, E)).astype(np.float64),
                    rng.uniform(53500, 57000, (R, E)) * 86400, 1 / tau, 1 / pre, -0.5 / tau ** 2, rng.choice([-1.0, 1.0], (R, E)),
                    rng.uniform(-7.0, -5.5, (R, E)) * np.log(10), rng.uniform(0, 6.4, (R, E)), rng.uniform(0, 1, (R, E))], axis=2)
    count = rng.choice([0, 1, E], R)
    count[:3] = [E, 0, 1]
    tab[0, :, 0] = [6, 6, 5, 4, 0]
    tab[0, :4, 1] = [0, 3, 0, 0]
    tab[0, 0, 2] = toa[eng.off[6] + 140]                                     # a TOA exactly at t0, in the first tile of the pulsar
    tab[0, 2, 2] = toa.max() + 1.0                                           # a decay after the last TOA: exactly 0
    tab[0, 3, 2:6] = [toa[eng.off[4]], 1e-3, 1e-3, -0.5e-6]                  # tau = 1000 s from the pulsar's first TOA on
    for r in range(R):
        tab[r, count[r]:] = np.nan
    return toa, np.ascontiguousarray(tab), count.astype(np.int32)


def _reference(eng, toa, freqs, tab, count):
    """(ref, bound, touched) [R, n_toa]: the long-double sum and its bound per element, and whether the element's pulsar holds a live event"""
    N = len(toa)
    ref, bound, touched = np.zeros((R, N), dtype=LD), np.zeros((R, N), dtype=LD), np.zeros((R, N), dtype=bool)
    for r in range(len(tab)):
        live = tab[r, :count[r]]
        for a in range(eng.P):
            if np.any(live[:, 0] == a):
                sl = slice(eng.off[a], eng.off[a + 1])
                ref[r, sl], bound[r, sl] = cr.term_ld(live, a, toa[sl], freqs[sl], eng._ce["ref_freq_mhz"])
                touched[r, sl] = True
    return ref, bound, touched


@pytest.mark.parametrize("pad", [3, 4])   # n_toa = 593: an even and an odd row stride
@pytest.mark.parametrize("accumulate", [0, 1])
def test_add_vs_long_double_on_a_ragged_array(ragged2, pad, accumulate):
    """pta_engine_chrom_event_add from given table rows against long double, element by element within the bound of
    chrom_event_reference.py; counts 0, 1 and E, NaN rows past a count never read, two events of different kinds in one pulsar.
    Accumulating, the elements of a (realisation, pulsar) without a live event and everything past n_toa keep their bits, -0.0 and a NaN
    payload included, and a realisation with count 0 is untouched; writing, they are +0.0.  Rows 13 .. 15 launched alone in other row
    slots are bit-equal to the batch."""
    from pta_replicator_amd import _lib, device as dv
    eng = ragged2
    P, N = eng.P, eng.n_toa
    ld = N + pad
    toa, tab, count = _tables(eng, seed=10 * pad + accumulate)
    freqs = _freqs(eng)
    rng = np.random.default_rng(7)
    base = rng.normal(size=(R, ld)) * 1e-7
    for a in QUIET:                                   # the pattern the skip must leave alone
        base[:, eng.off[a]] = NEG0
        base[:, eng.off[a] + 1] = NAN_PAYLOAD
    base[1, ::7] = NEG0                               # the count-0 realisation
    base[:, N] = NAN_PAYLOAD                          # past n_toa
    out, d_tab, d_count = dv.f64(base), dv.f64(tab), dv.i32(count)
    c = _lib.ChromEventEngine()
    c.n_psr, c.n_ev, c.toa_s, c.lnu = P, E, eng.d_toa_s.data_ptr(), eng._ce_lnu_device().data_ptr()
    c.tab, c.count = d_tab.data_ptr(), d_count.data_ptr()
    s = dv.stream_ptr()
    _lib.call("pta_engine_chrom_event_add", ctypes.byref(eng.plan), ctypes.byref(c), R, dv.ptr(out), ld, accumulate, s)
    got = out.cpu().numpy()
    bits, base_bits = got.view(np.uint64), base.view(np.uint64)
    assert np.array_equal(bits[:, N:], base_bits[:, N:])                        # the pad columns are untouched
    ref, bound, touched = _reference(eng, toa, freqs, tab, count)
    assert not touched[1].any() and touched[0, eng.off[6]:].all() and not touched[:, eng.off[1]:eng.off[3]].any()
    assert sum(not touched[r, eng.off[a]] for r in range(R) for a in range(P)) >= 2 * R
    if accumulate:
        assert np.array_equal(bits[:, :N][~touched], base_bits[:, :N][~touched])   # neither read nor written: the same bits
        assert np.array_equal(bits[1], base_bits[1])
    else:
        assert np.all(bits[:, :N][~touched] == 0)                                # +0.0 where there is no event
    g = got[:, :N][touched]
    assert np.all(np.isfinite(g))                                               # NaN rows past the counts were never read
    want = (base[:, :N] + ref if accumulate else ref)[touched]
    err = np.abs(g.astype(LD) - want)
    lim = bound[touched] + (np.spacing(np.abs(g)) if accumulate else 0)
    worst = float(np.max(err / np.where(lim > 0, lim, 1)))
    print(f"accumulate={accumulate} pad={pad}: worst deviation in units of the bound {worst:.3g}")
    assert np.all(err <= lim), worst
    # the decay after the last TOA and the underflowing one contribute exactly nothing where the reference says so
    late = slice(eng.off[5], eng.off[6])
    assert np.all(ref[0, late] == 0) and np.array_equal(got[0, late], base[0, late] + 0.0 if accumulate else np.zeros(eng.off[6] - eng.off[5]))
    assert np.count_nonzero(ref[0, eng.off[6]:]) == N - eng.off[6] and ref[0, eng.off[4]] != 0 and abs(ref[0, eng.off[4] + 40]) < LD(2) ** -1075
    assert got[0, eng.off[4] + 40] == (base[0, eng.off[4] + 40] if accumulate else 0.0)
    base2 = np.ascontiguousarray(base[13:16])
    out2 = dv.f64(base2)
    c.tab, c.count = d_tab.data_ptr() + 8 * 13 * E * 10, d_count.data_ptr() + 4 * 13
    _lib.call("pta_engine_chrom_event_add", ctypes.byref(eng.plan), ctypes.byref(c), 3, dv.ptr(out2), ld, accumulate, s)
    assert np.array_equal(out2.cpu().numpy().view(np.uint64), bits[13:16])
    if not accumulate and pad == 3:                                             # count = NULL: every row has E events
        full = tab.copy()
        dead = np.isnan(full[..., 0])
        full[dead] = [3, 2, 55000.0 * 86400, 1e-7, 1e-7, -0.5e-14, -1, -14.0, 2.0, 0.0]
        d_full = dv.f64(full)
        c.tab, c.count = d_full.data_ptr(), None
        _lib.call("pta_engine_chrom_event_add", ctypes.byref(eng.plan), ctypes.byref(c), R, dv.ptr(out), ld, 0, s)
        got = out.cpu().numpy()[:, :N]
        ref, bound, touched = _reference(eng, toa, freqs, full, np.full(R, E))
        assert np.all(np.abs(got.astype(LD) - ref) <= bound) and np.all(got[~touched] == 0) and touched[1].any()


def test_params_vs_numpy(ragged2):
    """pta_engine_chrom_event_params against NumPy from the label rows (the tolerance of test_gpu_burst.test_params_vs_numpy: pow and
    exp differ between host and device); the integer columns, the sign and t0 exact; rows past the count unwritten"""
    from pta_replicator_amd import _chrom_event as ce, _lib, device as dv
    eng = ragged2
    R_ = 11
    th = cr.random_theta(R_, E, eng.P, seed=8)
    src = dv.f64(np.stack([np.asarray(th[k], dtype=np.float64) for k in ce.KEYS], axis=2))
    count = np.array([0, 1, 2, E] * 3)[:R_].astype(np.int32)
    tab = torch.full((R_, E, 10), -7.0, dtype=torch.float64, device=src.device)
    d_count = dv.i32(count)
    c = _lib.ChromEventEngine()
    c.n_psr, c.n_ev, c.src, c.tab, c.count = eng.P, E, src.data_ptr(), tab.data_ptr(), d_count.data_ptr()
    _lib.call("pta_engine_chrom_event_params", ctypes.byref(c), R_, dv.stream_ptr())
    tab = tab.cpu().numpy()
    tau = 10 ** th["ce_log10_tau"]
    pre = np.where(np.isnan(th["ce_log10_tau_pre"]), tau, 10 ** np.nan_to_num(th["ce_log10_tau_pre"]))
    ref = np.stack([th["ce_psr"].astype(np.float64), th["ce_kind"].astype(np.float64), th["ce_t0_mjd"] * 86400.0, 1 / tau, 1 / pre, -0.5 / tau ** 2,
                    np.where(th["ce_sign"] < 0, -1.0, 1.0), th["ce_log10_a"] * np.log(10), th["ce_index"], th["ce_phase"] / (2 * np.pi)], axis=2)
    live = np.arange(E)[None, :] < count[:, None]
    assert np.all(tab[~live] == -7.0)
    for j in (0, 1, 2, 6, 8):
        assert np.array_equal(tab[live][:, j], ref[live][:, j]), j
    assert np.all(np.abs(tab[live] - ref[live]) <= 1e-14 * np.abs(ref[live]) + 1e-30)
    same = live & np.isnan(th["ce_log10_tau_pre"])
    assert same.any() and np.array_equal(tab[same][:, 3], tab[same][:, 4])          # NaN: tau_pre = tau


def _two_band_engine(n=E):
    eng = _engine()
    rng = np.random.default_rng(21)
    for p in eng.psrs:
        p.toas.freqs_mhz = cr.two_bands(rng, len(p.toas.freqs_mhz))
    return eng.set_chromatic_events(n)


def test_composition_with_generate_the_other_terms_td_and_a_statistic():
    from cw_reference import corner_sources, theta_of
    from test_gpu_burst import _theta as _burst_theta
    from test_gpu_fstat import SKY
    Rn = 21
    eng, plain = _two_band_engine(), _engine()
    base = plain.generate(Rn, r0=3).clone()
    # without the keys nothing changes, bit for bit, against an engine that never heard of set_chromatic_events
    assert torch.equal(eng.generate(Rn, r0=3), base)
    th = cr.random_theta(Rn, E, eng.P, seed=5, counts=True)
    th["ce_count"][:2] = [0, E]
    sig = eng.generate_per_signal(Rn, r0=3, theta=th)
    term = sig["chrom_event"]
    assert float(term.abs().max()) > 0 and not bool(term[0].any()) and "transient" not in sig
    total = eng.generate(Rn, r0=3, theta=th)
    assert torch.equal(total, base + term) and torch.equal(total, sig["total"])
    # the term of the NumPy evaluation, per pulsar, to the project's parity bound
    from pta_replicator_amd import _chrom_event as ce
    got = term.cpu().numpy()
    for r in (1, 7):
        for a, p in enumerate(eng.psrs):
            rows = [{c: th["ce_" + c][r, e] for c in ce.COLUMNS} for e in range(th["ce_count"][r]) if th["ce_psr"][r, e] == a]
            rows = [dict(row, kind=int(row["kind"])) for row in rows]
            ref = ce.term(eng.mjd[a].astype(np.float64) * 86400, p.toas.freqs_mhz, rows)
            assert np.max(np.abs(got[r, eng.off[a]:eng.off[a + 1]] - ref)) <= 1e-10 * max(np.sqrt(np.mean(ref ** 2)), 1e-300), (r, a)
    # chunks, row slots and batches: a realisation's term is the same bits
    part = eng.generate_per_signal(5, r0=3 + 7, theta={k: v[7:12] for k, v in th.items()})
    assert torch.equal(part["chrom_event"], term[7:12])
    assert torch.equal(eng.generate_per_signal(1, r0=3 + 9, theta={k: v[9:10] for k, v in th.items()})["chrom_event"], term[9:10])
    ws = eng.workspace_bytes
    eng.workspace_bytes = 1          # the smallest batches: the term batch by batch in other row slots
    small = eng.generate(Rn, r0=3, theta=th)
    eng.workspace_bytes = ws
    assert torch.equal(small, total)
    # names for the kinds, torch tensors, hyper keys
    named = dict(th, ce_kind=np.array(ce.KINDS)[th["ce_kind"]], ce_psr=torch.as_tensor(th["ce_psr"]), gwb_log10_A=np.full(Rn, -14.1))
    hbase = eng.generate(Rn, r0=3, theta={"gwb_log10_A": np.full(Rn, -14.1)}).clone()
    assert torch.equal(eng.generate(Rn, r0=3, theta=named), hbase + term)
    # with a CW source, a burst with memory and noise transients in the same realisation: the events come last
    eng.set_cw(tref=53000 * 86400.0).set_bwm().set_transients(2)
    cw, bwm, nt = theta_of(corner_sources(Rn, seed=6), True), _bwm_theta(Rn), _burst_theta(Rn, 0, 2, eng.P)
    both = eng.generate_per_signal(Rn, r0=3, theta=dict(th, **cw, **bwm, **nt))
    assert torch.equal(both["chrom_event"], term)
    assert torch.equal(both["total"], (((base + both["cw"]) + both["bwm"]) + both["transient"]) + term)
    # TD mode: deterministic keys only
    td = eng.generate_td(Rn, r0=3).clone()
    assert _sum_close(eng.generate_td(Rn, r0=3, theta=th), td, term)
    assert torch.equal(eng.generate_td(Rn, r0=3, theta=dict(th, **cw, **bwm, **nt)), (((td + both["cw"]) + both["bwm"]) + both["transient"]) + term)
    # the generation step of a statistic
    eng.prepare_f_statistic(np.array([3e-9, 2e-8]), sky=SKY)
    ref = eng.f_statistic(eng.generate(9, r0=2, theta={k: v[:9] for k, v in th.items()}))
    f = eng.generate_f_statistic(9, r0=2, theta={k: v[:9] for k, v in th.items()}, chunk=4)
    assert torch.equal(f["fp"], ref["fp"]) and torch.equal(f["fe"], ref["fe"])
    # with the chromatic process: it is added after the deterministic terms
    eng.set_chromatic_noise(-13.5, 3.0, components=8)
    ch = {"chrom_log10_A": np.full((Rn, eng.P), -13.2), "chrom_gamma": np.full((Rn, eng.P), 2.5)}
    sig = eng.generate_per_signal(Rn, r0=3, theta=dict(th, **ch))
    assert torch.equal(sig["chrom_event"], term) and torch.equal(sig["total"], eng.generate(Rn, r0=3, theta=dict(th, **ch)))
    assert _sum_close(sig["total"], base + term, sig["chrom"])


def test_sampled_labels(tmp_path_factory):
    from pta_replicator_amd import _chrom_event as ce
    Rn, n = 40, 4
    prior = dict(kind=["decay", "cusp", "bump", "annual"], log10_a=[(-6.5, -5.5), -6.0, (-7.0, -6.0), (-6.8, -6.2)], psr=[None, 2, None, None],
                 t0_mjd=[(54000.0, 56500.0), (55000.0, 55500.0), (53500.0, 57000.0), None], log10_tau=[(6.0, 7.5), (6.5, 7.0), (6.0, 7.0), None],
                 log10_tau_pre=[None, (6.0, 6.5), None, None], sign=[-1, "random", 1, -1], index=[2.0, (1.0, 4.4), 4.0, 2.0])
    eng = _two_band_engine(n)
    eng.set_chromatic_event_prior(**prior)
    rows, th = eng.generate_sampled(Rn, r0=4)
    assert set(th) == set(ce.KEYS)
    lo, hi = (x.reshape(n, 9) for x in ce.prior_bounds(eng._ce_prior))
    for j, c in enumerate(ce.COLUMNS):
        v = th["ce_" + c].cpu().numpy()
        assert v.shape == (Rn, n), c
        for e in range(n):
            if np.isnan(lo[e, j]):
                assert np.all(np.isnan(v[:, e])), (c, e)
            elif c == "psr":
                assert np.all(v[:, e] >= 0) and np.all(v[:, e] <= eng.P - 1)
            else:
                assert np.all(v[:, e] >= lo[e, j]) and np.all(v[:, e] <= hi[e, j]), (c, e)
                assert (v[:, e].std() > 0) == (hi[e, j] > lo[e, j]), (c, e)
    assert th["ce_psr"].dtype == torch.int32 and th["ce_kind"].dtype == torch.int32
    assert torch.equal(th["ce_kind"].cpu(), torch.tensor([[0, 1, 2, 3]] * Rn, dtype=torch.int32)) and bool((th["ce_psr"][:, 1] == 2).all())
    assert len(torch.unique(th["ce_psr"][:, 0])) > 2
    # the labels are the host twin's draws, bit for bit
    host = cr.build(tmp_path_factory.mktemp("chrom_event"))
    want = cr.uniform(host, eng.seed, 4, Rn, n, eng.P, lo, hi)
    for j, c in enumerate(ce.COLUMNS):
        assert np.array_equal(th["ce_" + c].cpu().numpy().astype(np.float64), want[:, :, j], equal_nan=True), c
    # the rows are generate(theta = the labels); labels are a pure function of (seed, r, slot)
    assert torch.equal(rows, eng.generate(Rn, r0=4, theta=th))
    th2 = eng.sample_theta(11, r0=4 + 9)
    for k in th:
        assert torch.equal(th2[k][~torch.isnan(th2[k].double())], th[k][9:20][~torch.isnan(th[k][9:20].double())]), k
    # every other label, and residuals - chrom_event, are those of the same engine without the event prior
    other = _two_band_engine(n).set_bwm()
    other.set_hyper_prior(gwb_log10_A=(-15, -14), rn_gamma=(2, 5))
    other.set_bwm_prior(log10_h=(-15.0, -13.5), t0_mjd=(54000.0, 56500.0))
    before = other.sample_theta(Rn, r0=4)
    rows_before = other.generate_sampled(Rn, r0=4)[0].clone()
    other.set_chromatic_event_prior(**prior)
    rows_after, after = other.generate_sampled(Rn, r0=4)
    assert set(after) == set(before) | set(th)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    for k in th:
        assert np.array_equal(after[k].cpu().numpy(), th[k].cpu().numpy(), equal_nan=True), k
    sig = other.generate_per_signal(Rn, r0=4, theta=after)
    assert torch.equal(rows_after, sig["total"]) and torch.equal(rows_after, rows_before + sig["chrom_event"])
