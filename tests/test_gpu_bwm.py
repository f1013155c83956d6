"""One burst with memory per realisation on the device: the golden add_gw_memory rows through the engine, pta_engine_bwm_add against
NumPy on a ragged array with unaligned rows, composition with generate / generate_td / the CW term, and the sampled labels."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import load, mjd_ld
from test_gpu_os import _engine, _psrs

pytestmark = pytest.mark.gpu

# the golden burst (oracle/gen_golden.py: add_gw_memory(p, 3e-14, 0.7, 5.1, 0.9, 55500.0))
GOLDEN = {"bwm_log10_h": np.log10(3e-14), "bwm_cos_gwtheta": np.cos(0.7), "bwm_gwphi": 5.1, "bwm_psi": 0.9, "bwm_t0_mjd": 55500.0}


def _theta(R, seed=3, t0=(53500.0, 57000.0)):
    rng = np.random.default_rng(seed)
    return {"bwm_log10_h": rng.uniform(-15, -13, R), "bwm_cos_gwtheta": rng.uniform(-1, 1, R), "bwm_gwphi": rng.uniform(0, 2 * np.pi, R),
            "bwm_psi": rng.uniform(0, np.pi, R), "bwm_t0_mjd": rng.uniform(*t0, R)}


def test_golden_add_gw_memory_through_the_engine():
    """the three pulsars of transients.npz, white noise only: both rows of generate_per_signal's "bwm" within 1e-10 relative RMS of the
    reference's add_gw_memory, exactly 0 before the epoch."""
    from pta_replicator_amd.engine import ReplicaEngine
    from pta_replicator_amd.simulate import ArrayTOAs, SimulatedPulsar, make_ideal
    z = load("transients.npz")
    psrs = []
    for i in range(3):
        p = SimulatedPulsar(toas=ArrayTOAs(mjd_ld(z, "", i), z[f"err_us_{i}"]), name=str(z["names"][i]),
                            loc={"RAJ": float(z["raj_hours"][i]), "DECJ": float(z["decj_deg"][i])})
        make_ideal(p)
        psrs.append(p)
    eng = ReplicaEngine(psrs, seed=1)
    eng.set_white_noise(efac=1.0)
    eng.set_bwm()
    sig = eng.generate_per_signal(2, theta={k: np.full(2, v) for k, v in GOLDEN.items()})
    assert set(sig) == {"wn", "total", "bwm"}
    got = sig["bwm"].cpu().numpy()
    assert np.array_equal(got[0], got[1])
    for a in range(3):
        g, ref = got[0, eng.off[a]:eng.off[a + 1]], z["gw_memory"][a]
        before = eng.mjd[a] * 86400 < 55500.0 * 86400
        assert 0 < before.sum() < len(g) and np.all(g[before] == 0.0)
        err = float(np.sqrt(np.mean((g - ref) ** 2) / np.mean(ref ** 2)))
        print(f"pulsar {a}: relative RMS deviation from the golden {err:.3g}")
        assert err <= 1e-10, (a, err)
    assert torch.equal(sig["total"], sig["wn"] + sig["bwm"])


COUNTS = [1, 15, 17, 64, 65, 130, 301]


@pytest.fixture(scope="module")
def ragged():
    """an engine over pulsars of COUNTS TOAs (odd offsets, a 301-TOA pulsar of two tiles), white noise only"""
    from pta_replicator_amd.engine import ReplicaEngine
    from pta_replicator_amd.simulate import ArrayTOAs, SimulatedPulsar, make_ideal
    rng = np.random.default_rng(5)
    psrs = []
    for a, n in enumerate(COUNTS):
        p = SimulatedPulsar(toas=ArrayTOAs(np.sort(rng.uniform(53000, 57500, n)), 0.5), name=f"J{a:04d}",
                            loc={"RAJ": float(rng.uniform(0, 24)), "DECJ": float(np.degrees(np.arcsin(rng.uniform(-1, 1))))})
        make_ideal(p)
        psrs.append(p)
    eng = ReplicaEngine(psrs, seed=2)
    eng.td_warmup = False
    eng.set_white_noise(efac=1.0)
    eng.prepare()
    assert list(eng.counts) == COUNTS and eng.plan.n_tiles == 8
    return eng


@pytest.mark.parametrize("pad", [3, 4])   # n_toa = 593: an even and an odd row stride (the rows' alignment then alternates)
@pytest.mark.parametrize("accumulate", [0, 1])
def test_bwm_add_vs_numpy_on_a_ragged_array(ragged, pad, accumulate):
    """pta_engine_bwm_add from given coef / t0 tables against NumPy, to <= 2 ulp per element; unaligned heads and tails, R = 19 (no
    multiple of the realisation group), nothing written past n_toa; epochs before all TOAs, after all TOAs and exactly on a TOA."""
    from pta_replicator_amd import _bwm, _lib, device as dv
    eng = ragged
    R, P, N = 19, eng.P, eng.n_toa
    ld = N + pad
    rng = np.random.default_rng(10 * pad + accumulate)
    toa = np.concatenate([m * 86400 for m in eng.mjd])
    coef = rng.normal(size=(R, P)) * 1e-15
    t0 = rng.uniform(53500, 57000, R) * 86400
    t0[0], t0[1], t0[2] = 52000 * 86400.0, 58000 * 86400.0, toa[eng.off[6] + 100]
    base = rng.normal(size=(R, ld)) * 1e-7
    out = dv.f64(base)
    d_coef, d_t0 = dv.f64(coef), dv.f64(t0)
    b = _lib.BwmEngine()
    b.n_psr, b.toa_s, b.coef, b.t0_s = P, eng.d_toa_s.data_ptr(), d_coef.data_ptr(), d_t0.data_ptr()
    s = dv.stream_ptr()
    _lib.call("pta_engine_bwm_add", ctypes.byref(eng.plan), ctypes.byref(b), R, dv.ptr(out), ld, accumulate, s)
    got = out.cpu().numpy()
    term = _bwm.ramp(np.repeat(coef, eng.counts, axis=1), t0[:, None], toa[None, :])
    ref = base[:, :N] + term if accumulate else term
    assert np.array_equal(got[:, N:], base[:, N:])                       # the pad columns are untouched
    ulp = np.abs(got[:, :N] - ref) / np.spacing(np.maximum(np.abs(ref), 1e-300))
    print(f"pad={pad} accumulate={accumulate}: max deviation {ulp.max():.1f} ulp")
    assert ulp.max() <= 2
    assert np.all(term[0] != 0) and np.all(term[1] == 0)                 # before every TOA: a ramp everywhere; after: nothing
    i = eng.off[6] + 100
    assert term[2, i] == 0 and np.all(term[2, eng.off[6]:i] == 0) and term[2, i + 1] != 0
    if not accumulate:
        assert np.array_equal(got[1, :N], np.zeros(N)) and got[2, i] == 0
    # rows 13 .. 15 alone, in other row slots of another buffer: bit-equal to the same rows of the batch
    base2 = np.ascontiguousarray(base[13:16])
    out2 = dv.f64(base2)
    b.coef, b.t0_s = d_coef.data_ptr() + 8 * 13 * P, d_t0.data_ptr() + 8 * 13
    _lib.call("pta_engine_bwm_add", ctypes.byref(eng.plan), ctypes.byref(b), 3, dv.ptr(out2), ld, accumulate, s)
    assert np.array_equal(out2.cpu().numpy(), got[13:16])


def test_bwm_params_vs_numpy(ragged):
    """pta_engine_bwm_params against NumPy's antenna patterns (f_statistic.antenna_patterns: the same m, n, Omega)"""
    from pta_replicator_amd import _bwm, _lib, device as dv, f_statistic as fst
    eng = ragged
    R, P = 11, eng.P
    th = _theta(R)
    src = dv.f64(np.stack([th[k] for k in _bwm.KEYS], axis=1))
    coef, t0 = dv.zeros((R, P)), dv.zeros((R,))
    b = _lib.BwmEngine()
    b.n_psr, b.phat, b.src, b.ld_src, b.coef, b.t0_s = P, eng._phat_device().data_ptr(), src.data_ptr(), 5, coef.data_ptr(), t0.data_ptr()
    _lib.call("pta_engine_bwm_params", ctypes.byref(b), R, dv.stream_ptr())
    phi = fst.antenna_patterns(eng._phat_device().cpu().numpy(), th["bwm_cos_gwtheta"], th["bwm_gwphi"])   # [P, R, 2]
    ref = 10 ** th["bwm_log10_h"][:, None] * (np.cos(2 * th["bwm_psi"])[:, None] * phi[:, :, 0].T + np.sin(2 * th["bwm_psi"])[:, None] * phi[:, :, 1].T)
    assert np.max(np.abs(coef.cpu().numpy() - ref)) <= 1e-12 * np.max(np.abs(ref))
    assert np.array_equal(t0.cpu().numpy(), th["bwm_t0_mjd"] * 86400.0)


def _sum_close(total, base, term):
    """total = base + term to the rounding of one sum"""
    total, base, term = (x.cpu().numpy() for x in (total, base, term))
    return np.all(np.abs(total - (base + term)) <= 2 * np.spacing(np.maximum(np.abs(total), np.abs(base))))


def test_composition_with_generate_cw_and_td():
    from cw_reference import corner_sources, theta_of
    R = 21
    eng = _engine()
    plain = _engine()
    base = eng.generate(R, r0=3).clone()
    eng.set_bwm()
    # without bwm keys nothing changes, bit for bit, against an engine that never heard of set_bwm
    assert torch.equal(eng.generate(R, r0=3), plain.generate(R, r0=3)) and torch.equal(base, plain.generate(R, r0=3))
    th = _theta(R)
    sig = eng.generate_per_signal(R, r0=3, theta=th)
    term = sig["bwm"]
    assert "cw" not in sig and float(term.abs().max()) > 0
    total = eng.generate(R, r0=3, theta=th)
    assert torch.equal(total, sig["total"]) and _sum_close(total, base, term)
    # chunks and row slots: a realisation's term is the same bits
    assert torch.equal(eng.generate_per_signal(5, r0=3 + 7, theta={k: v[7:12] for k, v in th.items()})["bwm"], term[7:12])
    # with hyper keys and as torch tensors
    hyper = {"gwb_log10_A": np.full(R, -14.1)}
    hbase = eng.generate(R, r0=3, theta=hyper).clone()
    assert torch.equal(eng.generate(R, r0=3, theta=dict(th, **hyper, bwm_psi=torch.as_tensor(th["bwm_psi"]))), hbase + term)
    # with a CW source in the same realisation: CW first, then the burst
    eng.set_cw(tref=53000 * 86400.0)
    cw = theta_of(corner_sources(R, seed=6), True)
    both = eng.generate_per_signal(R, r0=3, theta=dict(th, **cw))
    assert torch.equal(both["bwm"], term) and torch.equal(both["cw"], eng.generate_per_signal(R, r0=3, theta=cw)["cw"])
    assert torch.equal(both["total"], (base + both["cw"]) + term)
    # TD mode: deterministic keys only
    td = eng.generate_td(R, r0=3).clone()
    assert _sum_close(eng.generate_td(R, r0=3, theta=th), td, term)
    assert torch.equal(eng.generate_td(R, r0=3, theta=dict(th, **cw)), (td + both["cw"]) + term)


def test_generate_f_statistic_takes_the_burst():
    """the generation step of a statistic: the same rows as generate(theta=bwm), whatever the chunk"""
    from test_gpu_fstat import SKY
    R = 9
    eng = _engine().set_bwm()
    eng.prepare_f_statistic(np.array([3e-9, 2e-8]), sky=SKY)
    th = _theta(R)
    ref = eng.f_statistic(eng.generate(R, r0=2, theta=th))
    for chunk, td in ((4, False), (R, False)):
        got = eng.generate_f_statistic(R, r0=2, theta=th, chunk=chunk, td=td)
        assert torch.equal(got["fp"], ref["fp"]) and torch.equal(got["fe"], ref["fe"])
    ref_td = eng.f_statistic(eng.generate_td(R, r0=2, theta=th))
    assert torch.equal(eng.generate_f_statistic(R, r0=2, theta=th, chunk=4, td=True)["fp"], ref_td["fp"])


def test_sampled_labels():
    R = 40
    boxes = dict(log10_h=(-15.0, -13.5), t0_mjd=(54000.0, 56500.0))
    eng = _engine().set_bwm()
    eng.set_bwm_prior(**boxes)
    rows, th = eng.generate_sampled(R, r0=4)
    assert set(th) == {"bwm_log10_h", "bwm_cos_gwtheta", "bwm_gwphi", "bwm_psi", "bwm_t0_mjd"}
    lim = {"bwm_log10_h": boxes["log10_h"], "bwm_t0_mjd": boxes["t0_mjd"], "bwm_cos_gwtheta": (-1, 1), "bwm_gwphi": (0, 2 * np.pi),
           "bwm_psi": (0, np.pi)}
    for k, (lo, hi) in lim.items():
        v = th[k].cpu().numpy()
        assert v.shape == (R,) and np.all(v >= lo) and np.all(v <= hi) and v.std() > 0, k
    # the rows are generate(theta = the labels); labels are a pure function of (seed, r): r0 offsets and chunks are bit-equal
    assert torch.equal(rows, eng.generate(R, r0=4, theta=th))
    th2 = eng.sample_theta(11, r0=4 + 9)
    rows2, th3 = eng.generate_sampled(11, r0=4 + 9)
    for k in th:
        assert torch.equal(th2[k], th[k][9:20]) and torch.equal(th3[k], th[k][9:20]), k
    assert torch.equal(rows2, rows[9:20])
    # set_hyper_prior's and set_cw_prior's labels do not move when the burst prior is added
    other = _engine().set_cw()
    other.set_hyper_prior(gwb_log10_A=(-15, -14), rn_gamma=(2, 5))
    other.set_cw_prior(log10_mc=(8, 9.5), log10_fgw=(-8.7, -7.5), log10_h=(-15, -14))
    before = other.sample_theta(R, r0=4)
    rows_before = other.generate_sampled(R, r0=4)[0].clone()
    other.set_bwm().set_bwm_prior(**boxes)
    after = other.sample_theta(R, r0=4)
    assert set(after) == set(before) | set(th)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    for k in th:
        assert torch.equal(after[k], th[k]), k                          # the same seed: the same burst labels, whatever else is sampled
    rows_after, _ = other.generate_sampled(R, r0=4)
    term = other.generate_per_signal(R, r0=4, theta=after)["bwm"]
    assert _sum_close(rows_after, rows_before, term)
