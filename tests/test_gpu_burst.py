"""Sine-Gaussian wavelets per realisation on the device: the golden add_burst / add_noise_transient rows through the engine,
pta_engine_burst_add / pta_engine_transient_add against long-double NumPy on a ragged array with unaligned rows, the quadratic removal,
composition with generate / generate_td / the CW and BWM terms, and the sampled labels."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import load, mjd_ld
from test_burst_host import GWPHI, GWTHETA, PSI, WAVELET, fold, term_ld
from test_gpu_bwm import _sum_close, _theta as _bwm_theta, ragged   # noqa: F401  (ragged: the fixture)
from test_gpu_os import _engine

pytestmark = pytest.mark.gpu


def _theta(R, W=0, V=0, P=6, seed=3, counts=False):
    """random burst_* (W > 0) and nt_* (V > 0) keys; tau >= 1.6e7 s keeps every envelope over the 4500-day span a normal number"""
    rng = np.random.default_rng(seed)
    th = {}
    if W:
        th.update({"burst_cos_gwtheta": rng.uniform(-1, 1, R), "burst_gwphi": rng.uniform(0, 2 * np.pi, R), "burst_psi": rng.uniform(0, np.pi, R),
                   "burst_t0_mjd": rng.uniform(53500, 57000, (R, W)), "burst_log10_tau": rng.uniform(7.2, 8.0, (R, W)),
                   "burst_log10_f": rng.uniform(-8.5, -7.0, (R, W)), "burst_log10_a_plus": rng.uniform(-7.5, -6.5, (R, W)),
                   "burst_phase_plus": rng.uniform(0, 2 * np.pi, (R, W)), "burst_log10_a_cross": rng.uniform(-7.5, -6.5, (R, W)),
                   "burst_phase_cross": rng.uniform(0, 2 * np.pi, (R, W))})
        if counts:
            th["burst_count"] = rng.integers(0, W + 1, R)
    if V:
        th.update({"nt_psr": rng.integers(0, P, (R, V)), "nt_t0_mjd": rng.uniform(53500, 57000, (R, V)), "nt_log10_tau": rng.uniform(7.2, 8.0, (R, V)),
                   "nt_log10_f": rng.uniform(-8.5, -7.0, (R, V)), "nt_log10_a": rng.uniform(-7.0, -6.0, (R, V)),
                   "nt_phase": rng.uniform(0, 2 * np.pi, (R, V))})
        if counts:
            th["nt_count"] = rng.integers(0, V + 1, R)
    return th


def _golden_engine():
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
    return z, eng


def test_golden_burst_and_transient_through_the_engine():
    """the three 150-TOA pulsars of transients.npz, white noise only, R = 2: the "burst" entry of generate_per_signal with and without
    remove_quad and the "transient" entry with V = 3 (the plus wavelet in every pulsar), each within 1e-10 relative RMS of the
    reference's rows per pulsar, both rows equal, total = wn + burst (+ transient)"""
    z, eng = _golden_engine()
    R = 2
    th = {"burst_cos_gwtheta": np.full(R, np.cos(GWTHETA)), "burst_gwphi": np.full(R, GWPHI), "burst_psi": np.full(R, PSI)}
    th.update({"burst_" + k: np.full((R, 1), v) for k, v in WAVELET.items()})
    nt = {"nt_psr": np.tile(np.arange(3), (R, 1)), "nt_t0_mjd": np.full((R, 3), WAVELET["t0_mjd"]), "nt_log10_tau": np.full((R, 3), WAVELET["log10_tau"]),
          "nt_log10_f": np.full((R, 3), WAVELET["log10_f"]), "nt_log10_a": np.full((R, 3), WAVELET["log10_a_plus"]), "nt_phase": np.zeros((R, 3))}

    def check(got, key):
        got = got.cpu().numpy()
        assert np.array_equal(got[0], got[1])
        for a in range(3):
            g, ref = got[0, eng.off[a]:eng.off[a + 1]], z[key][a]
            err = float(np.sqrt(np.mean((g - ref) ** 2) / np.mean(ref ** 2)))
            print(f"{key} pulsar {a}: relative RMS deviation from the golden {err:.3g}")
            assert err <= 1e-10, (key, a, err)
    eng.set_burst(1).set_transients(3)
    sig = eng.generate_per_signal(R, theta=th)
    assert set(sig) == {"wn", "total", "burst"}
    check(sig["burst"], "burst")
    assert torch.equal(sig["total"], sig["wn"] + sig["burst"])
    sig = eng.generate_per_signal(R, theta=dict(th, **nt))
    assert set(sig) == {"wn", "total", "burst", "transient"}
    check(sig["transient"], "noise_transient")
    assert torch.equal(sig["total"], (sig["wn"] + sig["burst"]) + sig["transient"])
    eng.set_burst(1, remove_quad=True)
    sig = eng.generate_per_signal(R, theta=th)
    check(sig["burst"], "burst_quad")
    assert torch.equal(sig["total"], sig["wn"] + sig["burst"])


def _burst_tables(eng, R, W, seed):
    """random table rows of pta_engine_burst_add for the ragged engine: wav [R, W, 7], kk [R, P, 2], count [R] covering 0, 1 and W; row 1
    holds one wavelet 40 tau before the first TOA, rows past a count are NaN (never read)"""
    rng = np.random.default_rng(seed)
    toa = np.concatenate([m * 86400 for m in eng.mjd])
    tau = 10 ** rng.uniform(7.2, 8.0, (R, W))
    wav = np.stack([rng.uniform(53500, 57000, (R, W)) * 86400, -0.5 / tau ** 2, 10 ** rng.uniform(-8.5, -6.0, (R, W))]
                   + [rng.normal(size=(R, W)) * 1e-7 for _ in range(4)], axis=2)
    count = rng.choice([0, 1, W], R)
    count[:3] = [0, 1, W]
    wav[1, 0, :3] = [toa.min() - 40 * 1e6, -0.5 / 1e6 ** 2, 2e-8]
    for r in range(R):
        wav[r, count[r]:] = np.nan
    kk = rng.normal(size=(R, eng.P, 2))
    return toa, np.ascontiguousarray(wav), kk, count.astype(np.int32)


def _burst_ref(eng, toa, wav, kk, count):
    """(ref, bound) [R, n_toa] in long double from the table rows (test_burst_host.term_ld)"""
    R, N = len(wav), len(toa)
    ref, bound = np.zeros((R, N), dtype=np.longdouble), np.zeros((R, N), dtype=np.longdouble)
    for r in range(R):
        w = wav[r, :count[r]]
        for a in range(eng.P):
            if count[r]:
                C, S = fold(w, kk[r, a])
                sl = slice(eng.off[a], eng.off[a + 1])
                ref[r, sl], bound[r, sl] = term_ld(w[:, 0], w[:, 1], w[:, 2], C, S, toa[sl])
    return ref, bound


def _check_rows(got, base, ref, bound, accumulate, skip):
    """|got - (base +) ref| <= bound per element (accumulating: plus the rounding of the one add, an ulp of the sum)"""
    R = len(got)
    keep = np.array([r not in skip for r in range(R)])
    want = base + ref if accumulate else ref
    err = np.abs(got.astype(np.longdouble) - want)
    lim = bound + (np.spacing(np.abs(got)) if accumulate else 0)
    worst = float(np.max((err / np.where(lim > 0, lim, 1))[keep]))
    print(f"accumulate={accumulate}: worst deviation in units of the bound {worst:.3g}")
    assert np.all(err[keep] <= lim[keep]), worst


@pytest.mark.parametrize("pad", [3, 4])   # n_toa = 593: an even and an odd row stride
@pytest.mark.parametrize("accumulate", [0, 1])
def test_burst_add_vs_long_double_on_a_ragged_array(ragged, pad, accumulate):
    """pta_engine_burst_add from given tables against long double NumPy, element by element within the rounding bound of
    test_burst_host.term_ld; R = 19 (no multiple of the realisation group), W = 5 with counts 0, 1 and 5, nothing written past n_toa,
    a count-0 row exactly 0 (written) or untouched (accumulating), a wavelet 40 tau before the first TOA contributing exactly
    nothing, rows 13 .. 15 launched alone in other row slots bit-equal to the batch"""
    from pta_replicator_amd import _lib, device as dv
    eng = ragged
    R, W, P, N = 19, 5, eng.P, eng.n_toa
    ld = N + pad
    toa, wav, kk, count = _burst_tables(eng, R, W, seed=10 * pad + accumulate)
    rng = np.random.default_rng(7)
    base = rng.normal(size=(R, ld)) * 1e-7
    out, d_wav, d_kk, d_count = dv.f64(base), dv.f64(wav), dv.f64(kk), dv.i32(count)
    b = _lib.BurstEngine()
    b.n_psr, b.n_wav, b.toa_s = P, W, eng.d_toa_s.data_ptr()
    b.wav, b.kk, b.count = d_wav.data_ptr(), d_kk.data_ptr(), d_count.data_ptr()
    s = dv.stream_ptr()
    _lib.call("pta_engine_burst_add", ctypes.byref(eng.plan), ctypes.byref(b), R, dv.ptr(out), ld, accumulate, s)
    got = out.cpu().numpy()
    assert np.array_equal(got[:, N:], base[:, N:])                       # the pad columns are untouched
    assert np.all(np.isfinite(got))                                      # NaN rows past the counts were never read
    ref, bound = _burst_ref(eng, toa, wav, kk, count)
    _check_rows(got[:, :N], base[:, :N], ref, bound, accumulate, skip={1})
    for r in np.flatnonzero(count == 0).tolist() + [1]:                  # no wavelet, or one whose envelope is exactly 0 everywhere
        assert np.array_equal(got[r, :N], base[r, :N] if accumulate else np.zeros(N)), r
    assert np.count_nonzero(got[2, :N] != (base[2, :N] if accumulate else 0)) > N // 2
    base2 = np.ascontiguousarray(base[13:16])
    out2 = dv.f64(base2)
    b.wav, b.kk, b.count = d_wav.data_ptr() + 8 * 13 * W * 7, d_kk.data_ptr() + 8 * 13 * P * 2, d_count.data_ptr() + 4 * 13
    _lib.call("pta_engine_burst_add", ctypes.byref(eng.plan), ctypes.byref(b), 3, dv.ptr(out2), ld, accumulate, s)
    assert np.array_equal(out2.cpu().numpy(), got[13:16])
    if not accumulate and pad == 3:                                      # count = NULL: every row has W wavelets
        full = np.where(np.isnan(wav), 1.0, wav)
        full[..., 0] = np.where(np.isnan(wav[..., 0]), 55000.0 * 86400, wav[..., 0])
        full[..., 1] = np.where(np.isnan(wav[..., 1]), -0.5 / 3e7 ** 2, wav[..., 1])
        full[..., 2] = np.where(np.isnan(wav[..., 2]), 1e-8, wav[..., 2])
        full[1, 0] = full[1, 1]
        d_full = dv.f64(full)
        b.wav, b.kk, b.count = d_full.data_ptr(), d_kk.data_ptr(), None
        _lib.call("pta_engine_burst_add", ctypes.byref(eng.plan), ctypes.byref(b), R, dv.ptr(out), ld, 0, s)
        ref, bound = _burst_ref(eng, toa, full, kk, np.full(R, W))
        _check_rows(out.cpu().numpy()[:, :N], None, ref, bound, 0, skip=set())


@pytest.mark.parametrize("pad", [3, 4])
@pytest.mark.parametrize("accumulate", [0, 1])
def test_transient_add_vs_long_double_on_a_ragged_array(ragged, pad, accumulate):
    """pta_engine_transient_add likewise, V = 4: two transients in one pulsar, one in the 1-TOA pulsar, an nt_count of 0, a pulsar
    without a transient left exactly alone"""
    from pta_replicator_amd import _lib, device as dv
    eng = ragged
    R, V, P, N = 19, 4, eng.P, eng.n_toa
    ld = N + pad
    rng = np.random.default_rng(20 * pad + accumulate)
    toa = np.concatenate([m * 86400 for m in eng.mjd])
    tau = 10 ** rng.uniform(7.2, 8.0, (R, V))
    tab = np.stack([rng.integers(0, P, (R, V)).astype(np.float64), rng.uniform(53500, 57000, (R, V)) * 86400, -0.5 / tau ** 2,
                    10 ** rng.uniform(-8.5, -6.0, (R, V))] + [rng.normal(size=(R, V)) * 1e-7 for _ in range(2)], axis=2)
    tab[0, :, 0] = [6, 6, 0, 3]                 # two in the 301-TOA pulsar, one in the 1-TOA pulsar
    count = rng.choice([1, 2, V], R)
    count[:3] = [V, 0, 2]
    for r in range(R):
        tab[r, count[r]:] = np.nan
    tab = np.ascontiguousarray(tab)
    base = rng.normal(size=(R, ld)) * 1e-7
    out, d_tab, d_count = dv.f64(base), dv.f64(tab), dv.i32(count)
    t = _lib.TransientEngine()
    t.n_psr, t.n_wav, t.toa_s, t.tab, t.count = P, V, eng.d_toa_s.data_ptr(), d_tab.data_ptr(), d_count.data_ptr()
    s = dv.stream_ptr()
    _lib.call("pta_engine_transient_add", ctypes.byref(eng.plan), ctypes.byref(t), R, dv.ptr(out), ld, accumulate, s)
    got = out.cpu().numpy()
    assert np.array_equal(got[:, N:], base[:, N:]) and np.all(np.isfinite(got))
    ref, bound = np.zeros((R, N), dtype=np.longdouble), np.zeros((R, N), dtype=np.longdouble)
    for r in range(R):
        for a in range(P):
            w = tab[r, :count[r]]
            w = w[w[:, 0] == a]
            if len(w):
                sl = slice(eng.off[a], eng.off[a + 1])
                ref[r, sl], bound[r, sl] = term_ld(w[:, 1], w[:, 2], w[:, 3], w[:, 4], w[:, 5], toa[sl])
    _check_rows(got[:, :N], base[:, :N], ref, bound, accumulate, skip=set())
    assert np.array_equal(got[1, :N], base[1, :N] if accumulate else np.zeros(N))        # nt_count = 0
    quiet = slice(eng.off[1], eng.off[3])                                                # pulsars 1, 2 of row 0 carry no transient
    assert np.array_equal(got[0, quiet], base[0, quiet] if accumulate else np.zeros(eng.off[3] - eng.off[1]))
    assert got[0, 0] != (base[0, 0] if accumulate else 0) and np.all(ref[0, eng.off[6]:] != 0)
    out2 = dv.f64(np.ascontiguousarray(base[13:16]))
    t.tab, t.count = d_tab.data_ptr() + 8 * 13 * V * 6, d_count.data_ptr() + 4 * 13
    _lib.call("pta_engine_transient_add", ctypes.byref(eng.plan), ctypes.byref(t), 3, dv.ptr(out2), ld, accumulate, s)
    assert np.array_equal(out2.cpu().numpy(), got[13:16])


def test_remove_quad_on_a_ragged_array(ragged):
    """with remove_quad the term is orthogonal to (1, t, t^2) over every pulsar's TOAs: |Q_a^T term| <= 64 2^-52 ||term_a||_1 for every
    (r, a) with more than 3 TOAs (column sums of n <= 301 terms against unit-norm columns), the 1-TOA pulsar's term is 0, and the
    coefficients of a row are the same bits computed alone and in the batch"""
    from pta_replicator_amd import _burst, _lib, device as dv
    eng = ragged
    R, W, P, N = 19, 5, eng.P, eng.n_toa
    toa, wav, kk, count = _burst_tables(eng, R, W, seed=5)
    Q = _burst.quad_basis([m * 86400 for m in eng.mjd])
    assert Q.shape == (N, 3) and np.all(Q[:1] == 0)
    d_wav, d_kk, d_count, d_q, d_off = dv.f64(wav), dv.f64(kk), dv.i32(count), dv.f64(Q), dv.i32(np.asarray(eng.off, dtype=np.int32))
    plain, quad, c = dv.zeros((R, N)), dv.zeros((R, N)), dv.zeros((R, P, 3))
    b = _lib.BurstEngine()
    b.n_psr, b.n_wav, b.toa_s = P, W, eng.d_toa_s.data_ptr()
    b.wav, b.kk, b.count = d_wav.data_ptr(), d_kk.data_ptr(), d_count.data_ptr()
    s = dv.stream_ptr()
    _lib.call("pta_engine_burst_add", ctypes.byref(eng.plan), ctypes.byref(b), R, dv.ptr(plain), N, 0, s)
    b.psr_off, b.quad_q, b.quad_c = d_off.data_ptr(), d_q.data_ptr(), c.data_ptr()
    _lib.call("pta_engine_burst_add", ctypes.byref(eng.plan), ctypes.byref(b), R, dv.ptr(quad), N, 0, s)
    plain, quad, cc = plain.cpu().numpy(), quad.cpu().numpy(), c.cpu().numpy()
    assert np.all(quad[:, :1] == 0) and np.all(cc[:, 0] == 0)                              # the 1-TOA pulsar
    worst = 0.0
    for r in range(R):
        for a in range(1, P):
            sl = slice(eng.off[a], eng.off[a + 1])
            l1 = np.sum(np.abs(plain[r, sl]))
            proj = np.abs(Q[sl].T.astype(np.longdouble) @ quad[r, sl].astype(np.longdouble))
            if l1 > 0:
                worst = max(worst, float(proj.max() / l1) / 2.0 ** -52)
            assert np.all(proj <= 64 * 2.0 ** -52 * l1), (r, a)
            # the coefficients are the projection of the term the add kernel evaluates
            assert np.allclose(cc[r, a], Q[sl].T @ plain[r, sl], rtol=0, atol=64 * 2.0 ** -52 * l1)
    print(f"worst |Q^T term| / ||term||_1 = {worst:.3g} x 2^-52")
    assert np.all(quad[count == 0] == 0) and np.count_nonzero(quad[2]) > N // 2
    c2, quad2 = dv.zeros((3, P, 3)), dv.zeros((3, N))
    b.wav, b.kk, b.count, b.quad_c = d_wav.data_ptr() + 8 * 13 * W * 7, d_kk.data_ptr() + 8 * 13 * P * 2, d_count.data_ptr() + 4 * 13, c2.data_ptr()
    _lib.call("pta_engine_burst_add", ctypes.byref(eng.plan), ctypes.byref(b), 3, dv.ptr(quad2), N, 0, s)
    assert np.array_equal(c2.cpu().numpy(), cc[13:16]) and np.array_equal(quad2.cpu().numpy(), quad[13:16])


def test_params_vs_numpy(ragged):
    """pta_engine_burst_params / pta_engine_transient_params against NumPy: the table rows from the labels, rows past a count untouched"""
    from pta_replicator_amd import _burst, _lib, device as dv, f_statistic as fst
    eng = ragged
    R, W, V, P = 11, 3, 2, eng.P
    th = _theta(R, W, V, P, seed=8)
    sky = dv.f64(np.stack([th[k] for k in _burst.SKY_KEYS], axis=1))
    src = dv.f64(np.stack([th[k] for k in _burst.WAV_KEYS], axis=2))
    count = np.array([0, 1, 2, 3] * 3)[:R].astype(np.int32)
    wav, kk = torch.full((R, W, 7), -7.0, dtype=torch.float64, device=sky.device), dv.zeros((R, P, 2))
    b = _lib.BurstEngine()
    b.n_psr, b.n_wav, b.phat, b.sky, b.src, b.wav, b.kk = P, W, eng._phat_device().data_ptr(), sky.data_ptr(), src.data_ptr(), wav.data_ptr(), kk.data_ptr()
    d_count = dv.i32(count)
    b.count = d_count.data_ptr()
    _lib.call("pta_engine_burst_params", ctypes.byref(b), R, dv.stream_ptr())
    wav, kk = wav.cpu().numpy(), kk.cpu().numpy()
    ap, ac = 10 ** th["burst_log10_a_plus"], 10 ** th["burst_log10_a_cross"]
    ref = np.stack([th["burst_t0_mjd"] * 86400.0, -0.5 / (10 ** th["burst_log10_tau"]) ** 2, 10 ** th["burst_log10_f"],
                    ap * np.cos(th["burst_phase_plus"]), ap * np.sin(th["burst_phase_plus"]), ac * np.cos(th["burst_phase_cross"]),
                    ac * np.sin(th["burst_phase_cross"])], axis=2)
    live = np.arange(W)[None, :] < count[:, None]
    assert np.all(wav[~live] == -7.0) and np.array_equal(wav[live][:, 0], ref[live][:, 0])
    assert np.all(np.abs(wav[live] - ref[live]) <= 1e-14 * np.abs(ref[live]) + 1e-30)
    phi = fst.antenna_patterns(eng._phat_device().cpu().numpy(), th["burst_cos_gwtheta"], th["burst_gwphi"])   # [P, R, 2]
    fp, fc = phi[:, :, 0].T, phi[:, :, 1].T
    c2, s2 = np.cos(2 * th["burst_psi"])[:, None], np.sin(2 * th["burst_psi"])[:, None]
    ref_kk = np.stack([-(fp * c2 + fc * s2), fp * s2 - fc * c2], axis=2)
    assert np.max(np.abs(kk - ref_kk)) <= 1e-12 * np.max(np.abs(ref_kk))
    nsrc = dv.f64(np.stack([np.asarray(th[k], dtype=np.float64) for k in _burst.NT_KEYS], axis=2))
    tab = dv.zeros((R, V, 6))
    t = _lib.TransientEngine()
    t.n_psr, t.n_wav, t.src, t.tab = P, V, nsrc.data_ptr(), tab.data_ptr()
    _lib.call("pta_engine_transient_params", ctypes.byref(t), R, dv.stream_ptr())
    a = 10 ** th["nt_log10_a"]
    ref = np.stack([th["nt_psr"].astype(np.float64), th["nt_t0_mjd"] * 86400.0, -0.5 / (10 ** th["nt_log10_tau"]) ** 2, 10 ** th["nt_log10_f"],
                    a * np.cos(th["nt_phase"]), -a * np.sin(th["nt_phase"])], axis=2)
    tab = tab.cpu().numpy()
    assert np.array_equal(tab[..., :2], ref[..., :2]) and np.all(np.abs(tab - ref) <= 1e-14 * np.abs(ref) + 1e-30)


def test_term_matches_the_numpy_oracle():
    """the engine's burst and transient entries against the NumPy evaluation the list API's callables use (_burst.burst_term,
    _burst.waveform), per pulsar, to the project's parity bound"""
    from pta_replicator_amd import _burst
    from pta_replicator_amd.deterministic import antenna_patterns
    R, W, V = 3, 4, 3
    eng = _engine().set_burst(W).set_transients(V)
    th = _theta(R, W, V, eng.P, seed=21)
    sig = eng.generate_per_signal(R, r0=1, theta=th)
    burst, nt = sig["burst"].cpu().numpy(), sig["transient"].cpu().numpy()
    for r in range(R):
        ws = [{c: th["burst_" + c][r, w] for c in _burst.WAV_COLUMNS} for w in range(W)]
        for a, p in enumerate(eng.psrs):
            sl = slice(eng.off[a], eng.off[a + 1])
            t = eng.mjd[a] * 86400
            fp, fc, _ = antenna_patterns(p, np.arccos(th["burst_cos_gwtheta"][r]), th["burst_gwphi"][r])
            ref = _burst.burst_term(t, fp, fc, th["burst_psi"][r], ws)
            assert np.sqrt(np.mean((burst[r, sl] - ref) ** 2) / np.mean(ref ** 2)) <= 1e-10, (r, a)
            mine = [{c: th["nt_" + c][r, v] for c in _burst.NT_COLUMNS[1:]} for v in range(V) if th["nt_psr"][r, v] == a]
            ref = _burst.waveform(mine)(t) if mine else np.zeros(len(t))
            assert np.max(np.abs(nt[r, sl] - ref)) <= 1e-10 * max(np.sqrt(np.mean(ref ** 2)), 1e-300), (r, a)


def test_composition_with_generate_cw_bwm_and_td():
    from cw_reference import corner_sources, theta_of
    R, W, V = 21, 3, 2
    eng = _engine()
    plain = _engine()
    base = eng.generate(R, r0=3).clone()
    eng.set_burst(W).set_transients(V)
    # without the keys nothing changes, bit for bit, against an engine that never heard of set_burst / set_transients
    assert torch.equal(eng.generate(R, r0=3), plain.generate(R, r0=3)) and torch.equal(base, plain.generate(R, r0=3))
    th = _theta(R, W, V, eng.P, counts=True)
    bt = {k: v for k, v in th.items() if k.startswith("burst_")}
    nt = {k: v for k, v in th.items() if k.startswith("nt_")}
    sig = eng.generate_per_signal(R, r0=3, theta=th)
    burst, trans = sig["burst"], sig["transient"]
    assert "cw" not in sig and "bwm" not in sig and float(burst.abs().max()) > 0 and float(trans.abs().max()) > 0
    total = eng.generate(R, r0=3, theta=th)
    assert torch.equal(total, sig["total"]) and torch.equal(total, (base + burst) + trans)
    assert torch.equal(eng.generate(R, r0=3, theta=bt), base + burst) and torch.equal(eng.generate(R, r0=3, theta=nt), base + trans)
    assert torch.equal(eng.generate_per_signal(R, r0=3, theta=nt)["transient"], trans)
    # chunks and row slots: a realisation's terms are the same bits
    part = eng.generate_per_signal(5, r0=3 + 7, theta={k: v[7:12] for k, v in th.items()})
    assert torch.equal(part["burst"], burst[7:12]) and torch.equal(part["transient"], trans[7:12])
    ws = eng.workspace_bytes
    eng.workspace_bytes = 1          # the smallest batches: the term batch by batch in other row slots
    small = eng.generate(R, r0=3, theta=th)
    eng.workspace_bytes = ws
    assert torch.equal(small, total)
    # with hyper keys and as torch tensors
    hyper = {"gwb_log10_A": np.full(R, -14.1)}
    hbase = eng.generate(R, r0=3, theta=hyper).clone()
    mixed = dict(th, **hyper, burst_psi=torch.as_tensor(th["burst_psi"]), nt_psr=torch.as_tensor(th["nt_psr"]))
    assert torch.equal(eng.generate(R, r0=3, theta=mixed), (hbase + burst) + trans)
    # with a CW source and a burst with memory in the same realisation: CW, BWM, burst, transients
    eng.set_cw(tref=53000 * 86400.0).set_bwm()
    cw, bwm = theta_of(corner_sources(R, seed=6), True), _bwm_theta(R)
    both = eng.generate_per_signal(R, r0=3, theta=dict(th, **cw, **bwm))
    assert torch.equal(both["burst"], burst) and torch.equal(both["transient"], trans)
    assert torch.equal(both["total"], (((base + both["cw"]) + both["bwm"]) + burst) + trans)
    # TD mode: deterministic keys only
    td = eng.generate_td(R, r0=3).clone()
    assert _sum_close(eng.generate_td(R, r0=3, theta=bt), td, burst)
    assert torch.equal(eng.generate_td(R, r0=3, theta=dict(th, **cw, **bwm)), (((td + both["cw"]) + both["bwm"]) + burst) + trans)
    # remove_quad composes the same way
    eng.set_burst(W, remove_quad=True)
    q = eng.generate_per_signal(R, r0=3, theta=bt)
    assert not torch.equal(q["burst"], burst) and torch.equal(q["total"], base + q["burst"])
    assert torch.equal(eng.generate_per_signal(4, r0=3 + 9, theta={k: v[9:13] for k, v in bt.items()})["burst"], q["burst"][9:13])


def test_generate_f_statistic_takes_the_terms():
    """the generation step of a statistic: the same rows as generate(theta), whatever the chunk"""
    from test_gpu_fstat import SKY
    R = 9
    eng = _engine().set_burst(2).set_transients(2)
    eng.prepare_f_statistic(np.array([3e-9, 2e-8]), sky=SKY)
    th = _theta(R, 2, 2, eng.P, counts=True)
    ref = eng.f_statistic(eng.generate(R, r0=2, theta=th))
    for chunk in (4, R):
        got = eng.generate_f_statistic(R, r0=2, theta=th, chunk=chunk)
        assert torch.equal(got["fp"], ref["fp"]) and torch.equal(got["fe"], ref["fe"])
    ref_td = eng.f_statistic(eng.generate_td(R, r0=2, theta=th))
    assert torch.equal(eng.generate_f_statistic(R, r0=2, theta=th, chunk=4, td=True)["fp"], ref_td["fp"])


def test_sampled_labels():
    from pta_replicator_amd import _burst
    R, W, V = 40, 3, 4
    boxes = dict(t0_mjd=(54000.0, 56500.0), log10_tau=(7.0, 7.8), log10_f=(-8.5, -7.5), log10_a_plus=(-8.0, -7.0), log10_a_cross=(-8.5, -7.0))
    nboxes = dict(t0_mjd=(53500.0, 57000.0), log10_tau=(6.5, 7.5), log10_f=(-8.0, -7.0), log10_a=(-7.0, -6.0), phase=(0.0, 1.0))
    eng = _engine().set_burst(W).set_transients(V)
    eng.set_burst_prior(**boxes).set_transient_prior(**nboxes)
    rows, th = eng.generate_sampled(R, r0=4)
    assert set(th) == set(_burst.KEYS) | set(_burst.NT_KEYS)
    lim = {"burst_" + k: v for k, v in boxes.items()}
    lim.update({"burst_cos_gwtheta": (-1, 1), "burst_gwphi": (0, 2 * np.pi), "burst_psi": (0, np.pi), "burst_phase_plus": (0, 2 * np.pi),
                "burst_phase_cross": (0, 2 * np.pi)})
    lim.update({"nt_" + k: v for k, v in nboxes.items()})
    for k, (lo, hi) in lim.items():
        v = th[k].cpu().numpy()
        want = (R,) if k in _burst.SKY_KEYS else (R, W) if k.startswith("burst_") else (R, V)
        assert v.shape == want and np.all(v >= lo) and np.all(v <= hi) and v.std() > 0, k
    psr = th["nt_psr"]
    assert psr.dtype == torch.int32 and psr.shape == (R, V) and int(psr.min()) >= 0 and int(psr.max()) <= eng.P - 1
    assert len(torch.unique(psr)) == eng.P
    # the rows are generate(theta = the labels); labels are a pure function of (seed, r): r0 offsets and chunks are bit-equal
    assert torch.equal(rows, eng.generate(R, r0=4, theta=th))
    th2 = eng.sample_theta(11, r0=4 + 9)
    rows2, th3 = eng.generate_sampled(11, r0=4 + 9)
    for k in th:
        assert torch.equal(th2[k], th[k][9:20]) and torch.equal(th3[k], th[k][9:20]), k
    assert torch.equal(rows2, rows[9:20])
    # the hyper, CW and BWM labels of the same seed do not move when the new priors are added
    other = _engine().set_cw().set_bwm()
    other.set_hyper_prior(gwb_log10_A=(-15, -14), rn_gamma=(2, 5))
    other.set_cw_prior(log10_mc=(8, 9.5), log10_fgw=(-8.7, -7.5), log10_h=(-15, -14))
    other.set_bwm_prior(log10_h=(-15.0, -13.5), t0_mjd=(54000.0, 56500.0))
    before = other.sample_theta(R, r0=4)
    rows_before = other.generate_sampled(R, r0=4)[0].clone()
    other.set_burst(W).set_transients(V).set_burst_prior(**boxes).set_transient_prior(**nboxes)
    after = other.sample_theta(R, r0=4)
    assert set(after) == set(before) | set(th)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    for k in th:
        assert torch.equal(after[k], th[k]), k                          # the same seed: the same labels, whatever else is sampled
    rows_after, _ = other.generate_sampled(R, r0=4)
    sig = other.generate_per_signal(R, r0=4, theta=after)
    assert torch.equal(rows_after, sig["total"]) and _sum_close(rows_after, rows_before + sig["burst"], sig["transient"])
