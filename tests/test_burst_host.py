"""CPU checks of the per-realisation sine-Gaussian wavelets (set_burst / set_transients): the __host__ __device__ formulas of
csrc/pta_burst.h compiled with g++ (tests/burst/burst_host.cpp) against the reference's golden add_burst / add_noise_transient output
and a long-double evaluation of the expression, the label draw maps against philox_ref, the list-API twins against the golden, and
the validation of the configuration, the priors and theta on an engine that is configured but not prepared (no GPU needed: every
refusal happens before anything is launched)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from helpers import load, mjd_ld
from oracle import philox_ref
from test_bwm_host import _golden_pulsars, _p, _relrms

HERE = os.path.dirname(os.path.abspath(__file__))
LD = np.longdouble
# the golden burst (oracle/gen_golden.py: add_burst(p, 1.1, 4.0, burst_plus, burst_cross, psi=0.4, tref=53000 * 86400), one wavelet at
# tref + 2.2e8 s with tau = 4e7 s, f = 3e-8 Hz, A+ = 2e-7 s (a cosine), Ax = 1.3e-7 s (a sine: phase -pi/2))
GWTHETA, GWPHI, PSI = 1.1, 4.0, 0.4
SKY = np.array([np.cos(GWTHETA), GWPHI, PSI])
WAVELET = {"t0_mjd": 53000 + 2.2e8 / 86400, "log10_tau": np.log10(4e7), "log10_f": np.log10(3e-8), "log10_a_plus": np.log10(2e-7),
           "phase_plus": 0.0, "log10_a_cross": np.log10(1.3e-7), "phase_cross": -np.pi / 2}


@pytest.fixture(scope="module")
def bu(tmp_path_factory):
    out = tmp_path_factory.mktemp("burst") / "libbursthost.so"
    src = os.path.join(HERE, "burst", "burst_host.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", str(out)])
    lib = ctypes.CDLL(str(out))
    d, i, u64, p = ctypes.c_double, ctypes.c_int, ctypes.c_uint64, ctypes.POINTER(ctypes.c_double)
    lib.bu_uniform.argtypes = [u64, u64, i, i, p, p, p, p]
    lib.bu_nt_uniform.argtypes = [u64, u64, i, i, i, p, p, p]
    lib.bu_burst_tables.argtypes = [p, p, i, p, i, p, p]
    lib.bu_burst_term.argtypes = [p, i, d, d, p, i, p]
    lib.bu_nt_tables.argtypes = [p, i, p]
    lib.bu_nt_term.argtypes = [p, i, i, p, i, p]
    lib.bu_arg_zero.restype = d
    return lib


def _src(wavelets):
    from pta_replicator_amd import _burst
    return np.ascontiguousarray([[w[c] for c in _burst.WAV_COLUMNS] for w in wavelets], dtype=np.float64)


def burst_tables(bu, sky, wavelets, phats):
    """(wav [W, 7], kk [P, 2]) of the host twin"""
    src, phat = _src(wavelets), np.ascontiguousarray(phats, dtype=np.float64)
    W, P = len(src), len(phat)
    wav, kk = np.full((W, 7), np.nan), np.full((P, 2), np.nan)
    bu.bu_burst_tables(_p(np.ascontiguousarray(sky, dtype=np.float64)), _p(src), W, _p(phat), P, _p(wav), _p(kk))
    return wav, kk


def burst_term(bu, wav, kk_a, toa_s):
    out = np.full(len(toa_s), np.nan)
    bu.bu_burst_term(_p(np.ascontiguousarray(wav)), len(wav), float(kk_a[0]), float(kk_a[1]), _p(np.ascontiguousarray(toa_s)), len(toa_s), _p(out))
    return out


def fold(wav, kk_a):
    """(C, S) [W] as pta_burst_fold forms them (float64, no contraction)"""
    return kk_a[0] * wav[:, 3] + kk_a[1] * wav[:, 5], -(kk_a[0] * wav[:, 4] + kk_a[1] * wav[:, 6])


def term_ld(t0_s, nh, f, C, S, toa_s):
    """(ref, bound) in long double from float64 table columns [W]: ref = sum_w g_w (C_w cos 2 pi u_w + S_w sin 2 pi u_w), and the
    per-element rounding bound 2^-52 sum_w g_w (|C_w| + |S_w|) (16 + 4 |arg_w| + 4 pi |u_w|): 4.5 ulp for sin / cos (pta_rng.h), ~2 ulp
    for exp, the products and the sums, the roundings of the exponent's argument scaled by |arg| and the phase rounding by 2 pi |u|"""
    t = np.asarray(toa_s, dtype=LD)[None, :]
    t0_s, nh, f, C, S = (np.asarray(x, dtype=LD)[:, None] for x in (t0_s, nh, f, C, S))
    dt = t - t0_s
    arg, u = nh * dt * dt, f * dt
    g = np.exp(arg)
    pi = np.arctan(LD(1)) * 4
    ph = 2 * pi * (u - np.floor(u))
    ref = np.sum(g * (C * np.cos(ph) + S * np.sin(ph)), axis=0)
    bound = LD(2) ** -52 * np.sum(g * (abs(C) + abs(S)) * (16 + 4 * abs(arg) + 4 * pi * abs(u)), axis=0)
    return ref, bound


def reference_ld(toa_s, ra, dec, gwtheta, gwphi, psi, wavelets):
    """the reference's own expression (deterministic.py:732-776) in long double with the wavelet callables; a wavelet's epoch is
    t0_mjd * 86400 rounded to float64 seconds (the parameter the device holds, as add_gw_memory rounds its epoch)"""
    gwtheta, gwphi, psi = LD(gwtheta), LD(gwphi), LD(psi)
    ct, cp, st, sp = np.cos(gwtheta), np.cos(gwphi), np.sin(gwtheta), np.sin(gwphi)
    m = np.array([sp, -cp, LD(0)])
    n = np.array([-ct * cp, -ct * sp, st])
    om = np.array([-st * cp, -st * sp, -ct])
    pi = np.arctan(LD(1)) * 4
    ptheta, pphi = pi / 2 - LD(dec), LD(ra)
    phat = np.array([np.sin(ptheta) * np.cos(pphi), np.sin(ptheta) * np.sin(pphi), np.cos(ptheta)])
    fplus = LD(0.5) * (np.dot(m, phat) ** 2 - np.dot(n, phat) ** 2) / (1 + np.dot(om, phat))
    fcross = (np.dot(m, phat) * np.dot(n, phat)) / (1 + np.dot(om, phat))
    t = np.asarray(toa_s, dtype=LD)
    hp, hc = np.zeros_like(t), np.zeros_like(t)
    for w in wavelets:
        dt = t - LD(np.float64(w["t0_mjd"]) * 86400.0)
        g = np.exp(-LD(0.5) * (dt / LD(10) ** LD(w["log10_tau"])) ** 2)
        u = LD(10) ** LD(w["log10_f"]) * dt
        u = u - np.floor(u)
        hp = hp + LD(10) ** LD(w["log10_a_plus"]) * g * np.cos(2 * pi * u + LD(w["phase_plus"]))
        hc = hc + LD(10) ** LD(w["log10_a_cross"]) * g * np.cos(2 * pi * u + LD(w["phase_cross"]))
    c2, s2 = np.cos(2 * psi), np.sin(2 * psi)
    return -fplus * (hp * c2 - hc * s2) - fcross * (hp * s2 + hc * c2)


def test_stream_kinds_and_columns(bu):
    from pta_replicator_amd import _burst
    assert (_burst.STREAM_BURST, _burst.STREAM_NT) == (13, 14) == (bu.bu_stream_burst(), bu.bu_stream_nt())
    assert _burst.SKY_KEYS == ("burst_cos_gwtheta", "burst_gwphi", "burst_psi")
    assert _burst.WAV_KEYS == ("burst_t0_mjd", "burst_log10_tau", "burst_log10_f", "burst_log10_a_plus", "burst_phase_plus",
                               "burst_log10_a_cross", "burst_phase_cross")
    assert _burst.NT_KEYS == ("nt_psr", "nt_t0_mjd", "nt_log10_tau", "nt_log10_f", "nt_log10_a", "nt_phase")
    # below the skip threshold exp is exactly 0 in float64, and 38.7 tau lies below it
    assert np.exp(bu.bu_arg_zero()) == 0.0 and -0.5 * 38.7 ** 2 < bu.bu_arg_zero()


def test_golden_burst_and_long_double_reference(bu):
    """the header's tables and term against the unmodified reference's add_burst rows (1e-10 relative RMS per pulsar, the project's
    parity bound), with the quadratic removed through _burst.quad_basis as the device removes it, and against a long-double
    evaluation of the reference's expression to the per-element rounding bound"""
    from pta_replicator_amd import _burst
    z, psrs = _golden_pulsars()
    wav, kk = burst_tables(bu, SKY, [WAVELET], [p[1] for p in psrs])
    Q = _burst.quad_basis([p[0] for p in psrs])
    off = 0
    for a, (toa, phat, ra, dec) in enumerate(psrs):
        term = burst_term(bu, wav, kk[a], toa)
        err = _relrms(term, z["burst"][a])
        q = Q[off:off + len(toa)]
        off += len(toa)
        quad = term - q @ (q.T @ term)
        err_q = _relrms(quad, z["burst_quad"][a])
        print(f"pulsar {a}: relative RMS deviation from the golden burst {err:.3g}, burst_quad {err_q:.3g}")
        assert err <= 1e-10 and err_q <= 1e-10, (a, err, err_q)
        assert np.max(np.abs(q.T @ quad)) <= 64 * 2.0 ** -52 * np.sum(np.abs(term))
        # the reference's own expression in long double: within the rounding bound of the folded form
        ref = reference_ld(toa, ra, dec, GWTHETA, GWPHI, PSI, [WAVELET])
        C, S = fold(wav, kk[a])
        _, bound = term_ld(wav[:, 0], wav[:, 1], wav[:, 2], C, S, toa)
        worst = float(np.max(np.abs(term - ref) / bound))
        print(f"pulsar {a}: worst deviation from the long-double reference, in units of the bound: {worst:.3g}")
        assert np.all(np.abs(term - ref) <= bound), (a, worst)


def test_golden_noise_transient(bu):
    """the plus wavelet alone, one transient in every pulsar, against the reference's add_noise_transient rows"""
    z, psrs = _golden_pulsars()
    src = np.array([[a, WAVELET["t0_mjd"], WAVELET["log10_tau"], WAVELET["log10_f"], WAVELET["log10_a_plus"], 0.0] for a in range(3)])
    tab = np.full((3, 6), np.nan)
    bu.bu_nt_tables(_p(src), 3, _p(tab))
    assert np.array_equal(tab[:, 0], [0, 1, 2]) and np.all(tab[:, 1] == np.float64(WAVELET["t0_mjd"]) * 86400.0)
    for a, (toa, _, _, _) in enumerate(psrs):
        out = np.full(len(toa), np.nan)
        bu.bu_nt_term(_p(tab), 3, a, _p(np.ascontiguousarray(toa)), len(toa), _p(out))
        err = _relrms(out, z["noise_transient"][a])
        print(f"pulsar {a}: relative RMS deviation from the golden noise transient {err:.3g}")
        assert err <= 1e-10, (a, err)
        ref, bound = term_ld(tab[a:a + 1, 1], tab[a:a + 1, 2], tab[a:a + 1, 3], tab[a:a + 1, 4], tab[a:a + 1, 5], toa)
        assert np.all(np.abs(out - ref) <= bound), a


def test_per_element_rounding_bound(bu):
    """the term of the header against long double from the same table rows, element by element, on random wavelets and on the two
    stress cases: a wavelet 30 tau away from every TOA (|arg| = 450 and more) and f = 1e-6 Hz seen from the far end of the span
    (|u| of a few hundred turns)"""
    _, psrs = _golden_pulsars()
    rng = np.random.default_rng(11)
    span = (min(p[0].min() for p in psrs) / 86400, max(p[0].max() for p in psrs) / 86400)

    def wavelet(t0_mjd, tau, f):
        return {"t0_mjd": t0_mjd, "log10_tau": np.log10(tau), "log10_f": np.log10(f), "log10_a_plus": rng.uniform(-8, -6),
                "phase_plus": rng.uniform(0, 2 * np.pi), "log10_a_cross": rng.uniform(-8, -6), "phase_cross": rng.uniform(0, 2 * np.pi)}
    cases = [[wavelet(rng.uniform(*span), 10 ** rng.uniform(7.2, 8.0), 10 ** rng.uniform(-8.5, -7)) for _ in range(5)] for _ in range(6)]
    tau = (span[1] - span[0]) * 86400 / 6.5     # 30 tau before the first TOA, 36.5 tau before the last: arg from -450 to -666, still normal
    cases.append([wavelet(span[0] - 30 * tau / 86400, tau, 2e-8)])                     # 30 tau before the first TOA
    cases.append([wavelet(span[0], 3e8, 1e-6)])                                         # hundreds of turns at the far end
    cases.append([wavelet(span[0] - 30 * tau / 86400, tau, 1e-6), wavelet(span[1], 2e8, 1e-6), wavelet(0.5 * (span[0] + span[1]), 3e7, 1e-8)])
    worst = 0.0
    for k, ws in enumerate(cases):
        sky = np.array([rng.uniform(-1, 1), rng.uniform(0, 2 * np.pi), rng.uniform(0, np.pi)])
        wav, kk = burst_tables(bu, sky, ws, [p[1] for p in psrs])
        for a, (toa, _, _, _) in enumerate(psrs):
            got = burst_term(bu, wav, kk[a], toa)
            C, S = fold(wav, kk[a])
            ref, bound = term_ld(wav[:, 0], wav[:, 1], wav[:, 2], C, S, toa)
            assert np.all(np.isfinite(got)) and np.all(bound > 0)
            worst = max(worst, float(np.max(np.abs(got - ref) / bound)))
            assert np.all(np.abs(got - ref) <= bound), (k, a, float(np.max(np.abs(got - ref) / bound)))
    t0 = (cases[6][0]["t0_mjd"]) * 86400.0
    assert np.min(np.abs(psrs[0][0] - t0)) >= 29.9 * tau and abs(1e-6 * (psrs[0][0].max() - span[0] * 86400)) > 100
    print(f"worst deviation from long double in units of the bound: {worst:.3g}")
    # 40 tau away the envelope is exactly 0
    tau = 1.0e6
    wav, kk = burst_tables(bu, SKY, [wavelet(span[0] - 40 * tau / 86400, tau, 2e-8)], [psrs[0][1]])
    assert np.array_equal(burst_term(bu, wav, kk[0], psrs[0][0]), np.zeros(len(psrs[0][0])))


def test_uniform_maps_match_philox_ref(bu):
    """sky column j = pair j of stream (13, 0), column j of wavelet w = pair j of stream (13, 1 + w), column j of transient v = pair j
    of stream (14, v): the uniforms bit-equal to philox_ref's, the labels inside their boxes, nt_psr the floor of the U(0, P) draw"""
    from pta_replicator_amd import _burst
    from pta_replicator_amd.engine import stream_id
    seed, r0, R, W, V, P = 0x0123456789ABCDEF, 77, 5, 3, 4, 7
    sky, wav = np.zeros((R, 3)), np.zeros((R, W, 7))
    bu.bu_uniform(seed, r0, R, W, _p(np.zeros(10)), _p(np.ones(10)), _p(sky), _p(wav))
    nt = np.zeros((R, V, 6))
    lo1, hi1 = np.zeros(6), np.ones(6)
    lo1[0], hi1[0] = 0.25, 0.75     # (a unit box's floor would be 0 everywhere: columns 1 .. 5 carry the uniforms, column 0 below)
    bu.bu_nt_uniform(seed, r0, R, V, P, _p(lo1), _p(hi1), _p(nt))
    prior = _burst.make_prior(t0_mjd=(54000, 56000), log10_tau=(6.5, 7.5), log10_f=(-8, -8), log10_a_plus=(-8, -7), log10_a_cross=(-9, -7))
    lo, hi = _burst.prior_bounds(prior)
    assert lo[0] == -1 and hi[0] == 1 and hi[1] == 2 * np.pi and hi[2] == np.pi and (lo[3], hi[3]) == (54000, 56000) and hi[7] == 2 * np.pi
    sky2, wav2 = np.zeros((R, 3)), np.zeros((R, W, 7))
    bu.bu_uniform(seed, r0, R, W, _p(lo), _p(hi), _p(sky2), _p(wav2))
    nprior = _burst.make_nt_prior(t0_mjd=(54000, 56000), log10_tau=(6, 7), log10_f=(-8.5, -7), log10_a=(-7.5, -6.5))
    nlo, nhi = _burst.nt_prior_bounds(nprior, P)
    assert (nlo[0], nhi[0]) == (0, P) and (nlo[5], nhi[5]) == (0, 2 * np.pi)
    nt2 = np.zeros((R, V, 6))
    bu.bu_nt_uniform(seed, r0, R, V, P, _p(nlo), _p(nhi), _p(nt2))
    for r in range(R):
        _, u2 = philox_ref.uniform_pairs(seed, r0 + r, stream_id(_burst.STREAM_BURST, 0), 3)
        u2 = np.asarray(u2, dtype=np.float64)
        assert np.array_equal(sky[r], u2), r                                      # fma(1, u2, 0) = u2
        ref = lo[:3] + (hi[:3] - lo[:3]) * u2
        assert np.all(np.abs(sky2[r] - ref) <= np.spacing(np.abs(ref))) and np.all(sky2[r] >= lo[:3]) and np.all(sky2[r] <= hi[:3])
        for w in range(W):
            _, u2 = philox_ref.uniform_pairs(seed, r0 + r, stream_id(_burst.STREAM_BURST, 1 + w), 7)
            u2 = np.asarray(u2, dtype=np.float64)
            assert np.array_equal(wav[r, w], u2), (r, w)
            ref = lo[3:] + (hi[3:] - lo[3:]) * u2
            assert np.all(np.abs(wav2[r, w] - ref) <= np.spacing(np.abs(ref))) and np.all(wav2[r, w] >= lo[3:]) and np.all(wav2[r, w] <= hi[3:])
            assert wav2[r, w, 2] == -8.0                                          # a degenerate box gives its value
        for v in range(V):
            _, u2 = philox_ref.uniform_pairs(seed, r0 + r, stream_id(_burst.STREAM_NT, v), 6)
            u2 = np.asarray(u2, dtype=np.float64)
            assert np.array_equal(nt[r, v, 1:], u2[1:]) and nt[r, v, 0] == 0.0, (r, v)
            assert nt2[r, v, 0] == min(np.floor(P * u2[0]), P - 1) and 0 <= nt2[r, v, 0] <= P - 1
            ref = nlo[1:] + (nhi[1:] - nlo[1:]) * u2[1:]
            assert np.all(np.abs(nt2[r, v, 1:] - ref) <= np.spacing(np.abs(ref)))
    assert len(np.unique(nt2[:, :, 0])) > 2


# ---------------------------------------------------------------- the list-API twins ------------------------------------------------
def test_list_api_twins_match_the_golden():
    """add_wavelet_burst / add_wavelet_transient against transients.npz at 1e-12, as test_host_logic.py holds add_burst"""
    from pta_replicator_amd.deterministic import add_wavelet_burst, add_wavelet_transient
    from pta_replicator_amd.simulate import ArrayTOAs, SimulatedPulsar, make_ideal
    z = load("transients.npz")

    def fresh():
        out = []
        for i in range(3):
            p = SimulatedPulsar(toas=ArrayTOAs(mjd_ld(z, "", i), z[f"err_us_{i}"]), name=str(z["names"][i]),
                                loc={"RAJ": float(z["raj_hours"][i]), "DECJ": float(z["decj_deg"][i])})
            make_ideal(p)
            out.append(p)
        return out

    def sig(p, key):
        return np.asarray(p.added_signals_time[f"{p.name}_{key}"].value, dtype=np.float64)
    for case, rq in (("burst", False), ("burst_quad", True)):
        for a, p in enumerate(fresh()):
            add_wavelet_burst(p, GWTHETA, GWPHI, [WAVELET], psi=PSI, remove_quad=rq)
            err = _relrms(sig(p, "burst"), z[case][a])
            print(f"{case} pulsar {a}: {err:.3g}")
            assert err < 1e-12, (case, a, err)
    for a, p in enumerate(fresh()):
        add_wavelet_transient(p, [{"t0_mjd": WAVELET["t0_mjd"], "log10_tau": WAVELET["log10_tau"], "log10_f": WAVELET["log10_f"],
                                   "log10_a": WAVELET["log10_a_plus"], "phase": 0.0}])
        err = _relrms(sig(p, "noise_transient"), z["noise_transient"][a])
        assert err < 1e-12, (a, err)


# ---------------------------------------------------------------- validation (no GPU) -------------------------------
def _engine(burst=2, nt=3):
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
    eng.set_red_noise([-14.0, None, -13.5, -14.2], [3.0, None, 2.5, 4.0], components=10)
    eng.set_gwb(-14.5, 13. / 3.)
    if burst:
        assert eng.set_burst(n_wavelets=burst) is eng
    if nt:
        assert eng.set_transients(n=nt) is eng
    return eng


def _burst_theta(R, W):
    th = {"burst_cos_gwtheta": np.linspace(-1, 1, R), "burst_gwphi": np.full(R, 1.0), "burst_psi": np.full(R, 0.5)}
    th.update({"burst_t0_mjd": np.full((R, W), 55000.0), "burst_log10_tau": np.full((R, W), 7.0), "burst_log10_f": np.full((R, W), -8.0),
               "burst_log10_a_plus": np.full((R, W), -7.0), "burst_phase_plus": np.zeros((R, W)),
               "burst_log10_a_cross": np.full((R, W), -7.0), "burst_phase_cross": np.zeros((R, W))})
    return th


def _nt_theta(R, V):
    return {"nt_psr": np.zeros((R, V), dtype=np.int64), "nt_t0_mjd": np.full((R, V), 55000.0), "nt_log10_tau": np.full((R, V), 6.5),
            "nt_log10_f": np.full((R, V), -7.5), "nt_log10_a": np.full((R, V), -6.5), "nt_phase": np.zeros((R, V))}


def test_theta_refusals_before_any_launch():
    import torch
    R, W, V = 3, 2, 3
    eng = _engine(W, V)
    ok, nok = _burst_theta(R, W), _nt_theta(R, V)
    nan_w = np.full((R, W), 7.0)
    nan_w[1, 1] = np.nan
    cases = [
        ({k: v for k, v in ok.items() if k != "burst_gwphi"}, "burst_gwphi"),
        ({"burst_t0_mjd": ok["burst_t0_mjd"]}, "missing"),
        ({"burst_count": np.ones(R, dtype=np.int64)}, "missing"),
        (dict(ok, burst_psi=np.zeros(R + 1)), "shape"),
        (dict(ok, burst_t0_mjd=np.zeros(R)), "shape"),
        (dict(ok, burst_log10_f=np.zeros((R, W + 1))), "shape"),
        (dict(ok, burst_phase_plus=torch.zeros((R + 1, W), dtype=torch.float64)), "shape"),
        (dict(ok, burst_cos_gwtheta=np.array([0.0, 1.5, 0.0])), r"\|cos\|"),
        (dict(ok, burst_cos_gwtheta=np.array([0.0, -1.0000001, 0.0])), r"\|cos\|"),
        (dict(ok, burst_log10_tau=nan_w), "non-finite"),
        (dict(ok, burst_gwphi=torch.tensor([0.0, float("inf"), 0.0], dtype=torch.float64)), "non-finite"),
        (dict(ok, burst_count=np.array([0, W + 1, 1])), "counts must lie in 0 .. 2"),
        (dict(ok, burst_count=np.array([0, -1, 1])), "counts must lie"),
        (dict(ok, burst_count=np.array([0.0, 1.0, 1.0])), "integer"),
        (dict(ok, burst_count=np.array([0, 1])), "shape"),
        ({k: v for k, v in nok.items() if k != "nt_phase"}, "nt_phase"),
        (dict(nok, nt_psr=np.zeros((R, V + 1), dtype=np.int64)), "shape"),
        (dict(nok, nt_psr=np.full((R, V), 4)), r"0 \.\. P-1 = 3"),
        (dict(nok, nt_psr=np.full((R, V), -1)), r"0 \.\. P-1"),
        (dict(nok, nt_psr=np.full((R, V), 1.5)), r"0 \.\. P-1"),
        (dict(nok, nt_log10_a=np.full((R, V), np.nan)), "non-finite"),
        (dict(nok, nt_count=np.array([0, V + 1, 1])), "counts must lie in 0 .. 3"),
        (dict(ok, **dict(nok, nt_t0_mjd=np.full((R, V), np.inf))), "non-finite"),
    ]
    for theta, msg in cases:
        for call in (eng.generate, eng.generate_per_signal, eng.generate_td):
            with pytest.raises(ValueError, match=msg):
                call(R, theta=theta)
    # a value past the count is never read: NaN there is accepted by the validation
    hyper, det = eng._theta_parts(dict(ok, burst_log10_tau=nan_w, burst_count=np.array([2, 1, 0])), R)
    assert hyper is None and "burst_count" in det
    with pytest.raises(ValueError, match=r"no per-realisation wavelet burst configured \(set_burst\)"):
        _engine(burst=0).generate(R, theta=ok)
    with pytest.raises(ValueError, match=r"no per-realisation noise transients configured \(set_transients\)"):
        _engine(nt=0).generate(R, theta=nok)
    for extra in ({"rn_gamma": np.full((R, 4), 3.0)}, {"gwb_log10_A": np.full(R, -14.0)}):
        with pytest.raises(ValueError, match="TD mode"):
            eng.generate_td(R, theta=dict(ok, **extra))
    assert not eng._prepared


def test_theta_parts_carries_the_new_keys_in_the_second_member():
    from pta_replicator_amd import _burst, _bwm, _cw
    R, W, V = 3, 2, 3
    eng = _engine(W, V)
    th = dict(_burst_theta(R, W), **_nt_theta(R, V))
    hyper, det = eng._theta_parts(th, R)
    assert hyper is None and set(det) == set(_burst.KEYS) | set(_burst.NT_KEYS)
    assert _burst.has_keys(det) and _burst.has_nt_keys(det) and not _cw.has_keys(det) and not _bwm.has_keys(det)
    hyper, det = eng._theta_parts(dict(_nt_theta(R, V), gwb_log10_A=np.full(R, -14.0)), R)
    assert set(hyper) == {"gwb_log10_A"} and _burst.has_nt_keys(det) and not _burst.has_keys(det)
    hyper, det = eng._theta_parts(th, R, td=True)
    assert hyper is None and _burst.has_keys(det) and _burst.has_nt_keys(det)
    assert not eng._prepared


def test_configuration_and_prior_validation():
    eng = _engine(burst=0, nt=0)
    for bad in (0, 129, -1, 2.5, True):
        with pytest.raises(ValueError, match=r"1 \.\. 128"):
            eng.set_burst(n_wavelets=bad)
        with pytest.raises(ValueError, match=r"1 \.\. 128"):
            eng.set_transients(n=bad)
    assert eng._burst is None and eng._nt is None
    assert eng.set_burst(128, remove_quad=True)._burst == {"W": 128, "remove_quad": True} and eng.set_transients(128)._nt == {"V": 128}
    req = dict(t0_mjd=(54000, 56000), log10_tau=(6.5, 7.5), log10_f=(-8.5, -7.5), log10_a_plus=(-8, -7), log10_a_cross=(-8, -7))
    for k in req:
        with pytest.raises(ValueError, match=f"{k} is required"):
            eng.set_burst_prior(**{j: v for j, v in req.items() if j != k})
    nreq = dict(t0_mjd=(54000, 56000), log10_tau=(6, 7), log10_f=(-8.5, -7), log10_a=(-7.5, -6.5))
    for k in nreq:
        with pytest.raises(ValueError, match=f"{k} is required"):
            eng.set_transient_prior(**{j: v for j, v in nreq.items() if j != k})
    with pytest.raises(ValueError, match="lo <= hi"):
        eng.set_burst_prior(**dict(req, log10_tau=(7.5, 6.5)))
    with pytest.raises(ValueError, match="lo <= hi"):
        eng.set_burst_prior(**dict(req, phase_plus=(0, np.inf)))
    with pytest.raises(ValueError, match="lo <= hi"):
        eng.set_transient_prior(**dict(nreq, log10_a=(-6, -7)))
    with pytest.raises(ValueError, match=r"\[-1, 1\]"):
        eng.set_burst_prior(**dict(req, cos_gwtheta=(-2, 1)))
    with pytest.raises(ValueError, match=r"\(lo, hi\)"):
        eng.set_transient_prior(**dict(nreq, phase=(0, 1, 2)))
    with pytest.raises(ValueError, match="no prior"):
        _engine(burst=0, nt=0).generate_sampled(2)
    plain = _engine(burst=0, nt=0)
    assert plain.set_burst_prior(**req) is plain
    with pytest.raises(ValueError, match=r"set_burst"):
        plain.generate_sampled(2)
    plain = _engine(burst=0, nt=0)
    assert plain.set_transient_prior(**nreq) is plain
    with pytest.raises(ValueError, match=r"set_transients"):
        plain.generate_sampled(2)
    assert not eng._prepared and not plain._prepared
