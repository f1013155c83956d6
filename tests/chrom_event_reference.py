"""What the chromatic-event tests share: the g++ host twin of csrc/pta_chrom_event.h (tests/chrom_event/chrom_event_host.cpp), a
long-double evaluation of the definition from the table rows with its per-element rounding bound, and the arrays the cases use.

The bound.  u = 2^-53, X = |ln A| + |chi lnu| + |envelope argument|.  The header evaluates a term of kinds 0 - 2 as s exp(e),
e = fma(x, y, b), b = fma(chi, lnu, ln A).  Against an exact evaluation from the same table row the exponent is off by
    |chi lnu| u           lnu rounded to fp64
    (|ln A| + |chi lnu|) u  the fma that forms b
    |arg| u               t - t0 (bump: 2 |arg| u, the difference is squared, plus |arg| u for the square's rounding)
    X u                   the fma that forms e
that is <= C X u with C = 3 (bump: 4), and the term by (C X + D) u |term|, D = 3: 2 u for an exp within one ulp, 1 u for the
second-order terms of exp(delta) - 1 at X <= 800.  A subnormal result carries the format's absolute spacing 2^-1074 instead of a relative
precision, so that is added; the relative bound is held to <= 1e-12 wherever the reference is a normal number.
Kind 3 is s exp(b) sin(2 pi fr): the amplitude as above with C = 2 and D = 3 plus one ulp for the product, and the sine is absolute:
the turns ((u - floor u) + ul) + turns carry two roundings of numbers below 2 (2 * 2 u turns = 8 pi u radians), the sine's polynomial and
its argument's product less than 2 ulp more: 16 u of the amplitude covers them.  Its bound cannot be relative to the term (the sine has
zeros); it is held to <= 1e-12 of the amplitude.
A sum of n terms adds (n - 1) u sum |term| for the accumulator's roundings."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LD = np.longdouble
U = LD(2) ** -53
C_EXP, C_BUMP, C_ANNUAL, D = 3, 4, 2, 3     # the counts above
SINE_ABS = 16
YEAR = 31557600
COUNTS = [1, 15, 17, 64, 65, 130, 301]       # the ragged array of tests/test_gpu_bwm.py


def _p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def build(tmp_dir):
    """the host twin, compiled into tmp_dir"""
    out = os.path.join(str(tmp_dir), "libchromeventhost.so")
    src = os.path.join(HERE, "chrom_event", "chrom_event_host.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", out])
    lib = ctypes.CDLL(out)
    d, i, u64, p = ctypes.c_double, ctypes.c_int, ctypes.c_uint64, ctypes.POINTER(ctypes.c_double)
    lib.ce_uniform.argtypes = [u64, u64, i, i, i, p, p, p]
    lib.ce_tables.argtypes = [p, i, p]
    lib.ce_term.argtypes = [p, i, i, p, p, i, p]
    lib.ce_arg_zero.restype = d
    return lib


def uniform(lib, seed, r0, R, E, P, lo, hi):
    out = np.full((R, E, 9), np.nan)
    lib.ce_uniform(seed, r0, R, E, P, _p(np.ascontiguousarray(lo, dtype=np.float64)), _p(np.ascontiguousarray(hi, dtype=np.float64)), _p(out))
    return out


def tables(lib, src):
    """tab [E, 10] of the host twin from label rows src [E, 9]"""
    src = np.ascontiguousarray(src, dtype=np.float64)
    tab = np.full((len(src), 10), np.nan)
    lib.ce_tables(_p(src), len(src), _p(tab))
    return tab


def term_host(lib, tab, a, toa_s, lnu):
    tab, toa_s, lnu = (np.ascontiguousarray(x, dtype=np.float64) for x in (tab, toa_s, lnu))
    out = np.full(len(toa_s), np.nan)
    lib.ce_term(_p(tab), len(tab), int(a), _p(toa_s), _p(lnu), len(toa_s), _p(out))
    return out


def src_rows(events):
    """label rows [E, 9] from dicts over _chrom_event.COLUMNS (the optional columns at their defaults)"""
    from pta_replicator_amd import _chrom_event as ce
    dflt = {"psr": 0, "t0_mjd": 0.0, "log10_tau": 0.0, "log10_tau_pre": np.nan, "sign": -1.0, "index": 2.0, "phase": 0.0}
    return np.array([[ce.kind_code(ev[c]) if c == "kind" else ev.get(c, dflt.get(c)) for c in ce.COLUMNS] for ev in events], dtype=np.float64)


def event_ld(row, toa_s, freqs_mhz, ref_freq_mhz=1400.0):
    """(ref, bound, X) [N] in long double of one table row (float64 [10]) at every TOA: the definition s A (nu_ref / nu)^chi shape(t) with
    A = exp(ln A) and the row's t0, 1 / tau, 1 / tau_pre, -1/2 / tau^2, phase in turns; X = 0 where the term is 0 by definition"""
    t, nu = np.asarray(toa_s, dtype=LD), np.asarray(freqs_mhz, dtype=LD)
    kind, t0, itau, ipre, nh, s, lna, chi, turns = int(row[1]), *(LD(x) for x in row[2:])
    lnu = np.log(LD(ref_freq_mhz) / nu)
    amp = np.exp(lna + chi * lnu)
    base = abs(lna) + abs(chi * lnu)
    if kind == 3:
        x = t / LD(YEAR)
        sn = np.sin(8 * np.arctan(LD(1)) * ((x - np.floor(x)) + turns))
        return s * amp * sn, amp * ((C_ANNUAL * base + D + 1) * abs(sn) + SINE_ABS) * U, base
    dt = t - t0
    if kind == 2:
        arg, live, c = nh * dt * dt, np.ones(len(t), dtype=bool), C_BUMP
    else:
        arg = np.where(dt >= 0, -dt * itau, dt * ipre)
        live, c = (dt >= 0) | (kind == 1), C_EXP
    ref = np.where(live, s * amp * np.exp(arg), LD(0))
    X = np.where(live, base + abs(arg), LD(0))
    return ref, np.where(live, (c * X + D) * U * abs(ref) + LD(2) ** -1074, LD(0)), X


def term_ld(tab, a, toa_s, freqs_mhz, ref_freq_mhz=1400.0):
    """(ref, bound) [N] of the sum over the rows of tab [E, 10] that live in pulsar a, in long double"""
    N = len(toa_s)
    ref, bound, mag, n = np.zeros(N, dtype=LD), np.zeros(N, dtype=LD), np.zeros(N, dtype=LD), 0
    for row in np.asarray(tab):
        if int(row[0]) != a:
            continue
        r, b, _ = event_ld(row, toa_s, freqs_mhz, ref_freq_mhz)
        ref, bound, mag, n = ref + r, bound + b, mag + abs(r), n + 1
    if n > 1:
        bound = bound + (n - 1) * U * (mag + bound)
    return ref, bound


def two_bands(rng, n):
    """radio frequencies [MHz] in two bands with scatter"""
    return np.where(rng.integers(0, 2, n) == 1, 1400.0, 820.0) + rng.uniform(-60, 60, n)


def ragged_pulsars(seed=5):
    """the pulsars of test_gpu_bwm's ragged array (COUNTS TOAs: odd offsets, a 301-TOA pulsar of two tiles), given two radio bands"""
    from pta_replicator_amd.simulate import ArrayTOAs, SimulatedPulsar, make_ideal
    rng, frng = np.random.default_rng(seed), np.random.default_rng(seed + 1)
    psrs = []
    for a, n in enumerate(COUNTS):
        p = SimulatedPulsar(toas=ArrayTOAs(np.sort(rng.uniform(53000, 57500, n)), 0.5, freqs_mhz=two_bands(frng, n)), name=f"J{a:04d}",
                            loc={"RAJ": float(rng.uniform(0, 24)), "DECJ": float(np.degrees(np.arcsin(rng.uniform(-1, 1))))})
        make_ideal(p)
        psrs.append(p)
    return psrs


def random_theta(R, E, P, seed=3, counts=False):
    """random ce_* keys of every kind; tau >= 3e6 s"""
    rng = np.random.default_rng(seed)
    th = {"ce_psr": rng.integers(0, P, (R, E)), "ce_kind": rng.integers(0, 4, (R, E)), "ce_t0_mjd": rng.uniform(53500, 57000, (R, E)),
          "ce_log10_tau": rng.uniform(6.5, 7.8, (R, E)), "ce_log10_tau_pre": np.where(rng.integers(0, 2, (R, E)) == 1, np.nan, rng.uniform(6.0, 7.0, (R, E))),
          "ce_log10_a": rng.uniform(-7.0, -5.5, (R, E)), "ce_sign": rng.choice([-1.0, 1.0, -0.3, 2.0], (R, E)), "ce_index": rng.uniform(0, 6.4, (R, E)),
          "ce_phase": rng.uniform(0, 2 * np.pi, (R, E))}
    if counts:
        th["ce_count"] = rng.integers(0, E + 1, R)
    return th
