"""NumPy reference of the chromatic Gaussian process (not product code): weights, basis, prior, the term from given deviates, and the
deviates themselves from the NumPy twin of the device's draws (oracle/philox_ref.py) on stream (10, pulsar).  No number in it comes
from the device, and nothing is imported from the package under test.

    dt_i = (nu_ref / nu_i)^chi sum_k F_ik sqrt(phi_k) z_k
    F[:, 2k] = sin(2 pi f_k t), F[:, 2k + 1] = cos(2 pi f_k t), f_k = (k + 1) / Tspan, t = TDB seconds
    phi = A^2 (f / f_yr)^-gamma / (12 pi^2 Tspan) yr^3
"""
import numpy as np

STREAM_CHROM = 10
FIELD_LOG10_A, FIELD_GAMMA = 6, 7   # stream (7, field) of the prior boxes, pair = pulsar
YEAR = 365.25 * 86400.0


def weights(freqs_mhz, index=2.0, ref_freq_mhz=1400.0):
    return (ref_freq_mhz / np.asarray(freqs_mhz, dtype=np.float64)) ** index


def weights_longdouble(freqs_mhz, index=2.0, ref_freq_mhz=1400.0):
    """the same in extended precision: exp(chi log(nu_ref / nu))"""
    x = np.longdouble(ref_freq_mhz) / np.asarray(freqs_mhz, dtype=np.longdouble)
    return np.exp(np.longdouble(index) * np.log(x))


def frequencies(tdb_s, components):
    T = tdb_s.max() - tdb_s.min()
    return 1.0 * np.arange(1, components + 1) / T, T


def basis(tdb_s, components):
    """F [N, 2 components]"""
    f, _ = frequencies(tdb_s, components)
    arg = 2 * np.pi * tdb_s[:, None] * f[None, :]
    F = np.empty((len(tdb_s), 2 * components))
    F[:, 0::2], F[:, 1::2] = np.sin(arg), np.cos(arg)
    return F


def prior(tdb_s, components, log10_A, gamma):
    """phi [2 components]"""
    f, T = frequencies(tdb_s, components)
    freqs = np.repeat(f, 2)
    return (10 ** log10_A) ** 2 * (freqs * YEAR) ** (-gamma) / (12 * np.pi ** 2 * T) * YEAR ** 3


def term(tdb_s, freqs_mhz, components, log10_A, gamma, z, index=2.0, ref_freq_mhz=1400.0):
    """the delay [N] from the deviates z [2 components]; log10_A None = no process"""
    if log10_A is None or gamma is None:
        return np.zeros(len(tdb_s))
    y = np.sqrt(prior(tdb_s, components, log10_A, gamma)) * z
    return weights(freqs_mhz, index, ref_freq_mhz) * (basis(tdb_s, components) @ y)


def draws(seed, r, a, components, fast=False):
    """z [2 components] of pulsar a in realisation r: pair c >> 1, branch c & 1 of stream (10, a)"""
    from oracle import philox_ref as ph
    z = np.empty(2 * components)
    z[0::2], z[1::2] = ph.normal_pairs(seed, r, ph.stream_id(STREAM_CHROM, a), components, fast=fast)
    return z


def prior_labels(seed, r0, R, field, lo, hi):
    """[R, P] labels of a box draw: lo + (hi - lo) u (one fma), u = uniform u2 of pair = pulsar of stream (7, field)"""
    from oracle import philox_ref as ph
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    out = np.empty((R, len(lo)))
    for r in range(R):
        _, u2 = ph.uniform_pairs(seed, r0 + r, ph.stream_id(7, field), len(lo))
        out[r] = lo + (hi - lo) * np.asarray(u2)
    return out
