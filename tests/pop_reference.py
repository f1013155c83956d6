"""NumPy twin of the population path (TEST INFRASTRUCTURE): the Poisson sampler of csrc/pta_pop.h on oracle.philox_ref, with the flag
that marks a draw whose decision sits within rounding of equality, and the loudest-k selection of pta_pop_draw_select.

A draw is BORDERLINE when one of its decisions has
    |u2 - cdf| <= 1e-12 cdf                           (inversion: the comparison u2 > cdf), or
    |lhs - rhs| <= 2^-40 max(1, k |log lambda|)       (PTRS: the log test),
the only places where exp / log / lgamma of another library can change the outcome: everything else the sampler does is IEEE +, *, /,
sqrt and floor in a fixed order, the same bits in NumPy, g++ -ffp-contract=off and on the device.
"""
import numpy as np
from scipy.special import gammaln

from oracle import philox_ref

STREAM_POP = 11
INVERSION_BELOW, NORMAL_FROM = 10.0, float(1 << 20)
INVERSION_STEPS, PTRS_ATTEMPTS = 255, 64
BORDER_INV, BORDER_PTRS = 1e-12, 2.0 ** -40


def uniforms(seed, rho, cell, attempt=0):
    """(u1 in (0, 1], u2 in [0, 1)) of the Philox block (pair = cell, stream (POP, attempt), realisation rho) of every draw"""
    rho = np.asarray(rho, dtype=np.uint64)
    ctr = np.zeros((len(rho), 4), dtype=np.uint32)
    ctr[:, 0] = np.asarray(cell, dtype=np.uint32)
    ctr[:, 1] = np.uint32(philox_ref.stream_id(STREAM_POP, attempt))
    ctr[:, 2] = (rho & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    ctr[:, 3] = (rho >> np.uint64(32)).astype(np.uint32)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32)
    v = philox_ref.philox4x32_10(ctr, key).astype(np.uint64)
    one = np.uint64(0x3FF0000000000000)
    a = (((v[:, 0] << np.uint64(32)) | v[:, 1]) >> np.uint64(12)) | one
    b = (((v[:, 2] << np.uint64(32)) | v[:, 3]) >> np.uint64(12)) | one
    return 2.0 - a.view(np.float64), b.view(np.float64) - 1.0


def _inversion(lam, u2):
    n = np.zeros(len(lam))
    flag = np.zeros(len(lam), dtype=bool)
    p = np.exp(-lam)
    cdf = p.copy()
    idx = np.arange(len(lam))
    for step in range(INVERSION_STEPS + 1):
        flag[idx] |= np.abs(u2[idx] - cdf) <= BORDER_INV * cdf
        go = u2[idx] > cdf
        if step == INVERSION_STEPS or not go.any():
            break
        idx, p, cdf = idx[go], p[go], cdf[go]
        n[idx] += 1
        p = p * (lam[idx] / n[idx])
        cdf = cdf + p
    return n, flag


def _ptrs(seed, rho, cell, lam):
    m = len(lam)
    out, flag, attempts = np.floor(lam + 0.5), np.zeros(m, dtype=bool), np.zeros(m, dtype=np.int32)
    slam, loglam = np.sqrt(lam), np.log(lam)
    b = 0.931 + 2.53 * slam
    a = -0.059 + 0.02483 * b
    invalpha = 1.1239 + 1.1328 / (b - 3.4)
    vr = 0.9277 - 3.6224 / (b - 2.0)
    log_invalpha = np.log(invalpha)
    idx = np.arange(m)
    for j in range(PTRS_ATTEMPTS):
        if not len(idx):
            break
        u1, u2 = uniforms(seed, rho[idx], cell[idx], j)
        attempts[idx] = j + 1
        U, V = u2 - 0.5, u1
        us = 0.5 - np.abs(U)
        with np.errstate(divide="ignore", invalid="ignore"):
            k = np.floor((2.0 * a[idx] / us + b[idx]) * U + lam[idx] + 0.43)
            quick = (us >= 0.07) & (V <= vr[idx])
            reject = ~quick & ((k < 0.0) | ((us < 0.013) & (V > us)))
            test = ~quick & ~reject
            kk = np.where(test, k, 1.0)
            lhs = np.log(V) + log_invalpha[idx] - np.log(a[idx] / (us * us) + b[idx])
            rhs = -lam[idx] + kk * loglam[idx] - gammaln(kk + 1.0)
        flag[idx] |= test & (np.abs(lhs - rhs) <= BORDER_PTRS * np.maximum(1.0, kk * np.abs(loglam[idx])))
        accept = quick | (test & (lhs <= rhs))
        out[idx[accept]] = k[accept]
        idx = idx[~accept]
    return out, flag, attempts


def poisson(seed, rho, cell, lam, z0=None):
    """(N, borderline flag, Philox blocks consumed) of every draw (rho[i], cell[i]) at the rate lam[i].  z0: the deviates of the normal
    regime, one per draw (read where lam >= 2^20); None takes philox_ref's libm Box-Muller, which follows the device to ~1e-16."""
    rho, cell, lam = np.asarray(rho, dtype=np.uint64), np.asarray(cell, dtype=np.uint32), np.asarray(lam, dtype=np.float64)
    n, flag, attempts = np.zeros(len(lam)), np.zeros(len(lam), dtype=bool), np.zeros(len(lam), dtype=np.int32)
    inv = np.flatnonzero((lam > 0) & (lam < INVERSION_BELOW))
    if len(inv):
        _, u2 = uniforms(seed, rho[inv], cell[inv], 0)
        n[inv], flag[inv] = _inversion(lam[inv], u2)
        attempts[inv] = 1
    pt = np.flatnonzero((lam >= INVERSION_BELOW) & (lam < NORMAL_FROM))
    if len(pt):
        n[pt], flag[pt], attempts[pt] = _ptrs(seed, rho[pt], cell[pt], lam[pt])
    nm = np.flatnonzero(lam >= NORMAL_FROM)
    if len(nm):
        if z0 is None:
            u1, u2 = uniforms(seed, rho[nm], cell[nm], 0)
            rad = np.sqrt(np.maximum(-2.0 * np.log(u1), 1e-300))
            z = rad * np.cos(2.0 * np.pi * u2)
        else:
            z = np.asarray(z0, dtype=np.float64)[nm]
        n[nm] = np.maximum(0.0, np.floor(lam[nm] + np.sqrt(lam[nm]) * z + 0.5))
        attempts[nm] = 1
    return n, flag, attempts


def weights(counts, hs2, fo, T_obs):
    """w = ((N hs2) fo) T_obs, the reference's operation order (deterministic.py:651)"""
    return ((np.asarray(counts, dtype=np.float64) * hs2) * fo) * T_obs


def select(w, fo, fobs, k):
    """the selection of one realisation: cells binned by np.digitize(fo, fobs) - 1 (outside [0, F) dropped), per bin the <= k cells with
    the largest w > 0, ties to the lower cell index, concatenated bin-major.  Returns (cell [n_sel] int, count [F] int, free_spec [F]
    long double = 1e-100 + the sum of the rest, members [F] = cells per bin)."""
    w = np.asarray(w, dtype=np.float64)
    F = len(fobs) - 1
    k_of = np.digitize(fo, fobs) - 1
    cells, count, free, members = [], np.zeros(F, dtype=np.int64), np.zeros(F, dtype=np.longdouble), np.zeros(F, dtype=np.int64)
    for b in range(F):
        mem = np.flatnonzero(k_of == b)
        order = mem[np.lexsort((mem, -w[mem]))]
        top = order[:k]
        top = top[w[top] > 0]
        rest = np.setdiff1d(mem, top)
        cells.append(top)
        count[b], members[b] = len(top), len(mem)
        free[b] = np.longdouble(1e-100) + np.sum(w[rest].astype(np.longdouble))
    return np.concatenate(cells).astype(np.int64), count, free, members
