"""Reference side of the common-process tests (not product code): the host twin of the device formulas (tests/cproc/cproc_host.cpp,
compiled once per session), long-double evaluations of the two sums the kernels form, the deviates from the NumPy twin of the device's
draws (oracle/philox_ref.py) on stream (12, process), and small synthetic arrays.  Nothing in it is computed by the device.

    y_ac = sum_p sqrt(phi_pc) sum_j B_p[a, j] z_pcj,   dt_{a,i} = sum_k y_a,2k sin(2 pi (k+1) x_i) + y_a,2k+1 cos(2 pi (k+1) x_i)
    x_i = frac(t_i / T),  z_pcj = deviate n = c rho_p + j of stream (12, p): pair n >> 1, branch n & 1
"""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

STREAM_CPROC = 12
FIELD_LOG10_A, FIELD_GAMMA = 8, 9   # stream (7, field) of the prior boxes, pair = process
YEAR = 365.25 * 86400.0
U = 2.0 ** -53                      # unit roundoff of float64
LD = np.longdouble
HERE = os.path.dirname(os.path.abspath(__file__))

_lib = None


def twin():
    """the host twin, compiled with g++ -ffp-contract=off on first use"""
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="cproc"), "libcprochost.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(HERE, "cproc", "cproc_host.cpp"),
                               "-o", out])
        lib = ctypes.CDLL(out)
        i, u64, d, p = ctypes.c_int, ctypes.c_uint64, ctypes.c_double, ctypes.POINTER(ctypes.c_double)
        pi, pl = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int64)
        lib.cp_draws.argtypes = [u64, u64, i, i, i, p]
        lib.cp_coef.argtypes = [u64, u64, i, i, i, pi, pi, p, pl, p, d, i, p, p, p]
        lib.cp_mix.argtypes, lib.cp_mix.restype = [p, p, i], d
        lib.cp_synth.argtypes = [p, i, p, i, p]
        lib.cp_draw_field.argtypes = [u64, u64, i, i, i, p, p, p]
        _lib = lib
    return _lib


def _p(a):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def twin_draws(seed, r, p, rho, kp):
    z = np.zeros(kp * rho)
    twin().cp_draws(seed, r, p, rho, kp, _p(z))
    return z.reshape(kp, rho)


def twin_coef(seed, r, P, K, kp, Bs, amp, T, log10_A=None, gamma=None):
    """coef [P, K] of one realisation by the twin; log10_A / gamma [n_proc] or None (configured)"""
    n = len(Bs)
    rho = [B.shape[1] for B in Bs]
    flat = np.ascontiguousarray(np.concatenate([np.ascontiguousarray(B).ravel() for B in Bs]))
    boff = np.concatenate([[0], np.cumsum([B.size for B in Bs])])[:n].astype(np.int64)
    coef = np.zeros((P, K))
    kp_c, rho_c = (ctypes.c_int * n)(*kp), (ctypes.c_int * n)(*rho)
    theta = log10_A is not None
    lA = np.ascontiguousarray(log10_A if theta else np.zeros(n), dtype=np.float64)
    g = np.ascontiguousarray(gamma if theta else np.zeros(n), dtype=np.float64)
    twin().cp_coef(seed, r, P, n, K, kp_c, rho_c, _p(flat), boff.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), _p(np.ascontiguousarray(amp)),
                   float(T), int(theta), _p(lA), _p(g), _p(coef))
    return coef


def twin_synth(coef, sc1):
    """[n] of coef [K] and sc1 [n, 2] by the twin of the add kernel's loop"""
    coef, sc1 = np.ascontiguousarray(coef, dtype=np.float64), np.ascontiguousarray(sc1, dtype=np.float64)
    out = np.zeros(len(sc1))
    twin().cp_synth(_p(coef), len(coef), _p(sc1), len(sc1), _p(out))
    return out


def draws(seed, r, p, rho, kp):
    """z [kp, rho] of process p in realisation r from philox_ref: deviate n = c rho + j is branch n & 1 of pair n >> 1 of stream (12, p)"""
    from oracle import philox_ref as ph
    n = kp * rho
    z = np.empty(2 * ((n + 1) // 2))
    z[0::2], z[1::2] = ph.normal_pairs(seed, r, ph.stream_id(STREAM_CPROC, p), (n + 1) // 2)
    return z[:n].reshape(kp, rho)


def prior_phi(nf, T, log10_A, gamma):
    """phi [2 nf] at f_k = k / T, Tspan = T"""
    freqs = np.repeat(np.arange(1, nf + 1) / float(T), 2)
    return (10 ** log10_A) ** 2 * (freqs * YEAR) ** (-gamma) / (12 * np.pi ** 2 * T) * YEAR ** 3


def pi_ld():
    return LD(4) * np.arctan(LD(1))


def basis_ld(t, T, nf):
    """F [N, 2 nf] in long double from x = frac(t / T) formed in long double: sin / cos(2 pi k x)"""
    x = np.asarray(t, dtype=np.float64).astype(LD) / LD(T)
    x = x - np.floor(x)
    arg = (LD(2) * pi_ld()) * x[:, None] * np.arange(1, nf + 1).astype(LD)[None, :]
    F = np.empty((len(x), 2 * nf), dtype=LD)
    F[:, 0::2], F[:, 1::2] = np.sin(arg), np.cos(arg)
    return F


def synth_ld(coef, t, T):
    """(value [N] long double, bound [N]) of sum_c coef_c F_ic and the issue's bound 8 n_f u sum_c |coef_c| on the float64 twin /
    kernel: every harmonic k carries <= 3 k u from the rotations and the rounded (s_1, c_1), times sqrt 2 for the sin / cos pair, plus
    2 n_f u from the accumulation"""
    coef = np.asarray(coef, dtype=np.float64)
    nf = len(coef) // 2
    val = basis_ld(t, T, nf) @ coef.astype(LD)
    return val, np.full(len(t), 8 * nf * U * float(np.sum(np.abs(coef))))


def mix_ld(B, z):
    """(value [P] long double, sum_j |B z| [P]) of sum_j B[a, j] z_j"""
    B, z = np.asarray(B, dtype=np.float64).astype(LD), np.asarray(z, dtype=np.float64).astype(LD)
    return B @ z, np.abs(B) @ np.abs(z)


def gamma_n(n):
    """n u / (1 - n u): the rigorous form of 'n roundings' (Higham's gamma_n)"""
    return n * U / (1 - n * U)


def make_psrs(counts, seed=11, span=(53000.0, 57500.0), offsets=None):
    """synthetic pulsars with the given TOA counts at random sky positions, sorted MJDs over `span`"""
    from pta_replicator_amd.simulate import ArrayTOAs, SimulatedPulsar, make_ideal
    rng = np.random.default_rng(seed)
    out = []
    for a, n in enumerate(counts):
        mjd = np.sort(rng.uniform(span[0], span[1], n))
        err = rng.uniform(0.2, 0.9, n)
        p = SimulatedPulsar(toas=ArrayTOAs(mjd, err, flags=[{"f": "A"}] * n, freqs_mhz=np.full(n, 1400.0)), name=f"J{a:04d}",
                            loc={"RAJ": float(rng.uniform(0, 24)), "DECJ": float(np.degrees(np.arcsin(rng.uniform(-1, 1))))})
        make_ideal(p)
        out.append(p)
    return out


def rank2_orf(P, seed=3):
    """a positive semi-definite [P, P] array of rank 2 (1 for P = 1) with a unit diagonal where it can have one"""
    rng = np.random.default_rng(seed)
    V = rng.normal(size=(P, min(2, P)))
    V /= np.linalg.norm(V, axis=1, keepdims=True)
    return V @ V.T
