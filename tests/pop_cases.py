"""Shared pieces of the population tests (tests/test_pop_host.py, tests/test_gpu_pop.py): the g++ build of csrc/pta_pop.h, the reference
record with the helper functions it was made with, synthetic populations and a small engine."""
import ctypes
import importlib
import os
import subprocess

import numpy as np

from helpers import load

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 0x5EED0B0B0123
LAMBDAS = (0.0, 1e-6, 1e-3, 0.5, 3.0, 9.999, 10.0, 10.001, 37.5, 1e3, float((1 << 20) - 1))
NORMAL_LAMBDAS = (float(1 << 20), 1e9, 1e12)
FLAG_CAP = 1e-4   # the twin may flag at most this fraction of a test's draws as borderline


def build_host(tmpdir):
    """the g++ build of pta_pop.h (tests/pop/pop_host.cpp), -ffp-contract=off like the product"""
    out = os.path.join(str(tmpdir), "libpophost.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(HERE, "pop", "pop_host.cpp"), "-o", out])
    lib = ctypes.CDLL(out)
    vp, u64, i64, d = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int64, ctypes.c_double
    lib.ph_poisson.argtypes = [u64, vp, vp, vp, i64, vp, vp]
    lib.ph_normal_z0.argtypes = [u64, vp, vp, i64, vp]
    lib.ph_regime.argtypes = [d]
    lib.ph_weight.argtypes, lib.ph_weight.restype = [d, d, d, d], d
    return lib


def host_poisson(lib, seed, rho, cell, lam):
    """(N, attempts) of the g++ build for every draw"""
    rho, cell, lam = (np.ascontiguousarray(x, dtype=t) for x, t in ((rho, np.uint64), (cell, np.uint32), (lam, np.float64)))
    out, att = np.empty(len(lam)), np.empty(len(lam), dtype=np.int32)
    lib.ph_poisson(seed, rho.ctypes.data, cell.ctypes.data, lam.ctypes.data, len(lam), out.ctypes.data, att.ctypes.data)
    return out, att


def host_z0(lib, seed, rho, cell):
    rho, cell = np.ascontiguousarray(rho, dtype=np.uint64), np.ascontiguousarray(cell, dtype=np.uint32)
    z = np.empty(len(rho))
    lib.ph_normal_z0(seed, rho.ctypes.data, cell.ctypes.data, len(rho), z.ctypes.data)
    return z


def draws(n, r0=0, per_real=500):
    """(rho, cell) of n draws: per_real scattered cell indices in each of n / per_real consecutive realisations from r0"""
    i = np.arange(n, dtype=np.uint64)
    rho = np.uint64(r0) + i // np.uint64(per_real)
    cell = ((i % np.uint64(per_real)) * np.uint64(7919) + np.uint64(13)).astype(np.uint32)
    return rho, cell


class RecordHelpers:
    """the helper functions the reference record tests/golden/population.npz was made with (the oracle's holodeck stand-in), in the
    layout of _population.Population: with them the host bookkeeping reproduces the record's numbers bit for bit"""
    _u = importlib.import_module("oracle._stubs.holodeck.utils")
    _c = importlib.import_module("oracle._stubs.holodeck.cosmo")
    component_masses = staticmethod(lambda mt, mr: tuple(RecordHelpers._u.m1m2_from_mtmr(mt, mr)))
    chirp_mass = staticmethod(_u.chirp_mass)
    comoving_distance_cm = staticmethod(_c.z_to_dcom)
    gw_strain_source = staticmethod(_u.gw_strain_source)


def record():
    """the reference record and its outlier_per_bin"""
    return load("population.npz"), 4


def synthetic(sizes, seed=3, lam=(1e-2, 1e3), T_obs=10 * 365.25 * 86400.0, outside=7):
    """(vals [4, B], number [B], fobs [F + 1], T_obs) with sizes[b] cells in bin b and `outside` cells beyond the edges, in shuffled cell
    order; number log-uniform over lam"""
    rng = np.random.default_rng(seed)
    F = len(sizes)
    fobs = np.arange(1, F + 2) / T_obs
    fo = np.concatenate([rng.uniform(fobs[b] * 1.0001, fobs[b + 1] * 0.9999, n) for b, n in enumerate(sizes)]
                        + [np.r_[rng.uniform(0.2, 0.9, outside // 2) * fobs[0], rng.uniform(1.1, 2.0, outside - outside // 2) * fobs[-1]]])
    B = len(fo)
    fo = fo[rng.permutation(B)]
    msol = 1.988409870698051e33
    vals = np.array([10 ** rng.uniform(8.5, 10.3, B) * msol, rng.uniform(0.1, 1.0, B), rng.uniform(0.02, 2.0, B), fo])
    number = 10 ** rng.uniform(np.log10(lam[0]), np.log10(lam[1]), B)
    return vals, number, fobs, T_obs


def user_spec(fobs):
    from pta_replicator_amd import _population
    fc = _population.f_centers(fobs)
    return np.array([fc, 1e-15 * (fc / fc[0]) ** (-2.0 / 3.0)]).T


def engine(fobs, toas=(37, 64, 129, 200, 257, 513), seed=11, cw=True):
    """an engine of len(toas) pulsars with a userSpec GWB on the bin centres of fobs and the reference's CW flags; not prepared"""
    from pta_replicator_amd.engine import ReplicaEngine
    from pta_replicator_amd.simulate import ArrayTOAs, SimulatedPulsar, make_ideal
    rng = np.random.default_rng(seed)
    psrs = []
    for i, n in enumerate(toas):
        mjd = np.sort(rng.uniform(53000.0, 53000.0 + 3652.0, n)).astype(np.longdouble)
        p = SimulatedPulsar(toas=ArrayTOAs(mjd, np.full(n, 0.5)), name=f"J{i:04d}+0000",
                            loc={"RAJ": float(rng.uniform(0, 24)), "DECJ": float(rng.uniform(-60, 60))})
        make_ideal(p)
        psrs.append(p)
    eng = ReplicaEngine(psrs, seed=seed)
    eng.set_white_noise(efac=1.0)
    eng.set_gwb(None, None, userSpec=user_spec(fobs))
    if cw:
        eng.set_cw(psrTerm=True, evolve=True, phase_approx=False, tref=53000 * 86400.0, pdist=1.0)
    return eng
