"""The launch-plan queries of the C ABI: declared in include/pta_replicator_amd.h, exported by the library, bound by the ctypes layer with
the declared arity, additive to ABI version 8, refusing bad sizes with PTA_E_ARG, and equal for random sizes to the launch arithmetic
the launchers have always used (written out again below: the queries move that arithmetic, they must not change it).  No GPU."""
import ctypes
import re
import subprocess

import numpy as np

from test_abi import declared

PLANS = ("pta_os_project_plan", "pta_lnl_apply_plan", "pta_fstat_project_plan", "pta_gwb_mix_batched_plan", "pta_fstat_fe_plan",
         "pta_bwm_stat_plan", "pta_tm_project_plan")
PTA_E_ARG = -1


def cdiv(a, b):
    return -(-a // b)


def test_symbols_are_declared_exported_and_bound():
    from pta_replicator_amd import _lib
    d = declared()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = set(re.findall(r" T (pta_\w+)", syms))
    for name in PLANS:
        assert name in d and name in exported and name in _lib.EXPORTS, name
        assert len(getattr(_lib.lib, name).argtypes) == d[name], name
        assert name[:-5] in d and name[:-5] in _lib._PLAN_FIELDS, name          # one query per launcher, named after it
    assert _lib.lib.pta_abi_version() == 8
    header = open(__import__("test_abi").HEADER).read()
    assert "#define PTA_ABI_VERSION 8" in header


def test_bad_sizes_are_refused_without_gpu():
    from pta_replicator_amd import _lib
    lib = _lib.lib
    out = (ctypes.c_int32 * 4)()

    def refused(name, *sizes):
        for i in range(4):
            out[i] = -77
        rc = getattr(lib, name)(*sizes, out)
        assert rc == PTA_E_ARG and name in _lib.last_error(), (name, sizes, rc, _lib.last_error())
        assert list(out) == [-77] * 4, "a refused query writes nothing"
    for name, good in (("pta_os_project_plan", (28, 8, 100)), ("pta_lnl_apply_plan", (8, 60, 5, 100)), ("pta_fstat_project_plan", (30, 8, 100)),
                       ("pta_gwb_mix_batched_plan", (17, 5, 300, 0)), ("pta_fstat_fe_plan", (5, 3, 10, 17)), ("pta_bwm_stat_plan", (5, 3, 10, 17)),
                       ("pta_tm_project_plan", (3, 8, 100))):
        assert getattr(lib, name)(*good, out) == 0, name
        assert getattr(lib, name)(*good, None) == PTA_E_ARG and "NULL" in _lib.last_error(), name
        for i in range(len(good)):
            if name == "pta_gwb_mix_batched_plan" and i == 3:
                continue                                     # variant: any value but 0 is the GEMM
            for bad in (0, -1):
                refused(name, *[bad if k == i else v for k, v in enumerate(good)])
    refused("pta_os_project_plan", 65, 8, 100)               # C: 1 .. PTA_OS_CMAX
    refused("pta_os_project_plan", 28, 65536, 100)
    refused("pta_lnl_apply_plan", 8, 129, 5, 100)            # K: 1 .. PTA_LNL_KMAX
    refused("pta_lnl_apply_plan", 65536, 60, 5, 100)
    refused("pta_lnl_apply_plan", 1, 60, 16 * 65535 + 1, 1)  # gz = ceil(G / 16) > 65535
    refused("pta_fstat_project_plan", 31, 8, 100)            # C: even
    refused("pta_fstat_project_plan", 4098, 8, 100)
    refused("pta_fstat_project_plan", 30, 65536, 100)
    refused("pta_fstat_project_plan", 30, 8, 64 * 65535 + 1)
    refused("pta_gwb_mix_batched_plan", 17, 65536, 300, 0)   # one realisation per grid row of the LDS kernel
    assert lib.pta_gwb_mix_batched_plan(81, 65536, 300, 0, out) == 0 and list(out)[:3] == [0, 0, 0]      # the GEMM walks R in batches
    for name in ("pta_fstat_fe_plan", "pta_bwm_stat_plan"):
        refused(name, 1, 3, 10, 17)                          # P: 2 .. PTA_FSTAT_PMAX
        refused(name, 129, 3, 10, 17)
    refused("pta_fstat_fe_plan", 5, 2049, 10, 17)            # 2 J <= PTA_FSTAT_CMAX
    assert lib.pta_bwm_stat_plan(5, 4096, 10, 17, out) == 0
    refused("pta_bwm_stat_plan", 5, 4097, 10, 17)
    refused("pta_tm_project_plan", 13, 8, 100)               # m: 1 .. PTA_FIT_MMAX
    refused("pta_tm_project_plan", 3, 65536, 100)
    refused("pta_tm_project_plan", 3, 8, 8 * 65535 + 1)


# ---------------------------------------------------------------- the launch arithmetic, as the launchers have had it ----------
def _os(C, P, R):
    rw = 2 if cdiv(R, 128) * P >= 1024 else 1
    return {"rw": rw, "ct": (C + 15) // 16, "grid_x": cdiv(R, 64 * rw)}


def _lnl(P, K, G, R):
    g_per = min(16, max(1, G * P * cdiv(R, 128) // 4096))
    return {"kt": (K + 15) // 16, "g_per": g_per, "gz": cdiv(G, g_per)}


def _fsp(C, P, R):
    bm, bn = 128, 128 if C > 64 else (64 if C > 32 else 32)
    if P * cdiv(R, bm) * cdiv(C, bn) < 2048:
        bm = 64
    if P * cdiv(R, bm) * cdiv(C, bn) < 2048 and bn == 128:
        bn = 64
    return {"bm": bm, "bn": bn}


def _mix(P, R, npts, variant):
    if variant != 0 or P > 80:
        return {"nta": 0, "tpw": 0, "grid_x": 0}
    ntile = cdiv(npts, 64)
    tpw = ntile if (R >= 512 or ntile <= 4) else 4
    return {"nta": (P + 15) // 16, "tpw": tpw, "grid_x": cdiv(ntile, tpw)}


def _sky(jb):
    def f(P, J, R, S):
        nz = min(max(1, 4096 // (cdiv(S, 64) * cdiv(J, jb))), (R + 7) // 8, 65535)
        rchunk = (R + nz - 1) // nz
        return {"ks": (P + 3) // 4, "rchunk": rchunk, "ngz": cdiv(R, rchunk)}
    return f


def _tm(m, P, R):
    return {"m": m, "grid_y": cdiv(R, 8)}


def _log_int(rng, lo, hi):
    return int(np.exp(rng.uniform(np.log(lo), np.log(hi + 1)))) if rng.uniform() < 0.7 else int(rng.integers(lo, hi + 1))


def test_plans_equal_the_launch_arithmetic_at_random_sizes():
    from pta_replicator_amd import _lib
    rng = np.random.default_rng(2024)
    L = lambda lo, hi: min(hi, max(lo, _log_int(rng, lo, hi)))
    draws = {
        "pta_os_project": (_os, lambda: (L(1, 64), L(1, 65535), L(1, 3000000))),
        "pta_lnl_apply": (_lnl, lambda: (L(1, 65535), L(1, 128), L(1, 65535), L(1, 3000000))),
        "pta_fstat_project": (_fsp, lambda: (2 * L(1, 2048), L(1, 65535), L(1, 4000000))),
        "pta_gwb_mix_batched": (_mix, lambda: (L(1, 120), L(1, 65535), L(1, 100000), int(rng.integers(0, 3)))),
        "pta_fstat_fe": (_sky(8), lambda: (L(2, 128), L(1, 2048), L(1, 3000000), L(1, 500000))),
        "pta_bwm_stat": (_sky(16), lambda: (L(2, 128), L(1, 4096), L(1, 3000000), L(1, 500000))),
        "pta_tm_project": (_tm, lambda: (L(1, 12), L(1, 65535), L(1, 8 * 65535))),
    }
    for name, (ref, draw) in draws.items():
        seen = set()
        for _ in range(4000):
            sizes = draw()
            want = ref(*sizes)
            got = _lib.launch_plan(name, *sizes)
            assert got == want, (name, sizes, got, want)
            seen.add(tuple(want.values())[:2])
        assert len(seen) >= 4, (name, len(seen))   # the draws spread over the instances
    # and at the thresholds themselves
    assert [_lib.launch_plan("pta_os_project", 28, 68, R)["rw"] for R in (1920, 1921)] == [1, 2]
    assert [_lib.launch_plan("pta_lnl_apply", 68, 60, G, 1)["g_per"] for G in (120, 121, 963, 964)] == [1, 2, 15, 16]
    assert [_lib.launch_plan("pta_gwb_mix_batched", 68, R, 300, 0)["tpw"] for R in (511, 512)] == [4, 5]
    assert _lib.launch_plan("pta_fstat_fe", 5, 17, 300, 2560) == {"ks": 2, "rchunk": 9, "ngz": 34}
