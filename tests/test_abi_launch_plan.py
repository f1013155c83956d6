"""The launch-plan queries of the C ABI: declared in include/pta_replicator_amd.h, exported by the library, bound by the ctypes layer with
the declared arity, additive to ABI version 8, refusing bad sizes with PTA_E_ARG, and equal for random sizes to the launch arithmetic
the launchers have always used (written out again below: the queries move that arithmetic, they must not change it).  No GPU."""
import ctypes
import re
import subprocess

import numpy as np

from test_abi import declared

PLANS = ("pta_os_project_plan", "pta_lnl_apply_plan", "pta_fstat_project_plan", "pta_gwb_mix_batched_plan", "pta_fstat_fe_plan",
         "pta_bwm_stat_plan", "pta_tm_project_plan", "pta_dgemm_plan")
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


def test_dgemm_plan_refuses_what_pta_dgemm_refuses():
    from pta_replicator_amd import _lib
    lib = _lib.lib
    out = (ctypes.c_int32 * 8)()
    good = dict(transB=1, M=300, N=130, K=46, lda=60, ska=1, ldb=60, sA=18000, sB=7800, offA=0, offB=0, lower=1, algo=2, batch=2)

    def ask(**kw):
        for i in range(8):
            out[i] = -77
        return lib.pta_dgemm_plan(*{**good, **kw}.values(), out)
    assert ask() == 0 and list(out)[:5] == [7, 128, 3, 5, 1] and list(out)[5:] == [-77] * 3
    assert lib.pta_dgemm_plan(*good.values(), None) == PTA_E_ARG and "NULL" in _lib.last_error()
    for kw in (dict(M=0), dict(N=0), dict(K=0), dict(batch=0), dict(M=-1), dict(N=-1), dict(K=-1), dict(batch=65536), dict(offA=16), dict(offB=-1),
               dict(algo=0, M=65536), dict(M=128 * 65535 + 1), dict(M=64 * 65535 + 1, N=5)):
        assert ask(**kw) == PTA_E_ARG and "pta_dgemm_plan" in _lib.last_error(), (kw, _lib.last_error())
        assert list(out) == [-77] * 8, "a refused query writes nothing"
    assert ask(algo=0, M=65535) == 0 and ask(M=128 * 65535) == 0 and ask(M=64 * 65535, N=5) == 0 and ask(batch=65535) == 0


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


DGEMM_VALU_N, DGEMM_VALU_T, DGEMM_MFMA_N, DGEMM_MFMA_T, DGEMM_M128_N, DGEMM_M128_T, DGEMM_M128_TV, DGEMM_GLDS_E0, DGEMM_GLDS_E1 = range(9)


def _dgemm(transB, M, N, K, lda, ska, ldb, sA, sB, offA, offB, lower, algo, batch):
    """pta_dgemm_launch's choice as it stood before it moved into pta_dgemm_choose"""
    mode = 1 if lower else 0
    if algo == 0:
        return {"kernel": DGEMM_VALU_T if transB else DGEMM_VALU_N, "tile": 0, "lower_mode": mode, "grid_x": cdiv(N, 128), "grid_y": M}
    if algo >= 1 and M >= 256 and N >= 128 and K >= 32:
        gx, gy = cdiv(N, 128), cdiv(M, 128)
        if lower and M == N:
            nt = cdiv(M, 128)
            gx, gy, lower, mode = nt * (nt + 1) // 2, 1, 2, 2
        vec = bool(transB) and ska == 1 and K % 2 == 0 and lda % 2 == 0 and ldb % 2 == 0 and sA % 2 == 0 and sB % 2 == 0 and offA % 16 == 0 \
            and offB % 16 == 0
        if lower == 1 and M > N and vec and algo >= 2:
            nt, mt = cdiv(N, 128), cdiv(M, 128)
            gx, gy, mode = nt * (nt + 1) // 2 + (mt - nt) * nt, 1, 3
        if vec and algo >= 2:
            kern = DGEMM_GLDS_E1 if algo == 3 else DGEMM_GLDS_E0
        elif vec:
            kern = DGEMM_M128_TV
        else:
            kern = DGEMM_M128_T if transB else DGEMM_M128_N
        return {"kernel": kern, "tile": 128, "lower_mode": mode, "grid_x": gx, "grid_y": gy}
    return {"kernel": DGEMM_MFMA_T if transB else DGEMM_MFMA_N, "tile": 64, "lower_mode": mode, "grid_x": cdiv(N, 64), "grid_y": cdiv(M, 64)}


def test_dgemm_plan_equals_the_launch_arithmetic_at_random_arguments():
    from pta_replicator_amd import _lib
    rng = np.random.default_rng(419)
    seen = set()
    for _ in range(20000):
        M, N, K = (int(rng.choice([int(rng.integers(1, 700)), int(rng.integers(250, 262)), int(rng.integers(120, 136)), int(rng.integers(28, 36))]))
                   for _ in range(3))
        if rng.uniform() < 0.3:
            N = M
        near = lambda: int(rng.integers(0, 4000)) if rng.uniform() < 0.3 else 2 * int(rng.integers(0, 2000))    # mostly even
        args = (int(rng.integers(0, 2)), M, N, K, near(), 1 if rng.uniform() < 0.8 else int(rng.integers(1, 4)), near(), near(), near(),
                int(rng.choice([0, 0, 0, 8])), int(rng.choice([0, 0, 0, 8])), int(rng.integers(0, 2)), int(rng.integers(0, 4)), int(rng.integers(1, 5)))
        want = _dgemm(*args)
        got = _lib.launch_plan("pta_dgemm", *args)
        assert got == want, (args, got, want)
        seen.add((want["kernel"], want["lower_mode"]))
    assert len(seen) == 25, sorted(seen)     # every (instance, lower mode) pair the launcher can produce
    # offsets that are no multiple of 8 cannot come from a double pointer, but the predicate is "% 16 == 0"
    assert _lib.launch_plan("pta_dgemm", 1, 256, 128, 32, 40, 1, 40, 0, 0, 4, 0, 0, 2, 1)["kernel"] == DGEMM_M128_T


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
