"""The common-process entry points of the C ABI: declared in include/pta_replicator_amd.h, exported by the library, bound by the ctypes
layer with the declared arity, additive to ABI version 8, the struct laid out as the header declares it, and refusing bad arguments
with PTA_E_ARG before any device call.  No GPU."""
import ctypes
import re
import subprocess

from test_abi import declared

CPROC = ("pta_engine_cproc_coef", "pta_engine_cproc_add")
PTA_E_ARG = -1
X = 4096   # a non-NULL, 16-byte aligned stand-in: every call below is refused before a pointer is used


def test_symbols_are_declared_exported_and_bound():
    from pta_replicator_amd import _lib
    d = declared()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = set(re.findall(r" T (pta_\w+)", syms))
    for name in CPROC:
        assert name in d and name in exported and name in _lib.EXPORTS, name
        assert len(getattr(_lib.lib, name).argtypes) == d[name], name
    assert d["pta_engine_cproc_coef"] == 5 and d["pta_engine_cproc_add"] == 7
    assert set(_lib.EXPORTS) == set(d)
    assert _lib.lib.pta_abi_version() == 8
    header = open(__import__("test_abi").HEADER).read()
    assert "#define PTA_ABI_VERSION 8" in header
    # the struct's fields as the header declares them, in order and in type (arrays of PTA_CPROC_MAX = 4)
    body = re.search(r"typedef struct \{([^}]*)\} pta_cproc_engine;", re.sub(r"/\*.*?\*/", "", header, flags=re.S)).group(1)
    decl = re.findall(r"([\w ]+?[\s\*]+)(\w+)(\[PTA_CPROC_MAX\])?;", body)
    assert [name for _, name, _ in decl] == [f[0] for f in _lib.CprocEngine._fields_]
    scalar = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
    for (ctype, name, arr), (_, bound) in zip(decl, _lib.CprocEngine._fields_):
        want = ctypes.c_void_p if "*" in ctype else scalar[ctype.strip()]
        if arr:
            assert issubclass(bound, ctypes.Array) and bound._length_ == _lib.CPROC_MAX == 4 and bound._type_ is want, (name, ctype, bound)
        else:
            assert bound is want, (name, ctype, bound)
    S = _lib.CprocEngine
    assert ctypes.sizeof(S) == 16 + 16 + 16 + 32 + 8 * 7
    assert (S.kp.offset, S.rho.offset, S.B.offset, S.amp.offset, S.tspan.offset, S.log10_A.offset, S.gamma.offset, S.ld_theta.offset,
            S.sc1.offset, S.coef.offset) == (16, 32, 48, 80, 88, 96, 104, 112, 120, 128)
    # the structs and entries beside it are what they were
    assert ctypes.sizeof(_lib.ChromEngine) == 16 + 8 * 9 and ctypes.sizeof(_lib.BwmEngine) == 56 and ctypes.sizeof(_lib.CwEngine) == 80
    for name in ("pta_engine_chrom_coef", "pta_engine_chrom_add", "pta_engine_bwm_add", "pta_engine_wn_add", "pta_engine_synth"):
        assert name in exported, name


def _plan(_lib, n_psr=3, n_toa=100, n_tiles=3):
    p = _lib.EnginePlan()
    p.n_psr, p.n_toa, p.n_tiles = n_psr, n_toa, n_tiles
    p.tile_psr = p.tile_start = p.tile_count = X
    return p


def _cproc(_lib, kp=(14, 6), rho=(1, 3), B=(X, X), **kw):
    c = _lib.CprocEngine()
    c.n_psr, c.n_proc, c.k, c.ld_theta, c.tspan = 3, 2, 14, 2, 3.0e8
    for p in range(2):
        c.kp[p], c.rho[p], c.B[p] = kp[p], rho[p], B[p]
    for f in ("amp", "log10_A", "gamma", "sc1", "coef"):
        setattr(c, f, X)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_argument_errors_without_gpu():
    from pta_replicator_amd import _lib
    lib = _lib.lib
    R, N = 7, 100

    def refused(rc, what):
        assert rc == PTA_E_ARG and what in _lib.last_error(), (rc, _lib.last_error())
    # ---- pta_engine_cproc_coef(cproc, seed, r0, R, stream)
    coef = lambda c, R_=R: lib.pta_engine_cproc_coef(ctypes.byref(c), 1, 0, R_, None)   # noqa: E731
    refused(lib.pta_engine_cproc_coef(None, 1, 0, R, None), "NULL argument")
    refused(coef(_cproc(_lib, amp=None)), "NULL table")
    refused(coef(_cproc(_lib, coef=None)), "NULL table")
    refused(coef(_cproc(_lib), 0), "R=0")
    refused(coef(_cproc(_lib), -2), "R=-2")
    refused(coef(_cproc(_lib, n_psr=0)), "n_psr=0")
    refused(coef(_cproc(_lib, n_proc=0)), "n_proc=0")
    refused(coef(_cproc(_lib, n_proc=5)), "n_proc=5")
    refused(coef(_cproc(_lib, k=0)), "k=0")
    refused(coef(_cproc(_lib, k=13)), "k=13 (k must be even")
    refused(coef(_cproc(_lib, k=66)), "k=66")
    refused(coef(_cproc(_lib, B=(X, None))), "NULL factor of process 1")
    refused(coef(_cproc(_lib, rho=(1, 4))), "rho[1]=4")          # a rank above n_psr
    refused(coef(_cproc(_lib, rho=(0, 3))), "rho[0]=0")
    refused(coef(_cproc(_lib, kp=(14, 16))), "kp[1]=16")         # more columns than k
    refused(coef(_cproc(_lib, kp=(7, 6))), "kp[0]=7")
    refused(coef(_cproc(_lib, kp=(14, 0))), "kp[1]=0")
    refused(coef(_cproc(_lib, tspan=0.0)), "tspan=0")
    refused(coef(_cproc(_lib, tspan=float("inf"))), "tspan=inf")
    refused(coef(_cproc(_lib, tspan=float("nan"))), "tspan=nan")
    refused(coef(_cproc(_lib, gamma=None)), "gamma missing")
    refused(coef(_cproc(_lib, ld_theta=1)), "ld_theta=1")
    refused(coef(_cproc(_lib, k=64, kp=(64, 6)), 1 << 26), "too large")
    # ---- pta_engine_cproc_add(plan, cproc, R, out, ld_out, accumulate, stream)
    def add(plan=None, c=None, R_=R, out=X, ld_out=N):
        plan = _plan(_lib) if plan is None else plan
        c = _cproc(_lib) if c is None else c
        return lib.pta_engine_cproc_add(ctypes.byref(plan), ctypes.byref(c), R_, out, ld_out, 1, None)
    refused(lib.pta_engine_cproc_add(None, ctypes.byref(_cproc(_lib)), R, X, N, 1, None), "NULL argument")
    refused(lib.pta_engine_cproc_add(ctypes.byref(_plan(_lib)), None, R, X, N, 1, None), "NULL argument")
    refused(add(out=None), "NULL argument")
    for f in ("tile_psr", "tile_start", "tile_count"):
        broken = _plan(_lib)
        setattr(broken, f, None)
        refused(add(plan=broken), "tiles / basis table / coef missing")
    for f in ("sc1", "coef"):
        refused(add(c=_cproc(_lib, **{f: None})), "tiles / basis table / coef missing")
    refused(add(c=_cproc(_lib, k=13)), "k=13 (k must be even")
    refused(add(c=_cproc(_lib, k=0)), "k=0")
    refused(add(c=_cproc(_lib, k=66)), "k=66")
    refused(add(R_=0), "R=0")
    refused(add(plan=_plan(_lib, n_psr=4)), "n_psr=3/4")                     # n_psr mismatch with the plan
    refused(add(ld_out=N - 1), "ld_out=99")                                  # ld_out < n_toa
    refused(add(plan=_plan(_lib, n_tiles=0)), "n_tiles=0")
    refused(add(out=X + 4), "8-byte aligned")
    refused(add(c=_cproc(_lib, sc1=X + 8)), "16-byte aligned")
    refused(add(c=_cproc(_lib, coef=X + 8)), "16-byte aligned")
    refused(add(R_=16 * 65535 + 1), "too large for one launch")
