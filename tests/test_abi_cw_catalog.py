"""The CW-catalogue entry points of the C ABI: declared in include/pta_replicator_amd.h, exported by the library, bound by the ctypes
layer with the declared arity, additive to ABI version 8, and refusing bad arguments with PTA_E_ARG before any device call.  No GPU."""
import ctypes
import re
import subprocess

from test_abi import declared

CATALOG = ("pta_cw_catalog_uniform", "pta_engine_cw_catalog_params", "pta_engine_cw_catalog_add")
PTA_E_ARG = -1
X = 4096   # a non-NULL stand-in: every call below is refused before a pointer is used


def test_symbols_are_declared_exported_and_bound():
    from pta_replicator_amd import _lib
    d = declared()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = set(re.findall(r" T (pta_\w+)", syms))
    for name in CATALOG:
        assert name in d and name in exported and name in _lib.EXPORTS, name
        assert len(getattr(_lib.lib, name).argtypes) == d[name], name
    assert _lib.lib.pta_abi_version() == 8
    header = open(__import__("test_abi").HEADER).read()
    assert "#define PTA_CW_CATALOG_NPAR_EVOLVE 16" in header and "#define PTA_CW_CATALOG_NPAR_FOLDED 8" in header
    assert _lib.CW_CATALOG_NPAR == (16, 8, 8)
    # the struct's fields as the header declares them, in order
    body = re.search(r"typedef struct \{([^}]*)\} pta_cw_catalog_engine;", re.sub(r"/\*.*?\*/", "", header, flags=re.S)).group(1)
    fields = re.findall(r"(\w+);", body)
    assert fields == [f[0] for f in _lib.CwCatalogEngine._fields_]
    # the single-source structs and entries are what they were
    assert ctypes.sizeof(_lib.CwEngine) == 80 and "pta_engine_cw_add" in exported and "pta_cw_uniform" in exported


def _plan(_lib, n_psr=3, n_toa=100, n_tiles=3):
    p = _lib.EnginePlan()
    p.n_psr, p.n_toa, p.n_tiles = n_psr, n_toa, n_tiles
    p.tile_psr = p.tile_start = p.tile_count = X
    return p


def _cat(_lib, **kw):
    c = _lib.CwCatalogEngine()
    c.n_psr, c.n_src, c.mode, c.psr_term, c.amp_is_h, c.has_pdist = 3, 5, 0, 1, 1, 0
    c.phat = c.pdist = c.toa_s = c.src = c.par = X
    c.ld_src, c.ld_pdist = 40, 0
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_argument_errors_without_gpu():
    from pta_replicator_amd import _lib
    lib = _lib.lib
    R, N = 7, 100

    def refused(rc, what):
        assert rc == PTA_E_ARG and what in _lib.last_error(), (rc, _lib.last_error())
    # ---- pta_cw_catalog_uniform(seed, r0, R, S, lo, hi, out, stream)
    for null in range(3):
        p = [None if i == null else X for i in range(3)]
        refused(lib.pta_cw_catalog_uniform(1, 0, R, 5, p[0], p[1], p[2], None), "NULL")
    refused(lib.pta_cw_catalog_uniform(1, 0, 0, 5, X, X, X, None), "R=0")
    refused(lib.pta_cw_catalog_uniform(1, 0, -1, 5, X, X, X, None), "R=-1")
    refused(lib.pta_cw_catalog_uniform(1, 0, R, 0, X, X, X, None), "S=0")
    refused(lib.pta_cw_catalog_uniform(1, 0, 1, 0x1000001, X, X, X, None), "S=16777217")       # S - 1 > 0xFFFFFF
    refused(lib.pta_cw_catalog_uniform(1, 0, 1 << 20, 1 << 10, X, X, X, None), "too large")
    # ---- pta_engine_cw_catalog_params(cw, R, stream)
    par = lambda c, R_=R: lib.pta_engine_cw_catalog_params(ctypes.byref(c) if c is not None else None, R_, None)   # noqa: E731
    refused(lib.pta_engine_cw_catalog_params(None, R, None), "NULL")
    for f in ("src", "phat", "par", "pdist"):
        refused(par(_cat(_lib, **{f: None})), "NULL table")
    refused(par(_cat(_lib), 0), "R=0")
    refused(par(_cat(_lib, n_psr=0)), "n_psr=0")
    refused(par(_cat(_lib, n_src=0)), "n_src=0")
    refused(par(_cat(_lib, n_src=0x1000001, ld_src=8 * 0x1000001), 1), "24-bit")
    for m in (-1, 3):
        refused(par(_cat(_lib, mode=m)), f"mode={m}")
    refused(par(_cat(_lib, ld_src=39)), "ld_src")
    refused(par(_cat(_lib, has_pdist=1, ld_pdist=2)), "ld_pdist")
    refused(par(_cat(_lib, n_src=1 << 20, ld_src=8 << 20), 1 << 10), "too large")
    # ---- pta_engine_cw_catalog_add(plan, cw, R, out, ld_out, accumulate, stream)
    def add(plan=None, c=None, R_=R, out=X, ld_out=N):
        plan = _plan(_lib) if plan is None else plan
        c = _cat(_lib) if c is None else c
        return lib.pta_engine_cw_catalog_add(ctypes.byref(plan), ctypes.byref(c), R_, out, ld_out, 1, None)
    refused(lib.pta_engine_cw_catalog_add(None, ctypes.byref(_cat(_lib)), R, X, N, 1, None), "NULL")
    refused(lib.pta_engine_cw_catalog_add(ctypes.byref(_plan(_lib)), None, R, X, N, 1, None), "NULL")
    refused(add(out=None), "NULL")
    for f in ("toa_s", "par"):
        refused(add(c=_cat(_lib, **{f: None})), "missing")
    broken = _plan(_lib)
    broken.tile_count = None
    refused(add(plan=broken), "missing")
    refused(add(R_=0), "R=0")
    refused(add(c=_cat(_lib, n_src=0)), "n_src=0")
    refused(add(c=_cat(_lib, n_src=0x1000001), R_=1), "24-bit")
    for m in (-1, 3):
        refused(add(c=_cat(_lib, mode=m)), f"mode={m}")
    refused(add(plan=_plan(_lib, n_psr=4)), "n_psr=3/4")                     # n_psr mismatch with the plan
    refused(add(ld_out=N - 1), "ld_out=99")                                  # ld_out < n_toa
    refused(add(plan=_plan(_lib, n_tiles=0)), "n_tiles=0")
    refused(add(c=_cat(_lib, n_src=1), R_=4 * 65535 + 1), "too large for one launch")   # realisation groups > 65535
