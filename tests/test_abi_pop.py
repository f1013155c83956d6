"""The population entry points of the C ABI: declared in include/pta_replicator_amd.h, exported by the library, bound by the ctypes layer
with the declared arity and argument types, additive to ABI version 8, and refusing bad arguments with PTA_E_ARG before any device
call.  No GPU."""
import ctypes
import re
import subprocess
from ctypes import POINTER, c_int, c_int64, c_uint64, c_void_p

from test_abi import HEADER, declared

POP = ("pta_pop_draw_select", "pta_pop_theta")
PTA_E_ARG = -1
X = 4096   # a non-NULL stand-in: every call below is refused before a pointer is used


def test_symbols_are_declared_exported_and_bound():
    from pta_replicator_amd import _lib, _pop
    d = declared()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = set(re.findall(r" T (pta_\w+)", syms))
    for name in POP:
        assert name in d and name in exported and name in _lib.EXPORTS, name
        assert len(getattr(_lib.lib, name).argtypes) == d[name], name
    assert _lib.lib.pta_abi_version() == 8
    P, V = POINTER(_lib.PopPlan), c_void_p
    assert _lib.lib.pta_pop_draw_select.argtypes == [P, c_uint64, c_uint64, c_int, V, c_int64, V, c_int64, V, V, V, V, V, V]
    assert _lib.lib.pta_pop_theta.argtypes == [P, c_int, V, V, V, V, V, V, V, V, V, V, V, c_int64, V]
    header = open(HEADER).read()
    for name, val in (("PTA_POP_KMAX", _lib.POP_KMAX), ("PTA_POP_FMAX", _lib.POP_FMAX), ("PTA_POP_CHUNK", _lib.POP_CHUNK)):
        assert re.search(rf"#define {name} {val}\b", header), name
    assert (_pop.KMAX, _pop.FMAX) == (_lib.POP_KMAX, _lib.POP_FMAX) == (128, 64)
    body = re.search(r"typedef struct \{([^}]*)\} pta_pop_plan;", re.sub(r"/\*.*?\*/", "", header, flags=re.S)).group(1)
    assert re.findall(r"(\w+);", body) == [f[0] for f in _lib.PopPlan._fields_]
    assert ctypes.sizeof(_lib.PopPlan) == 88
    # the sampler's constants, as the header and the host module state them
    src = open(HEADER.replace("include/pta_replicator_amd.h", "pta_replicator_amd/csrc/pta_pop.h")).read()
    assert "#define PTA_STREAM_POP 11u" in src and "#define PTA_POP_NORMAL_FROM 1048576.0" in src and "#define PTA_POP_INVERSION_BELOW 10.0" in src
    assert (_pop.INVERSION_BELOW, _pop.NORMAL_FROM) == (10.0, 1048576.0)
    # the catalogue entries it feeds are what they were
    assert ctypes.sizeof(_lib.CwCatalogEngine) == 96 and "pta_cw_catalog_uniform" in exported


def _plan(_lib, **kw):
    p = _lib.PopPlan()
    p.n_cells, p.n_sorted, p.n_bins, p.k, p.t_obs = 100, 90, 6, 4, 3e8
    p.cell_ptr = p.number = p.hs2 = p.fo = p.orig = p.log10_mc = p.log10_fo = p.log10_dl = X
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_argument_errors_without_gpu():
    from pta_replicator_amd import _lib
    lib = _lib.lib

    def refused(rc, what):
        assert rc == PTA_E_ARG and what in _lib.last_error(), (rc, _lib.last_error())

    def draw(plan=None, R=3, counts=None, ldc=0, cout=None, ldo=0, out=(X,) * 5):
        plan = _plan(_lib) if plan is None else plan
        return lib.pta_pop_draw_select(ctypes.byref(plan), 1, 0, R, counts, ldc, cout, ldo, *out, None)
    refused(lib.pta_pop_draw_select(None, 1, 0, 3, None, 0, None, 0, X, X, X, X, X, None), "NULL argument")
    for j in range(5):
        refused(draw(out=tuple(None if i == j else X for i in range(5))), "NULL argument")
    for f in ("cell_ptr", "number", "hs2", "fo", "orig"):
        refused(draw(_plan(_lib, **{f: None})), "NULL table")
    refused(draw(R=0), "R=0")
    refused(draw(_plan(_lib, n_cells=0)), "n_cells=0")
    refused(draw(_plan(_lib, n_sorted=101)), "n_sorted=101")
    refused(draw(_plan(_lib, n_bins=0)), "n_bins=0")
    refused(draw(_plan(_lib, n_bins=65)), "n_bins=65")
    refused(draw(_plan(_lib, k=0)), "k=0")
    refused(draw(_plan(_lib, k=129)), "k=129")
    refused(draw(_plan(_lib, n_bins=64, k=128), R=1 << 18), "too large")
    refused(draw(_plan(_lib, t_obs=0.0)), "t_obs")
    refused(draw(counts=X, ldc=99), "ld_counts=99")
    refused(draw(cout=X, ldo=99), "ld_counts_out=99")

    def theta(plan=None, R=3, args=(X,) * 11, ld_hc=6):
        plan = _plan(_lib) if plan is None else plan
        return lib.pta_pop_theta(ctypes.byref(plan), R, *args, ld_hc, None)
    refused(lib.pta_pop_theta(None, 3, *(X,) * 11, 6, None), "NULL argument")
    for j in range(11):
        refused(theta(args=tuple(None if i == j else X for i in range(11))), "NULL argument")
    for f in ("log10_mc", "log10_fo", "log10_dl"):
        refused(theta(_plan(_lib, **{f: None})), "NULL table")
    refused(theta(R=0), "R=0")
    refused(theta(_plan(_lib, k=129)), "k=129")
    refused(theta(ld_hc=5), "ld_hc=5")
