"""The chromatic-event entry points of the C ABI: declared in include/pta_replicator_amd.h ahead of the wavelet burst section, exported by
the library, bound by the ctypes layer with the declared arity, additive to ABI version 8, the struct laid out as a C compiler lays the
header's out, and refusing bad arguments with PTA_E_ARG before any device call.  No GPU."""
import ctypes
import os
import re
import subprocess

from test_abi import HEADER, ROOT, declared
from test_abi_burst import BURST

CE = ("pta_chrom_event_uniform", "pta_engine_chrom_event_params", "pta_engine_chrom_event_add")
PTA_E_ARG = -1
X = 4096   # a non-NULL, 16-byte aligned stand-in: every call below is refused before a pointer is used


def test_symbols_are_declared_exported_and_bound():
    from pta_replicator_amd import _chrom_event, _lib
    d = declared()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = set(re.findall(r" T (pta_\w+)", syms))
    for name in CE:
        assert name in d and name in exported and name in _lib.EXPORTS, name
        assert len(getattr(_lib.lib, name).argtypes) == d[name], name
    assert [d[n] for n in CE] == [9, 3, 7]
    assert set(_lib.EXPORTS) == set(d) and exported >= set(d)
    assert {n for n in exported if "chrom_event" in n} == set(CE)
    assert _lib.lib.pta_abi_version() == 8
    header = open(HEADER).read()
    assert "#define PTA_ABI_VERSION 8" in header and "#define PTA_CE_EMAX 128" in header and _chrom_event.E_MAX == 128
    assert "#define PTA_CE_NCOL 9" in header and "#define PTA_CE_NTAB 10" in header
    assert (len(_chrom_event.COLUMNS), len(_chrom_event.TABLE)) == (9, 10)
    for j, c in enumerate(_chrom_event.COLUMNS):      # the label and table column names, in order
        assert f"#define PTA_CE_COL_{c.upper()} {j}\n" in header, c
    for j, c in enumerate(("PSR", "KIND", "T0", "INV_TAU", "INV_TAU_PRE", "NH", "SIGN", "LNA", "CHI", "TURNS")):
        assert f"#define PTA_CE_TAB_{c} {j}\n" in header, c
    # the section lies after every older entry and before the first wavelet burst entry
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    first_ce, last_ce = min(text.index(n + "(") for n in CE), max(text.index(n + "(") for n in CE)
    assert last_ce < min(text.index(n + "(") for n in BURST)
    for name in d:
        if name not in CE and name not in BURST:
            assert text.index(name + "(") < first_ce, name
    body = re.search(r"typedef struct \{([^}]*)\} pta_chrom_event_engine;", text).group(1)
    assert re.findall(r"(\w+);", body) == [f[0] for f in _lib.ChromEventEngine._fields_]
    # the structs beside it are what they were
    assert ctypes.sizeof(_lib.BurstEngine) == 88 and ctypes.sizeof(_lib.TransientEngine) == 40 and ctypes.sizeof(_lib.BwmEngine) == 56


def test_struct_layout_matches_a_compiled_probe(tmp_path):
    """sizeof and every field offset of the struct as gcc lays out the header's declaration = the ctypes binding's"""
    from pta_replicator_amd import _lib
    bound = _lib.ChromEventEngine
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pta_replicator_amd.h"', 'int main(void) {',
             '  printf("%zu", sizeof(pta_chrom_event_engine));']
    lines += [f'  printf(" %zu", offsetof(pta_chrom_event_engine, {f[0]}));' for f in bound._fields_]
    lines += ['  printf("\\n");', '  return 0;', '}']
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    want = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    got = [ctypes.sizeof(bound)] + [getattr(bound, f[0]).offset for f in bound._fields_]
    assert got == want, (got, want)
    assert ctypes.sizeof(bound) == 8 + 8 * 5


def _plan(_lib, n_psr=3, n_toa=100, n_tiles=3):
    p = _lib.EnginePlan()
    p.n_psr, p.n_toa, p.n_tiles = n_psr, n_toa, n_tiles
    p.tile_psr = p.tile_start = p.tile_count = X
    return p


def _ce(_lib, **kw):
    c = _lib.ChromEventEngine()
    c.n_psr, c.n_ev = 3, 2
    c.toa_s = c.lnu = c.src = c.tab = X
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_argument_errors_without_gpu():
    from pta_replicator_amd import _lib
    lib = _lib.lib
    R, N = 7, 100

    def refused(rc, what):
        assert rc == PTA_E_ARG and what in _lib.last_error(), (rc, _lib.last_error())
    # ---- pta_chrom_event_uniform(seed, r0, R, E, P, lo, hi, out, stream)
    for null in range(3):
        p = [None if i == null else X for i in range(3)]
        refused(lib.pta_chrom_event_uniform(1, 0, R, 2, 3, p[0], p[1], p[2], None), "pta_chrom_event_uniform: NULL")
    refused(lib.pta_chrom_event_uniform(1, 0, 0, 2, 3, X, X, X, None), "R=0")
    refused(lib.pta_chrom_event_uniform(1, 0, -1, 2, 3, X, X, X, None), "R=-1")
    refused(lib.pta_chrom_event_uniform(1, 0, R, 0, 3, X, X, X, None), "E=0")
    refused(lib.pta_chrom_event_uniform(1, 0, R, 129, 3, X, X, X, None), "E=129")
    refused(lib.pta_chrom_event_uniform(1, 0, R, 2, 0, X, X, X, None), "P=0")
    refused(lib.pta_chrom_event_uniform(1, 0, 1 << 30, 2, 3, X, X, X, None), "too large")
    # ---- pta_engine_chrom_event_params(ce, R, stream)
    par = lambda c, R_=R: lib.pta_engine_chrom_event_params(ctypes.byref(c), R_, None)   # noqa: E731
    refused(lib.pta_engine_chrom_event_params(None, R, None), "pta_engine_chrom_event_params: NULL argument")
    for f in ("src", "tab"):
        refused(par(_ce(_lib, **{f: None})), "NULL table")
    refused(par(_ce(_lib), 0), "R=0")
    refused(par(_ce(_lib, n_ev=0)), "n_ev=0")
    refused(par(_ce(_lib, n_ev=129)), "n_ev=129")
    refused(par(_ce(_lib, n_ev=128), 1 << 25), "too large")

    # ---- pta_engine_chrom_event_add(plan, ce, R, out, ld_out, accumulate, stream)
    def add(plan=None, c=None, R_=R, out=X, ld_out=N):
        plan = _plan(_lib) if plan is None else plan
        c = _ce(_lib) if c is None else c
        return lib.pta_engine_chrom_event_add(ctypes.byref(plan), ctypes.byref(c), R_, out, ld_out, 1, None)
    refused(lib.pta_engine_chrom_event_add(None, ctypes.byref(_ce(_lib)), R, X, N, 1, None), "pta_engine_chrom_event_add: NULL argument")
    refused(lib.pta_engine_chrom_event_add(ctypes.byref(_plan(_lib)), None, R, X, N, 1, None), "NULL argument")
    refused(add(out=None), "NULL argument")
    for f in ("toa_s", "lnu", "tab"):
        refused(add(c=_ce(_lib, **{f: None})), "missing")
    for f in ("tile_psr", "tile_start", "tile_count"):
        broken = _plan(_lib)
        setattr(broken, f, None)
        refused(add(plan=broken), "missing")
    refused(add(R_=0), "R=0")
    refused(add(plan=_plan(_lib, n_psr=4)), "n_psr=3/4")
    refused(add(ld_out=N - 1), "ld_out=99")
    refused(add(plan=_plan(_lib, n_tiles=0)), "n_tiles=0")
    refused(add(c=_ce(_lib, n_ev=0)), "n_ev=0")
    refused(add(c=_ce(_lib, n_ev=129)), "n_ev=129")
    refused(add(out=X + 4), "8-byte aligned")
    refused(add(R_=4 * 65535 + 1), "too large for one launch")
