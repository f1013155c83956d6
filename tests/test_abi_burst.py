"""The wavelet burst / noise-transient entry points of the C ABI: declared in include/pta_replicator_amd.h after the existing entries,
exported by the library, bound by the ctypes layer with the declared arity, additive to ABI version 8, the structs laid out as a C
compiler lays the header's out, and refusing bad arguments with PTA_E_ARG before any device call.  No GPU."""
import ctypes
import os
import re
import subprocess

from test_abi import HEADER, ROOT, declared

BURST = ("pta_burst_uniform", "pta_transient_uniform", "pta_engine_burst_params", "pta_engine_burst_quad", "pta_engine_burst_add",
         "pta_engine_transient_params", "pta_engine_transient_add")
PTA_E_ARG = -1
X = 4096   # a non-NULL, 16-byte aligned stand-in: every call below is refused before a pointer is used


def test_symbols_are_declared_exported_and_bound():
    from pta_replicator_amd import _burst, _lib
    d = declared()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = set(re.findall(r" T (pta_\w+)", syms))
    for name in BURST:
        assert name in d and name in exported and name in _lib.EXPORTS, name
        assert len(getattr(_lib.lib, name).argtypes) == d[name], name
    assert [d[n] for n in BURST] == [9, 9, 3, 3, 7, 3, 7]
    assert set(_lib.EXPORTS) == set(d)
    assert _lib.lib.pta_abi_version() == 8
    header = open(HEADER).read()
    assert "#define PTA_ABI_VERSION 8" in header and "#define PTA_BURST_WMAX 128" in header and _burst.W_MAX == 128
    assert "#define PTA_BURST_NSKY 3" in header and "#define PTA_BURST_NCOL 7" in header and "#define PTA_NT_NCOL 6" in header
    assert (len(_burst.SKY_COLUMNS), len(_burst.WAV_COLUMNS), len(_burst.NT_COLUMNS)) == (3, 7, 6)
    # entries only, after everything the header declared before: the new section follows the last existing declaration
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    first_new = min(text.index(n + "(") for n in BURST)
    for name in d:
        if name not in BURST:
            assert text.index(name + "(") < first_new, name
    # the structs' fields as the header declares them, in order
    for struct, bound in (("pta_burst_engine", _lib.BurstEngine), ("pta_transient_engine", _lib.TransientEngine)):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, text).group(1)
        assert re.findall(r"(\w+);", body) == [f[0] for f in bound._fields_], struct
    # the structs and entries beside them are what they were
    assert ctypes.sizeof(_lib.BwmEngine) == 56 and ctypes.sizeof(_lib.CwEngine) == 80 and ctypes.sizeof(_lib.CwCatalogEngine) == 96
    for name in ("pta_engine_bwm_add", "pta_bwm_uniform", "pta_engine_cw_catalog_add", "pta_engine_synth"):
        assert name in exported, name


def test_struct_layouts_match_a_compiled_probe(tmp_path):
    """sizeof and every field offset of the two structs as gcc lays out the header's declarations = the ctypes bindings'"""
    from pta_replicator_amd import _lib
    structs = (("pta_burst_engine", _lib.BurstEngine), ("pta_transient_engine", _lib.TransientEngine))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pta_replicator_amd.h"', 'int main(void) {']
    for cname, bound in structs:
        lines.append(f'  printf("%zu", sizeof({cname}));')
        lines += [f'  printf(" %zu", offsetof({cname}, {f[0]}));' for f in bound._fields_]
        lines.append('  printf("\\n");')
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).splitlines()
    for (cname, bound), line in zip(structs, out):
        want = [int(x) for x in line.split()]
        got = [ctypes.sizeof(bound)] + [getattr(bound, f[0]).offset for f in bound._fields_]
        assert got == want, (cname, got, want)
    assert ctypes.sizeof(_lib.BurstEngine) == 8 + 8 * 10 and ctypes.sizeof(_lib.TransientEngine) == 8 + 8 * 4


def _plan(_lib, n_psr=3, n_toa=100, n_tiles=3):
    p = _lib.EnginePlan()
    p.n_psr, p.n_toa, p.n_tiles = n_psr, n_toa, n_tiles
    p.tile_psr = p.tile_start = p.tile_count = X
    return p


def _burst(_lib, **kw):
    b = _lib.BurstEngine()
    b.n_psr, b.n_wav = 3, 2
    b.phat = b.toa_s = b.sky = b.src = b.wav = b.kk = X
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def _nt(_lib, **kw):
    t = _lib.TransientEngine()
    t.n_psr, t.n_wav = 3, 2
    t.toa_s = t.src = t.tab = X
    for k, v in kw.items():
        setattr(t, k, v)
    return t


def test_argument_errors_without_gpu():
    from pta_replicator_amd import _lib
    lib = _lib.lib
    R, N = 7, 100

    def refused(rc, what):
        assert rc == PTA_E_ARG and what in _lib.last_error(), (rc, _lib.last_error())
    # ---- pta_burst_uniform(seed, r0, R, W, lo, hi, sky, wav, stream)
    for null in range(4):
        p = [None if i == null else X for i in range(4)]
        refused(lib.pta_burst_uniform(1, 0, R, 2, p[0], p[1], p[2], p[3], None), "NULL")
    refused(lib.pta_burst_uniform(1, 0, 0, 2, X, X, X, X, None), "R=0")
    refused(lib.pta_burst_uniform(1, 0, R, 0, X, X, X, X, None), "W=0")
    refused(lib.pta_burst_uniform(1, 0, R, 129, X, X, X, X, None), "W=129")
    refused(lib.pta_burst_uniform(1, 0, 1 << 30, 2, X, X, X, X, None), "too large")
    # ---- pta_transient_uniform(seed, r0, R, V, P, lo, hi, out, stream)
    for null in range(3):
        p = [None if i == null else X for i in range(3)]
        refused(lib.pta_transient_uniform(1, 0, R, 2, 3, p[0], p[1], p[2], None), "NULL")
    refused(lib.pta_transient_uniform(1, 0, -1, 2, 3, X, X, X, None), "R=-1")
    refused(lib.pta_transient_uniform(1, 0, R, 129, 3, X, X, X, None), "V=129")
    refused(lib.pta_transient_uniform(1, 0, R, 2, 0, X, X, X, None), "P=0")
    refused(lib.pta_transient_uniform(1, 0, 1 << 30, 2, 3, X, X, X, None), "too large")
    # ---- pta_engine_burst_params(burst, R, stream)
    par = lambda b, R_=R: lib.pta_engine_burst_params(ctypes.byref(b), R_, None)   # noqa: E731
    refused(lib.pta_engine_burst_params(None, R, None), "NULL argument")
    for f in ("sky", "src", "phat", "wav", "kk"):
        refused(par(_burst(_lib, **{f: None})), "NULL table")
    refused(par(_burst(_lib), 0), "R=0")
    refused(par(_burst(_lib, n_psr=0)), "n_psr=0")
    refused(par(_burst(_lib, n_wav=0)), "n_wav=0")
    refused(par(_burst(_lib, n_wav=129)), "n_wav=129")
    refused(par(_burst(_lib, n_psr=1 << 20), 1 << 12), "too large")
    # ---- pta_engine_burst_quad(burst, R, stream)
    quad = lambda b, R_=R: lib.pta_engine_burst_quad(ctypes.byref(b), R_, None)   # noqa: E731
    full = dict(psr_off=X, quad_q=X, quad_c=X)
    refused(lib.pta_engine_burst_quad(None, R, None), "NULL argument")
    for f in ("psr_off", "quad_q", "quad_c", "toa_s", "wav", "kk"):
        refused(quad(_burst(_lib, **dict(full, **{f: None}))), "missing")
    refused(quad(_burst(_lib, **full), 0), "R=0")
    refused(quad(_burst(_lib, **full), 65536), "R=65536")
    # ---- pta_engine_burst_add(plan, burst, R, out, ld_out, accumulate, stream)
    def add(plan=None, b=None, R_=R, out=X, ld_out=N):
        plan = _plan(_lib) if plan is None else plan
        b = _burst(_lib) if b is None else b
        return lib.pta_engine_burst_add(ctypes.byref(plan), ctypes.byref(b), R_, out, ld_out, 1, None)
    refused(lib.pta_engine_burst_add(None, ctypes.byref(_burst(_lib)), R, X, N, 1, None), "NULL argument")
    refused(lib.pta_engine_burst_add(ctypes.byref(_plan(_lib)), None, R, X, N, 1, None), "NULL argument")
    refused(add(out=None), "NULL argument")
    for f in ("toa_s", "wav", "kk"):
        refused(add(b=_burst(_lib, **{f: None})), "missing")
    for f in ("tile_psr", "tile_start", "tile_count"):
        broken = _plan(_lib)
        setattr(broken, f, None)
        refused(add(plan=broken), "missing")
    refused(add(R_=0), "R=0")
    refused(add(plan=_plan(_lib, n_psr=4)), "n_psr=3/4")
    refused(add(ld_out=N - 1), "ld_out=99")
    refused(add(plan=_plan(_lib, n_tiles=0)), "n_tiles=0")
    refused(add(b=_burst(_lib, n_wav=200)), "n_wav=200")
    refused(add(out=X + 4), "8-byte aligned")
    refused(add(R_=4 * 65535 + 1), "too large for one launch")
    refused(add(b=_burst(_lib, quad_q=X)), "remove_quad needs")
    # ---- pta_engine_transient_params(nt, R, stream) / pta_engine_transient_add(plan, nt, R, out, ld_out, accumulate, stream)
    tpar = lambda t, R_=R: lib.pta_engine_transient_params(ctypes.byref(t), R_, None)   # noqa: E731
    refused(lib.pta_engine_transient_params(None, R, None), "NULL argument")
    for f in ("src", "tab"):
        refused(tpar(_nt(_lib, **{f: None})), "NULL table")
    refused(tpar(_nt(_lib), 0), "R=0")
    refused(tpar(_nt(_lib, n_wav=0)), "n_wav=0")
    refused(tpar(_nt(_lib, n_wav=128), 1 << 25), "too large")

    def tadd(plan=None, t=None, R_=R, out=X, ld_out=N):
        plan = _plan(_lib) if plan is None else plan
        t = _nt(_lib) if t is None else t
        return lib.pta_engine_transient_add(ctypes.byref(plan), ctypes.byref(t), R_, out, ld_out, 1, None)
    refused(lib.pta_engine_transient_add(None, ctypes.byref(_nt(_lib)), R, X, N, 1, None), "NULL argument")
    refused(tadd(out=None), "NULL argument")
    for f in ("toa_s", "tab"):
        refused(tadd(t=_nt(_lib, **{f: None})), "missing")
    refused(tadd(R_=0), "R=0")
    refused(tadd(plan=_plan(_lib, n_psr=4)), "n_psr=3/4")
    refused(tadd(ld_out=N - 1), "ld_out=99")
    refused(tadd(t=_nt(_lib, n_wav=129)), "n_wav=129")
    refused(tadd(out=X + 4), "8-byte aligned")
    refused(tadd(R_=4 * 65535 + 1), "too large for one launch")
