"""The chromatic-process entry points of the C ABI: declared in include/pta_replicator_amd.h, exported by the library, bound by the
ctypes layer with the declared arity, additive to ABI version 8, the struct laid out as the header declares it, and refusing bad
arguments with PTA_E_ARG before any device call.  No GPU."""
import ctypes
import re
import subprocess

from test_abi import declared

CHROM = ("pta_engine_chrom_coef", "pta_engine_chrom_add")
PTA_E_ARG = -1
X = 4096   # a non-NULL stand-in: every call below is refused before a pointer is used


def test_symbols_are_declared_exported_and_bound():
    from pta_replicator_amd import _lib
    d = declared()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = set(re.findall(r" T (pta_\w+)", syms))
    for name in CHROM:
        assert name in d and name in exported and name in _lib.EXPORTS, name
        assert len(getattr(_lib.lib, name).argtypes) == d[name], name
    assert d["pta_engine_chrom_coef"] == 5 and d["pta_engine_chrom_add"] == 7
    assert set(_lib.EXPORTS) == set(d)
    assert _lib.lib.pta_abi_version() == 8
    header = open(__import__("test_abi").HEADER).read()
    assert "#define PTA_ABI_VERSION 8" in header
    # the struct's fields as the header declares them, in order and in type
    body = re.search(r"typedef struct \{([^}]*)\} pta_chrom_engine;", re.sub(r"/\*.*?\*/", "", header, flags=re.S)).group(1)
    decl = re.findall(r"([\w ]+?[\s\*]+)(\w+);", body)
    assert [name for _, name in decl] == [f[0] for f in _lib.ChromEngine._fields_]
    for (ctype, name), (_, bound) in zip(decl, _lib.ChromEngine._fields_):
        want = ctypes.c_void_p if "*" in ctype else {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}[ctype.strip()]
        assert bound is want, (name, ctype, bound)
    assert ctypes.sizeof(_lib.ChromEngine) == 16 + 8 * 9 and _lib.ChromEngine.Ft.offset == 16 and _lib.ChromEngine.coef.offset == 80
    # the structs and entries beside it are what they were
    assert ctypes.sizeof(_lib.BwmEngine) == 56 and ctypes.sizeof(_lib.CwEngine) == 80 and ctypes.sizeof(_lib.WnHyper) == 24 + 8 * 17
    for name in ("pta_engine_rn_coef", "pta_engine_rn_coef_hyper", "pta_engine_bwm_add", "pta_engine_wn_add", "pta_engine_synth"):
        assert name in exported, name


def _plan(_lib, n_psr=3, n_toa=100, n_tiles=3):
    p = _lib.EnginePlan()
    p.n_psr, p.n_toa, p.n_tiles = n_psr, n_toa, n_tiles
    p.tile_psr = p.tile_start = p.tile_count = X
    return p


def _chrom(_lib, **kw):
    c = _lib.ChromEngine()
    c.n_psr, c.k, c.ldf, c.ld_theta = 3, 14, 100, 3
    for f in ("Ft", "amp", "f", "tspan", "log10_A", "gamma", "coef"):
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
    # ---- pta_engine_chrom_coef(chrom, seed, r0, R, stream)
    coef = lambda c, R_=R: lib.pta_engine_chrom_coef(ctypes.byref(c), 1, 0, R_, None)   # noqa: E731
    refused(lib.pta_engine_chrom_coef(None, 1, 0, R, None), "NULL argument")
    refused(coef(_chrom(_lib, amp=None)), "NULL table")
    refused(coef(_chrom(_lib, coef=None)), "NULL table")
    refused(coef(_chrom(_lib), 0), "R=0")
    refused(coef(_chrom(_lib), -2), "R=-2")
    refused(coef(_chrom(_lib, n_psr=0)), "n_psr=0")
    refused(coef(_chrom(_lib, k=0)), "k=0")
    refused(coef(_chrom(_lib, k=13)), "k=13 (k must be even)")
    for f in ("gamma", "f", "tspan"):
        refused(coef(_chrom(_lib, **{f: None})), "gamma / f / tspan missing")
    refused(coef(_chrom(_lib, ld_theta=2)), "ld_theta=2")
    refused(coef(_chrom(_lib, n_psr=1 << 10, ld_theta=1 << 10, k=1 << 12), 1 << 12), "too large")
    # ---- pta_engine_chrom_add(plan, chrom, R, out, ld_out, accumulate, stream)
    def add(plan=None, c=None, R_=R, out=X, ld_out=N):
        plan = _plan(_lib) if plan is None else plan
        c = _chrom(_lib) if c is None else c
        return lib.pta_engine_chrom_add(ctypes.byref(plan), ctypes.byref(c), R_, out, ld_out, 1, None)
    refused(lib.pta_engine_chrom_add(None, ctypes.byref(_chrom(_lib)), R, X, N, 1, None), "NULL argument")
    refused(lib.pta_engine_chrom_add(ctypes.byref(_plan(_lib)), None, R, X, N, 1, None), "NULL argument")
    refused(add(out=None), "NULL argument")
    for f in ("tile_psr", "tile_start", "tile_count"):
        broken = _plan(_lib)
        setattr(broken, f, None)
        refused(add(plan=broken), "tiles / design matrix / coef missing")
    for f in ("Ft", "coef"):
        refused(add(c=_chrom(_lib, **{f: None})), "tiles / design matrix / coef missing")
    refused(add(c=_chrom(_lib, k=13)), "k=13 (k must be even)")
    refused(add(c=_chrom(_lib, k=0)), "k=0")
    refused(add(R_=0), "R=0")
    refused(add(plan=_plan(_lib, n_psr=4)), "n_psr=3/4")                     # n_psr mismatch with the plan
    refused(add(ld_out=N - 1), "ld_out=99")                                  # ld_out < n_toa
    refused(add(c=_chrom(_lib, ldf=N - 1)), "ldf=99")                        # a design-matrix row shorter than the TOAs
    refused(add(plan=_plan(_lib, n_tiles=0)), "n_tiles=0")
    refused(add(out=X + 4), "8-byte aligned")
    refused(add(plan=_plan(_lib, n_tiles=1 << 22), R_=(1 << 31) - 1), "too large for one launch")   # realisation groups x tiles >= 2^31
