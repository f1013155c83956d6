"""The per-realisation white-noise entry points of the C ABI: declared in include/pta_replicator_amd.h, exported by the library, bound
by the ctypes layer with the declared arity, additive to ABI version 8, the struct laid out as the header declares it, and refusing
bad arguments with PTA_E_ARG before any device call.  No GPU."""
import ctypes
import re
import subprocess

from test_abi import declared

WN = ("pta_engine_wn_params", "pta_engine_wn_add")
PTA_E_ARG = -1
X = 4096   # a non-NULL stand-in: every call below is refused before a pointer is used


def test_symbols_are_declared_exported_and_bound():
    from pta_replicator_amd import _lib
    d = declared()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = set(re.findall(r" T (pta_\w+)", syms))
    for name in WN:
        assert name in d and name in exported and name in _lib.EXPORTS, name
        assert len(getattr(_lib.lib, name).argtypes) == d[name], name
    assert _lib.lib.pta_abi_version() == 8
    header = open(__import__("test_abi").HEADER).read()
    assert "#define PTA_WN_HYPER_GMAX 16" in header and _lib.WN_HYPER_GMAX == 16
    # the struct's fields as the header declares them, in order and in type
    body = re.search(r"typedef struct \{([^}]*)\} pta_engine_wn_hyper;", re.sub(r"/\*.*?\*/", "", header, flags=re.S)).group(1)
    decl = re.findall(r"([\w ]+?[\s\*]+)(\w+);", body)
    assert [name for _, name in decl] == [f[0] for f in _lib.WnHyper._fields_]
    for (ctype, name), (_, bound) in zip(decl, _lib.WnHyper._fields_):
        want = ctypes.c_void_p if "*" in ctype else {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}[ctype.strip()]
        assert bound is want, (name, ctype, bound)
    assert ctypes.sizeof(_lib.WnHyper) == 24 + 8 * 17 and _lib.WnHyper.sigma.offset == 24 and _lib.WnHyper.ec.offset == 152
    # the structs and entries beside it are what they were
    assert ctypes.sizeof(_lib.BwmEngine) == 56 and ctypes.sizeof(_lib.CwEngine) == 80
    assert "pta_engine_bwm_add" in exported and "pta_hyper_uniform_field" in exported and "pta_engine_synth" in exported


def _plan(_lib, n_psr=3, n_toa=100, n_tiles=3):
    p = _lib.EnginePlan()
    p.n_psr, p.n_toa, p.n_tiles = n_psr, n_toa, n_tiles
    p.tile_psr = p.tile_start = p.tile_count = p.tile_ep0 = p.tile_epn = p.idx_in_psr = p.epoch_of = X
    return p


def _wn(_lib, **kw):
    w = _lib.WnHyper()
    w.n_psr, w.n_wn, w.n_ec, w.max_per_psr = 3, 6, 5, 2
    w.ld_efac = w.ld_equad = 6
    w.ld_ecorr = 5
    for f in ("sigma", "wn_group", "ec_group", "wn_psr0", "ec_psr0", "efac_conf", "equad_conf", "ecorr_conf", "efac", "log10_equad", "log10_ecorr",
              "ea", "eb", "ec"):
        setattr(w, f, X)
    for k, v in kw.items():
        setattr(w, k, v)
    return w


def test_argument_errors_without_gpu():
    from pta_replicator_amd import _lib
    lib = _lib.lib
    R, N = 7, 100

    def refused(rc, what):
        assert rc == PTA_E_ARG and what in _lib.last_error(), (rc, _lib.last_error())
    # ---- pta_engine_wn_params(wn, R, stream)
    par = lambda w, R_=R: lib.pta_engine_wn_params(ctypes.byref(w), R_, None)   # noqa: E731
    refused(lib.pta_engine_wn_params(None, R, None), "NULL argument")
    refused(par(_wn(_lib, ea=None, eb=None, ec=None)), "NULL tables")
    refused(par(_wn(_lib, eb=None)), "go together")
    refused(par(_wn(_lib, ea=None)), "go together")
    refused(par(_wn(_lib), 0), "R=0")
    refused(par(_wn(_lib), -2), "R=-2")
    refused(par(_wn(_lib, n_wn=0)), "n_wn=0")
    refused(par(_wn(_lib, efac_conf=None)), "configured efac / equad missing")
    refused(par(_wn(_lib, equad_conf=None)), "configured efac / equad missing")
    refused(par(_wn(_lib, n_ec=0)), "n_ec=0")
    refused(par(_wn(_lib, ecorr_conf=None)), "configured ecorr missing")
    refused(par(_wn(_lib, ld_efac=5)), "ld_efac=5")
    refused(par(_wn(_lib, ld_equad=2)), "ld_equad=2")
    refused(par(_wn(_lib, ld_ecorr=4)), "ld_ecorr=4")
    refused(par(_wn(_lib, n_wn=1 << 20, ld_efac=1 << 20, ld_equad=1 << 20), 1 << 12), "too large")
    # ---- pta_engine_wn_add(plan, wn, seed, r0, R, out, ld_out, accumulate, stream)
    def add(plan=None, w=None, R_=R, out=X, ld_out=N):
        plan = _plan(_lib) if plan is None else plan
        w = _wn(_lib) if w is None else w
        return lib.pta_engine_wn_add(ctypes.byref(plan), ctypes.byref(w), 1, 0, R_, out, ld_out, 1, None)
    refused(lib.pta_engine_wn_add(None, ctypes.byref(_wn(_lib)), 1, 0, R, X, N, 1, None), "NULL argument")
    refused(lib.pta_engine_wn_add(ctypes.byref(_plan(_lib)), None, 1, 0, R, X, N, 1, None), "NULL argument")
    refused(add(out=None), "NULL argument")
    for f in ("tile_psr", "tile_count", "tile_ep0", "tile_epn", "idx_in_psr"):
        broken = _plan(_lib)
        setattr(broken, f, None)
        refused(add(plan=broken), "tile table / idx_in_psr missing")
    refused(add(w=_wn(_lib, ea=None, eb=None, ec=None)), "nothing to add")
    refused(add(w=_wn(_lib, eb=None)), "go together")
    for f in ("sigma", "wn_group", "wn_psr0"):
        refused(add(w=_wn(_lib, **{f: None})), "sigma / wn_group / wn_psr0 missing")
    refused(add(w=_wn(_lib, n_wn=0)), "n_wn=0")
    for f in ("ec_group", "ec_psr0"):
        refused(add(w=_wn(_lib, **{f: None})), "epoch_of missing")
    no_epochs = _plan(_lib)
    no_epochs.epoch_of = None
    refused(add(plan=no_epochs), "epoch_of missing")
    refused(add(w=_wn(_lib, n_ec=-1)), "n_ec=-1")
    refused(add(R_=0), "R=0")
    refused(add(plan=_plan(_lib, n_psr=4)), "n_psr=3/4")                     # n_psr mismatch with the plan
    refused(add(ld_out=N - 1), "ld_out=99")                                  # ld_out < n_toa
    refused(add(plan=_plan(_lib, n_tiles=0)), "n_tiles=0")
    refused(add(w=_wn(_lib, max_per_psr=0)), "max_per_psr=0")
    refused(add(w=_wn(_lib, max_per_psr=17)), "max_per_psr=17")
    refused(add(out=X + 4), "8-byte aligned")
    refused(add(R_=8 * 65535 + 1), "too large for one launch")               # realisation groups > 65535
