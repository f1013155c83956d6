"""The burst-with-memory entry points of the C ABI: declared in include/pta_replicator_amd.h, exported by the library, bound by the
ctypes layer with the declared arity, additive to ABI version 8, and refusing bad arguments with PTA_E_ARG before any device call.
No GPU."""
import ctypes
import re
import subprocess

from test_abi import declared

BWM = ("pta_bwm_uniform", "pta_engine_bwm_params", "pta_engine_bwm_add", "pta_bwm_stat")
PTA_E_ARG = -1
X = 4096   # a non-NULL stand-in: every call below is refused before a pointer is used


def test_symbols_are_declared_exported_and_bound():
    from pta_replicator_amd import _bwm, _lib
    d = declared()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = set(re.findall(r" T (pta_\w+)", syms))
    for name in BWM:
        assert name in d and name in exported and name in _lib.EXPORTS, name
        assert len(getattr(_lib.lib, name).argtypes) == d[name], name
    assert _lib.lib.pta_abi_version() == 8
    header = open(__import__("test_abi").HEADER).read()
    assert "#define PTA_BWM_NSRC 5" in header and _bwm.N_SRC == 5
    # the struct's fields as the header declares them, in order
    body = re.search(r"typedef struct \{([^}]*)\} pta_bwm_engine;", re.sub(r"/\*.*?\*/", "", header, flags=re.S)).group(1)
    fields = re.findall(r"(\w+);", body)
    assert fields == [f[0] for f in _lib.BwmEngine._fields_]
    assert ctypes.sizeof(_lib.BwmEngine) == 56
    # the CW structs and entries are what they were
    assert ctypes.sizeof(_lib.CwEngine) == 80 and "pta_engine_cw_add" in exported and "pta_cw_uniform" in exported


def _plan(_lib, n_psr=3, n_toa=100, n_tiles=3):
    p = _lib.EnginePlan()
    p.n_psr, p.n_toa, p.n_tiles = n_psr, n_toa, n_tiles
    p.tile_psr = p.tile_start = p.tile_count = X
    return p


def _bwm_engine(_lib, **kw):
    b = _lib.BwmEngine()
    b.n_psr, b.ld_src = 3, 5
    b.phat = b.toa_s = b.src = b.coef = b.t0_s = X
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def test_argument_errors_without_gpu():
    from pta_replicator_amd import _lib
    lib = _lib.lib
    R, N = 7, 100

    def refused(rc, what):
        assert rc == PTA_E_ARG and what in _lib.last_error(), (rc, _lib.last_error())
    # ---- pta_bwm_uniform(seed, r0, R, lo, hi, out, stream)
    for null in range(3):
        p = [None if i == null else X for i in range(3)]
        refused(lib.pta_bwm_uniform(1, 0, R, p[0], p[1], p[2], None), "NULL")
    refused(lib.pta_bwm_uniform(1, 0, 0, X, X, X, None), "R=0")
    refused(lib.pta_bwm_uniform(1, 0, -1, X, X, X, None), "R=-1")
    refused(lib.pta_bwm_uniform(1, 0, 1 << 30, X, X, X, None), "too large")
    # ---- pta_engine_bwm_params(bwm, R, stream)
    par = lambda b, R_=R: lib.pta_engine_bwm_params(ctypes.byref(b), R_, None)   # noqa: E731
    refused(lib.pta_engine_bwm_params(None, R, None), "NULL")
    for f in ("src", "phat", "coef", "t0_s"):
        refused(par(_bwm_engine(_lib, **{f: None})), "NULL table")
    refused(par(_bwm_engine(_lib), 0), "R=0")
    refused(par(_bwm_engine(_lib, n_psr=0)), "n_psr=0")
    refused(par(_bwm_engine(_lib, ld_src=4)), "ld_src")
    refused(par(_bwm_engine(_lib, n_psr=1 << 20), 1 << 12), "too large")
    # ---- pta_engine_bwm_add(plan, bwm, R, out, ld_out, accumulate, stream)
    def add(plan=None, b=None, R_=R, out=X, ld_out=N):
        plan = _plan(_lib) if plan is None else plan
        b = _bwm_engine(_lib) if b is None else b
        return lib.pta_engine_bwm_add(ctypes.byref(plan), ctypes.byref(b), R_, out, ld_out, 1, None)
    refused(lib.pta_engine_bwm_add(None, ctypes.byref(_bwm_engine(_lib)), R, X, N, 1, None), "NULL")
    refused(lib.pta_engine_bwm_add(ctypes.byref(_plan(_lib)), None, R, X, N, 1, None), "NULL")
    refused(add(out=None), "NULL")
    for f in ("toa_s", "coef", "t0_s"):
        refused(add(b=_bwm_engine(_lib, **{f: None})), "missing")
    broken = _plan(_lib)
    broken.tile_count = None
    refused(add(plan=broken), "missing")
    refused(add(R_=0), "R=0")
    refused(add(plan=_plan(_lib, n_psr=4)), "n_psr=3/4")                     # n_psr mismatch with the plan
    refused(add(ld_out=N - 1), "ld_out=99")                                  # ld_out < n_toa
    refused(add(plan=_plan(_lib, n_tiles=0)), "n_tiles=0")
    refused(add(out=X + 4), "8-byte aligned")
    refused(add(R_=16 * 65535 + 1), "too large for one launch")              # realisation groups > 65535
    # ---- pta_bwm_stat(Q, ld_q, P, C, J, R, phi, S, Minv, fb, ld_fb, amp, ld_amp, fb_max, ld_max, fb_arg, ld_arg, part_val, part_arg, stream)
    P, C, J, S = 5, 4, 3, 7

    def stat(Q=X, ld_q=P * C, P_=P, C_=C, J_=J, R_=R, phi=X, S_=S, Minv=X, fb=X, ld_fb=J * S, amp=None, ld_amp=0, mx=None, ld_max=0, arg=None, ld_arg=0,
             pv=None, pa=None):
        return lib.pta_bwm_stat(Q, ld_q, P_, C_, J_, R_, phi, S_, Minv, fb, ld_fb, amp, ld_amp, mx, ld_max, arg, ld_arg, pv, pa, None)
    for f in ("Q", "phi", "Minv"):
        refused(stat(**{f: None}), "NULL")
    refused(stat(P_=1), "P=1")
    refused(stat(P_=_lib.FSTAT_PMAX + 1, ld_q=(_lib.FSTAT_PMAX + 1) * C), f"P={_lib.FSTAT_PMAX + 1}")
    refused(stat(J_=0), "J=0")
    refused(stat(C_=2), "C=2")                                                # C < J
    refused(stat(C_=_lib.FSTAT_CMAX + 1, ld_q=P * (_lib.FSTAT_CMAX + 1)), f"C={_lib.FSTAT_CMAX + 1}")
    refused(stat(R_=0), "R=0")
    refused(stat(S_=0), "S=0")
    refused(stat(ld_q=P * C - 1), "ld_q")
    refused(stat(ld_fb=J * S - 1), "ld_fb")
    refused(stat(mx=X, arg=X), "one output mode")
    refused(stat(amp=X, ld_amp=2 * J * S - 2), "ld_amp")
    refused(stat(amp=X, ld_amp=2 * J * S + 1), "ld_amp")
    refused(stat(amp=X + 8, ld_amp=2 * J * S), "16-byte aligned")
    refused(stat(fb=None), "fb_max, fb_arg and the workspaces")
    refused(stat(fb=None, mx=X, arg=X, pv=X), "fb_max, fb_arg and the workspaces")
    refused(stat(fb=None, amp=X, mx=X, arg=X, pv=X, pa=X), "amp needs fb")
    refused(stat(fb=None, mx=X, ld_max=J - 1, arg=X, ld_arg=J, pv=X, pa=X), "ld_max")
