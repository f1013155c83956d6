"""The F-statistic entry points of the C ABI: declared in include/pta_replicator_amd.h, exported by the library, bound by the ctypes
layer with the declared arity, additive to ABI version 8, and refusing bad arguments with PTA_E_ARG before any device call.  No GPU."""
import re
import subprocess

from test_abi import declared

FSTAT = ("pta_fstat_project", "pta_fstat_fp", "pta_fstat_fe", "pta_fstat_fe_tiles")
PTA_E_ARG = -1
X = 4096   # a non-NULL, 16-byte aligned stand-in: every call below is refused before a pointer is used


def test_symbols_are_declared_exported_and_bound():
    from pta_replicator_amd import _lib
    d = declared()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = set(re.findall(r" T (pta_\w+)", syms))
    for name in FSTAT:
        assert name in d and name in exported and name in _lib.EXPORTS, name
        assert len(getattr(_lib.lib, name).argtypes) == d[name], name
    assert _lib.lib.pta_abi_version() == 8
    assert _lib.FSTAT_CMAX == 4096 and _lib.FSTAT_PMAX == 128
    header = open(__import__("test_abi").HEADER).read()
    assert "#define PTA_FSTAT_CMAX 4096" in header and "#define PTA_FSTAT_PMAX 128" in header and "#define PTA_FSTAT_SKY_TILE 64" in header
    # 16 sky points per partial maximum, whole tiles of 64
    assert [_lib.lib.pta_fstat_fe_tiles(s) for s in (0, 1, 16, 64, 65, 768)] == [0, 4, 4, 4, 8, 48]


def test_argument_errors_without_gpu():
    from pta_replicator_amd import _lib
    lib = _lib.lib
    P, J, R, S, N = 3, 5, 7, 9, 100
    C = 2 * J

    def refused(rc, what):
        assert rc == PTA_E_ARG and what in _lib.last_error(), (rc, _lib.last_error())
    # ---- pta_fstat_project(Wt, ldw, C, psr_off, P, rows, ld_rows, R, Q, ld_q, stream)
    for null in range(4):
        p = [None if i == null else X for i in range(4)]
        refused(lib.pta_fstat_project(p[0], N, C, p[1], P, p[2], N, R, p[3], P * C, None), "NULL")
    for c in (0, 1, 3, 4098):                                       # C: even, 2 .. 4096
        refused(lib.pta_fstat_project(X, N, c, X, P, X, N, R, X, P * max(c, 1), None), "pta_fstat_project")
    refused(lib.pta_fstat_project(X, N, C, X, 0, X, N, R, X, P * C, None), "pta_fstat_project")
    refused(lib.pta_fstat_project(X, N, C, X, 65536, X, N, R, X, 65536 * C, None), "pta_fstat_project")
    refused(lib.pta_fstat_project(X, N, C, X, P, X, N, 0, X, P * C, None), "pta_fstat_project")
    refused(lib.pta_fstat_project(X, N, C, X, P, X, N, R, X, P * C - 1, None), "ld_q")
    refused(lib.pta_fstat_project(X, 0, C, X, P, X, N, R, X, P * C, None), "ldw")
    refused(lib.pta_fstat_project(X, N, C, X, P, X, 0, R, X, P * C, None), "ld_rows")
    refused(lib.pta_fstat_project(X, N, C, X, P, X, N, 128 * 65535 + 1, X, P * C, None), "exceeds one launch")
    # ---- pta_fstat_fp(Q, ld_q, P, J, R, Ginv, fp, ld_fp, stream)
    for null in range(3):
        p = [None if i == null else X for i in range(3)]
        refused(lib.pta_fstat_fp(p[0], P * C, P, J, R, p[1], p[2], J, None), "NULL")
    refused(lib.pta_fstat_fp(X, P * C, 0, J, R, X, X, J, None), "pta_fstat_fp")
    refused(lib.pta_fstat_fp(X, P * C, P, 0, R, X, X, J, None), "pta_fstat_fp")
    refused(lib.pta_fstat_fp(X, P * 4098, P, 2049, R, X, X, 2049, None), "pta_fstat_fp")
    refused(lib.pta_fstat_fp(X, P * C, P, J, 0, X, X, J, None), "pta_fstat_fp")
    refused(lib.pta_fstat_fp(X, P * C - 2, P, J, R, X, X, J, None), "ld_q")
    refused(lib.pta_fstat_fp(X, P * C + 1, P, J, R, X, X, J, None), "ld_q")           # odd: the sin / cos pairs are read as one 16-byte load
    refused(lib.pta_fstat_fp(X, P * C, P, J, R, X, X, J - 1, None), "ld_fp")
    refused(lib.pta_fstat_fp(X + 8, P * C, P, J, R, X, X, J, None), "aligned")
    # ---- pta_fstat_fe(Q, ld_q, P, J, R, phi, S, Minv, fe, ld_fe, fe_max, ld_max, fe_arg, ld_arg, part_val, part_arg, stream)
    def fe(Q=X, ld_q=P * C, P_=P, J_=J, R_=R, phi=X, S_=S, Minv=X, out=X, ld_fe=J * S, mx=None, ld_max=0, arg=None, ld_arg=0, pv=None, pa=None):
        return lib.pta_fstat_fe(Q, ld_q, P_, J_, R_, phi, S_, Minv, out, ld_fe, mx, ld_max, arg, ld_arg, pv, pa, None)
    refused(fe(Q=None), "NULL")
    refused(fe(phi=None), "NULL")
    refused(fe(Minv=None), "NULL")
    refused(fe(P_=1, ld_q=C), "pta_fstat_fe")                      # the coherent statistic needs two pulsars
    refused(fe(P_=129, ld_q=129 * C), "pta_fstat_fe")
    refused(fe(J_=0), "pta_fstat_fe")
    refused(fe(J_=2049, ld_q=P * 4098, ld_fe=2049 * S), "pta_fstat_fe")
    refused(fe(R_=0), "pta_fstat_fe")
    refused(fe(S_=0), "pta_fstat_fe")
    refused(fe(ld_q=P * C - 1), "ld_q")
    refused(fe(ld_fe=J * S - 1), "ld_fe")
    refused(fe(mx=X, ld_max=J, arg=X, ld_arg=J), "one output mode")           # the map and the maxima in one call
    refused(fe(out=None, ld_fe=0), "fe_max")                                   # neither
    refused(fe(out=None, ld_fe=0, mx=X, ld_max=J, arg=X, ld_arg=J), "part_val")   # the maxima without their workspaces
    refused(fe(out=None, ld_fe=0, mx=X, ld_max=J, arg=None, ld_arg=J, pv=X, pa=X), "fe_arg")
    refused(fe(out=None, ld_fe=0, mx=X, ld_max=J - 1, arg=X, ld_arg=J, pv=X, pa=X), "ld_max")
    refused(fe(out=None, ld_fe=0, mx=X, ld_max=J, arg=X, ld_arg=J - 1, pv=X, pa=X), "ld_arg")
