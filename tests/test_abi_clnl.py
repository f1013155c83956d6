"""The correlated-likelihood entry points of the C ABI: declared in include/pta_replicator_amd.h, exported by the library, bound by the
ctypes layer with the declared arity, additive to ABI version 8, and refusing bad arguments with PTA_E_ARG before any device call.  No GPU."""
import re
import subprocess

from test_abi import declared

CLNL = ("pta_clnl_mix", "pta_clnl_assemble", "pta_clnl_rhs", "pta_clnl_solve", "pta_clnl_finish")
PTA_E_ARG = -1
X = 4096   # a non-NULL stand-in: every call below is refused before a pointer is used


def test_symbols_are_declared_exported_and_bound():
    from pta_replicator_amd import _lib
    d = declared()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = set(re.findall(r" T (pta_\w+)", syms))
    for name in CLNL:
        assert name in d and name in exported and name in _lib.EXPORTS, name
        assert len(getattr(_lib.lib, name).argtypes) == d[name], name
    assert _lib.lib.pta_abi_version() == 8
    assert _lib.CLNL_CMAX == 64 and _lib.CLNL_NORF == 4


def test_argument_errors_without_gpu():
    from pta_replicator_amd import _lib
    lib = _lib.lib
    P, C, rho, R, G = 5, 6, 3, 7, 4
    n = rho * C
    T, gref = 3.0e8, 13. / 3.

    def refused(rc, what):
        assert rc == PTA_E_ARG and what in _lib.last_error(), (rc, _lib.last_error())
    # pta_clnl_mix: C beyond 64, rho beyond P, P C beyond the LDS budget, short leading dimensions, NULL operands
    refused(lib.pta_clnl_mix(X, P * 65, P, 65, R, X, rho, X, rho * 65, None), "pta_clnl_mix")
    refused(lib.pta_clnl_mix(X, P * C, P, C, R, X, P + 1, X, (P + 1) * C, None), "pta_clnl_mix")
    refused(lib.pta_clnl_mix(X, P * C, P, C, R, X, 0, X, n, None), "pta_clnl_mix")
    refused(lib.pta_clnl_mix(X, 200 * 64, 200, 64, R, X, rho, X, rho * 64, None), "pta_clnl_mix")
    refused(lib.pta_clnl_mix(X, P * C, P, C, 0, X, rho, X, n, None), "pta_clnl_mix")
    refused(lib.pta_clnl_mix(X, P * C - 1, P, C, R, X, rho, X, n, None), "ld_y")
    refused(lib.pta_clnl_mix(X, P * C, P, C, R, X, rho, X, n - 1, None), "ld_yp")
    for null in range(3):
        p = [None if i == null else X for i in range(3)]
        refused(lib.pta_clnl_mix(p[0], P * C, P, C, R, p[1], rho, p[2], n, None), "NULL")
    # pta_clnl_assemble
    refused(lib.pta_clnl_assemble(X, rho, 65, gref, T, X, X, G, X, None), "pta_clnl_assemble")
    refused(lib.pta_clnl_assemble(X, 0, C, gref, T, X, X, G, X, None), "pta_clnl_assemble")
    refused(lib.pta_clnl_assemble(X, 2000, 64, gref, T, X, X, G, X, None), "pta_clnl_assemble")
    refused(lib.pta_clnl_assemble(X, rho, C, gref, T, X, X, 0, X, None), "pta_clnl_assemble")
    refused(lib.pta_clnl_assemble(X, rho, C, gref, T, X, X, 65536, X, None), "pta_clnl_assemble")
    refused(lib.pta_clnl_assemble(X, rho, C, gref, 0.0, X, X, G, X, None), "Tspan")
    refused(lib.pta_clnl_assemble(X, rho, C, float("nan"), T, X, X, G, X, None), "gamma_ref")
    for null in range(4):
        p = [None if i == null else X for i in range(4)]
        refused(lib.pta_clnl_assemble(p[0], rho, C, gref, T, p[1], p[2], G, p[3], None), "NULL")
    # pta_clnl_rhs
    refused(lib.pta_clnl_rhs(X, n, rho, 65, R, gref, T, X, X, G, X, R, None), "pta_clnl_rhs")
    refused(lib.pta_clnl_rhs(X, n, rho, C, R, gref, -1.0, X, X, G, X, R, None), "Tspan")
    refused(lib.pta_clnl_rhs(X, n, rho, C, 0, gref, T, X, X, G, X, R, None), "pta_clnl_rhs")
    refused(lib.pta_clnl_rhs(X, n - 1, rho, C, R, gref, T, X, X, G, X, R, None), "ld_yp")
    refused(lib.pta_clnl_rhs(X, n, rho, C, R, gref, T, X, X, G, X, R - 1, None), "ld_v")
    for null in range(4):
        p = [None if i == null else X for i in range(4)]
        refused(lib.pta_clnl_rhs(p[0], n, rho, C, R, gref, T, p[1], p[2], G, p[3], R, None), "NULL")
    # pta_clnl_solve
    refused(lib.pta_clnl_solve(X, 0, G, X, R, R, X, R, None), "pta_clnl_solve")
    refused(lib.pta_clnl_solve(X, 65536, G, X, R, R, X, R, None), "pta_clnl_solve")
    refused(lib.pta_clnl_solve(X, n, 0, X, R, R, X, R, None), "pta_clnl_solve")
    refused(lib.pta_clnl_solve(X, n, 65536, X, R, R, X, R, None), "pta_clnl_solve")
    refused(lib.pta_clnl_solve(X, n, G, X, R, 0, X, R, None), "pta_clnl_solve")
    refused(lib.pta_clnl_solve(X, n, G, X, R - 1, R, X, R, None), "ld_v")
    refused(lib.pta_clnl_solve(X, n, G, X, R, R, X, R - 1, None), "ld_quad")
    for null in range(3):
        p = [None if i == null else X for i in range(3)]
        refused(lib.pta_clnl_solve(p[0], n, G, p[1], R, R, p[2], R, None), "NULL")
    # pta_clnl_finish
    refused(lib.pta_clnl_finish(X, 0, G, X, R, R, X, R, None), "pta_clnl_finish")
    refused(lib.pta_clnl_finish(X, n, 0, X, R, R, X, R, None), "pta_clnl_finish")
    refused(lib.pta_clnl_finish(X, n, G, X, R, 0, X, R, None), "pta_clnl_finish")
    refused(lib.pta_clnl_finish(X, n, G, X, R - 1, R, X, R, None), "ld_quad")
    refused(lib.pta_clnl_finish(X, n, G, X, R, R, X, R - 1, None), "ld_g")
    for null in range(3):
        p = [None if i == null else X for i in range(3)]
        refused(lib.pta_clnl_finish(p[0], n, G, p[1], R, R, p[2], R, None), "NULL")
