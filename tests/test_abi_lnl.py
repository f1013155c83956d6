"""The likelihood entry points of the C ABI: declared in include/pta_replicator_amd.h, exported by the library, bound by the ctypes
layer with the declared arity, additive to ABI version 8, and refusing bad arguments with PTA_E_ARG before any device call.  No GPU."""
import re
import subprocess

from test_abi import declared

LNL = ("pta_lnl_quad", "pta_lnl_factor", "pta_lnl_apply", "pta_lnl_reduce")
PTA_E_ARG = -1
X = 4096   # a non-NULL stand-in: every call below is refused before a pointer is used


def test_symbols_are_declared_exported_and_bound():
    from pta_replicator_amd import _lib
    d = declared()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = set(re.findall(r" T (pta_\w+)", syms))
    for name in LNL:
        assert name in d and name in exported and name in _lib.EXPORTS, name
        assert len(getattr(_lib.lib, name).argtypes) == d[name], name
    assert _lib.lib.pta_abi_version() == 8
    assert _lib.LNL_KMAX == 128


def test_argument_errors_without_gpu():
    from pta_replicator_amd import _lib
    lib = _lib.lib
    P, K, C, G, R = 2, 40, 12, 3, 5

    def refused(rc, what):
        assert rc == PTA_E_ARG and what in _lib.last_error(), (rc, _lib.last_error())
    # K > 128, C > K, NULL operands
    refused(lib.pta_lnl_factor(X, P, 129, C, G, X, X, X, None), "pta_lnl_factor")
    refused(lib.pta_lnl_factor(X, P, K, K + 1, G, X, X, X, None), "pta_lnl_factor")
    refused(lib.pta_lnl_factor(X, P, 0, 0, G, X, X, X, None), "pta_lnl_factor")
    refused(lib.pta_lnl_factor(X, P, K, C, 0, X, X, X, None), "pta_lnl_factor")
    for null in range(4):
        ptrs = [None if i == null else X for i in range(4)]
        refused(lib.pta_lnl_factor(ptrs[0], P, K, C, G, ptrs[1], ptrs[2], ptrs[3], None), "NULL")
    refused(lib.pta_lnl_apply(X, X, X, P, 129, C, G, X, P * 132, 64, 132, R, X, X, X, X, P * R, R, None), "pta_lnl_apply")
    refused(lib.pta_lnl_apply(X, X, X, P, K, K + 1, G, X, P * 43, 64, 43, R, X, X, X, X, P * R, R, None), "pta_lnl_apply")
    refused(lib.pta_lnl_apply(X, X, X, P, K, C, G, X, P * 43 - 1, 64, 43, R, X, X, X, X, P * R, R, None), "ld_q")
    refused(lib.pta_lnl_apply(X, X, X, P, K, C, G, X, P * 43, 64, 43, R, X, X, X, X, P * R, R - 1, None), "ld_a")
    refused(lib.pta_lnl_apply(X, X, X, P, K, C, G, X, P * 43, 64, K - 1, R, X, X, X, X, P * R, R, None), "Kt")
    for null in range(8):
        p = [None if i == null else X for i in range(8)]
        refused(lib.pta_lnl_apply(p[0], p[1], p[7], P, K, C, G, p[2], P * 43, 64, 43, R, p[3], p[4], p[5], p[6], P * R, R, None), "NULL")
    refused(lib.pta_lnl_quad(X, 100, R, X, P, X, None, None, None, None, X, P * 132, 64, 129, 3, X, 100, X, None), "pta_lnl_quad")
    refused(lib.pta_lnl_quad(X, 100, R, X, P, X, None, None, None, None, X, P * 43, 64, K, 17, X, 100, X, None), "pta_lnl_quad")
    refused(lib.pta_lnl_quad(X, 100, R, X, P, X, None, None, None, None, None, 0, 64, K, 3, X, 100, X, None), "timing-model rows")
    refused(lib.pta_lnl_quad(X, 100, R, X, P, X, None, None, None, None, X, P * 43, 64, K, 3, None, 100, X, None), "timing-model rows")
    refused(lib.pta_lnl_quad(X, 100, R, X, P, X, X, None, X, X, X, P * 43, 64, K, 3, X, 100, X, None), "epoch lists")
    refused(lib.pta_lnl_quad(None, 100, R, X, P, X, None, None, None, None, X, P * 43, 64, K, 3, X, 100, X, None), "NULL")
    refused(lib.pta_lnl_quad(X, 100, R, X, P, X, None, None, None, None, X, P * 43, 64, K, 3, X, 100, None, None), "NULL")
    refused(lib.pta_lnl_reduce(None, P * R, R, P, G, R, X, R, None), "NULL")
    refused(lib.pta_lnl_reduce(X, P * R, R - 1, P, G, R, X, R, None), "pta_lnl_reduce")
    refused(lib.pta_lnl_reduce(X, P * R, R, P, G, R, X, R - 1, None), "pta_lnl_reduce")
