"""The per-realisation GWB spectrum entry points of the C ABI: declared in include/pta_replicator_amd.h, exported by the library, bound by
the ctypes layer with the declared arity, additive to ABI version 8, and refusing bad arguments with PTA_E_ARG before any device
call.  No GPU."""
import re
import subprocess

from test_abi import declared

SPECTRUM = ("pta_gwb_spectrum_scale_user", "pta_hyper_uniform_field", "pta_os_matched_prior_spec")
PTA_E_ARG = -1
X = 4096   # a non-NULL stand-in: every call below is refused before a pointer is used


def test_symbols_are_declared_exported_and_bound():
    from pta_replicator_amd import _lib
    d = declared()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = set(re.findall(r" T (pta_\w+)", syms))
    for name in SPECTRUM:
        assert name in d and name in exported and name in _lib.EXPORTS, name
        assert len(getattr(_lib.lib, name).argtypes) == d[name], name
    assert _lib.lib.pta_abi_version() == 8
    # appended: what was bound before keeps its place
    assert _lib.EXPORTS[-3:] == SPECTRUM
    assert "pta_gwb_spectrum_scale" in exported and "pta_hyper_uniform" in exported and "pta_os_matched_prior" in exported


def test_argument_errors_without_gpu():
    from pta_replicator_amd import _lib
    lib = _lib.lib
    Nf, M, R = 3000, 14, 8

    def refused(rc, what):
        assert rc == PTA_E_ARG and what in _lib.last_error(), (rc, _lib.last_error())
    # ---- pta_gwb_spectrum_scale_user(seg, dx, dxp, hcf0, Nf, M, R, log10_hc, ld_hc, scale, ld_scale, stream)
    def scale(p=(X,) * 6, Nf_=Nf, M_=M, R_=R, ld_hc=M, ld_scale=Nf):
        return lib.pta_gwb_spectrum_scale_user(p[0], p[1], p[2], p[3], Nf_, M_, R_, p[4], ld_hc, p[5], ld_scale, None)
    for null in range(6):
        refused(scale(tuple(None if i == null else X for i in range(6))), "NULL")
    refused(scale(M_=1, ld_hc=1), "M=1")
    refused(scale(M_=0), "M=0")
    refused(scale(M_=4097, ld_hc=4097), "M=4097")
    refused(scale(ld_hc=M - 1), "ld_hc=13")
    refused(scale(ld_scale=Nf - 1), "ld_scale=2999")
    refused(scale(R_=0), "R=0")
    refused(scale(Nf_=2, ld_scale=2), "Nf=2")
    refused(scale(R_=1 << 20, ld_scale=1 << 12), "too large")
    refused(scale(R_=1 << 20, ld_hc=1 << 12), "too large")
    # ---- pta_hyper_uniform_field(seed, r0, R, n_par, field, lo, hi, out, stream)
    for null in range(3):
        p = [None if i == null else X for i in range(3)]
        refused(lib.pta_hyper_uniform_field(1, 0, R, M, 1, p[0], p[1], p[2], None), "NULL")
    refused(lib.pta_hyper_uniform_field(1, 0, 0, M, 1, X, X, X, None), "R=0")
    refused(lib.pta_hyper_uniform_field(1, 0, R, 0, 1, X, X, X, None), "n_par=0")
    refused(lib.pta_hyper_uniform_field(1, 0, R, M, -1, X, X, X, None), "field=-1")
    refused(lib.pta_hyper_uniform_field(1, 0, R, M, 1 << 24, X, X, X, None), "24-bit")
    refused(lib.pta_hyper_uniform_field(1, 0, 1 << 20, 1 << 11, 1, X, X, X, None), "too large")
    # ---- pta_os_matched_prior_spec(R, P, K_rn, C, rn_f, rn_tspan, rn_phi, rn_log10_A, rn_gamma, T, seg, dx, dxp, M, log10_hc, ld_hc, s, b, stream)
    def prior(R_=R, P=5, K_rn=20, C=10, rn=(X, X, X), th=(X, X), T=4e8, tab=(X, X, X), M_=M, hc=X, ld_hc=M, s=X, b=X):
        return lib.pta_os_matched_prior_spec(R_, P, K_rn, C, rn[0], rn[1], rn[2], th[0], th[1], T, tab[0], tab[1], tab[2], M_, hc, ld_hc, s, b, None)
    for null in range(3):
        refused(prior(tab=tuple(None if i == null else X for i in range(3))), "NULL")
    refused(prior(hc=None), "NULL")
    refused(prior(s=None), "NULL")
    refused(prior(b=None), "NULL")
    refused(prior(M_=1, ld_hc=1), "M=1")
    refused(prior(ld_hc=M - 1), "ld_hc=13")
    refused(prior(R_=0), "R=0")
    refused(prior(C=9), "C=9")
    refused(prior(C=66), "C=66")
    refused(prior(rn=(None, X, X)), "red-noise tables")
    refused(prior(th=(X, None)), "come together")
    refused(prior(T=0.0), "T=0")
    refused(prior(R_=1 << 20, ld_hc=1 << 12), "too large")
