"""The GWB frequency-to-time entry points called directly on the cases of tests/gwb_cases.py, against the long double host reference
of the header's contract and within its derived fp64 bound (tests/gwb_reference.py) at every output: pta_gwb_czt_setup + pta_gwb_czt
in replay and on-chip-draw form, pta_gwb_czt_scaled, pta_gwb_twiddle + pta_gwb_idft, pta_gwb_twiddle_sym + pta_gwb_idft_rng and
pta_gwb_idft_rng_scaled.  The absolute anchor of these kernels: the 1e-12 comparisons of test_gpu_kernels.py and
test_gpu_czt_lean.py hold them to NumPy's fp64 ifft and to one another.

Every call writes into a NaN-filled buffer with one guard row: a NaN inside the window is a failure (the contract reads no bin
outside 1 .. Nf-2, and the scaled cases hold NaN there), anything but NaN outside it is one too.  The four tables of
pta_gwb_czt_setup are checked on their own, and every refusal is asserted as a refusal - the shapes the launchers refuse are never
launched.

Worst |got - ref| / bound measured on the MI355X over every case and variant of a family (1 = at the bound; printed per case,
`pytest -s`, and per family by the last test; DESIGN.md 2 quotes them):
  chirp-z   replay 0.216   on-chip draws 0.181 (both at Nf = 4, npts = 1)   scaled 0.067   rng_fast 0.006 of its own bound
  DFT-GEMM  0.142 (algo 0, Nf = 600, i0 = 3400)   symmetric 0.136   symmetric scaled 0.113   rng_fast 0.006
  FB        0.096 of its share
The same figure for an fp64 NumPy chirp-z on the CPU (tests/test_gwb_reference_host.py) is 0.014 to 0.053; at the large shapes
(Nf = 3000, 3499) the kernels, whose twiddles are chained products, are at 0.021 (variant 1, table twiddles) to 0.031 against
NumPy's 0.018 to 0.022."""
import ctypes

import numpy as np
import pytest

import gwb_cases as gc
from gwb_reference import (C_FFT, FFT_N, HAVE_LONG_DOUBLE, L, TAU, U, bound, chirp_ld, dft4096_ld, unit_ld)

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not HAVE_LONG_DOUBLE, reason="no 80-bit long double on this host")]

CZT = [c["name"] for c in gc.CASES if gc.czt_fits(c)]
PLAIN = [c["name"] for c in gc.CASES if "scale" not in c["extras"]]
SCALED = [c["name"] for c in gc.CASES if "scale" in c["extras"]]
VARIANTS = (0, 1, 25, 10 + 15 + 16, 10 + 15 + 32, 10 + 15 + 64, 137)
IDENTICAL = (25, 10 + 15 + 16, 10 + 15 + 32, 10 + 15 + 64, 137, 0)     # "all steps from 25 up are bit-identical to each other"
LADDER = (11, 13, 17, 18)
LADDER_CASES = {"A-fit4095", "A-nf3-n1", "A-nf4-n2", "B-kf512", "B-kf1024", "C-i0-3400", "D-1024", "D-37", "E-p65", "H-fast"}
WORST = {}


@pytest.fixture(scope="module")
def gpu():
    import torch
    from pta_replicator_amd import _lib, device as dv
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return dict(torch=torch, lib=_lib, dv=dv, s=dv.stream_ptr(), tabs={})


def _note(family, name, frac):
    WORST[family] = max(WORST.get(family, 0.0), frac)
    print(f"{family} {name}: {frac:.3f} of the bound")


def _tables(gpu, c):
    """(sqrtC, [pre, FB, tw, post]) on the device, once per case"""
    if c["name"] not in gpu["tabs"]:
        dv = gpu["dv"]
        sq = dv.f64(gc.operands(c)["sqrtC"])
        tabs = [dv.empty((2 * FFT_N,)), dv.empty((2 * FFT_N,)), dv.empty((2 * FFT_N,)), dv.empty((2 * c["npts"],))]
        gpu["lib"].call("pta_gwb_czt_setup", dv.ptr(sq), c["Nf"], c["npts"], c["i0"], gc.INV_DT, *[dv.ptr(x) for x in tabs], gpu["s"])
        gpu["tabs"][c["name"]] = (sq, tabs)
    return gpu["tabs"][c["name"]]


def _out(gpu, c):
    M = c["R"] * c["P"]
    return gpu["torch"].full((M + 1, c["npts"] + c["pad"]), float("nan"), dtype=gpu["torch"].float64, device="cuda")


def _window(G, c):
    """the [R P, npts] window of a result buffer as NumPy, after checking that nothing else was written and nothing left out"""
    g = G.cpu().numpy()
    M, npts = c["R"] * c["P"], c["npts"]
    assert np.all(np.isnan(g[M])) and np.all(np.isnan(g[:M, npts:])), "a store outside the window"
    assert np.all(np.isfinite(g[:M, :npts])), "an output left unwritten, or a NaN read from a bin the contract never reads"
    return g[:M, :npts]


def _fraction(g, c, res, b):
    rows = list(gc.operands(c)["rows"])
    return float(np.max(np.abs(g[rows].astype(L) - res["ref"]).astype(np.float64) / b))


def _w_device(gpu, c, ldw):
    """the replay rows interleaved (re, im) with row stride ldw >= 2 Nf, NaN in the padding"""
    w = gc.operands(c)["w"]
    M, Nf = c["R"] * c["P"], c["Nf"]
    h = np.full((M, ldw), np.nan)
    h[:, 0:2 * Nf:2], h[:, 1:2 * Nf:2] = w[0], w[1]
    return gpu["dv"].f64(h)


@pytest.mark.parametrize("name", CZT)
def test_chirp_z_replay(gpu, name):
    """pta_gwb_czt with w given: ldw = 2 Nf, or 2 Nf + 6 with NaN behind every row where the case pads; then ldw = 0, one shared row"""
    c = gc.BY_NAME[name]
    dv, lib = gpu["dv"], gpu["lib"]
    res = gc.reference(name, replay=True)
    b = bound(res, "czt", c["Nf"], c["npts"], c["i0"], drawn=False)
    tp = [dv.ptr(x) for x in _tables(gpu, c)[1]]
    ldw = 2 * c["Nf"] + (6 if c["pad"] else 0)
    w_d = _w_device(gpu, c, ldw)
    got = {}
    for v in VARIANTS + (LADDER if name in LADDER_CASES else ()):
        G = _out(gpu, c)
        lib.call("pta_gwb_czt", 0, 0, dv.ptr(w_d), ldw, c["R"], c["P"], c["Nf"], c["npts"], c["i0"], *tp, dv.ptr(G), G.shape[1], v, 0, gpu["s"])
        got[v] = _window(G, c)
        f = _fraction(got[v], c, res, b)
        _note("chirp-z replay", f"{name} variant {v}", f)
        assert f <= 1.0, (name, v, f)
    for v in IDENTICAL:
        assert np.array_equal(got[v], got[25]), (name, v)
    for v in (0, 1):
        G = _out(gpu, c)
        lib.call("pta_gwb_czt", 0, 0, dv.ptr(w_d), 0, c["R"], c["P"], c["Nf"], c["npts"], c["i0"], *tp, dv.ptr(G), G.shape[1], v, 0, gpu["s"])
        g = _window(G, c)
        assert res["ref"].shape[0] >= 1 and gc.operands(c)["rows"][0] == 0
        err = np.abs(g.astype(L) - res["ref"][0][None, :]).astype(np.float64) / b[0][None, :]
        assert float(err.max()) <= 1.0 and np.array_equal(g, np.broadcast_to(g[0], g.shape)), (name, v)


@pytest.mark.parametrize("name", [n for n in CZT if n in PLAIN])
def test_chirp_z_draws_on_chip(gpu, name):
    """pta_gwb_czt with w == NULL against the host's own draws (oracle/philox_ref through a long double Box-Muller)"""
    c = gc.BY_NAME[name]
    dv, lib = gpu["dv"], gpu["lib"]
    fast = gc.operands(c)["fast"]
    res = gc.reference(name)
    b = bound(res, "czt", c["Nf"], c["npts"], c["i0"], drawn=True, fast=fast)
    tp = [dv.ptr(x) for x in _tables(gpu, c)[1]]
    got = {}
    for v in VARIANTS + (LADDER if name in LADDER_CASES else ()):
        G = _out(gpu, c)
        lib.call("pta_gwb_czt", gc.SEED, c["r0"], None, 0, c["R"], c["P"], c["Nf"], c["npts"], c["i0"], *tp, dv.ptr(G), G.shape[1], v, int(fast),
                 gpu["s"])
        got[v] = _window(G, c)
        f = _fraction(got[v], c, res, b)
        _note("chirp-z on-chip rng_fast" if fast else "chirp-z on-chip", f"{name} variant {v}", f)
        assert f <= 1.0, (name, v, f)
    for v in IDENTICAL:
        assert np.array_equal(got[v], got[25]), (name, v)


@pytest.mark.parametrize("name", [n for n in CZT if n in SCALED])
def test_chirp_z_scaled(gpu, name):
    """pta_gwb_czt_scaled, variants 0 and 1: row r P + a takes scale row r, bins 1 .. Nf-2 of it and no other"""
    c = gc.BY_NAME[name]
    dv, lib = gpu["dv"], gpu["lib"]
    op = gc.operands(c)
    res = gc.reference(name)
    b = bound(res, "czt", c["Nf"], c["npts"], c["i0"], drawn=True, scaled=True, fast=op["fast"])
    tp = [dv.ptr(x) for x in _tables(gpu, c)[1]]
    sc = dv.f64(op["scale"])
    for v in (0, 1):
        G = _out(gpu, c)
        lib.call("pta_gwb_czt_scaled", gc.SEED, c["r0"], None, 0, c["R"], c["P"], c["Nf"], c["npts"], c["i0"], *tp, dv.ptr(G), G.shape[1], v,
                 int(op["fast"]), dv.ptr(sc), op["ld_scale"], gpu["s"])
        f = _fraction(_window(G, c), c, res, b)
        _note("chirp-z scaled rng_fast" if op["fast"] else "chirp-z scaled", f"{name} variant {v}", f)
        assert f <= 1.0, (name, v, f)


@pytest.mark.parametrize("name", gc.IDS)
def test_dft_gemm_replay(gpu, name):
    """pta_gwb_twiddle + pta_gwb_idft, algos 0 (VALU) and 1 (MFMA), i0 = 0 included; ldt = npts + 3"""
    c = gc.BY_NAME[name]
    dv, lib = gpu["dv"], gpu["lib"]
    res = gc.reference(name, replay=True)
    b = bound(res, "gemm", c["Nf"], c["npts"], c["i0"], drawn=False)
    Nf, npts, M = c["Nf"], c["npts"], c["R"] * c["P"]
    ldt = npts + 3
    T = gpu["torch"].full((2 * (Nf - 2) + 1, ldt), float("nan"), dtype=gpu["torch"].float64, device="cuda")
    sq = dv.f64(gc.operands(c)["sqrtC"])
    lib.call("pta_gwb_twiddle", dv.ptr(sq), Nf, npts, c["i0"], gc.INV_DT, dv.ptr(T), ldt, gpu["s"])
    t = T.cpu().numpy()
    assert np.all(np.isnan(t[-1])) and np.all(np.isfinite(t[:-1]))
    ldw = 2 * Nf + (6 if c["pad"] else 0)
    w_d = _w_device(gpu, c, ldw)
    for algo in (0, 1):
        G = _out(gpu, c)
        lib.call("pta_gwb_idft", dv.ptr(w_d), ldw, M, Nf, dv.ptr(T), ldt, npts, dv.ptr(G), G.shape[1], algo, gpu["s"])
        f = _fraction(_window(G, c), c, res, b)
        _note("DFT-GEMM", f"{name} algo {algo}", f)
        assert f <= 1.0, (name, algo, f)


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("name", gc.IDS)
def test_symmetric_dft_gemm_draws_on_chip(gpu, name, variant):
    """pta_gwb_twiddle_sym + pta_gwb_idft_rng, or pta_gwb_idft_rng_scaled where the case has a scale: even and odd windows, windows
    that do not fill the last tile of 16 columns, one sample"""
    c = gc.BY_NAME[name]
    dv, lib = gpu["dv"], gpu["lib"]
    op = gc.operands(c)
    scaled = op["scale"] is not None
    res = gc.reference(name)
    b = bound(res, "sym", c["Nf"], c["npts"], c["i0"], drawn=True, scaled=scaled, fast=op["fast"])
    Nf, npts = c["Nf"], c["npts"]
    nrot = ctypes.c_int64(0)
    nsym = lib.lib.pta_gwb_twiddle_sym_size(Nf, npts, variant, ctypes.byref(nrot))
    Tsym, rot = dv.empty((nsym,)), dv.empty((nrot.value,))
    sq = dv.f64(op["sqrtC"])
    lib.call("pta_gwb_twiddle_sym", dv.ptr(sq), Nf, npts, c["i0"], gc.INV_DT, dv.ptr(Tsym), dv.ptr(rot), variant, gpu["s"])
    G = _out(gpu, c)
    if scaled:
        sc = dv.f64(op["scale"])
        lib.call("pta_gwb_idft_rng_scaled", gc.SEED, c["r0"], c["R"], c["P"], Nf, dv.ptr(Tsym), dv.ptr(rot), npts, dv.ptr(G), G.shape[1],
                 variant, int(op["fast"]), dv.ptr(sc), op["ld_scale"], gpu["s"])
    else:
        lib.call("pta_gwb_idft_rng", gc.SEED, c["r0"], c["R"], c["P"], Nf, dv.ptr(Tsym), dv.ptr(rot), npts, dv.ptr(G), G.shape[1], variant,
                 int(op["fast"]), gpu["s"])
    f = _fraction(_window(G, c), c, res, b)
    _note("symmetric DFT-GEMM" + (" scaled" if scaled else "") + (" rng_fast" if op["fast"] else ""), f"{name} variant {variant}", f)
    assert f <= 1.0, (name, variant, f)


def _rev8(m):
    """the frequency a radix-8 decimation-in-frequency transform of 4096 points leaves at position m: its four octal digits reversed"""
    return ((m & 7) << 9) | (((m >> 3) & 7) << 6) | (((m >> 6) & 7) << 3) | ((m >> 9) & 7)


@pytest.mark.parametrize("name", ["A-fit4095", "A-nf3-n1", "A-nf4-n2", "B-kf512", "C-i0-3400", "C-i0-above-kf", "D-1025", "C-i0-1"])
def test_chirp_z_tables(gpu, name):
    """tw, pre, post entry by entry against long double, at the figures of the bound's derivation: an entry of unit modulus from an
    exact argument within 3 u, from a rounded one within TAU u, one more u per product; FB, the chirp's spectrum / 4096 in the
    [q][b] slot order of the header (logical position 8 b + q of the digit-reversed spectrum at slot q 512 + b), within the
    per-element share of the norm-wise (TAU + C_FFT) u || chirp ||_2 / 64, over 64 again, against the long double DFT by the definition"""
    c = gc.BY_NAME[name]
    Nf, npts, i0 = c["Nf"], c["npts"], c["i0"]
    n, Kf = 2 * Nf - 2, Nf - 2
    sqrtC = gc.operands(c)["sqrtC"]
    pre, FB, tw, post = (x.cpu().numpy().reshape(-1, 2) for x in _tables(gpu, c)[1])
    cs, sn = unit_ld(2 * np.arange(FFT_N), FFT_N)
    assert np.max(np.hypot((tw[:, 0] - cs).astype(np.float64), (tw[:, 1] + sn).astype(np.float64))) <= 3 * U
    k = np.arange(1, Kf + 1, dtype=np.int64)
    pc, ps = unit_ld(k * k, n)
    err = np.hypot((pre[:Kf, 0] - sqrtC[k] * pc).astype(np.float64), (pre[:Kf, 1] - sqrtC[k] * ps).astype(np.float64))
    assert np.max(err / sqrtC[k]) <= (TAU + 1) * U and np.all(pre[Kf:] == 0.0)
    j = i0 + np.arange(npts, dtype=np.int64)
    qc, qs = unit_ld(j * j, n)
    amp = L(2) * L(gc.INV_DT) / L(n)
    err = np.hypot((post[:, 0] - amp * qc).astype(np.float64), (post[:, 1] - amp * qs).astype(np.float64))
    assert np.max(err) / float(amp) <= (TAU + 2) * U
    lo = min(i0 - Kf, 0)      # the header: FB holds the lags from min(i0 - Kf, 0) on (with i0 > Kf more than the window needs)
    br, bi = chirp_ld(Nf, npts, i0, lo=lo)
    Xr, Xi = dft4096_ld(br, bi)
    m = np.arange(FFT_N)
    slot = (m & 7) * (FFT_N // 8) + (m >> 3)
    f = _rev8(m)
    err = np.hypot((FB[slot, 0] - Xr[f] / FFT_N).astype(np.float64), (FB[slot, 1] - Xi[f] / FFT_N).astype(np.float64))
    share = (TAU + C_FFT) * U * np.sqrt(float(i0 + npts - 1 - lo)) / FFT_N
    frac = float(np.max(err) / share)
    _note("chirp spectrum table", name, frac)
    assert frac <= 1.0


def test_refusals_without_a_launch(gpu):
    """every shape or argument the launchers must refuse comes back as PTA_E_ARG, with the output buffer untouched"""
    dv, lib, raw = gpu["dv"], gpu["lib"], gpu["lib"].lib
    assert (raw.pta_gwb_czt_fits(600, 600, 3600), raw.pta_gwb_czt_fits(3499, 600, 10), raw.pta_gwb_czt_fits(3500, 600, 10)) == (0, 1, 0)
    assert (raw.pta_gwb_czt_fits(600, 600, 3498), raw.pta_gwb_czt_fits(600, 600, 3497), raw.pta_gwb_czt_fits(600, 600, 0)) == (0, 1, 0)
    sq = dv.f64(np.ones(3600))
    tabs = [dv.zeros((2 * FFT_N,)), dv.zeros((2 * FFT_N,)), dv.zeros((2 * FFT_N,)), dv.zeros((2 * 600,))]
    tp = [dv.ptr(x) for x in tabs]
    G = gpu["torch"].full((6, 600), float("nan"), dtype=gpu["torch"].float64, device="cuda")
    w = dv.zeros((6, 2 * 3500))
    sc = dv.f64(np.ones((2, 3600)))
    E_ARG = -1
    for Nf, npts, i0 in ((600, 600, 3600), (600, 600, 3498), (3500, 600, 10), (600, 600, 0)):
        assert raw.pta_gwb_czt_setup(dv.ptr(sq), Nf, npts, i0, gc.INV_DT, *tp, gpu["s"]) == E_ARG
        assert "does not fit" in lib.last_error()
        assert raw.pta_gwb_czt(1, 0, None, 0, 2, 3, Nf, npts, i0, *tp, dv.ptr(G), 600, 0, 0, gpu["s"]) == E_ARG
        assert raw.pta_gwb_czt(1, 0, dv.ptr(w), 2 * Nf, 2, 3, Nf, npts, i0, *tp, dv.ptr(G), 600, 0, 0, gpu["s"]) == E_ARG
        assert raw.pta_gwb_czt_scaled(1, 0, None, 0, 2, 3, Nf, npts, i0, *tp, dv.ptr(G), 600, 0, 0, dv.ptr(sc), 3600, gpu["s"]) == E_ARG
    Nf, npts, i0 = 601, 600, 10
    assert raw.pta_gwb_czt_scaled(1, 0, None, 0, 2, 3, Nf, npts, i0, *tp, dv.ptr(G), 600, 0, 0, dv.ptr(sc), Nf - 2, gpu["s"]) == E_ARG
    assert raw.pta_gwb_czt_scaled(1, 0, dv.ptr(w), 2 * Nf, 2, 3, Nf, npts, i0, *tp, dv.ptr(G), 600, 0, 0, dv.ptr(sc), Nf, gpu["s"]) == E_ARG
    assert raw.pta_gwb_czt_scaled(1, 0, None, 0, 2, 3, Nf, npts, i0, *tp, dv.ptr(G), 600, 25, 0, dv.ptr(sc), Nf, gpu["s"]) == E_ARG
    for v in (2, 9, 12, 26, 138, -1):
        assert raw.pta_gwb_czt(1, 0, None, 0, 2, 3, Nf, npts, i0, *tp, dv.ptr(G), 600, v, 0, gpu["s"]) == E_ARG, v
    assert raw.pta_gwb_czt(1, 0, dv.ptr(w), 2 * Nf - 1, 2, 3, Nf, npts, i0, *tp, dv.ptr(G), 600, 0, 0, gpu["s"]) == E_ARG
    assert raw.pta_gwb_czt(1, 0, None, 0, 2, 3, Nf, npts, i0, *tp, dv.ptr(G), 599, 0, 0, gpu["s"]) == E_ARG
    nrot = ctypes.c_int64(0)
    nsym = raw.pta_gwb_twiddle_sym_size(Nf, npts, 1, ctypes.byref(nrot))
    Tsym, rot = dv.zeros((nsym,)), dv.zeros((nrot.value,))
    assert raw.pta_gwb_idft_rng_scaled(1, 0, 2, 3, Nf, dv.ptr(Tsym), dv.ptr(rot), npts, dv.ptr(G), 600, 1, 0, dv.ptr(sc), Nf - 2, gpu["s"]) == E_ARG
    assert raw.pta_gwb_idft_rng_scaled(1, 0, 2, 3, Nf, dv.ptr(Tsym), dv.ptr(rot), npts, dv.ptr(G), 600, 1, 0, None, Nf, gpu["s"]) == E_ARG
    gpu["torch"].cuda.synchronize()
    assert bool(gpu["torch"].isnan(G).all())


def test_worst_fractions_are_reported():
    """(last in the file) the figures DESIGN.md quotes"""
    for family in sorted(WORST):
        print(f"worst fraction of the bound, {family}: {WORST[family]:.3f}")
