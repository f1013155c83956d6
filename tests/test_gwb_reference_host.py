"""The long double reference of the GWB frequency-to-time stage (tests/gwb_reference.py) and its derived bound, on the CPU, before any
kernel is trusted to them.  On every case of tests/gwb_cases.py:

  * an fp64 NumPy evaluation of the chirp-z algebra - pre-chirp, zero-padded 4096-point FFT, product with the FFT of the wrapped
    chirp, inverse FFT, post-chirp, with correctly rounded tables and libm deviates - stays inside the chirp-z bound, and so does
    the fp64 Hermitian-packed ifft of oracle.pta_oracle.gwb_time_series; a plain fp64 matrix product stays inside the DFT-GEMM
    bound.  The worst fraction per case is printed (pytest -s; 0.014 to 0.053 for the chirp-z evaluation, 0.011 to 0.056 for the
    ifft, 0.027 to 0.148 for the matrix product) and asserted: none above 0.5 - a bound filled to more than a half is no bound for a
    kernel with more roundings than NumPy's - and the better of the two transforms at 0.01 or more - one filled to less than a
    hundredth sees nothing.
  * each of fourteen deliberately wrong evaluations, and one table entry perturbed by 1e-13, leaves the bound by a stated factor at
    some output of every case that exercises it.

Which cases exercise which defect (EXERCISES below is the machine-readable form):
  every case: wrap_low, wrap_high (the chirp's lowest and highest lag dropped: outputs 0 and npts - 1 lose bins Kf and 1),
      window_start (i0 - 1 for i0), bin_shift (bin k + 1 for k), dc_kept, nyquist_kept, factor_2, imag_sign, post_conj, table_1e-13
  cases that draw with P >= 2: stream_swap (pulsar a ^ 1 where it exists);  every case that draws: pair_shift (pair k - 1 for bin k)
  cases with r0 >= 2^32: counter_32 (the high word of the realisation dropped)
  scaled cases: scale_col (column k - 1 for k); scaled cases with P >= 2: scale_row (row in place of row // P, modulo R)

THE FACTORS.  sqrtC, the draws and the scale are O(1) against each other, so a wrong term moves an output by a fraction 1 / sqrt(Kf)
of A2 or more against a bound of 2e-13 A2 at most: FACTOR = 1e6 leaves five orders in hand at Kf = 3497 and is a condition on the
operands, not a tolerance.  Under rng_fast the bound is 2e-5 sqrt 2 A1, A1 = amp sum_k |sqrtC_k s_k| near 0.9 sqrt(Kf) A2.  A defect
that changes a whole row moves an output by about A2 and cannot leave that bound by more than about 4e4 / sqrt(Kf), 1600 at Kf = 599
(the largest rng_fast case): FACTOR_FAST = 1e2 keeps one order in hand.  A defect of ONE bin in one output (BIN_DEFECTS: the chirp's
wrap, DC, Nyquist) moves it by |a_k|, or half of it, against a bound Kf bins wide: 0.5 |w_k| / (2.8e-5 Kf) = 30 |w_k| at Kf = 599 -
FACTOR_FAST_BIN = 10 is what a draw of a third of a standard deviation still reaches.
table_1e-13 perturbs ONE post-chirp entry by 1e-13 relative, the entry of the largest |G0| of row 0: it moves that output by
1e-13 |G0|, and the bound there is u (c kappa A2 + 13.3 vmod) with |G0| about 3 A2 at the maximum over a long window - a ratio of
5 at best.  Its factor is computed from the bound: the perturbed evaluation must miss by at least 1e-13 |G0| / bound - 0.5 (the
honest evaluation's own error, at most half the bound, may cancel that much) and that figure must exceed TABLE_MIN = 1.5.  31 of
the 36 cases chirp-z accepts reach it; rng_fast does not, nor a two-sample window whose |G0| is small against A2.  A single perturbed entry of the pre-chirp or of the convolution
chirp moves an output by 1e-13 |a_k| = 1e-13 A2 / sqrt(Kf), below every honest evaluation's rounding: no bound can see it.

At most SKIP_SHARE of the (case, defect) pairs may be skipped, and every defect is caught by two cases or more."""
import numpy as np
import pytest

import gwb_cases as gc
from gwb_reference import FFT_N, HAVE_LONG_DOUBLE, L, bound, chirp_ld, drawn_w, unit_ld
from oracle import pta_oracle as po

pytestmark = pytest.mark.skipif(not HAVE_LONG_DOUBLE, reason="no 80-bit long double on this host")

FACTOR, FACTOR_FAST, FACTOR_FAST_BIN, TABLE_MIN, SKIP_SHARE = 1e6, 1e2, 10.0, 1.5, 0.35
BIN_DEFECTS = {"wrap_low", "wrap_high", "dc_kept", "nyquist_kept"}


def _operands(c, defect=None):
    """(sqrtC s)[rows, Nf] and w[rows, Nf] complex, in fp64, as the case draws them; the defects of the operands applied"""
    op = gc.operands(c)
    Nf, P, R, rows = c["Nf"], c["P"], c["R"], np.array(op["rows"])
    r0 = c["r0"] & 0xFFFFFFFF if defect == "counter_32" else c["r0"]
    draw_rows = [(row // P) * P + ((row % P) ^ 1 if ((row % P) ^ 1) < P else row % P) for row in rows] if defect == "stream_swap" else rows
    re, im = drawn_w(gc.SEED, r0, [int(r) for r in draw_rows], P, Nf, "fast" if op["fast"] else "f64")
    w = re + 1j * im
    if defect == "pair_shift":
        w = np.roll(w, 1, axis=1)
    amp = np.broadcast_to(op["sqrtC"], w.shape).copy()
    if op["scale"] is not None:
        srow = rows % R if defect == "scale_row" else rows // P
        s = np.ones((len(rows), Nf))
        s[:, 1:Nf - 1] = op["scale"][srow][:, 0:Nf - 2] if defect == "scale_col" else op["scale"][srow][:, 1:Nf - 1]
        s[:, 0] = s[:, Nf - 1] = 1.0      # (the contract reads neither; dc_kept and nyquist_kept need a finite value there)
        amp *= s
    return amp, w


def emulate_czt(c, defect=None, table_at=None):
    """G0[rows, npts] by the chirp-z algebra in fp64 NumPy"""
    Nf, npts, i0 = c["Nf"], c["npts"], c["i0"]
    n, Kf = 2 * Nf - 2, Nf - 2
    amp_k, w = _operands(c, defect)
    if defect == "imag_sign":
        w = np.conj(w)
    k = np.arange(1, Kf + 1, dtype=np.int64)
    kk = k + 1 if defect == "bin_shift" else k
    pc, ps = unit_ld(k * k, n)
    y = np.zeros((w.shape[0], FFT_N), dtype=complex)
    y[:, :Kf] = (amp_k[:, kk] * w[:, kk]) * (pc.astype(np.float64) + 1j * ps.astype(np.float64))
    lo, hi = i0 - Kf + (defect == "wrap_low"), i0 + npts - 2 - (defect == "wrap_high")
    br, bi = chirp_ld(Nf, npts, i0)
    b = br.astype(np.float64) + 1j * bi.astype(np.float64)
    keep = np.zeros(FFT_N, dtype=bool)
    keep[np.arange(lo, hi + 1) % FFT_N] = True
    b[~keep] = 0.0
    conv = np.fft.ifft(np.fft.fft(y, axis=1) * np.fft.fft(b)[None, :], axis=1)
    j = i0 + np.arange(npts, dtype=np.int64)
    qc, qs = unit_ld(j * j, n)
    a = 2.0 * gc.INV_DT / n
    if defect == "factor_2":
        a = gc.INV_DT / n
    post = a * qc.astype(np.float64) + 1j * (a * qs.astype(np.float64))
    if defect == "post_conj":
        post = np.conj(post)
    if defect == "table_1e-13":
        post[table_at] *= 1.0 + 1e-13
    start = i0 - 1 - (defect == "window_start")
    G = np.real(conv[:, (start + np.arange(npts)) % FFT_N] * post[None, :])
    if defect == "dc_kept":          # the Hermitian-packed spectrum's bin 0: 1 / (n dt) Re a_0
        G = G + (gc.INV_DT / n) * np.real(amp_k[:, 0] * w[:, 0])[:, None]
    if defect == "nyquist_kept":     # and bin Nf - 1: (-1)^j / (n dt) Re a_{Nf - 1}
        G = G + (gc.INV_DT / n) * np.real(amp_k[:, -1] * w[:, -1])[:, None] * np.where(j % 2, -1.0, 1.0)[None, :]
    return G


def hermitian_ifft(c):
    Nf, npts, i0 = c["Nf"], c["npts"], c["i0"]
    amp_k, w = _operands(c)
    Res_f = amp_k * w
    Res_f[:, 0] = 0
    Res_f[:, -1] = 0
    return po.gwb_time_series(Res_f, gc.DT)[:, (i0 + np.arange(npts)) % (2 * Nf - 2)]


def dft_gemm(c):
    Nf, npts, i0 = c["Nf"], c["npts"], c["i0"]
    n, Kf = 2 * Nf - 2, Nf - 2
    amp_k, w = _operands(c)
    k = np.arange(1, Kf + 1, dtype=np.int64)
    ct, st = unit_ld(2 * ((k[:, None] * (i0 + np.arange(npts, dtype=np.int64))[None, :]) % n), n)
    ct, st = ct.astype(np.float64), st.astype(np.float64)
    return (2.0 * gc.INV_DT / n) * ((amp_k[:, k] * w.real[:, k]) @ ct - (amp_k[:, k] * w.imag[:, k]) @ st)


def excess(G, res, b):
    """max |G - ref| / bound; inf where a value is missing (the contract reads no NaN, so a NaN is a failure)"""
    assert G.shape == res["ref"].shape
    if not np.all(np.isfinite(G)):
        return np.inf
    return float(np.max(np.abs(G.astype(L) - res["ref"]).astype(np.float64) / b))


EXERCISES = {
    "wrap_low": lambda c: True, "wrap_high": lambda c: True, "window_start": lambda c: True, "bin_shift": lambda c: True,
    "dc_kept": lambda c: True, "nyquist_kept": lambda c: True, "factor_2": lambda c: True, "imag_sign": lambda c: True,
    "post_conj": lambda c: True,
    "scale_row": lambda c: "scale" in c["extras"] and c["P"] >= 2,
    "scale_col": lambda c: "scale" in c["extras"],
    "stream_swap": lambda c: c["P"] >= 2,
    "counter_32": lambda c: c["r0"] >= 2 ** 32,
    "pair_shift": lambda c: True,
}
CZT_CASES = [c for c in gc.CASES if gc.czt_fits(c)]


def test_the_cases_are_the_ones_asked_for():
    c = gc.BY_NAME
    edge = lambda x: x["Nf"] - 2 + x["npts"] - 2
    assert edge(c["A-fit4095"]) == 4095 and gc.czt_fits(c["A-fit4095"]) and not gc.czt_fits(dict(c["A-fit4095"], Nf=3500))
    assert not gc.czt_fits(dict(Nf=600, npts=600, i0=3600)) and gc.czt_fits(c["C-i0-3400"]) and not gc.czt_fits(c["C-i0-0"])
    assert {(x["Nf"], x["npts"]) for x in gc.CASES} >= {(3, 1), (3, 2), (4, 1), (4, 2)}
    assert {x["Nf"] - 2 for x in gc.CASES} >= {511, 512, 513, 1024, 1025}
    assert {x["i0"] for x in gc.CASES} >= {0, 1, 2, 10, 3400} and c["C-i0-above-kf"]["i0"] > c["C-i0-above-kf"]["Nf"] - 2
    for i0 in (1, 10):
        assert {x["i0"] - 2 + x["npts"] for x in gc.CASES if x["i0"] == i0} >= {1023, 1024, 1025}
    assert {x["npts"] for x in gc.CASES if x["i0"] == 1} >= {1015, 1016}
    assert c["D-above"]["i0"] - 1 >= 1024 and {x["P"] for x in gc.CASES} >= {1, 3, 65}
    assert all(x["R"] * x["P"] <= 12 or x["Nf"] <= 50 for x in gc.CASES) and all(len(gc.operands(x)["rows"]) <= 12 for x in gc.CASES)
    assert sum(x["r0"] >= 2 ** 32 for x in gc.CASES) >= 4 and sum(x["pad"] == 5 for x in gc.CASES) >= 8
    sc = [x for x in gc.CASES if "scale" in x["extras"]]
    assert all(x["R"] >= 3 for x in sc) and {x["extras"]["scale"] for x in sc} == {-1, 3}
    for x in sc:
        s = gc.operands(x)["scale"]
        assert np.all(np.isnan(s[:, 0])) and np.all(np.isnan(s[:, x["Nf"] - 1:])) and np.all(np.isfinite(s[:, 1:x["Nf"] - 1]))
        assert all(np.median(np.abs(s[r, 1:x["Nf"] - 1] / s[0, 1:x["Nf"] - 1] - 1)) > 0.2 for r in range(1, x["R"]))      # visibly different rows
    fast = [x for x in gc.CASES if x["extras"].get("fast")]
    assert sum("scale" in x["extras"] for x in fast) >= 2 and sum("scale" not in x["extras"] for x in fast) >= 2
    seen = {m: sum(bool(on(x)) for x in CZT_CASES) for m, on in EXERCISES.items()}
    assert all(v >= 2 for v in seen.values()), seen
    skipped = sum(not on(x) for x in CZT_CASES for on in EXERCISES.values())
    assert skipped <= SKIP_SHARE * len(CZT_CASES) * len(EXERCISES), skipped


_table_caught = []


@pytest.mark.parametrize("name", gc.IDS)
def test_fp64_passes_and_every_defect_fails(name):
    c = gc.BY_NAME[name]
    op = gc.operands(c)
    res = gc.reference(name)
    shape = (c["Nf"], c["npts"], c["i0"])
    scaled = op["scale"] is not None
    bg = bound(res, "gemm", *shape, drawn=True, scaled=scaled, fast=op["fast"])
    g = excess(dft_gemm(c), res, bg)
    if not gc.czt_fits(c):
        print(f"{name}: fp64 matrix product at {g:.3f} of the DFT-GEMM bound (chirp-z refuses the shape)")
        assert g <= 0.5
        return
    bz = bound(res, "czt", *shape, drawn=True, scaled=scaled, fast=op["fast"])
    z, h = excess(emulate_czt(c), res, bz), excess(hermitian_ifft(c), res, bz)
    print(f"{name}: fp64 chirp-z at {z:.3f}, Hermitian ifft at {h:.3f} of the chirp-z bound; matrix product at {g:.3f} of the DFT-GEMM bound")
    lo = 0.0 if op["fast"] else 0.01      # rng_fast: emulation and reference share the fp32 deviates, nothing fills 2e-5
    assert lo <= max(z, h) and z <= 0.5 and h <= 0.5 and g <= 0.5
    for m, on in EXERCISES.items():
        if on(c):
            factor = (FACTOR_FAST_BIN if m in BIN_DEFECTS else FACTOR_FAST) if op["fast"] else FACTOR
            x = excess(emulate_czt(c, m), res, bz)
            print(f"    {m}: {x:.3g}")
            assert x >= factor, (m, x)
    at = int(np.argmax(np.abs(res["ref"][0])))
    want = float(1e-13 * np.abs(res["ref"][0, at]) / bz[0, at]) - 0.5
    if want >= TABLE_MIN:
        x = excess(emulate_czt(c, "table_1e-13", table_at=at), res, bz)
        print(f"    table_1e-13: {x:.3g} (at least {want:.3g})")
        assert x >= want
        _table_caught.append(name)


def test_the_table_perturbation_is_caught_often_enough():
    """(after the cases above, in file order) two cases or more, as for every other defect"""
    if len(_table_caught) < 2:
        for c in CZT_CASES:      # run on its own: redo the count
            res = gc.reference(c["name"])
            op = gc.operands(c)
            bz = bound(res, "czt", c["Nf"], c["npts"], c["i0"], drawn=True, scaled=op["scale"] is not None, fast=op["fast"])
            at = int(np.argmax(np.abs(res["ref"][0])))
            if float(1e-13 * np.abs(res["ref"][0, at]) / bz[0, at]) - 0.5 >= TABLE_MIN and c["name"] not in _table_caught:
                _table_caught.append(c["name"])
    print("table_1e-13 is held to its factor in", len(_table_caught), "cases:", _table_caught)
    assert len(_table_caught) >= 2
