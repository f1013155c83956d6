"""Host reference of the GWB frequency-to-time stage (pta_gwb_czt, pta_gwb_czt_scaled, pta_gwb_twiddle + pta_gwb_idft,
pta_gwb_twiddle_sym + pta_gwb_idft_rng, pta_gwb_idft_rng_scaled), evaluated in 80-bit long double from the contract in
include/pta_replicator_amd.h (the block above pta_gwb_twiddle, the chirp-z comment, the per-realisation spectrum) - test
infrastructure, not product code, and not a transcription of any kernel: a direct sum, no chirp, no FFT, no symmetry.

    G0[row, jj] = amp sum_{k=1}^{Nf-2} sqrtC[k] s[row // P, k] (Re w[row, k] cos(2 pi q / n) - Im w[row, k] sin(2 pi q / n))
    n = 2 Nf - 2,  amp = 2 / (n dt),  q = (k (i0 + jj)) mod n in integers,  s = 1 without a scale

w comes from the caller (replay) or is drawn: row = r P + a takes pair k of stream (GWB, a) of realisation r0 + r as (Re, Im) of bin k
(header: "pair k -> (Re, Im) of w[a,k]"; tests/helpers.host_draws builds w[a, :] from pairs 0 .. Nf-1 in order), the Philox uniforms
of oracle/philox_ref.py pushed through synth_reference's long double Box-Muller (rng_fast: philox_ref's fp32 twin).  pi is a decimal
string: numpy.pi is the fp64 one.

Next to the value the reference returns what the bound is made of: with a_k = sqrtC_k s_k w_k (complex) and v_jj = sum_k a_k e^{+i theta},
    vmod = amp |v_jj|  (G0 = amp Re v_jj),    A2 = amp ||a||_2,    A1 = amp sum_k |sqrtC_k s_k|.

THE BOUND.  u = 2^-53.  It is derived for a class of fp64 evaluations, not fitted to a kernel, and it has two kinds of terms:
  (e) element-wise and rigorous - what multiplies one output only;
  (n) the per-element share of a rigorous NORM-wise bound.  A 4096-point convolution by FFT, or a sum of 2 Kf products, cancels: the
      outputs are of order A2 while sum_k |a_k| is sqrt(Kf) larger, and an element-wise worst case (all roundings aligned in one output)
      is larger by that factor again - sqrt(4096) = 64 for the convolution, up to 84 for the sum.  Such a bound holds trivially and
      sees nothing.  What holds rigorously is the norm: || error ||_2 <= C u || result ||_2 over the 4096 outputs of the convolution
      (Higham, ASNA, Thm 24.2, carried through the three transforms), with C the LINEAR sum of every stage's worst case.  The bound
      charges each output C u times the rms output - its equal share.  This is not a theorem per element: it fails if the roundings
      are at their worst cases AND concentrate in few outputs.  The margin against the spread over elements is that C adds worst cases
      linearly where roundings of different stages add in quadrature at a third of them; tests/test_gwb_reference_host.py measures
      how much of the bound an honest fp64 evaluation fills (0.014 to 0.053 chirp-z, 0.027 to 0.148 matrix product) and holds seeded
      defects to the factor by which they must miss it.
A table entry e^{i pi x} from sincospi(x) of a quotient of exact integers, x < 2: x rounds once, |d angle| <= 2 pi u, each component
within one ulp <= 2 u, |d entry| <= TAU u with TAU = 2 pi + 3.  A complex product with FMA: 2 u (Jeannerod et al. 2017).

Chirp-z (pre-chirp, 4096-point FFT, product with the chirp's spectrum, inverse FFT, post-chirp):
  input     (n) s w (1), sqrtC x table (1), table (TAU), complex product (2):                         C_IN = TAU + 4
                drawn on chip, the deviate is within 6 ulp <= 12 u of the long double one (the project's own assertion,
                test_device_deviates_within_a_few_ulp_of_an_80_bit_box_muller):                        + 12
  one FFT   (n) a radix-8 pass: three levels of sums (3), the odd branch's 1/sqrt 2 (2), the twiddle product (2) and the twiddle
                itself, the worst of a set built from one table entry (3: exact argument) by squarings and products - w2 8, w4 18,
                w3 13, w7 = w3 w4 33: 40 per pass with twiddles, 5 for the last, four passes:          C_FFT = 125
  spectrum  (n) of the chirp: table + one FFT (the 1/4096 is exact):                                   TAU + C_FFT
  product   (n)                                                                                         2
  post      (e) table (TAU), amp = 2 inv_dt / n (1), amp x table (1), the product's real part (2):    C_POST = TAU + 4, on vmod
  The norm of the convolution is at most kappa sqrt(4096) ||a||_2 with kappa = max |DFT(chirp)| / 64 (1.2 to 1.5 for the large
  shapes, below 0.1 for Nf = 3), so the (n) terms of the transforms carry kappa; the input's share carries max(1, kappa), which is
  the element-wise truth when one bin is all there is:
      bound = u ((C_IN [+ 12]) max(1, kappa) + (3 C_FFT + TAU + 2) kappa) A2 + u C_POST vmod

DFT as a GEMM (a table T of amp sqrtC_k (cos, -sin), then 2 Kf products accumulated in fp64 in some order):
  table     (n) entry (TAU), amp_k (2), amp_k x entry (1) [+ 1 scale, + 12 drawn]:                     C_T = TAU + 3
  symmetric (n) form only: the rotation of the draw, table (TAU) and product (2);  (e) the last e -+ o (1), on vmod
  sum       (n) N = 2 Kf additions, each within u of a partial sum.  The partial sums are sums of independent draws times bounded
                factors, of mean square at most A2^2; N roundings |d_i| <= u of mean zero (Higham and Mary 2019) then give, by
                Hoeffding, |error| <= LAMBDA u sqrt(N) A2 except with probability 2 exp(-LAMBDA^2 / 2) = 5e-11 per output at
                LAMBDA = 7, 1e-4 over the million outputs of the suite - whatever the order of summation.
      bound = u (C_T [+ 1] [+ 12] [+ TAU + 2] + 7 sqrt(2 Kf)) A2 [+ u vmod]

rng_fast = 1 replaces the deviates' 12 u by the 2e-5 per component that synth_reference carries (test_fast_rng_math_mode), worst
case over the bins as there: 2e-5 sqrt 2 A1."""
import functools

import numpy as np

from oracle import philox_ref
from synth_reference import HAVE_LONG_DOUBLE, L, U, deviate_pairs  # noqa: F401  (re-exported)

PI = L("3.14159265358979323846264338327950288419716939937510")
FFT_N = 4096
TAU = 2 * np.pi + 3
C_IN, C_FFT, C_POST, C_DRAWN = TAU + 4, 125.0, TAU + 4, 12.0
C_CZT = 3 * C_FFT + TAU + 2
C_T, C_ROT, LAMBDA = TAU + 3, TAU + 2, 7.0
FAST = 2e-5 * np.sqrt(2.0)


def unit_ld(q, m):
    """(cos, sin)(pi q / m) in long double for an integer array q, reduced modulo 2 m in integers first"""
    x = (np.asarray(q, dtype=np.int64) % (2 * m)).astype(L) * (PI / L(m))
    return np.cos(x), np.sin(x)


def drawn_w(seed, r0, rows, P, Nf, mode):
    """w[len(rows), Nf] as (re, im): pair k of stream (GWB, row % P) of realisation r0 + row // P is bin k; mode as deviate_pairs"""
    k = np.arange(Nf)
    dt = L if mode == "ld" else np.float64
    re, im = np.empty((len(rows), Nf), dtype=dt), np.empty((len(rows), Nf), dtype=dt)
    for i, row in enumerate(rows):
        re[i], im[i] = deviate_pairs(seed, r0 + row // P, philox_ref.stream_id(philox_ref.STREAM_GWB, row % P), k, mode)
    return re, im


def gwb_reference(sqrtC, Nf, npts, i0, inv_dt, rows, P, w=None, seed=0, r0=0, scale=None, fast=False):
    """dict(ref, vmod, A2, A1) for the rows `rows` (row = r P + a) of one call: ref [len(rows), npts] long double, vmod likewise in
    fp64, A2 and A1 [len(rows)] in fp64.  w: (re, im) [M, Nf] of a replay, or None to draw.  scale [R, >= Nf - 1] or None."""
    rows = [int(r) for r in rows]
    n, Kf = 2 * Nf - 2, Nf - 2
    k = np.arange(1, Kf + 1, dtype=np.int64)
    if w is None:
        wre, wim = drawn_w(seed, r0, rows, P, Nf, "fast" if fast else "ld")
    else:
        wre, wim = np.asarray(w[0])[rows], np.asarray(w[1])[rows]
    c = np.broadcast_to(np.asarray(sqrtC, dtype=L)[k], (len(rows), Kf)).copy()
    if scale is not None:
        c *= np.stack([np.asarray(scale[row // P], dtype=L)[k] for row in rows])
    are, aim = c * wre[:, k].astype(L), c * wim[:, k].astype(L)
    q = (k[:, None] * (i0 + np.arange(npts, dtype=np.int64))[None, :]) % n
    ct, st = unit_ld(2 * np.arange(n), n)
    ct, st = ct[q], st[q]
    amp = L(2) * L(inv_dt) / L(n)
    vre, vim = are @ ct - aim @ st, are @ st + aim @ ct
    return dict(ref=amp * vre, vmod=(amp * np.sqrt(vre * vre + vim * vim)).astype(np.float64),
                A2=(amp * np.sqrt(np.sum(are * are + aim * aim, axis=1))).astype(np.float64),
                A1=(amp * np.sum(np.abs(c), axis=1)).astype(np.float64), Kf=Kf)


def chirp_ld(Nf, npts, i0, lo=None):
    """the convolution chirp of the header's chirp-z form, b_u = e^{-i pi u^2 / n} on the lags u = j - k in [i0 - Kf, i0 + npts - 2]
    that the window needs (from `lo` instead where given: a table may hold more lags than are needed, as long as no two share a
    slot - they only reach outputs outside the window), wrapped modulo 4096, (re, im) in long double; zero elsewhere"""
    n, Kf = 2 * Nf - 2, Nf - 2
    u = np.arange(i0 - Kf if lo is None else lo, i0 + npts - 1, dtype=np.int64)
    assert len(u) <= FFT_N
    c, s = unit_ld(u * u, n)
    br, bi = np.zeros(FFT_N, dtype=L), np.zeros(FFT_N, dtype=L)
    br[u % FFT_N], bi[u % FFT_N] = c, -s
    return br, bi


@functools.lru_cache(maxsize=None)
def kappa(Nf, npts, i0):
    """max |DFT_4096(chirp)| / sqrt(4096): a constant of the shape, so fp64 is plenty"""
    br, bi = chirp_ld(Nf, npts, i0)
    return float(np.max(np.abs(np.fft.fft(br.astype(np.float64) + 1j * bi.astype(np.float64)))) / np.sqrt(FFT_N))


def dft4096_ld(xr, xi):
    """X_f = sum_m x_m e^{-2 pi i f m / 4096} in long double, by the definition (512 frequencies at a time)"""
    c, s = unit_ld(2 * np.arange(FFT_N), FFT_N)
    m = np.arange(FFT_N, dtype=np.int64)
    nz = np.flatnonzero((xr != 0) | (xi != 0))
    Xr, Xi = np.empty(FFT_N, dtype=L), np.empty(FFT_N, dtype=L)
    for f0 in range(0, FFT_N, 512):
        idx = (m[f0:f0 + 512, None] * nz[None, :]) % FFT_N
        cc, ss = c[idx], s[idx]
        Xr[f0:f0 + 512] = cc @ xr[nz] + ss @ xi[nz]
        Xi[f0:f0 + 512] = cc @ xi[nz] - ss @ xr[nz]
    return Xr, Xi


def bound(res, family, Nf, npts, i0, drawn, scaled=False, fast=False):
    """fp64 error an evaluation of `family` ("czt", "gemm", "sym") is allowed at every output of gwb_reference's result (docstring)"""
    A2, vmod = res["A2"][:, None], res["vmod"]
    dev = C_DRAWN if drawn and not fast else 0.0
    if family == "czt":
        kp = kappa(Nf, npts, i0)
        b = U * (((C_IN + dev) * max(1.0, kp) + C_CZT * kp) * A2 + C_POST * vmod)
    else:
        c = C_T + dev + (1.0 if scaled else 0.0) + LAMBDA * np.sqrt(2.0 * res["Kf"])
        b = U * (c + (C_ROT if family == "sym" else 0.0)) * A2 + (U * vmod if family == "sym" else 0.0)
    if fast:
        b = b + FAST * res["A1"][:, None]
    return np.broadcast_to(b, vmod.shape).astype(np.float64)
