"""The long double residuals of the TD path (tests/td_reference.py) and their derived bounds, on the CPU, before any kernel is held
to them.

FILL.  On every family and order of the table below LAPACK's factor and an fp64 NumPy emulation of each algorithm class -
unblocked; block-inverse with 64- and with 128-column blocks (the group's inverse in block form); left-looking block-inverse -
must fill at most HALF of their bound: a condition on the inputs and on the bound, not a tolerance on a kernel.  The worst
fraction per family is printed (pytest -s).  Measured: 0.25 to 0.38 at n = 2 (one or two roundings against gamma_3), 0.005 to 0.09
from n = 65 up - bound (s), LAPACK and unblocked: rho_c 3 to 34 against n + 1; bound (w), block-inverse: 0.005 to 0.07.  On Lo and X
from n = 130 up the block-inverse emulations must LEAVE bound (s) - by 1.9 to 62 on Lo (rho_c 550 to 18 700), by 114 on X - while
bound (w) holds: that failure is the test of bound (s)'s discrimination, and of the conditioning term's necessity.  X, cond 1e12, is
the conventional schedules' family: LAPACK factors it at every order here (np.linalg.cholesky would raise), the block-inverse
emulations lose positive definiteness on it from n = 300 up and are run on it up to n = 130 only.

DEFECTS.  Each seeded defect is the factor a kernel with that defect would return - where the defect is in an update, the honest
factor of the wrongly updated Schur complement - and must leave the bound of its class by FACTOR = 10 on W and Q.  On Lo the factor
is recorded (printed) and asserted above 1 only: there the conditioning term E of bound (w) is legitimately large below the
ill-conditioned diagonal blocks (K of order 1e3 and more) and hides more; bound (s) has no such term, and on it Lo is held to
FACTOR as well.  The single wrong entry, 1e-12 max|L|, sits in column 0: there S_i0 = |L_i0| L_00 is the entry's own product, the
residual is 1e-12 max|L| / |L_i0| >= 9007 u of it and the bound (n + 1) u, or (n + 1 + 4 f128 + 6) u with E, which in column 0 is
exact since K e_0 = e_0: a factor of 18 at least at n = 300, whatever the matrix.  The same error at (3 n / 4, n / 3) is recorded
only ("entry_1e-12_inner": 52 on W, 5.8 on Q, 5.6 on Lo under bound (s)): a TD factor's first 60 columns carry the red noise and are
1e2 to 1e4 times its later pivots, so S there is made of products the wrong entry's own product is small against - an error scaled
to max|L| legitimately hides in a row of small entries.  The defects sit at n = 300 (groups [0, 44), [44, 172), [172, 300): a narrow first block, three groups) except
the pivot: a relative error e in one pivot's reciprocal square root shows as 2 e in its column's residual whatever the matrix -
2e-13 = 1801 u against (n + 1) u - so a factor of 10 needs n + 1 <= 180, and it is seeded at n = 150.

THE REFERENCE ITSELF is compared with mpmath (50 digits) at n <= 8: the long double D, S, covariance and draw agree with it to the
rounding of their own sums, gamma^ld_{k+2} of the terms' moduli with u_ld = 2^-64."""
import numpy as np
import pytest

import td_cases as tc
import td_reference as tr
from td_reference import HAVE_LONG_DOUBLE, LD, U

pytestmark = pytest.mark.skipif(not HAVE_LONG_DOUBLE, reason="no 80-bit long double on this host")

HALF, FACTOR = 0.5, 10.0
FILL_ORDERS = (2, 65, 130, 300)
FILL_ORDERS_700 = ("lapack", "inverse128")      # n = 700: the figures the issue quotes, on two factors (a residual costs 2 s there)
N_DEFECT, N_PIVOT = 300, 150
RECORDED = ("entry_1e-12_inner",)               # printed, asserted above 1 only (docstring)


def _fill(A, L, cls):
    """(fraction of the class's bound, fraction of bound (s), rho_n) of a factor"""
    D, S = tr.cholesky_residual(A, L)
    bs = tr.bound_s(S)
    fs = tr.rho_c(D, bs) * U
    if cls is None:
        return fs, fs, tr.rho_n(D, A)
    return tr.rho_c(D, bs + tr.e_term(L, cls)) * U, fs, tr.rho_n(D, A)


@pytest.mark.parametrize("fam", tc.FAMILIES)
def test_honest_factors_fill_at_most_half_of_their_bound(fam):
    worst = {}
    for n in FILL_ORDERS + (700,):
        A = tc.family(fam, n)["A"]
        factors = {"lapack": (np.linalg.cholesky(A), None)}      # family X: LAPACK factors it at sigma = 1e-9 s, as td_cases says
        for name, (fn, cls) in tc.EMULATIONS.items():
            if (n < 700 or name in FILL_ORDERS_700) and (fam != "X" or cls is None or n <= 130):   # X: the conventional schedules' family
                factors[name] = (fn(A), cls)
        for name, (L, cls) in factors.items():
            f, fs, rn = _fill(A, L, cls)
            worst[name] = max(worst.get(name, 0.0), round(f, 4))
            print(f"{fam} n={n} {name}: fill {f:.4f}  bound (s) alone {fs:.3f}  rho_n {rn:.1f}")
            assert f <= HALF, (fam, n, name, f)
            if fam in ("Lo", "X") and cls is not None and n >= 130:
                assert fs > 1.0, (fam, n, name, fs)       # the conditioning term is needed: bound (s) alone rejects the class
    print(f"{fam}: worst fraction per class {worst}")


def _schur_factor(A, L, c, schur):
    """the factor whose columns < c are L's and whose trailing part is the honest factor of `schur` (lower triangle read)"""
    out = np.tril(L).copy()
    out[c:, c:] = tc.chol_unblocked(schur)
    return out


def _defects(fam, n):
    """name -> (A, defective factor, class of bound); LinAlgError inside = the defect left the Schur complement indefinite"""
    A = tc.family(fam, n)["A"]
    L = np.linalg.cholesky(A)
    g = tr.groups(n, 128)
    f, c2 = g[0][1], g[-1][0]                  # end of the narrow first block, start of the last group
    out = {}
    E = L.copy(); E[3 * n // 4, 0] += 1e-12 * np.max(np.abs(L))
    out["entry_1e-12"] = E
    E2 = L.copy(); E2[3 * n // 4, n // 3] += 1e-12 * np.max(np.abs(L))
    out["entry_1e-12_inner"] = E2
    S1 = np.tril(A[f:, f:] - L[f:, :f] @ L[f:, :f].T)              # the Schur complement behind the first block
    r, c = slice(32, 48), slice(16, 32)                            # one 16 x 16 tile of it, below its diagonal
    T = S1.copy(); T[r, c] += L[f:][r, f - 4:f] @ L[f:][c, f - 4:f].T
    out["tile_k_slab"] = lambda: _schur_factor(A, L, f, T)
    T2 = S1.copy(); T2[r, c] -= L[f:][r, :f] @ L[f:][c, :f].T
    out["tile_twice"] = lambda: _schur_factor(A, L, f, T2)
    other = np.linalg.cholesky(tc.family(fam, n, seed=1)["A"])
    c0, c1 = g[1]
    i = c1 + 7
    Wr = L.copy(); Wr[i, c0:c1] = (L[i, c0:c1] @ L[c0:c1, c0:c1].T) @ tc._inv_lower(other[c0:c1, c0:c1]).T
    out["next_matrix_block"] = Wr
    out["narrow_last_column"] = lambda: _schur_factor(A, L, f, np.tril(A[f:, f:] - L[f:, :f - 1] @ L[f:, :f - 1].T))
    out["left_one_block_short"] = lambda: _schur_factor(A, L, c2, np.tril(A[c2:, c2:] - L[c2:, :c2 - 128] @ L[c2:, :c2 - 128].T))
    return A, out


def _pivot_defect(fam):
    A = tc.family(fam, N_PIVOT)["A"]
    L = np.linalg.cholesky(A)
    L[0:, 0] *= 1.0 + 1e-13
    return A, L


def _miss(A, L, cls):
    D, S = tr.cholesky_residual(A, L)
    b = tr.bound_s(S) if cls is None else tr.bound_w(L, S, cls)
    return tr.rho_c(D, b) * U


@pytest.mark.parametrize("cls", [None, 64, 128])
@pytest.mark.parametrize("fam", ("W", "Q", "Lo"))
def test_seeded_factor_defects_leave_the_bound(fam, cls):
    A, defects = _defects(fam, N_DEFECT)
    cases = [(k, A, v) for k, v in defects.items()] + [("pivot_rsqrt_1e-13", *_pivot_defect(fam))]
    for name, Am, Ld in cases:
        need = FACTOR if (fam != "Lo" or cls is None) and name not in RECORDED else 1.0
        try:
            miss = _miss(Am, Ld() if callable(Ld) else Ld, cls)
        except np.linalg.LinAlgError:
            miss = np.inf                       # an indefinite Schur complement: the kernel's info reports it
        print(f"{fam} class {cls or 's'} {name}: outside the bound by {miss:.3g}")
        assert miss >= need, (fam, cls, name, miss)


def test_seeded_assembly_defects_leave_the_bound():
    for fam in ("Q", "Lo"):
        d = tc.td_inputs(258, 5, **{**tc._TD[fam], "ecorr": 1e-7}, shuffle=True)
        C, mag = tr.cov_reference(d["Ft"], d["phi"], d["sigma2"], d["epoch_of"], d["ecorr2"])
        b = tr.cov_bound(mag, len(d["phi"]))
        honest = np.tril(tc.cov_fp64(d))
        assert tr.rho_c(np.abs(honest - C), b) * U <= HALF
        r, c = slice(128, 144), slice(16, 32)
        drop = honest.copy(); drop[r, c] -= d["phi"][0] * np.outer(d["Ft"][0, r], d["Ft"][0, c])
        i, j = [(i, j) for i in range(130, 258) for j in range(100) if d["epoch_of"][i] != d["epoch_of"][j]][0]
        cross = honest.copy(); cross[i, j] += d["ecorr2"][i]      # an epoch number that only matches another block's TOA
        for name, bad in (("phi_term_dropped", drop), ("ecorr_across_blocks", cross)):
            miss = tr.rho_c(np.abs(bad - C), b) * U
            print(f"{fam} assembly {name}: outside the bound by {miss:.3g}")
            assert miss >= FACTOR, (fam, name, miss)


def test_seeded_draw_defects_leave_the_bound():
    rng = np.random.default_rng(3)
    for fam in ("Q", "Lo"):
        n = 257
        L = tc.chol_unblocked(tc.family(fam, n)["A"])
        z = rng.standard_normal((5, n))
        ref, mag = tr.trmm_reference(L, z)
        b = tr.trmm_bound(mag, n, drawn=True)
        honest = z @ L.T
        assert tr.rho_c_rect(np.abs(honest - ref), b) * U <= HALF
        strict = honest.copy(); strict[:, 100] -= L[100, 100] * z[:, 100]                       # j <= i made j < i on row 100
        short = honest.copy()
        for i in range(n - 4, n):
            short[:, i] -= z[:, n - 4:i + 1] @ L[i, n - 4:i + 1]                                 # the last strip's K extent cut 4 short
        for name, bad in (("strict_lower_row", strict), ("k_extent_4_short", short)):
            miss = tr.rho_c_rect(np.abs(bad - ref), b) * U
            print(f"{fam} draw {name}: outside the bound by {miss:.3g}")
            assert miss >= FACTOR, (fam, name, miss)


def test_reference_against_mpmath():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    u_ld = 2.0 ** -64
    def g_ld(k):
        return k * u_ld / (1 - k * u_ld)
    def to_ld(x):
        hi = float(x)
        return LD(hi) + LD(float(x - mp.mpf(hi)))
    for fam, n in (("W", 8), ("Q", 7), ("Lo", 8), ("Lo", 1), ("Q", 2)):
        d = tc.family(fam, n)
        A, L = d["A"], np.linalg.cholesky(d["A"])
        D, S = tr.cholesky_residual(A, L)
        for i in range(n):
            for j in range(i + 1):
                s = sum(mp.mpf(L[i, k]) * mp.mpf(L[j, k]) for k in range(j + 1))
                sa = sum(abs(mp.mpf(L[i, k]) * mp.mpf(L[j, k])) for k in range(j + 1))
                tol = g_ld(n + 2) * (float(sa) + abs(A[i, j]))
                assert abs(D[i, j] - to_ld(abs(mp.mpf(A[i, j]) - s))) <= tol and abs(S[i, j] - to_ld(sa)) <= tol, (fam, n, i, j)
        if fam == "W":
            continue
        C, mag = tr.cov_reference(d["Ft"], d["phi"], d["sigma2"], d["epoch_of"], d["ecorr2"])
        K = len(d["phi"])
        z = np.random.default_rng(n).standard_normal((2, n))
        ref, zmag = tr.trmm_reference(L, z)
        for i in range(n):
            for j in range(i + 1):
                terms = [mp.mpf(d["phi"][c]) * mp.mpf(d["Ft"][c, i]) * mp.mpf(d["Ft"][c, j]) for c in range(K)]
                if i == j:
                    terms.append(mp.mpf(d["sigma2"][i]))
                if d["epoch_of"] is not None and d["epoch_of"][i] == d["epoch_of"][j]:
                    terms.append(mp.mpf(d["ecorr2"][i]))
                sa = sum(abs(t) for t in terms)
                assert abs(C[i, j] - to_ld(sum(terms))) <= g_ld(K + 4) * float(sa) and abs(mag[i, j] - to_ld(sa)) <= g_ld(K + 4) * float(sa)
            for r in range(2):
                t = [mp.mpf(L[i, j]) * mp.mpf(z[r, j]) for j in range(i + 1)]
                assert abs(ref[r, i] - to_ld(sum(t))) <= g_ld(n + 2) * float(sum(abs(x) for x in t))
