"""Host reference of the dense time-domain (TD) path - covariance assembly (pta_td_cov_assemble_all / _walk), Cholesky factorisation
(pta_potrf_batched_ex / _ws, pta_potrf_ragged, pta_td_assemble_potrf, pta_gwb_orf_factor) and the draw L z (pta_td_trmm_rng) -
evaluated in 80-bit long double from the contracts in include/pta_replicator_amd.h: test infrastructure, not product code, and not
a transcription of any kernel.  Every tolerance the TD reference tests use is an expression of this module.  u = 2^-53,
gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed. - "ASNA" - Lemma 3.1).

THE FACTOR is judged by its RESIDUAL, not by its distance from another factor: on a covariance of condition 1e9 two correct fp64
factors differ by cond * u, a wrong one need not differ by more.  cholesky_residual(A, L) forms, over the lower triangle and in long
double from the fp64 inputs,
    D = |A - L L^T|,     S = |L| |L^T|,     rho_c = max D / S / u  (componentwise),     rho_n = ||D||_F / (u ||tril A||_F)  (normwise).
Long double carries 11 more bits than fp64: the sums that form D and S round at 2^-64 n S, 1/2048 of u S per term - nothing, next to
bounds of n u S.

BOUND (s) - conventional Cholesky: every entry of L is a_ij minus an inner product, divided by a pivot or square-rooted, in ANY
order of summation, with or without FMA, in any blocking (a blocked right- or left-looking order only reorders the sums):
    D <= gamma_{n+1} S   componentwise   (ASNA Thm 10.3),   i.e.   rho_c <= (n + 1) / (1 - (n + 1) u).
A theorem per element, asserted as it stands: PTA_POTRF_SUBSTITUTION, PTA_POTRF_VALU, pta_gwb_orf_factor.

BOUND (w) - the schedules that solve the rows below a diagonal block by a PRODUCT with its explicit inverse (the default of
pta_potrf_batched_ex: 64 x 64 inverses; the workspace scheme, pta_potrf_ragged and pta_td_assemble_potrf: 128-column W_jj;
PTA_POTRF_DIAG64; PTA_POTRF_SOLVE_ROWS).  Block geometry, read from csrc/pta_potrf.hip: every recursion gives the remainder to its
LEFT part, so all 64-column boundaries lie at n - 64 k and all 128-column boundaries at n - 128 k (the first block is the narrow
one: f128 = nbo - 128 (nb - 1) of the header's panel rule); a 128-column group [c0, c1) wider than 64 is two base blocks
[c0, c1 - 64), [c1 - 64, c1).
  The inverse.  A base block L1 (w <= 64 columns) is inverted inside its factorisation sweep (pta_potf2_sweep): once row j of
  X = L1^-1 is final, X[i, :] -= L1[i, j] X[j, :] for i > j - every column of X by forward substitution, "Method 1" of ASNA 14.2.1
  (Du Croz and Higham, Stability of methods for matrix inversion, IMA J. Numer. Anal. 12 (1992), section 2) in its axpy order.  Its
  computed columns solve (L1 + dL_j) x_j = e_j, |dL_j| <= gamma_w |L1| (ASNA Thm 8.5), hence |X^ - L1^-1| <= gamma_w |L1^-1| |L1| |X^|.
  The sweep multiplies by r = fl(1 / sqrt d) (hardware seed, two Newton steps: within 2 u) instead of dividing, stores -L r r and
  the consumer takes the diagonal as fl(1 / L_jj): six more roundings per entry at the most, C_SWEEP = 6.  A 128-column group is
  inverted in block form (k_diag128, k_inv_blocks): W = [[X1, 0], [-X2 (L21 X1), X2]], two 64-term products, gamma_128 |X2||L21||X1|.
  With  M = [[|X1|, 0], [|X2| |L21| |X1|, |X2|]] >= |L11^-1|  entrywise (in place of |L11^-1|, which the block form cannot be bounded
  by: |X2 L21 X1| <= |X2||L21||X1| points the wrong way) all three contributions to W21 - dX2, dX1, the products - are entries of
  M |L11| M, since |L1| |X1| >= |L1 X1| = I:
      |dW| <= (b + C_SWEEP) u  M |L11| M        (first order; b = the group's width, M = |L11^-1| for a single base block).
  The rows below.  In the workspace scheme block j of a panel is ONE product X_j = fl([X_<j | B_j] S_j^T) with the strip
  S_j = [-T^_j | W^_jj], T^_j = fl(W^_jj L11[j, <j]), of inner length kp = (last column of block j) - (first column of the panel);
  B_j holds the rows as the earlier PANELS left them (conventional sums: bound (s)).  With R_j = B_j - X_<j L_j<^T:
      X_j L_jj^T - R_j = R_j dW^T L_jj^T - X_<j dT^T L_jj^T + dP L_jj^T,
      |dT| <= gamma_kp |W^||L_j<|,     |dP| <= gamma_kp (|B_j||W^T| + |X_<j||T^T|),     |T^| <= |W^||L_j<|,
  and |R_j|, |B_j|, |X_<j||L_j<^T| <= P_j := sum_{k <= j, k in the panel} |X_k||L_jk^T| to first order (B_j = sum_k X_k L_jk^T).
  With K = M^T |L_jj^T| (b x b):  |R_j dW^T L_jj^T| <= (b + C_SWEEP) u P_j K K,  the other two <= kp u P_j K + 2 kp u P_j K:
      E = u P_j K (3 kp I + (b + C_SWEEP) K)        on the entries of L below diagonal block j, zero elsewhere.
  The strips ARE carried through: P_j runs over the whole panel up to block j, not over block j alone.  The single-block forms -
  the 64-column solves of pta_potrf_batched_ex (X = fl(B W^T), B fully updated, kp = b), the rows of a panel's own diagonal block,
  the second base block of a group against the first's X1 (k_diag128: L21 = A21 X1^T) - are the case "panel = the block itself"
  of the same expression and are dominated entrywise by it (P_j only grows with the panel, K's diagonal blocks are the base
  blocks' own K).  PTA_POTRF_SOLVE_ROWS computes the same strips' products in another launch shape: same bound.
      D <= gamma_{n+1} S + E.
  K is formed in long double from the RETURNED factor's diagonal blocks.  A constant of this bound changes only with a line above.

ASSEMBLY.  C_ij = sum_c phi_c Ft_ci Ft_cj + (i == j) sigma2_i + (epoch_of_i == epoch_of_j) ecorr2_i: K products of three factors
(two roundings each, whichever operand phi is folded into), K + 1 additions in any order:
    |C^ - C| <= gamma_{K+3} (sum_c |phi_c Ft_ci Ft_cj| + sigma2 + ecorr2)       per element.
The fused pta_td_assemble_potrf factors that C without storing it: its residual is taken against the long double C and is allowed
the factor's bound plus this one.

DRAW.  out_i = sum_{j <= i} L_ij z_j, at most n terms in any order:  |out^ - out| <= gamma_n sum_j |L_ij||z_j|  with z read from
memory.  With z generated in registers the reference draws it (synth_reference.deviate_pairs, long double Box-Muller) and every
deviate is charged the 12 u by which the device's may differ (C_DRAWN of gwb_reference: the project's own 6 ulp assertion):
+ 12 u sum_j |L_ij||z_j|."""
import numpy as np

from synth_reference import HAVE_LONG_DOUBLE, L as LD, U, deviate_pairs  # noqa: F401  (re-exported)

ROWS = 64          # row block of the long double products
C_SWEEP = 6.0      # roundings of the inversion sweep beyond forward substitution's own (docstring)
C_DRAWN = 12.0     # u per deviate generated on the device


def gamma(k):
    return k * U / (1.0 - k * U)


def _lower_product(X, Y):
    """tril(X Y^T) for long double X, Y [n, k], in row blocks: only the columns a row block's lower triangle needs"""
    n = X.shape[0]
    out = np.zeros((n, n), dtype=LD)
    for i0 in range(0, n, ROWS):
        i1 = min(n, i0 + ROWS)
        out[i0:i1, :i1] = X[i0:i1] @ Y[:i1].T
    return np.tril(out)


def cholesky_residual(A, L):
    """(D, S) = (|A - L L^T|, |L||L^T|) over the lower triangle, long double [n, n] (zero above the diagonal).  A: fp64 or long
    double, only its lower triangle is read; L: the fp64 factor, only its lower triangle is read."""
    Ll = np.tril(np.asarray(L)).astype(LD)
    D = np.abs(np.tril(np.asarray(A).astype(LD)) - _lower_product(Ll, Ll))
    S = _lower_product(np.abs(Ll), np.abs(Ll))
    return D, S


def rho_c(D, bound_over_u):
    """max D / (bound / u) over the lower triangle: against S the componentwise backward error in units of u"""
    lo = np.tril_indices(D.shape[0])
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(D[lo] == 0, 0.0, D[lo] / bound_over_u[lo])
    return float(np.max(q) / U)


def rho_c_rect(D, bound_over_u):
    """the same over every entry of a rectangular result (the draw)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(D == 0, 0.0, D / bound_over_u)
    return float(np.max(q) / U)


def rho_n(D, A):
    return float(np.sqrt(np.sum(D * D)) / (U * np.sqrt(np.sum(np.tril(np.asarray(A).astype(LD)) ** 2))))


def bound_s(S):
    return gamma(S.shape[0] + 1) * S


def groups(n, b):
    """the end-aligned b-column blocks of an order-n factor, first one narrower: [(c0, c1)]"""
    f = n - b * ((n - 1) // b)
    edges = [0] + list(range(f, n + 1, b))
    return list(zip(edges[:-1], edges[1:]))


def panels_uniform(n, nbo):
    """first columns of the panels of a uniform batch (header: the first panel also takes n mod 128 columns)"""
    if n <= nbo:
        return [0]
    return [0] + list(range(nbo + n % 128, n, nbo))


def panels_ragged(n, nbo):
    """first columns of the panels of a matrix in an end-aligned ragged batch: boundaries at n - nbo k"""
    return [0] + list(range(n - nbo * ((n - 1) // nbo), n, nbo))


def _tri_inv(T):
    """inverse of a lower triangular long double matrix by forward substitution, row by row"""
    w = T.shape[0]
    X = np.zeros((w, w), dtype=LD)
    for i in range(w):
        r = -(T[i, :i] @ X[:i])
        r[i] += 1
        X[i] = r / T[i, i]
    return X


def inverse_majorant(L11):
    """M of the docstring for one diagonal block (long double, lower): |L11^-1| for a base block, the block form's majorant for a
    group of two"""
    w = L11.shape[0]
    if w <= 64:
        return np.abs(_tri_inv(L11))
    m = w - 64
    X1, X2 = np.abs(_tri_inv(L11[:m, :m])), np.abs(_tri_inv(L11[m:, m:]))
    M = np.zeros((w, w), dtype=LD)
    M[:m, :m], M[m:, m:] = X1, X2
    M[m:, :m] = X2 @ np.abs(L11[m:, :m]) @ X1
    return M


def e_term(L, b, panels=None):
    """E of bound (w) [n, n] long double: b = 64 or 128, panels = first columns of the panels (None: every block its own panel)"""
    Ll = np.abs(np.tril(np.asarray(L)).astype(LD))
    n = Ll.shape[0]
    E = np.zeros((n, n), dtype=LD)
    for c0, c1 in groups(n, b):
        L11 = np.tril(np.asarray(L)[c0:c1, c0:c1]).astype(LD)
        w = c1 - c0
        if w > 64:      # the second base block against the first's inverse, inside the group
            m = c1 - 64
            K1 = inverse_majorant(L11[:w - 64, :w - 64]).T @ np.abs(L11[:w - 64, :w - 64]).T
            P1 = Ll[m:c1, c0:m] @ Ll[c0:m, c0:m].T
            E[m:c1, c0:m] = U * (P1 @ K1 @ (3 * (m - c0) * np.eye(m - c0, dtype=LD) + (m - c0 + C_SWEEP) * K1))
        if c1 == n:
            break
        p0 = c0 if panels is None else max(p for p in panels if p <= c0)
        K = inverse_majorant(L11).T @ np.abs(L11).T
        P = Ll[c1:, p0:c1] @ Ll[c0:c1, p0:c1].T
        E[c1:, c0:c1] = U * (P @ K @ (3 * (c1 - p0) * np.eye(w, dtype=LD) + (w + C_SWEEP) * K))
    return E


def bound_w(L, S, b, panels=None):
    return bound_s(S) + e_term(L, b, panels)


def cov_reference(Ft, phi, sigma2, epoch_of=None, ecorr2=None):
    """(C, mag) long double [n, n], lower triangle: the header's covariance and the sum of the moduli of its terms.  Ft [K, n] or
    None (K = 0), phi [K], sigma2 [n], epoch_of / ecorr2 [n] or both None."""
    n = len(sigma2)
    s2 = np.asarray(sigma2).astype(LD)
    C, mag = np.diag(s2), np.diag(np.abs(s2))
    if Ft is not None and len(phi):
        F = np.asarray(Ft)[:len(phi), :n].astype(LD)
        G = F * np.asarray(phi).astype(LD)[:, None]
        C = C + _lower_product(G.T.copy(), F.T.copy())
        mag = mag + _lower_product(np.abs(G).T.copy(), np.abs(F).T.copy())
    if epoch_of is not None:
        e = np.asarray(epoch_of)
        same = (e[:, None] == e[None, :])
        ec = np.where(same, np.asarray(ecorr2).astype(LD)[:, None], LD(0))
        C, mag = C + ec, mag + np.abs(ec)
    return np.tril(C), np.tril(mag)


def cov_bound(mag, K):
    return gamma(K + 3) * mag


def trmm_reference(L, z):
    """(ref, mag) long double [R, n]: sum_{j <= i} L_ij z_rj and sum_j |L_ij||z_rj|; L fp64 (lower triangle read), z [R, n]"""
    Ll = np.tril(np.asarray(L)).astype(LD)
    zl = np.asarray(z).astype(LD)
    return zl @ Ll.T, np.abs(zl) @ np.abs(Ll).T


def trmm_bound(mag, n, drawn):
    return (gamma(n) + (C_DRAWN * U if drawn else 0.0)) * mag


def drawn_z(seed, real, stream, n):
    """deviates 0 .. n-1 of a TD stream in long double: deviate j = branch j & 1 of pair j >> 1 (header: pta_td_trmm_rng)"""
    z0, z1 = deviate_pairs(seed, real, stream, np.arange((n + 1) // 2))
    return np.stack([z0, z1], axis=1).reshape(-1)[:n]
