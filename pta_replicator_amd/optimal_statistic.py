"""Host preparation of the Hellings-Downs cross-correlation optimal statistic (fixed-noise OS), pure NumPy.

For pulsar a with N_a TOAs, noise covariance C_a and timing-model design matrix M_a:

    F_a      N_a x 2 n_f sin/cos Fourier basis at f_k = k / T (T = span of the whole array), column order of
             create_fourier_design_matrix_red (even columns sin(2 pi f t), odd columns cos)
    S_k      unit-amplitude power-law spectrum per column, f_yr^(gamma - 3) f_k^-gamma / (12 pi^2 T)
    C_a      diag((efac sigma)^2 + (efac equad | equad)^2) + ECORR epoch blocks + F_rn diag(phi_rn) F_rn^T
             (+ A_gw^2 F diag(S) F^T with the GWB auto-term)
    P_a^-1   C^-1 - C^-1 M (M^T C^-1 M)^-1 M^T C^-1           (timing model marginalised)
    W_a      S^1/2 F^T P_a^-1                                [2 n_f, N_a]
    Z_a      W_a F S^1/2                                      [2 n_f, 2 n_f]
    den_ab   tr(Z_a Z_b)

and per realisation Y_ra = W_a r_a, num_rab = Y_ra . Y_rb, A2_r = sum_{a<b} G_ab num_rab / sum_{a<b} G_ab^2 den_ab for every
overlap reduction function G, sigma(A2) = (sum G^2 den)^-1/2.  The per-realisation half runs on the device (pta_os_project,
pta_os_pairs); this module builds W, Z, den and the pair weights once, and holds a NumPy evaluation of the per-realisation half
(``os_from_rows``) for tests.

C_a^-1 is applied through Woodbury on the low-rank part (red noise and GWB columns scaled by sqrt(phi), so the capacitance matrix
I + U^T N^-1 U has eigenvalues >= 1) and Sherman-Morrison per ECORR epoch for N^-1: no N_a x N_a matrix is ever formed.  Every
pulsar's covariance is divided by its mean white-noise variance before any solve (the statistic is invariant; the solves see
O(1) numbers), as prepare_timing_projection does for its weights.
"""
import numpy as np

from .constants import YEAR_IN_SEC

ORF_NAMES = ("hd", "monopole", "dipole")


def fourier_basis(toas_s, nf, T):
    """F [N, 2 nf]: column 2k = sin(2 pi f_k t), 2k + 1 = cos(2 pi f_k t), f_k = (k + 1) / T."""
    f = np.arange(1, nf + 1) / float(T)
    arg = 2 * np.pi * np.asarray(toas_s, dtype=np.float64)[:, None] * f[None, :]
    F = np.empty((len(toas_s), 2 * nf))
    F[:, 0::2], F[:, 1::2] = np.sin(arg), np.cos(arg)
    return F


def unit_spectrum(nf, T, gamma=13. / 3.):
    """S [2 nf]: the unit-amplitude power-law variance of each sin / cos column, f_yr^(gamma-3) f^-gamma / (12 pi^2 T)."""
    f = np.repeat(np.arange(1, nf + 1) / float(T), 2)
    fyr = 1.0 / YEAR_IN_SEC
    return fyr ** (gamma - 3.0) * f ** (-gamma) / (12 * np.pi ** 2 * T)


def pair_geometry(pos):
    """(pair_a, pair_b, cos zeta) of the pairs a < b (row-major upper triangle) of unit vectors pos [P, 3]."""
    pos = np.asarray(pos, dtype=np.float64)
    ia, ib = np.triu_indices(len(pos), 1)
    c = np.clip(np.sum(pos[ia] * pos[ib], axis=1), -1.0, 1.0)
    return ia.astype(np.int32), ib.astype(np.int32), c


def hd(cos_zeta):
    """standard Hellings-Downs curve 1/2 - x/4 + 3/2 x ln x, x = (1 - cos zeta) / 2 (1/2 at x = 0)."""
    x = (1.0 - np.asarray(cos_zeta, dtype=np.float64)) / 2.0
    with np.errstate(divide="ignore", invalid="ignore"):
        g = 0.5 - x / 4.0 + 1.5 * x * np.log(x)
    return np.where(x > 0, g, 0.5)


def orf_weights(orfs, pair_a, pair_b, cos_zeta, P):
    """(names, G [n_orf, n_pairs]) for ORF names ("hd", "monopole", "dipole") or user [P, P] arrays."""
    names, rows = [], []
    for k, o in enumerate(orfs):
        if isinstance(o, str):
            if o == "hd":
                g = hd(cos_zeta)
            elif o == "monopole":
                g = np.ones_like(cos_zeta)
            elif o == "dipole":
                g = cos_zeta.copy()
            else:
                raise ValueError(f"unknown ORF {o!r}: expected one of {ORF_NAMES} or a [P, P] array")
            names.append(o)
        else:
            m = np.asarray(o, dtype=np.float64)
            if m.shape != (P, P) or not np.all(np.isfinite(m)):
                raise ValueError(f"a user ORF must be a finite [{P}, {P}] array, got shape {m.shape}")
            g = m[pair_a, pair_b]
            names.append(f"orf{k}")
        rows.append(g)
    if not rows:
        raise ValueError("at least one ORF is needed")
    return names, np.stack(rows)


def _epoch_sums(y, epoch_of, E):
    """[E, k] row sums of y [N, k] per epoch (every epoch holds at least one TOA)."""
    o = np.argsort(epoch_of, kind="stable")
    starts = np.searchsorted(epoch_of[o], np.arange(E))
    return np.add.reduceat(y[o], starts, axis=0)


class _NoiseInverse:
    """N^-1 of N = diag(d) + sum_e j_e 1_e 1_e^T (white noise + ECORR), Sherman-Morrison per epoch."""

    def __init__(self, d, epoch_of=None, j=None):
        self.d = d
        self.ep = None
        if epoch_of is not None and j is not None and np.any(j > 0):
            self.ep = np.asarray(epoch_of, dtype=np.int64)
            E = len(j)
            if np.any(np.bincount(self.ep, minlength=E) == 0):
                raise ValueError("every ECORR epoch must hold at least one TOA")
            s = _epoch_sums((1.0 / d)[:, None], self.ep, E)[:, 0]
            self.g = j / (1.0 + j * s)
            self.E = E

    def __call__(self, x):
        y = x / self.d[:, None]
        if self.ep is not None:
            s = _epoch_sums(y, self.ep, self.E)
            y = y - (self.g[:, None] * s)[self.ep] / self.d[:, None]
        return y


def pulsar_operator(sigma2, F, S, epoch_of=None, ecorr=None, F_rn=None, phi_rn=None, gw_amp2=0.0, M=None):
    """(W [2 nf, N], Z [2 nf, 2 nf]) of one pulsar.

    sigma2 [N] white-noise variances; F [N, 2 nf] the OS basis, S [2 nf] its unit spectrum; epoch_of [N] / ecorr [E] the ECORR
    epoch of every TOA and the epochs' ecorr [s] (or None); F_rn [N, K] / phi_rn [K] the red-noise basis and prior variances (or None);
    gw_amp2 = A_gw^2 of the GWB auto-term (0 = none); M [N, m] the timing-model design matrix (or None)."""
    sigma2 = np.asarray(sigma2, dtype=np.float64)
    if not np.all(sigma2 > 0):
        raise ValueError("white-noise variances must be positive")
    s = float(np.mean(sigma2))            # every covariance term is divided by s: O(1) solves
    Ninv = _NoiseInverse(sigma2 / s, epoch_of, None if ecorr is None else np.asarray(ecorr, dtype=np.float64) ** 2 / s)
    cols = []
    if F_rn is not None and phi_rn is not None:
        keep = np.asarray(phi_rn) > 0
        if np.any(keep):
            cols.append(F_rn[:, keep] * np.sqrt(np.asarray(phi_rn)[keep] / s)[None, :])
    if gw_amp2 > 0:
        cols.append(F * np.sqrt(gw_amp2 * S / s)[None, :])
    G = F if M is None else np.concatenate([F, M], axis=1)
    CiG = Ninv(G)
    if cols:
        U = np.concatenate(cols, axis=1)
        NiU = Ninv(U)
        L = np.linalg.cholesky(np.eye(U.shape[1]) + U.T @ NiU)
        CiG = CiG - NiU @ _cho_solve(L, NiU.T @ G)
    nf2 = F.shape[1]
    PF = CiG[:, :nf2]
    if M is not None:
        PF = timing_projection(M, CiG[:, nf2:], PF, "C^-1")[0]
    rs = np.sqrt(S)
    W = (PF * rs[None, :]).T / s
    Z = rs[:, None] * (F.T @ PF) * rs[None, :] / s
    return W, 0.5 * (Z + Z.T)


def _cho_solve(L, B):
    return np.linalg.solve(L.T, np.linalg.solve(L, B))


def timing_projection(M, CiM, X, inv):
    """(X - C^-1 M (M^T C^-1 M)^-1 M^T X, Bn, dg): the timing model M [N, m] projected out of X = C^-1 Y [N, k], given CiM = C^-1 M;
    Bn = M^T C^-1 M over dg dg^T (unit diagonal), dg the square roots of its diagonal.  A singular M^T C^-1 M is refused; inv names
    the inverse in the message ("C^-1", or "N^-1" where C holds white noise and ECORR only)."""
    B = M.T @ CiM
    B = 0.5 * (B + B.T)
    dg = np.sqrt(np.abs(np.diag(B)))
    if not np.all(dg > 0):
        raise ValueError(f"M^T {inv} M is singular: a timing-model column vanishes on this pulsar's TOAs")
    Bn = B / dg[:, None] / dg[None, :]
    ev = np.linalg.eigvalsh(Bn)
    if ev[0] <= 1e-12 * ev[-1]:
        raise ValueError(f"M^T {inv} M is singular (condition {ev[-1] / max(ev[0], 1e-300):.3g}): the pulsar's TOAs do not "
                         "constrain its timing model")
    return X - CiM @ (np.linalg.solve(Bn, (M.T @ X) / dg[:, None]) / dg[:, None]), Bn, dg


def pick(x, a):
    """entry a of a per-pulsar list, None where the list itself is None"""
    return None if x is None else x[a]


def array_basis(toas_s, components, T=None, F_rn=None):
    """(nf, T, K_rn, U) - the prelude of prepare / prepare_matched / prepare_lnl: components checked, T = the span of the whole array
    where None, K_rn = the widest red-noise basis of F_rn (0 for None) held to K_rn + 2 nf <= MATCHED_KMAX, and per pulsar
    U = [F_rn | F] [N_a, K_rn + 2 nf] (a zero block where a pulsar has no red-noise basis)."""
    if not 1 <= int(components) <= 32:
        raise ValueError(f"components={components}: 1 .. 32 frequencies (2 n_f <= 64 columns)")
    nf = int(components)
    if T is None:
        T = max(float(np.max(t)) for t in toas_s) - min(float(np.min(t)) for t in toas_s)
    K_rn = 0 if F_rn is None else max([0] + [f.shape[1] for f in F_rn if f is not None])
    if K_rn + 2 * nf > MATCHED_KMAX:
        raise ValueError(f"K = K_rn + 2 n_f = {K_rn} + {2 * nf} exceeds the limit of {MATCHED_KMAX} columns per pulsar")
    U = []
    for a, t in enumerate(toas_s):
        Fr = pick(F_rn, a)
        U.append(np.concatenate([np.zeros((len(t), K_rn)) if Fr is None else Fr, fourier_basis(t, nf, T)], axis=1))
    return nf, T, K_rn, U


class OSPlan:
    """realisation-independent operands of the OS: W (list of [2 nf, N_a]), Z ([P, 2 nf, 2 nf]), den / pairs / weights."""

    def __init__(self, W, Z, pair_a, pair_b, cos_zeta, names, G, S=None, T=None):
        self.W, self.Z = W, Z
        self.S, self.T = S, T                                          # unit spectrum [C] and span (the per-frequency OS reports phi = a2 S)
        self.P, self.C = len(W), W[0].shape[0]
        self.counts = np.array([w.shape[1] for w in W])
        self.off = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int64)
        self.pair_a, self.pair_b, self.cos_zeta = pair_a, pair_b, cos_zeta
        self.zeta = np.arccos(cos_zeta)
        self.den = np.einsum("pij,pij->p", Z[pair_a], Z[pair_b])     # tr(Z_a Z_b), Z symmetric
        self.names, self.G = names, G
        norm = G ** 2 @ self.den
        if not np.all(norm > 0):
            bad = [n for n, v in zip(names, norm) if not v > 0]
            raise ValueError(f"ORF(s) {bad} vanish on every pair: their OS is undefined")
        self.sigma = norm ** -0.5
        self.weights = G / norm[:, None]                               # A2 = weights @ num
        self.sigma_pair = self.den ** -0.5

    def Wt(self):
        """[C, sum N_a]: W of every pulsar over the concatenated TOAs (the device operand of pta_os_project)."""
        return np.concatenate(self.W, axis=1)


def prepare(toas_s, sigma2, pos, components=14, gamma=13. / 3., orfs=ORF_NAMES, epoch_of=None, ecorr=None, F_rn=None,
            phi_rn=None, gw_amp2=0.0, M=None, T=None):
    """OSPlan of an array: per-pulsar lists toas_s [s], sigma2, epoch_of / ecorr (entries None = no ECORR), F_rn / phi_rn (None = no
    red noise), M (None = no timing model); pos [P, 3] unit vectors; T = span of the whole array (default: from toas_s)."""
    P = len(toas_s)
    nf, T, _, F = array_basis(toas_s, components, T)
    S = unit_spectrum(nf, T, gamma)
    pair_a, pair_b, cz = pair_geometry(pos)
    names, G = orf_weights(orfs, pair_a, pair_b, cz, P)
    W, Z = [], np.zeros((P, 2 * nf, 2 * nf))
    for a in range(P):
        Wa, Z[a] = pulsar_operator(sigma2[a], F[a], S, pick(epoch_of, a), pick(ecorr, a), pick(F_rn, a), pick(phi_rn, a), gw_amp2, pick(M, a))
        W.append(Wa)
    return OSPlan(W, Z, pair_a, pair_b, cz, names, G, S=S, T=float(T))


def project(plan, rows):
    """Y [R, P, C] = W_a r_a of rows [R, sum N_a] (NumPy)."""
    rows = np.atleast_2d(np.asarray(rows, dtype=np.float64))
    return np.stack([rows[:, plan.off[a]:plan.off[a + 1]] @ plan.W[a].T for a in range(plan.P)], axis=1)


def os_from_Y(plan, Y):
    """(A2 [R, n_orf], snr [R, n_orf], num [R, n_pairs]) from Y [R, P, C] (NumPy)."""
    num = np.einsum("rpc,rpc->rp", Y[:, plan.pair_a], Y[:, plan.pair_b])
    A2 = num @ plan.weights.T
    return A2, A2 / plan.sigma[None, :], num


def os_from_rows(plan, rows):
    """the whole per-realisation OS in NumPy: (A2, snr, num)."""
    return os_from_Y(plan, project(plan, rows))


# ---------------------------------------------------------------- per-frequency OS: the spectrum per realisation -------------
# Instead of one amplitude under the template S, one per Fourier bin.  Let a_j = phi_j / S_j be the GW variance of bin j over the
# unit template (a_j = A^2 for every j if the data follow the template).  For a pair p = (a < b), with column 2k / 2k + 1 the
# sin / cos of bin k,
#
#     n_p[k]    = X_a[2k] X_b[2k] + X_a[2k+1] X_b[2k+1]
#     D_p[k, j] = sum_{i in {2k, 2k+1}} sum_{l in {2j, 2j+1}} Z_a[i, l] Z_b[i, l]          (symmetric, PSD; sum_kj D_p = tr(Z_a Z_b))
#
# E[n_p] = G_p D_p a, under the null Cov(n_p) = D_p, and different pairs are uncorrelated: generalised least squares over the pairs is
#
#     b_o = sum_p G_o,p n_p,    F_o = sum_p G_o,p^2 D_p,    a_o = F_o^-1 b_o,    Cov(a_o) = F_o^-1                    ("full")
#
# and a_o[k] = b_o[k] / F_o[k, k], sigma = F_o[k, k]^-1/2 when the coupling between bins is ignored ("narrowband").  1^T b / 1^T F 1 is
# the broadband A2, 1^T F 1 = sum G^2 den.  phi = a S is the variance of one sin / cos coefficient [s^2]; in full mode, without the GW
# auto-term in the noise model, it does not depend on the template's index.  F is solved Jacobi-scaled (d^-1/2 F d^-1/2, d = diag F):
# with gamma = 13/3 the unscaled condition number is 4e5 at n_f = 6 already.
SPECTRUM_MODES = ("full", "narrowband")


def pair_blocks(Z, pair_a, pair_b):
    """D [..., n_pairs, n_f, n_f] of Z [..., P, C, C] (symmetric): D_p[k, j] = the sum of Z_a * Z_b over the 2 x 2 block (k, j)."""
    Z = np.asarray(Z, dtype=np.float64)
    nf = Z.shape[-1] // 2
    prod = Z[..., pair_a, :, :] * Z[..., pair_b, :, :]
    return prod.reshape(prod.shape[:-2] + (nf, 2, nf, 2)).sum(axis=(-3, -1))


def pair_numerators(X, pair_a, pair_b):
    """n [..., n_pairs, n_f] of X [..., P, C]: the sin and cos products of every bin."""
    X = np.asarray(X, dtype=np.float64)
    prod = X[..., pair_a, :] * X[..., pair_b, :]
    return prod.reshape(prod.shape[:-1] + (prod.shape[-1] // 2, 2)).sum(axis=-1)


def _scaled_cholesky(F):
    """(Fs, L, dinv, ok): Fs = d^-1/2 F d^-1/2 per matrix of F [..., n, n], its Cholesky factor, dinv = d^-1/2 and ok [...] = positive
    definite (the identity stands in for Fs and L where it is not)"""
    F = np.asarray(F, dtype=np.float64)
    n = F.shape[-1]
    d = np.diagonal(F, axis1=-2, axis2=-1)
    ok = np.all(d > 0, axis=-1)
    dinv = np.where(ok[..., None], d, 1.0) ** -0.5
    Fs = np.where(ok[..., None, None], dinv[..., :, None] * F * dinv[..., None, :], np.eye(n))
    try:
        L = np.linalg.cholesky(Fs)
    except np.linalg.LinAlgError:
        ok, L = ok.copy(), np.broadcast_to(np.eye(n), Fs.shape).copy()
        for i in np.ndindex(Fs.shape[:-2]):
            try:
                L[i] = np.linalg.cholesky(Fs[i])
            except np.linalg.LinAlgError:
                ok[i], Fs[i] = False, np.eye(n)
    return Fs, L, dinv, ok


def joint_weights(G, den):
    """(Wj [n, n_pairs], cov [n, n], sigma [n]): the generalised-least-squares fit of n ORFs AT ONCE to the pair numerators of the
    fixed-noise statistic.  With E[num_p] = den_p sum_k x_k G[k, p] and Var(num_p) = den_p (uncorrelated pairs), the estimate is
    x = F^-1 G num, F = G diag(den) G^T, Cov(x) = F^-1: x = num @ Wj.T with Wj = F^-1 G.  For the spherical-harmonic basis ORFs
    G[k] = basis[k][a, b] (spharmORFbasis.correlated_basis, the generation's own code) x_k estimates A^2 c_lm.  F is solved
    Jacobi-scaled (_scaled_cholesky).  Refuses fewer pairs than ORFs and an F that is not positive definite (to rounding)."""
    G, den = np.asarray(G, dtype=np.float64), np.asarray(den, dtype=np.float64)
    n, n_pairs = G.shape
    if n_pairs < n:
        raise ValueError(f"the joint fit of {n} ORFs needs at least as many pulsar pairs, got {n_pairs}")
    F = (G * den[None, :]) @ G.T
    _, L, dinv, ok = (x[0] for x in _scaled_cholesky(F[None]))
    # (the scaled F has a unit diagonal: a squared pivot at rounding level means ORFs that are collinear on this array's pairs)
    if not bool(ok) or not np.all(np.isfinite(L)) or np.min(np.diagonal(L)) ** 2 < 1e-13:
        raise ValueError(f"the joint fit of {n} ORFs is singular for this array (F = G diag(den) G^T is not positive definite)")
    Minv = np.linalg.solve(L, np.eye(n))            # L^-1 of the scaled factor
    cov = dinv[:, None] * (Minv.T @ Minv) * dinv[None, :]
    return cov @ G, cov, np.sqrt(np.diagonal(cov))


def spectrum_solve(F, b, mode="full", form="cholesky"):
    """(a2 [..., n_f], sigma) of F [..., n_f, n_f] and b [..., n_f] (leading axes broadcast; sigma has F's).  form "cholesky" is
    what the device evaluates (M = L^-1 of the scaled factor, a2 = d^-1/2 M^T M d^-1/2 b); "solve" goes through np.linalg.solve / inv
    without a factor, for error bars.  Where F is not positive definite (narrowband: a diagonal entry is not positive) both are NaN."""
    if mode not in SPECTRUM_MODES:
        raise ValueError(f"mode={mode!r}: one of {SPECTRUM_MODES}")
    F, b = np.asarray(F, dtype=np.float64), np.asarray(b, dtype=np.float64)
    n = F.shape[-1]
    if mode == "narrowband":
        d = np.diagonal(F, axis1=-2, axis2=-1)
        ok = np.all(d > 0, axis=-1)[..., None]
        d = np.where(ok, d, 1.0)
        a2, sigma = b / d, d ** -0.5
    else:
        Fs, L, dinv, ok = _scaled_cholesky(F)
        ok = ok[..., None]
        if form == "cholesky":
            M = np.linalg.solve(L, np.broadcast_to(np.eye(n), L.shape))
            y = M @ (dinv * b)[..., None]
            a2 = dinv * (np.swapaxes(M, -1, -2) @ y)[..., 0]
            sigma = dinv * np.sqrt(np.sum(M ** 2, axis=-2))
        elif form == "solve":
            a2 = dinv * np.linalg.solve(Fs, (dinv * b)[..., None])[..., 0]
            sigma = dinv * np.sqrt(np.diagonal(np.linalg.inv(Fs), axis1=-2, axis2=-1))
        else:
            raise ValueError(f"form={form!r}: 'cholesky' or 'solve'")
    return np.where(np.broadcast_to(ok, a2.shape), a2, np.nan), np.where(ok, sigma, np.nan)


def spectrum_fisher(plan):
    """F [n_orf, n_f, n_f] of the fixed-noise plan; ValueError if an ORF's F is not positive definite."""
    F = np.einsum("op,pkj->okj", plan.G ** 2, pair_blocks(plan.Z, plan.pair_a, plan.pair_b))
    ok = _scaled_cholesky(F)[3]
    if not np.all(ok):
        raise ValueError(f"the per-frequency Fisher matrix of ORF(s) {[n for n, v in zip(plan.names, ok) if not v]} is not positive definite")
    return F


def _spectrum_result(plan, F, b, mode, form="cholesky"):
    a2, sigma = spectrum_solve(F, b, mode, form)
    res = dict(a2=a2, sigma=sigma, snr=a2 / sigma, b=b, fisher=F)
    S = getattr(plan, "S", None)
    if S is not None:
        Sk = np.asarray(S)[0::2]
        res.update(phi=a2 * Sk, phi_sigma=sigma * Sk)
        if getattr(plan, "T", None) is not None:
            res["freqs"] = np.arange(1, len(Sk) + 1) / float(plan.T)
    return res


def spectrum_from_Y(plan, Y, mode="full"):
    """the per-frequency OS of Y [R, P, C] (NumPy): dict of a2, snr, phi, phi_sigma, b [R, n_orf, n_f], sigma [n_orf, n_f], fisher
    [n_orf, n_f, n_f], freqs [n_f]."""
    b = np.einsum("op,rpk->rok", plan.G, pair_numerators(Y, plan.pair_a, plan.pair_b))
    return _spectrum_result(plan, spectrum_fisher(plan), b, mode)


def spectrum_from_rows(plan, rows, mode="full"):
    """the whole per-realisation per-frequency OS in NumPy (spectrum_from_Y's dict)."""
    return spectrum_from_Y(plan, project(plan, rows), mode)


# ---------------------------------------------------------------- OS under per-realisation noise parameters -------------------
# The noise model follows theta per realisation: white noise, ECORR and the timing model stay fixed, red noise and the GWB
# auto-term change.  Per pulsar, with N' = N / s (white noise + ECORR over the mean white-noise variance s):
#
#     P0' = N'^-1 - N'^-1 M (M^T N'^-1 M)^-1 M^T N'^-1      (N'^-1 without a timing model)
#     U   = [F_rn | F]  [N_a, K],  K = K_rn + C
#     V   = U^T P0'     [K, N_a]            A = U^T P0' U  [K, K]
#
# are built once (matched_operator); per realisation and pulsar, with prior variances b [K] (matched_prior) and D = diag(sqrt b):
#
#     q = V r_a,   Mc = I + D A D = L L^T,   H = L^-1 D [q | A[:, F]]
#     X = S^1/2 (q_F - H_F^T h_q) / s          (= W_a(theta) r_a)
#     Z = S^1/2 (A_FF - H_F^T H_F) S^1/2 / s   (= Z_a(theta))
#
# and num_ab = X_a . X_b, den_ab = tr(Z_a Z_b) per realisation.  Mc has eigenvalues >= 1 for any finite theta.
MATCHED_KMAX = 128   # K = K_rn + C of pta_os_matched_solve (PTA_OSM_KMAX)


def matched_operator(sigma2, U, epoch_of=None, ecorr=None, M=None):
    """(V [K, N], A [K, K], s) of one pulsar: U [N, K] = [F_rn | F]; the other arguments as pulsar_operator's."""
    return _matched_operator(sigma2, U, epoch_of, ecorr, M)[:3]


def _matched_operator(sigma2, U, epoch_of, ecorr, M):
    """matched_operator's (V, A, s), then what lnl_operator builds on: N'^-1 (_NoiseInverse) and, with a timing model, (N'^-1 M, Bn,
    dg) of timing_projection (else None)"""
    sigma2 = np.asarray(sigma2, dtype=np.float64)
    if not np.all(sigma2 > 0):
        raise ValueError("white-noise variances must be positive")
    s = float(np.mean(sigma2))
    Ninv = _NoiseInverse(sigma2 / s, epoch_of, None if ecorr is None else np.asarray(ecorr, dtype=np.float64) ** 2 / s)
    PU, tm = Ninv(U), None
    if M is not None:
        NiM = Ninv(M)
        PU, Bn, dg = timing_projection(M, NiM, PU, "N^-1")
        tm = (NiM, Bn, dg)
    A = U.T @ PU
    return np.ascontiguousarray(PU.T), 0.5 * (A + A.T), s, Ninv, tm


class MatchedPlan:
    """theta-independent operands of the per-realisation-noise OS: V (list of [K, N_a]), A [P, K, K], s [P], S [C], the pairs and
    the ORF values G [n_orf, n_pairs]."""

    def __init__(self, V, A, s, S, K_rn, pair_a, pair_b, cos_zeta, names, G, nf, T):
        self.V, self.A, self.s, self.S = V, A, np.asarray(s, dtype=np.float64), S
        self.P, self.K, self.C, self.K_rn = len(V), A.shape[1], len(S), int(K_rn)
        self.counts = np.array([v.shape[1] for v in V])
        self.off = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int64)
        self.pair_a, self.pair_b, self.cos_zeta = pair_a, pair_b, cos_zeta
        self.zeta = np.arccos(cos_zeta)
        self.names, self.G = names, G
        self.nf, self.T = int(nf), float(T)
        if not np.all(np.sum(G ** 2, axis=1) > 0):
            bad = [n for n, g in zip(names, G) if not np.sum(g ** 2) > 0]
            raise ValueError(f"ORF(s) {bad} vanish on every pair: their OS is undefined")

    def Vt(self):
        """[K, sum N_a]: V of every pulsar over the concatenated TOAs (pta_os_project's operand, in blocks of <= 64 rows)."""
        return np.concatenate(self.V, axis=1)


def prepare_matched(toas_s, sigma2, pos, components=14, gamma=13. / 3., orfs=ORF_NAMES, epoch_of=None, ecorr=None, F_rn=None, M=None,
                    T=None):
    """MatchedPlan of an array; arguments as prepare()'s, without the prior variances (they come per realisation).  F_rn: None (no
    pulsar has red noise: K_rn = 0) or a per-pulsar list of [N_a, K_rn] bases (an entry None = a zero block)."""
    P = len(toas_s)
    nf, T, K_rn, U = array_basis(toas_s, components, T, F_rn)
    S = unit_spectrum(nf, T, gamma)
    pair_a, pair_b, cz = pair_geometry(pos)
    names, G = orf_weights(orfs, pair_a, pair_b, cz, P)
    V, A, s = [], np.zeros((P, K_rn + 2 * nf, K_rn + 2 * nf)), np.zeros(P)
    for a in range(P):
        Va, A[a], s[a] = matched_operator(sigma2[a], U[a], pick(epoch_of, a), pick(ecorr, a), pick(M, a))
        V.append(Va)
    return MatchedPlan(V, A, s, S, K_rn, pair_a, pair_b, cz, names, G, nf, T)


def rn_prior(f, tspan, log10_A, gamma):
    """sqrt(prior)^2 of red-noise coefficients at frequencies f: pta_rn_amp(f, tspan, log10_A, gamma)^2, same operations."""
    fyr = 1 / YEAR_IN_SEC
    prior = (10 ** log10_A) ** 2 * (f / fyr) ** (-gamma) / (12 * np.pi ** 2 * tspan) * YEAR_IN_SEC ** 3
    return np.sqrt(prior) ** 2


def matched_prior(R, s, rn_f=None, rn_tspan=None, rn_phi=None, rn_log10_A=None, rn_gamma=None, nf=0, T=1.0, gw_log10_A=None,
                  gw_gamma=None, gw_log10_hc=None, gw_nodes=None):
    """b [R, P, K]: prior variances over s of every (realisation, pulsar, column) - the NumPy form of pta_os_matched_prior and, with
    gw_log10_hc, of pta_os_matched_prior_spec.

    s [P]; rn_f [P, K_rn / 2], rn_tspan [P], rn_phi [P, K_rn] the configured prior variances (or all None: K_rn = 0); rn_log10_A,
    rn_gamma [R, P] (None = every pulsar as configured; NaN amplitude = that pulsar as configured); nf, T: the OS frequencies
    (k + 1) / T; gw_log10_A, gw_gamma [R] (None = no GW auto-term: those columns are 0).  gw_log10_hc [R, M] with gw_nodes [M] (in
    place of gw_log10_A / gw_gamma): a spectrum per realisation, log10 hc at the node frequencies gw_nodes [Hz] in the order given
    (sorted here as red_noise.gwb_spectrum_hcf sorts a userSpec), interpolated with the userSpec semantics; the GW columns are
    hc(f)^2 / (12 pi^2 f^3 T) / s."""
    s = np.asarray(s, dtype=np.float64)
    P = len(s)
    K_rn = 0 if rn_phi is None else np.shape(rn_phi)[1]
    b = np.zeros((R, P, K_rn + 2 * nf))
    if K_rn:
        phi = np.broadcast_to(np.asarray(rn_phi, dtype=np.float64), (R, P, K_rn)).copy()
        if rn_log10_A is not None:
            lA, g = np.asarray(rn_log10_A, dtype=np.float64), np.asarray(rn_gamma, dtype=np.float64)
            f = np.repeat(np.asarray(rn_f, dtype=np.float64), 2, axis=1)
            with np.errstate(invalid="ignore"):
                sampled = rn_prior(f[None], np.asarray(rn_tspan)[None, :, None], lA[:, :, None], g[:, :, None])
            phi = np.where(np.isnan(lA)[:, :, None], phi, sampled)
        b[:, :, :K_rn] = phi / s[None, :, None]
    if gw_log10_A is not None:
        lA, g = np.asarray(gw_log10_A, dtype=np.float64)[:, None], np.asarray(gw_gamma, dtype=np.float64)[:, None]
        f = np.repeat(np.arange(1, nf + 1) / float(T), 2)[None, :]
        fyr = 1.0 / YEAR_IN_SEC
        phi = 10.0 ** (2.0 * lA) * (fyr ** (g - 3.0) * f ** (-g) / (12 * np.pi ** 2 * T))
        b[:, :, K_rn:] = phi[:, None, :] / s[None, :, None]
    if gw_log10_hc is not None:
        if gw_log10_A is not None or gw_nodes is None:
            raise ValueError("matched_prior: gw_log10_hc comes with gw_nodes, in place of gw_log10_A / gw_gamma")
        from . import _hyper
        nodes = np.asarray(gw_nodes, dtype=np.float64)
        order, xp = _hyper.spec_nodes(np.stack([nodes, np.ones_like(nodes)], axis=1))
        f = np.arange(1, nf + 1) / float(T)
        hc = _hyper.spec_eval(_hyper.spec_tables(f, xp), np.asarray(gw_log10_hc, dtype=np.float64)[:, order])
        phi = np.repeat(hc ** 2 / (12 * np.pi ** 2 * f ** 3 * T), 2, axis=1)
        b[:, :, K_rn:] = phi[:, None, :] / s[None, :, None]
    return b


def matched_solve(A, b, q, S, s, form="cholesky"):
    """(X [..., C], Z [..., C, C]) of the small dense problems: A [..., K, K], b [..., K], q [..., K] (leading axes broadcast), S [C]
    the unit spectrum of the last C columns, s the mean white-noise variance (scalar or [...]).  form "cholesky" is what the device
    evaluates (H = L^-1 D [q | A_F]); "solve" is an independent route (Mc^-1 through np.linalg.solve, no factor) for error bars."""
    A, b, q = np.asarray(A, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(q, dtype=np.float64)
    K, C = A.shape[-1], len(S)
    d = np.sqrt(b)
    Mc = np.eye(K) + d[..., :, None] * A * d[..., None, :]
    rhs = d[..., :, None] * np.concatenate([q[..., :, None], np.broadcast_to(A[..., :, K - C:], q.shape + (C,))], axis=-1)
    if form == "cholesky":
        H = np.linalg.solve(np.linalg.cholesky(Mc), rhs)
        corr = np.swapaxes(H[..., :, 1:], -1, -2) @ H
    elif form == "solve":
        corr = np.swapaxes(rhs[..., :, 1:], -1, -2) @ np.linalg.solve(Mc, rhs)
    else:
        raise ValueError(f"form={form!r}: 'cholesky' or 'solve'")
    rs = np.sqrt(S)
    s = np.asarray(s, dtype=np.float64)
    X = rs * (q[..., K - C:] - corr[..., :, 0]) / s[..., None]
    Z = rs[:, None] * (A[..., K - C:, K - C:] - corr[..., :, 1:]) * rs[None, :] / s[..., None, None]
    return X, 0.5 * (Z + np.swapaxes(Z, -1, -2))


def matched_from_XZ(plan, X, Z):
    """the pair half: dict of num, den [R, n_pairs], A2, sigma, snr [R, n_orf], rho, sigma_pair [R, n_pairs] from X [R, P, C], Z [R, P, C, C]."""
    num = np.einsum("rpc,rpc->rp", X[:, plan.pair_a], X[:, plan.pair_b])
    den = np.einsum("rpij,rpij->rp", Z[:, plan.pair_a], Z[:, plan.pair_b])
    norm = den @ (plan.G ** 2).T
    A2 = (num @ plan.G.T) / norm
    sigma = norm ** -0.5
    return dict(X=X, Z=Z, num=num, den=den, A2=A2, sigma=sigma, snr=A2 / sigma, rho=num / den, sigma_pair=den ** -0.5)


def matched_from_rows(plan, rows, b, form="cholesky"):
    """the whole per-realisation OS under prior variances b [R, P, K] of rows [R, sum N_a], in NumPy (matched_from_XZ's dict)."""
    rows = np.atleast_2d(np.asarray(rows, dtype=np.float64))
    R = rows.shape[0]
    X, Z = np.zeros((R, plan.P, plan.C)), np.zeros((R, plan.P, plan.C, plan.C))
    for a in range(plan.P):
        q = rows[:, plan.off[a]:plan.off[a + 1]] @ plan.V[a].T
        X[:, a], Z[:, a] = matched_solve(plan.A[a], b[:, a], q, plan.S, plan.s[a], form=form)
    return matched_from_XZ(plan, X, Z)


def unpack_triangle(Zp, C):
    """symmetric [..., C, C] of packed lower triangles [..., C (C + 1) / 2] (entry (i, j <= i) at i (i + 1) / 2 + j)."""
    i, j = np.tril_indices(C)
    Z = np.zeros(np.shape(Zp)[:-1] + (C, C))
    Z[..., i, j] = Zp
    Z[..., j, i] = Zp
    return Z


def matched_spectrum_from_XZ(plan, X, Z, mode="full", form="cholesky"):
    """the per-frequency OS under per-realisation noise: X [R, P, C], Z [R, P, C, C] or packed [R, P, C (C + 1) / 2] (matched_solve's,
    pta_os_matched_solve's) -> spectrum_from_Y's dict with sigma [R, n_orf, n_f] and fisher [R, n_orf, n_f, n_f].  A (realisation,
    ORF) whose F is not positive definite is NaN.  form: spectrum_solve's, the second route for error bars."""
    X, Z = np.asarray(X, dtype=np.float64), np.asarray(Z, dtype=np.float64)
    C = X.shape[-1]
    if Z.ndim == X.ndim:
        Z = unpack_triangle(Z, C)
    G = np.asarray(plan.G, dtype=np.float64)
    b = np.einsum("op,rpk->rok", G, pair_numerators(X, plan.pair_a, plan.pair_b))
    F = np.einsum("op,rpkj->rokj", G ** 2, pair_blocks(Z, plan.pair_a, plan.pair_b))
    return _spectrum_result(plan, F, b, mode, form)


# ---------------------------------------------------------------- marginalised log-likelihood on a theta grid -----------------
# The noise model is the matched OS's (white noise, ECORR and the timing model fixed; red noise on the K_rn red-noise columns, a
# common uncorrelated process with the GWB spectrum on the last C columns).  With the timing model marginalised under a flat prior,
#
#     -2 ln L_a(r, theta) = [ r^T P0' r - || L^-1 D q ||^2 ] / s  +  2 sum_k ln L_kk  +  c_a
#     q = V r,  D = diag(sqrt b(theta)),  Mc = I + D A D = L L^T
#     c_a = ln det N_a + ln det(M^T N_a^-1 M) + (N_a - m) ln 2 pi                     (theta-independent)
#
# r^T P0' r = r^T N'^-1 r - || G r ||^2 with N' = diag(d) + ECORR epochs (Sherman-Morrison weights g_e) and G = chol(M^T N'^-1 M)^-1
# M^T N'^-1 (m rows).  It is evaluated as x^T N'^-1 x = sum x_i^2 / d_i - sum_e g_e (sum_{i in e} x_i / d_i)^2 of the fit residual
# x = r - H G r, H = M (M^T N'^-1 M)^-1/2: un-fitted rows carry most of their power inside the span of M, and the difference of the
# two large terms would lose (|r| / |x|)^2 eps (3e-11 of r^T P0' r on the engine's realisations).  Mc, L and ln det depend on (theta_g, pulsar) alone: one factorisation
# serves every realisation, which is what pta_lnl_factor / pta_lnl_apply do for a whole grid of theta.
def lnl_operator(sigma2, U, epoch_of=None, ecorr=None, M=None):
    """theta-independent operands of one pulsar's likelihood, a dict: V [K, N], A [K, K], s (matched_operator's), Gt [m, N] (the
    timing-model rows G; m = 0 without a timing model), Ht [m, N] (H^T, H G r = M beta_hat), dinv [N] = 1 / d, the epoch -> TOA lists ep_ptr [E + 1], ep_idx [sum of
    the epochs' sizes] (TOA indices within the pulsar, epochs in ascending order, TOAs of an epoch in TOA order; E = 0 without
    ECORR), ep_g [E], and the constant c."""
    V, A, s, Ninv, tm = _matched_operator(sigma2, U, epoch_of, ecorr, M)
    d = Ninv.d
    N = len(d)
    j = None if ecorr is None else np.asarray(ecorr, dtype=np.float64) ** 2 / s
    logdet_N = N * np.log(s) + float(np.sum(np.log(d)))
    ep_ptr, ep_idx, ep_g = np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0)
    if Ninv.ep is not None:
        order = np.argsort(Ninv.ep, kind="stable")
        ep_ptr = np.searchsorted(Ninv.ep[order], np.arange(Ninv.E + 1)).astype(np.int32)
        ep_idx, ep_g = order.astype(np.int32), Ninv.g
        se = _epoch_sums((1.0 / d)[:, None], Ninv.ep, Ninv.E)[:, 0]
        logdet_N += float(np.sum(np.log1p(j * se)))
    m = 0 if M is None else M.shape[1]
    Gt = Ht = np.zeros((0, N))
    c = logdet_N + (N - m) * np.log(2 * np.pi)
    if m:
        NiM, Bn, dg = tm                                      # matched_operator has refused a singular B
        Lb = np.linalg.cholesky(Bn)
        Gt = np.linalg.solve(Lb, (NiM / dg[None, :]).T)
        Ht = np.linalg.solve(Lb, (M / dg[None, :]).T)
        c += 2 * float(np.sum(np.log(dg))) + 2 * float(np.sum(np.log(np.diag(Lb)))) - m * np.log(s)
    return dict(V=V, A=A, s=s, Gt=np.ascontiguousarray(Gt), Ht=np.ascontiguousarray(Ht), dinv=1.0 / d, ep_ptr=ep_ptr, ep_idx=ep_idx, ep_g=ep_g, c=float(c))


class LnlPlan:
    """theta-independent operands of the likelihood of an array: per pulsar V [K, N_a], Gt [m, N_a], the epoch lists; A [P, K, K],
    s [P], c [P]; dinv over the concatenated TOAs.  The device reads Vt() (V and Gt stacked: K + m operator rows), dinv and the
    concatenated epoch lists of epochs()."""

    def __init__(self, ops, K_rn, nf, T):
        self.V, self.Gt, self.Ht = [o["V"] for o in ops], [o["Gt"] for o in ops], [o["Ht"] for o in ops]
        self.A = np.stack([o["A"] for o in ops])
        self.s, self.c = np.array([o["s"] for o in ops]), np.array([o["c"] for o in ops])
        self.P, self.K, self.K_rn, self.C = len(ops), self.A.shape[1], int(K_rn), 2 * int(nf)
        self.m = max(g.shape[0] for g in self.Gt)
        self.counts = np.array([v.shape[1] for v in self.V])
        self.off = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int64)
        self.dinv = np.concatenate([o["dinv"] for o in ops])
        self.ep = [(o["ep_ptr"], o["ep_idx"], o["ep_g"]) for o in ops]
        self.nf, self.T = int(nf), float(T)

    def Vt(self):
        """[K + m, sum N_a]: V, then the timing-model rows G (zero rows where a pulsar has fewer than m), over the concatenated TOAs."""
        out = np.zeros((self.K + self.m, int(self.off[-1])))
        for a in range(self.P):
            out[:self.K, self.off[a]:self.off[a + 1]] = self.V[a]
            out[self.K:self.K + self.Gt[a].shape[0], self.off[a]:self.off[a + 1]] = self.Gt[a]
        return out

    def Ht_all(self):
        """[m, sum N_a]: the rows of H^T of every pulsar over the concatenated TOAs (pta_lnl_quad's operand)."""
        out = np.zeros((self.m, int(self.off[-1])))
        for a in range(self.P):
            out[:self.Ht[a].shape[0], self.off[a]:self.off[a + 1]] = self.Ht[a]
        return out

    def epochs(self):
        """(psr_ep [P + 1], ep_ptr [E + 1], ep_idx [n_idx], ep_g [E]) int32 / float64: the pulsars' epochs concatenated, ep_idx
        holding TOA indices within the pulsar, ep_ptr offsets into ep_idx."""
        psr_ep, ptr, idx, g = [0], [np.zeros(1, dtype=np.int64)], [], []
        base = 0
        for p, i, w in self.ep:
            psr_ep.append(psr_ep[-1] + len(w))
            ptr.append(base + p[1:].astype(np.int64))
            idx.append(i)
            g.append(w)
            base += int(p[-1])
        return (np.asarray(psr_ep, dtype=np.int32), np.concatenate(ptr).astype(np.int32),
                np.concatenate(idx).astype(np.int32) if idx else np.zeros(0, dtype=np.int32), np.concatenate(g) if g else np.zeros(0))


def prepare_lnl(toas_s, sigma2, components=14, epoch_of=None, ecorr=None, F_rn=None, M=None, T=None):
    """LnlPlan of an array; arguments as prepare_matched()'s (no positions and no ORFs: the likelihood is a sum over pulsars)."""
    nf, T, K_rn, U = array_basis(toas_s, components, T, F_rn)
    ops = [lnl_operator(sigma2[a], U[a], pick(epoch_of, a), pick(ecorr, a), pick(M, a)) for a in range(len(U))]
    return LnlPlan(ops, K_rn, nf, T)


def lnl_quad(plan, rows):
    """r0 [R, P] = r_a^T P0' r_a of rows [R, sum N_a] (NumPy; the streaming pass of pta_lnl_quad and its timing-model term)."""
    rows = np.atleast_2d(np.asarray(rows, dtype=np.float64))
    out = np.zeros((rows.shape[0], plan.P))
    for a in range(plan.P):
        r = rows[:, plan.off[a]:plan.off[a + 1]]
        r = r - (r @ plan.Gt[a].T) @ plan.Ht[a]          # the residual of the timing-model fit
        w = r * plan.dinv[plan.off[a]:plan.off[a + 1]][None, :]
        t = np.sum(r * w, axis=1)
        ptr, idx, g = plan.ep[a]
        if len(g):
            es = np.add.reduceat(w[:, idx], ptr[:-1], axis=1)
            t = t - np.sum(g[None, :] * es ** 2, axis=1)
        out[:, a] = t
    return out


def lnl_solve(A, b, q, r0, s, c, form="cholesky"):
    """ln L [R, G] of one pulsar: A [K, K], b [G, K] prior variances over s, q [R, K] = V r, r0 [R] = r^T P0' r, s and c scalars.
    form "cholesky" is the device's route (factor Mc, y = L^-1 D q by substitution, || y ||^2, 2 sum ln L_kk); "solve" goes through
    np.linalg.solve and slogdet without a factor, for error bars."""
    A, b, q = np.asarray(A, dtype=np.float64), np.atleast_2d(np.asarray(b, dtype=np.float64)), np.atleast_2d(np.asarray(q, dtype=np.float64))
    K = A.shape[-1]
    d = np.sqrt(b)
    Mc = np.eye(K) + d[:, :, None] * A[None] * d[:, None, :]
    if form == "cholesky":
        L = np.linalg.cholesky(Mc)
        logdet = 2.0 * np.sum(np.log(np.diagonal(L, axis1=-2, axis2=-1)), axis=-1)
        quad = np.sum(np.linalg.solve(L, d[:, :, None] * q.T[None]) ** 2, axis=1)      # [G, R]
    elif form == "solve":
        logdet = np.linalg.slogdet(Mc)[1]
        dq = d[:, :, None] * q.T[None]                                                 # [G, K, R]
        quad = np.sum(dq * np.linalg.solve(Mc, dq), axis=1)
    else:
        raise ValueError(f"form={form!r}: 'cholesky' or 'solve'")
    r0 = np.asarray(r0, dtype=np.float64)
    return (-0.5 * ((r0[None, :] - quad) / s + logdet[:, None] + c)).T


def lnl_from_rows(plan, rows, b, form="cholesky"):
    """(lnl_pulsar [R, P, G], lnl [R, G]) of rows [R, sum N_a] under prior variances b [G, P, K] (matched_prior with the grid in
    place of the realisations), in NumPy; lnl sums the pulsars in ascending order."""
    rows = np.atleast_2d(np.asarray(rows, dtype=np.float64))
    b = np.asarray(b, dtype=np.float64)
    r0 = lnl_quad(plan, rows)
    lp = np.zeros((rows.shape[0], plan.P, b.shape[0]))
    tot = np.zeros((rows.shape[0], b.shape[0]))
    for a in range(plan.P):
        q = rows[:, plan.off[a]:plan.off[a + 1]] @ plan.V[a].T
        lp[:, a] = lnl_solve(plan.A[a], b[:, a], q, r0[:, a], plan.s[a], plan.c[a], form=form)
        tot = tot + lp[:, a]
    return lp, tot


GRID_KEYS = ("gwb_log10_A", "gwb_gamma", "rn_log10_A", "rn_gamma")


def theta_grid(P=None, **axes):
    """(grid, shape): the outer product of 1-D axes, flattened in C order (the first axis given varies slowest).  Axes are named
    by the keys of theta; gwb_* entries come out [G], rn_* entries [G, P] (the same value for every pulsar; needs P).  shape is
    the tuple of the axes' lengths: lnl.reshape(R, *shape) puts the grid back."""
    if not axes:
        raise ValueError("theta_grid: at least one axis")
    unknown = set(axes) - set(GRID_KEYS)
    if unknown:
        raise ValueError(f"theta_grid: unknown axes {sorted(unknown)} (expected a subset of {list(GRID_KEYS)})")
    vals = []
    for k, v in axes.items():
        v = np.asarray(v, dtype=np.float64)
        if v.ndim != 1 or v.size < 1:
            raise ValueError(f"theta_grid: axis {k!r} must be 1-D and non-empty, got shape {v.shape}")
        vals.append(v)
    mesh = np.meshgrid(*vals, indexing="ij")
    grid = {}
    for k, m in zip(axes, mesh):
        flat = np.ascontiguousarray(m.reshape(-1))
        if k.startswith("rn_"):
            if P is None:
                raise ValueError(f"theta_grid: axis {k!r} needs the number of pulsars P")
            flat = np.ascontiguousarray(np.repeat(flat[:, None], int(P), axis=1))
        grid[k] = flat
    return grid, tuple(len(v) for v in vals)


# ---------------------------------------------------------------- likelihood ratio of a correlated common process -------------
# The intrinsic noise C_a stays the configured one (white noise, ECORR, red noise, chromatic columns; no GWB auto-term: prepare with
# gw_amp2 = 0), the timing model is marginalised, and only the common process varies: coefficient covariance Gamma (x) diag(phi_g) on
# the array-wide Fourier basis, phi_g,k = A_g^2 unit_spectrum(gamma_g)_k, Gamma the [P, P] ORF.  With Gamma = B B^T (B [P, rho]), the
# plan's W_a = S^1/2 F_a^T P~_a and Z_a = W_a F_a S^1/2 at gamma_ref, Y_a = W_a r_a and d_g,k = sqrt(phi_g,k / S_k),
#
#     T   = (B^T (x) I) blockdiag(Z_a) (B (x) I)     [rho C, rho C]   T[(i, k), (j, l)] = sum_a B[a, i] B[a, j] Z_a[k, l]
#     Y'  = (B^T (x) I) Y                            [rho C]
#     M_g = I + D_g T D_g = L_g L_g^T,  D_g = I_rho (x) diag(d_g)     eigenvalues >= 1
#     ln L(r | g, Gamma) - ln L(r | noise only) = 1/2 || L_g^-1 D_g Y' ||^2 - sum_i ln L_g,ii
#
# (Woodbury and the determinant lemma on C + F (Gamma (x) phi) F^T.)  T depends on the ORF alone, M_g on (grid point, ORF): one
# factorisation serves every realisation (pta_clnl_assemble, pta_potrf_batched_ex, pta_clnl_solve).
CLNL_ORF_NAMES = ("hd", "monopole", "dipole", "curn")


def _orf_from_pairs(name, pair_a, pair_b, cos_zeta, P):
    if name not in CLNL_ORF_NAMES:
        raise ValueError(f"unknown ORF {name!r}: expected one of {CLNL_ORF_NAMES} or a [P, P] array")
    cz = np.asarray(cos_zeta, dtype=np.float64)
    v = {"hd": hd(cz), "monopole": np.ones_like(cz), "dipole": cz, "curn": np.zeros_like(cz)}[name]
    G = np.eye(P)
    G[pair_a, pair_b] = v
    G[pair_b, pair_a] = v
    return G


def _symmetric(m):
    """symmetric to rounding: |m - m^T| <= 1e-12 max|m|"""
    return bool(np.all(np.abs(m - m.T) <= 1e-12 * max(float(np.max(np.abs(m))), 1e-300)))


def _orf_array(o, P):
    m = np.asarray(o, dtype=np.float64)
    if m.shape != (P, P) or not np.all(np.isfinite(m)):
        raise ValueError(f"a user ORF must be a finite [{P}, {P}] array, got shape {m.shape}")
    if not _symmetric(m):
        raise ValueError("a user ORF must be symmetric")
    return 0.5 * (m + m.T)


def orf_matrix(name_or_array, pos):
    """Gamma [P, P] of unit vectors pos [P, 3]: a name of CLNL_ORF_NAMES ("hd": the Hellings-Downs curve of the pair angles,
    "monopole": 1, "dipole": cos zeta, "curn": 0 off the diagonal; unit diagonal), or a symmetric finite [P, P] array, used as given."""
    pos = np.asarray(pos, dtype=np.float64)
    P = len(pos)
    if isinstance(name_or_array, str):
        return _orf_from_pairs(name_or_array, *pair_geometry(pos), P)
    return _orf_array(name_or_array, P)


def orf_factor(Gamma):
    """B [P, rho] with B B^T = Gamma by numpy.linalg.eigh: the eigenvalues above 1e-12 lambda_max are kept (a singular ORF has
    rho < P: monopole 1, dipole 3); an eigenvalue below -1e-10 lambda_max (not positive semi-definite) and rank 0 are refused."""
    Gamma = np.asarray(Gamma, dtype=np.float64)
    if Gamma.ndim != 2 or Gamma.shape[0] != Gamma.shape[1] or not np.all(np.isfinite(Gamma)):
        raise ValueError(f"an ORF must be a finite square array, got shape {Gamma.shape}")
    if not _symmetric(Gamma):
        raise ValueError("an ORF must be symmetric")
    w, V = np.linalg.eigh(0.5 * (Gamma + Gamma.T))
    wmax = float(w[-1])
    if not wmax > 0:
        raise ValueError("an ORF of rank 0 (no positive eigenvalue) describes no common process")
    if w[0] < -1e-10 * wmax:
        raise ValueError(f"the ORF is not positive semi-definite: eigenvalue {w[0]:.3g} (largest {wmax:.3g})")
    keep = w > 1e-12 * wmax
    return V[:, keep] * np.sqrt(w[keep])[None, :]


class ClnlPlan:
    """operands of the correlated likelihood ratio: the OSPlan (prepared with gw_amp2 = 0) and per ORF its name, Gamma, B [P, rho]
    and T [rho C, rho C]"""

    def __init__(self, os_plan, names, Gammas, Bs, Ts, gamma_ref):
        self.os, self.names, self.Gamma, self.B, self.T_orf = os_plan, names, Gammas, Bs, Ts
        self.P, self.C, self.nf, self.T = os_plan.P, os_plan.C, os_plan.C // 2, float(os_plan.T)
        self.gamma_ref = float(gamma_ref)
        self.rho = [b.shape[1] for b in Bs]
        self.n = [r * self.C for r in self.rho]


def clnl_plan(os_plan, orfs, gamma_ref=13. / 3.):
    """ClnlPlan of an OSPlan built with gw_amp2 = 0 at gamma_ref, and 1 .. 4 ORFs (names of CLNL_ORF_NAMES or [P, P] arrays)."""
    orfs = (orfs,) if isinstance(orfs, str) else tuple(orfs)
    if not 1 <= len(orfs) <= 4:
        raise ValueError(f"{len(orfs)} ORFs: one plan holds 1 .. 4")
    P, C = os_plan.P, os_plan.C
    names, Gs, Bs, Ts = [], [], [], []
    for k, o in enumerate(orfs):
        if isinstance(o, str):
            G = _orf_from_pairs(o, os_plan.pair_a, os_plan.pair_b, os_plan.cos_zeta, P)
            names.append(o)
        else:
            G = _orf_array(o, P)
            names.append(f"orf{k}")
        B = orf_factor(G)
        T = np.einsum("ai,aj,akl->ikjl", B, B, os_plan.Z).reshape(B.shape[1] * C, B.shape[1] * C)
        Gs.append(G)
        Bs.append(B)
        Ts.append(0.5 * (T + T.T))
    return ClnlPlan(os_plan, names, Gs, Bs, Ts, gamma_ref)


def clnl_scale(nf, T, gamma_ref, log10_A, gamma):
    """d [G, 2 nf]: d_g,k = 10^log10_A_g (f_k yr)^((gamma_ref - gamma_g) / 2), the square root of the grid point's spectrum over the
    unit spectrum at gamma_ref (pta_clnl_scale of csrc/pta_clnl.h, same operations)"""
    lA, g = np.atleast_1d(np.asarray(log10_A, dtype=np.float64)), np.atleast_1d(np.asarray(gamma, dtype=np.float64))
    f = np.repeat(np.arange(1, int(nf) + 1) / float(T), 2)
    return 10.0 ** lA[:, None] * (f[None, :] * YEAR_IN_SEC) ** ((float(gamma_ref) - g[:, None]) / 2.0)


def clnl_ratio(T, Yp, D, form="cholesky"):
    """(lnl_ratio [R, G], scale [R, G]) of one ORF: T [n, n], Yp [R, n] the mixed projections, D [G, n] the diagonals of D_g.
    M_g = I + D_g T D_g, v = D_g Y'; form "cholesky" is the device's route (factor M_g, substitution, sum of squares, sum of ln L_ii);
    "solve" goes through np.linalg.solve and slogdet without a factor, for error bars.  scale = v^T v / 2 + | ln det M_g |: the size
    of the two terms the ratio is the difference of."""
    T, Yp, D = np.asarray(T, dtype=np.float64), np.atleast_2d(np.asarray(Yp, dtype=np.float64)), np.atleast_2d(np.asarray(D, dtype=np.float64))
    M = np.eye(T.shape[0])[None] + D[:, :, None] * T[None] * D[:, None, :]
    v = D[:, :, None] * Yp.T[None]                                                      # [G, n, R]
    if form == "cholesky":
        L = np.linalg.cholesky(M)
        half_logdet = np.sum(np.log(np.diagonal(L, axis1=-2, axis2=-1)), axis=-1)
        quad = np.sum(np.linalg.solve(L, v) ** 2, axis=1)
    elif form == "solve":
        half_logdet = 0.5 * np.linalg.slogdet(M)[1]
        quad = np.sum(v * np.linalg.solve(M, v), axis=1)
    else:
        raise ValueError(f"form={form!r}: 'cholesky' or 'solve'")
    return (0.5 * quad - half_logdet[:, None]).T, (0.5 * np.sum(v * v, axis=1) + 2.0 * np.abs(half_logdet)[:, None]).T


def clnl_from_rows(plan, rows, log10_A, gamma, form="cholesky", with_scale=False):
    """lnl_ratio [R, n_orf, G] of rows [R, sum N_a] at the grid points (log10_A [G], gamma [G]), in NumPy, in one of the two forms of
    clnl_ratio; with_scale: (lnl_ratio, scale), scale [R, n_orf, G] the size of the terms it is the difference of."""
    rows = np.atleast_2d(np.asarray(rows, dtype=np.float64))
    Y = project(plan.os, rows)
    R, C = rows.shape[0], plan.C
    d = clnl_scale(plan.nf, plan.T, plan.gamma_ref, log10_A, gamma)
    out, scale = np.zeros((R, len(plan.names), d.shape[0])), np.zeros((R, len(plan.names), d.shape[0]))
    for o, (B, T) in enumerate(zip(plan.B, plan.T_orf)):
        rho = B.shape[1]
        Yp = np.einsum("ai,rac->ric", B, Y).reshape(R, rho * C)
        out[:, o, :], scale[:, o, :] = clnl_ratio(T, Yp, np.tile(d, (1, rho)), form)
    return (out, scale) if with_scale else out
