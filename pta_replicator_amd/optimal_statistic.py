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
        CiM = CiG[:, nf2:]
        A = M.T @ CiM
        A = 0.5 * (A + A.T)
        dg = np.sqrt(np.abs(np.diag(A)))
        if not np.all(dg > 0):
            raise ValueError("M^T C^-1 M is singular: a timing-model column vanishes on this pulsar's TOAs")
        An = A / dg[:, None] / dg[None, :]
        ev = np.linalg.eigvalsh(An)
        if ev[0] <= 1e-12 * ev[-1]:
            raise ValueError(f"M^T C^-1 M is singular (condition {ev[-1] / max(ev[0], 1e-300):.3g}): the pulsar's TOAs do not "
                             "constrain its timing model")
        PF = PF - CiM @ (np.linalg.solve(An, (M.T @ PF) / dg[:, None]) / dg[:, None])
    rs = np.sqrt(S)
    W = (PF * rs[None, :]).T / s
    Z = rs[:, None] * (F.T @ PF) * rs[None, :] / s
    return W, 0.5 * (Z + Z.T)


def _cho_solve(L, B):
    return np.linalg.solve(L.T, np.linalg.solve(L, B))


class OSPlan:
    """realisation-independent operands of the OS: W (list of [2 nf, N_a]), Z ([P, 2 nf, 2 nf]), den / pairs / weights."""

    def __init__(self, W, Z, pair_a, pair_b, cos_zeta, names, G):
        self.W, self.Z = W, Z
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
    if not 1 <= int(components) <= 32:
        raise ValueError(f"components={components}: 1 .. 32 frequencies (2 n_f <= 64 columns)")
    nf = int(components)
    if T is None:
        T = max(float(np.max(t)) for t in toas_s) - min(float(np.min(t)) for t in toas_s)
    S = unit_spectrum(nf, T, gamma)
    pair_a, pair_b, cz = pair_geometry(pos)
    names, G = orf_weights(orfs, pair_a, pair_b, cz, P)

    def pick(x, a):
        return None if x is None else x[a]
    W, Z = [], np.zeros((P, 2 * nf, 2 * nf))
    for a in range(P):
        F = fourier_basis(toas_s[a], nf, T)
        Wa, Za = pulsar_operator(sigma2[a], F, S, pick(epoch_of, a), pick(ecorr, a), pick(F_rn, a), pick(phi_rn, a), gw_amp2, pick(M, a))
        W.append(Wa)
        Z[a] = Za
    return OSPlan(W, Z, pair_a, pair_b, cz, names, G)


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
