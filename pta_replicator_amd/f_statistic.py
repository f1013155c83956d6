"""Host preparation of the continuous-wave F-statistics (fixed-noise Fp and earth-term Fe), pure NumPy.

For pulsar a with N_a TOAs t [s], noise covariance C_a (white noise + ECORR + red noise, optionally the GWB auto-term: what
optimal_statistic.pulsar_operator assembles), timing-model design matrix M_a and a grid of GW frequencies f_j [Hz], j < J:

    P_a^-1   C^-1 - C^-1 M (M^T C^-1 M)^-1 M^T C^-1                         (timing model marginalised)
    E_aj     [sin 2 pi f_j t, cos 2 pi f_j t]                               [N_a, 2]
    W_a      rows 2 j, 2 j + 1 = E_aj^T P_a^-1                              [2 J, N_a]
    G_aj     E_aj^T P_a^-1 E_aj                                             [2, 2]

and per realisation q_raj = W_a[2 j : 2 j + 2] r_a,

    Fp[r, j]    = 1/2 sum_a q_raj^T G_aj^-1 q_raj                                    (Ellis, Siemens & Creighton 2012)
    Fe[r, j, s] = 1/2 N_rjs^T M_js^-1 N_rjs,   N_rjs = sum_a phi_as (x) q_raj,       (Babak & Sesana 2012; Ellis et al. 2012)
                  M_js = sum_a (phi_as phi_as^T) (x) G_aj                            [4, 4]

phi_as = (F+_a, Fx_a) at sky point s of a grid (cos_gwtheta [S], gwphi [S]), with the expressions and angle conventions of
deterministic.cw_source_params - the statistic matches what set_cw injects.  The 4-vector order is (+ sin, + cos, x sin, x cos).  The
conventional f^-1/3 scaling of the basis cancels in both statistics and is left out; t is used as it stands (both are invariant
under a common epoch).  Under the model's own noise 2 Fp ~ chi^2(2 P) and 2 Fe ~ chi^2(4); a monochromatic earth-term source at
(f_j, Omega_s) gives 2 Fe ~ chi^2(4; rho^2), rho^2 = sum_a s_a^T P_a^-1 s_a.

The per-realisation half runs on the device (pta_fstat_project, pta_fstat_fp, pta_fstat_fe); this module builds W, G^-1, phi and
M^-1 once by calling optimal_statistic.pulsar_operator (Woodbury on the low-rank part, Sherman-Morrison per ECORR epoch, no
N_a x N_a matrix), and holds a NumPy evaluation of the per-realisation half (``fstat_from_rows``) for tests.
"""
import numpy as np

from . import optimal_statistic as ost

SINGULAR = 1e-12   # smallest / largest eigenvalue of a normalised G_aj or M_js at which it is refused (pulsar_operator's criterion)
# packed upper triangle of the symmetric 4 x 4 M_js^-1, row-major: (0,0) (0,1) (0,2) (0,3) (1,1) (1,2) (1,3) (2,2) (2,3) (3,3)
TRI_I, TRI_J = np.triu_indices(4)


def check_freqs(freqs):
    f = np.atleast_1d(np.asarray(freqs, dtype=np.float64))
    if f.ndim != 1 or f.size < 1:
        raise ValueError(f"freqs must be a non-empty 1-D array of GW frequencies [Hz], got shape {np.shape(freqs)}")
    if not np.all(np.isfinite(f)) or np.any(f <= 0):
        raise ValueError("freqs must be finite and > 0 [Hz]")
    return np.ascontiguousarray(f)


def check_sky(sky):
    """(cos_gwtheta [S], gwphi [S]) validated, or None."""
    if sky is None:
        return None
    if not isinstance(sky, (tuple, list)) or len(sky) != 2:
        raise ValueError("sky must be None or a (cos_gwtheta [S], gwphi [S]) pair")
    c, p = (np.atleast_1d(np.asarray(x, dtype=np.float64)) for x in sky)
    if c.ndim != 1 or c.shape != p.shape or c.size < 1:
        raise ValueError(f"sky: cos_gwtheta and gwphi must be 1-D of one length S >= 1, got shapes {c.shape} and {p.shape}")
    if not np.all(np.isfinite(c)) or not np.all(np.isfinite(p)):
        raise ValueError("sky: non-finite values")
    if np.any(np.abs(c) > 1):
        raise ValueError("sky: |cos_gwtheta| > 1")
    return np.ascontiguousarray(c), np.ascontiguousarray(p)


def cw_basis(toas_s, freqs):
    """E [N, 2 J]: column 2 j = sin(2 pi f_j t), 2 j + 1 = cos(2 pi f_j t)."""
    arg = 2 * np.pi * np.asarray(toas_s, dtype=np.float64)[:, None] * np.asarray(freqs, dtype=np.float64)[None, :]
    E = np.empty((arg.shape[0], 2 * arg.shape[1]))
    E[:, 0::2], E[:, 1::2] = np.sin(arg), np.cos(arg)
    return E


def antenna_patterns(phat, cos_gwtheta, gwphi):
    """phi [P, S, 2] = (F+, Fx) of pulsars phat [P, 3] at the sky points, the expressions of deterministic.cw_source_params:
    m = (sin gwphi, -cos gwphi, 0), n = (-cos gwtheta cos gwphi, -cos gwtheta sin gwphi, sin gwtheta), Omega = (-sin gwtheta cos gwphi,
    -sin gwtheta sin gwphi, -cos gwtheta); F+ = 1/2 ((m.p)^2 - (n.p)^2) / (1 + Omega.p), Fx = (m.p)(n.p) / (1 + Omega.p)."""
    phat = np.atleast_2d(np.asarray(phat, dtype=np.float64))
    gwtheta = np.arccos(np.asarray(cos_gwtheta, dtype=np.float64))
    gwphi = np.asarray(gwphi, dtype=np.float64)
    cgt, cgp, sgt, sgp = np.cos(gwtheta), np.cos(gwphi), np.sin(gwtheta), np.sin(gwphi)
    m = np.stack([sgp, -cgp, np.zeros_like(sgp)], axis=1)
    n = np.stack([-cgt * cgp, -cgt * sgp, sgt], axis=1)
    om = np.stack([-sgt * cgp, -sgt * sgp, -cgt], axis=1)
    mp, npd, op = phat @ m.T, phat @ n.T, phat @ om.T           # [P, S]
    if np.any(1 + op <= 1e-12):
        raise ValueError("sky: a sky point coincides with a pulsar's direction (1 + Omega.p = 0): the antenna pattern is undefined")
    return np.stack([0.5 * (mp ** 2 - npd ** 2) / (1 + op), (mp * npd) / (1 + op)], axis=2)


def _refuse_singular(A, what):
    """A [..., k, k] symmetric: refuse when the smallest eigenvalue of A / sqrt(diag diag^T) is <= SINGULAR of its largest; returns
    (normalised A, sqrt(diag))."""
    dg = np.sqrt(np.abs(np.diagonal(A, axis1=-2, axis2=-1)))
    if not np.all(dg > 0):
        raise ValueError(f"{what} is singular: a basis column vanishes under the noise model")
    An = A / dg[..., :, None] / dg[..., None, :]
    ev = np.linalg.eigvalsh(An)
    bad = ev[..., 0] <= SINGULAR * ev[..., -1]
    if np.any(bad):
        i = np.unravel_index(int(np.argmax(bad)), bad.shape)
        raise ValueError(f"{what} is singular at index {tuple(int(x) for x in i)} (condition "
                         f"{ev[i + (-1,)] / max(ev[i + (0,)], 1e-300):.3g}): the data do not constrain sin / cos at that frequency "
                         "(e.g. a frequency the timing-model fit absorbs)")
    return An, dg


def _sym_inverse(A, what):
    An, dg = _refuse_singular(A, what)
    inv = np.linalg.inv(An) / dg[..., :, None] / dg[..., None, :]
    return 0.5 * (inv + np.swapaxes(inv, -1, -2))


class FStatPlan:
    """realisation-independent operands: W (list of [2 J, N_a]), G, Ginv [P, J, 2, 2], freqs [J]; with a sky grid phi [P, S, 2], M,
    Minv [J, S, 4, 4] and the grid itself (else None)."""

    def __init__(self, freqs, W, G, phi=None, sky=None, white=None):
        self.freqs, self.W, self.G = freqs, W, G
        self.P, self.J = len(W), len(freqs)
        if white is not None:
            # white [P, J, 2] = sum_i E_i^2 / sigma_i^2 bounds diag G from above (P^-1 <= N^-1 <= diag(sigma^2)^-1): a sin / cos
            # column the timing model spans leaves rounding noise only, which the normalised criterion below cannot see
            gone = np.diagonal(G, axis1=-2, axis2=-1) <= SINGULAR * white
            if np.any(gone):
                a, j = (int(x) for x in np.argwhere(gone)[0][:2])
                raise ValueError(f"G_aj = E^T P^-1 E is singular at pulsar {a}, frequency {j} ({freqs[j]:.6g} Hz): the timing-model fit "
                                 "absorbs sin / cos at that frequency")
        self.counts = np.array([w.shape[1] for w in W])
        self.off = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int64)
        self.Ginv = _sym_inverse(G, "G_aj = E^T P^-1 E")
        self.phi, self.sky, self.M, self.Minv, self.S = phi, sky, None, None, 0
        if phi is not None:
            if self.P < 2:
                raise ValueError("the coherent Fe statistic needs at least two pulsars (M_js is singular for one); Fp alone works without "
                                 "a sky grid")
            self.S = phi.shape[1]
            pp = phi[:, :, :, None] * phi[:, :, None, :]                              # [P, S, 2, 2]
            M = np.einsum("aspq,ajkl->jspkql", pp, G).reshape(self.J, self.S, 4, 4)
            self.M = 0.5 * (M + np.swapaxes(M, -1, -2))
            self.Minv = _sym_inverse(self.M, "M_js = sum_a (phi phi^T) (x) G_aj")

    def Wt(self):
        """[2 J, sum N_a]: W of every pulsar over the concatenated TOAs (the device operand of pta_fstat_project)."""
        return np.concatenate(self.W, axis=1)

    def Ginv_packed(self):
        """[P, J, 3]: (G^-1_00, G^-1_01, G^-1_11) - pta_fstat_fp's operand."""
        return np.ascontiguousarray(np.stack([self.Ginv[..., 0, 0], self.Ginv[..., 0, 1], self.Ginv[..., 1, 1]], axis=-1))

    def Minv_packed(self):
        """[J, S, 10]: the upper triangle of M_js^-1, row-major - pta_fstat_fe's operand."""
        return np.ascontiguousarray(self.Minv[..., TRI_I, TRI_J])


def prepare(toas_s, sigma2, freqs, phat=None, sky=None, epoch_of=None, ecorr=None, F_rn=None, phi_rn=None, M=None):
    """FStatPlan of an array: per-pulsar lists toas_s [s], sigma2, epoch_of / ecorr (entries None = no ECORR), F_rn / phi_rn (None = no
    low-rank term; the GWB auto-term enters as further columns of F_rn with prior variances A_gw^2 S), M (None = no timing model);
    freqs [J] in Hz; sky = (cos_gwtheta [S], gwphi [S]) with phat [P, 3] the pulsars' unit vectors (_cw.pulsar_vectors), or None."""
    freqs = check_freqs(freqs)
    sky = check_sky(sky)
    P, J = len(toas_s), len(freqs)
    if sky is not None and P < 2:
        raise ValueError("the coherent Fe statistic needs at least two pulsars (M_js is singular for one); Fp alone works without a sky "
                         "grid")
    pick = ost.pick
    W, G, white = [], np.zeros((P, J, 2, 2)), np.zeros((P, J, 2))
    ones = np.ones(2 * J)
    for a in range(P):
        E = cw_basis(toas_s[a], freqs)
        Wa, Za = ost.pulsar_operator(sigma2[a], E, ones, pick(epoch_of, a), pick(ecorr, a), pick(F_rn, a), pick(phi_rn, a), 0.0, pick(M, a))
        W.append(np.ascontiguousarray(Wa))
        j2 = 2 * np.arange(J)
        G[a, :, 0, 0], G[a, :, 0, 1], G[a, :, 1, 1] = Za[j2, j2], Za[j2, j2 + 1], Za[j2 + 1, j2 + 1]
        G[a, :, 1, 0] = G[a, :, 0, 1]
        white[a] = np.sum(E ** 2 / np.asarray(sigma2[a], dtype=np.float64)[:, None], axis=0).reshape(J, 2)
    phi = None
    if sky is not None:
        if phat is None:
            raise ValueError("a sky grid needs the pulsars' unit vectors")
        phi = antenna_patterns(phat, sky[0], sky[1])
    return FStatPlan(freqs, W, G, phi, sky, white)


def project(plan, rows):
    """Q [R, P, 2 J] = W_a r_a of rows [R, sum N_a] (NumPy)."""
    rows = np.atleast_2d(np.asarray(rows, dtype=np.float64))
    return np.stack([rows[:, plan.off[a]:plan.off[a + 1]] @ plan.W[a].T for a in range(plan.P)], axis=1)


def fp_from_Q(Ginv, Q):
    """Fp [R, J] from Ginv [P, J, 2, 2] and Q [R, P, 2 J]."""
    q = Q.reshape(Q.shape[0], Q.shape[1], -1, 2)
    return 0.5 * np.einsum("rajk,ajkl,rajl->rj", q, Ginv, q)


def fe_from_Q(phi, Minv, Q):
    """Fe [R, J, S] from phi [P, S, 2], Minv [J, S, 4, 4] and Q [R, P, 2 J]."""
    R, P = Q.shape[:2]
    q = Q.reshape(R, P, -1, 2)
    N = np.einsum("asp,rajk->rjspk", phi, q).reshape(R, q.shape[2], phi.shape[1], 4)
    return 0.5 * np.einsum("rjsu,jsuv,rjsv->rjs", N, Minv, N)


def fstat_from_rows(plan, rows):
    """the whole per-realisation half in NumPy: (Fp [R, J], Fe [R, J, S] or None without a sky grid)."""
    Q = project(plan, rows)
    return fp_from_Q(plan.Ginv, Q), None if plan.phi is None else fe_from_Q(plan.phi, plan.Minv, Q)
