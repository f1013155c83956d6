"""Host preparation of the Earth-term burst-with-memory (BWM) matched filter, pure NumPy.

A two-amplitude F-statistic on a grid of burst epochs t0_j [s], j < J, and sky points Omega_s, s < S.  For pulsar a with N_a TOAs
t [s] (t = mjd * 86400, the time the injected ramp of _bwm / pta_bwm.h runs on), noise covariance C_a (white noise + ECORR + red noise,
optionally the GWB auto-term: what optimal_statistic.pulsar_operator assembles) and timing-model design matrix M_a:

    P_a^-1   C^-1 - C^-1 M (M^T C^-1 M)^-1 M^T C^-1                         (timing model marginalised, exactly as in f_statistic.py)
    e_aj     max(t - t0_j, 0)                                               the ramp template [N_a]
    W_a      row j = e_aj^T P_a^-1                                          [J, N_a]
    g_aj     e_aj^T P_a^-1 e_aj

and per realisation q_raj = W_a[j] . r_a,

    N_rjs = sum_a phi_as q_raj  (a 2-vector),   M_js = sum_a phi_as phi_as^T g_aj  [2, 2]
    Fb[r, j, s] = 1/2 N_rjs^T M_js^-1 N_rjs,    A_rjs = M_js^-1 N_rjs = (h cos 2psi, h sin 2psi)   the amplitude estimate

phi_as = (F+_a, Fx_a) at sky point s (f_statistic.antenna_patterns: the m, n, Omega of deterministic.add_gw_memory), so the statistic
matches what set_bwm injects: s_a = h (cos 2psi F+ + sin 2psi Fx) e_a.  Under the model's own noise 2 Fb ~ chi^2(2); a burst at
(t0_j, Omega_s) gives Fb = rho^2 / 2 on its noiseless term, rho^2 = sum_a s_a^T P_a^-1 s_a, and A recovers (h cos 2psi, h sin 2psi).

A pulsar can be insensitive to an epoch: all its TOAs before t0_j (e = 0), or all after it (e is linear in t and the spin-down fit
absorbs it, leaving rounding noise of either sign).  white_aj = sum_i e_i^2 / sigma_i^2 bounds g_aj from above; where g_aj <= SINGULAR
white_aj (or white_aj = 0) W_a[j] and g_aj are set to exactly zero - that pulsar contributes nothing at that epoch, which is not an
error.  A singular M_js is: an epoch outside every pulsar's span, or fewer than two sensitive pulsars.

The per-realisation half runs on the device (pta_fstat_project, pta_bwm_stat); this module builds W, g, phi and M^-1 once and holds a
NumPy evaluation of the per-realisation half (``bwm_from_rows``) for tests.

Out of scope: the pulsar term and the single-pulsar ramp statistic, a statistic matched to per-realisation noise parameters theta,
more than one burst per realisation, maximising over a continuous epoch (the epochs are a grid).
"""
import numpy as np

from . import f_statistic as fst
from . import optimal_statistic as ost

SINGULAR = fst.SINGULAR   # g_aj / white_aj, and smallest / largest eigenvalue of a normalised M_js, at which they count as zero


def check_epochs(t0):
    """[J] burst epochs validated (finite, 1-D, non-empty), in the unit they were given."""
    t = np.atleast_1d(np.asarray(t0, dtype=np.float64))
    if t.ndim != 1 or t.size < 1:
        raise ValueError(f"the burst epochs must be a non-empty 1-D array, got shape {np.shape(t0)}")
    if not np.all(np.isfinite(t)):
        raise ValueError("the burst epochs must be finite")
    return np.ascontiguousarray(t)


def ramp_basis(toas_s, t0_s):
    """E [N, J]: column j = max(t - t0_j, 0)."""
    return np.maximum(np.asarray(toas_s, dtype=np.float64)[:, None] - np.asarray(t0_s, dtype=np.float64)[None, :], 0.0)


def _inverse_2x2(M, t0_s):
    """M [J, S, 2, 2] symmetric -> its inverse, refusing a singular M_js (the normalised-eigenvalue criterion of
    f_statistic._refuse_singular) with the epoch and the sky point named."""
    dg = np.sqrt(np.abs(np.diagonal(M, axis1=-2, axis2=-1)))
    ok = np.all(dg > 0, axis=-1)
    Mn = M / np.where(dg > 0, dg, 1.0)[..., :, None] / np.where(dg > 0, dg, 1.0)[..., None, :]
    ev = np.linalg.eigvalsh(Mn)
    bad = ~ok | (ev[..., 0] <= SINGULAR * ev[..., -1])
    if np.any(bad):
        j, s = (int(x) for x in np.argwhere(bad)[0])
        raise ValueError(f"M_js = sum_a (phi phi^T) g_aj is singular at epoch {j} (MJD {t0_s[j] / 86400.0:.6f}), sky point {s}: fewer than "
                         "two pulsars are sensitive to a burst at that epoch (it lies outside their data, or the timing-model fit "
                         "absorbs its ramp)")
    inv = np.linalg.inv(Mn) / dg[..., :, None] / dg[..., None, :]
    return 0.5 * (inv + np.swapaxes(inv, -1, -2))


class BwmPlan:
    """realisation-independent operands: t0_s [J], W (list of [J, N_a]), g [P, J], phi [P, S, 2], M and Minv [J, S, 2, 2], the sky grid."""

    def __init__(self, t0_s, W, g, phi, sky):
        self.t0_s, self.W, self.g, self.phi, self.sky = t0_s, W, g, phi, sky
        self.P, self.J, self.S = len(W), len(t0_s), phi.shape[1]
        self.counts = np.array([w.shape[1] for w in W])
        self.off = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int64)
        pp = phi[:, :, :, None] * phi[:, :, None, :]                      # [P, S, 2, 2]
        M = np.einsum("aspq,aj->jspq", pp, g)
        self.M = 0.5 * (M + np.swapaxes(M, -1, -2))
        self.Minv = _inverse_2x2(self.M, t0_s)

    @property
    def C(self):
        """operator rows of the device projection: J rounded up to even (pta_fstat_project wants an even count)"""
        return self.J + (self.J & 1)

    def Wt(self):
        """[C, sum N_a]: W of every pulsar over the concatenated TOAs, a zero row for the pad (the device operand of pta_fstat_project)."""
        Wt = np.zeros((self.C, int(self.off[-1])))
        Wt[:self.J] = np.concatenate(self.W, axis=1)
        return Wt

    def Minv_packed(self):
        """[J, S, 3]: (M^-1_00, M^-1_01, M^-1_11) - pta_bwm_stat's operand."""
        return np.ascontiguousarray(np.stack([self.Minv[..., 0, 0], self.Minv[..., 0, 1], self.Minv[..., 1, 1]], axis=-1))


def prepare(toas_s, sigma2, t0_s, phat, sky, epoch_of=None, ecorr=None, F_rn=None, phi_rn=None, M=None):
    """BwmPlan of an array: per-pulsar lists toas_s [s], sigma2, epoch_of / ecorr (entries None = no ECORR), F_rn / phi_rn (None = no
    low-rank term; the GWB auto-term enters as further columns of F_rn with prior variances A_gw^2 S), M (None = no timing model); t0_s
    [J] burst epochs in seconds (mjd * 86400); sky = (cos_gwtheta [S], gwphi [S]) with phat [P, 3] the pulsars' unit vectors
    (_cw.pulsar_vectors)."""
    t0_s = check_epochs(t0_s)
    sky = fst.check_sky(sky)
    if sky is None:
        raise ValueError("the BWM statistic needs a sky grid: sky = (cos_gwtheta [S], gwphi [S])")
    P, J = len(toas_s), len(t0_s)
    if P < 2:
        raise ValueError("the BWM statistic needs at least two pulsars (M_js is singular for one)")
    if phat is None:
        raise ValueError("a sky grid needs the pulsars' unit vectors")
    pick = ost.pick
    W, g = [], np.zeros((P, J))
    ones = np.ones(J)
    for a in range(P):
        E = ramp_basis(toas_s[a], t0_s)
        Wa, Za = ost.pulsar_operator(sigma2[a], E, ones, pick(epoch_of, a), pick(ecorr, a), pick(F_rn, a), pick(phi_rn, a), 0.0, pick(M, a))
        ga = np.diag(Za).copy()
        white = np.sum(E ** 2 / np.asarray(sigma2[a], dtype=np.float64)[:, None], axis=0)
        gone = (white == 0) | (ga <= SINGULAR * white)    # no TOA after the epoch, or a ramp the timing-model fit absorbs
        Wa = np.array(Wa)
        Wa[gone] = 0.0
        ga[gone] = 0.0
        W.append(np.ascontiguousarray(Wa))
        g[a] = ga
    phi = fst.antenna_patterns(phat, sky[0], sky[1])
    return BwmPlan(t0_s, W, g, phi, sky)


def project(plan, rows):
    """Q [R, P, J] = W_a r_a of rows [R, sum N_a] (NumPy)."""
    rows = np.atleast_2d(np.asarray(rows, dtype=np.float64))
    return np.stack([rows[:, plan.off[a]:plan.off[a + 1]] @ plan.W[a].T for a in range(plan.P)], axis=1)


def bwm_from_Q(phi, Minv, Q):
    """(Fb [R, J, S], A [R, J, S, 2]) from phi [P, S, 2], Minv [J, S, 2, 2] and Q [R, P, J]."""
    N = np.einsum("asp,raj->rjsp", phi, Q)
    A = np.einsum("jspq,rjsq->rjsp", Minv, N)
    return 0.5 * np.einsum("rjsp,rjsp->rjs", N, A), A


def bwm_from_rows(plan, rows):
    """the whole per-realisation half in NumPy: (Fb [R, J, S], A [R, J, S, 2])."""
    return bwm_from_Q(plan.phi, plan.Minv, project(plan, rows))
