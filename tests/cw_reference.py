"""Host references of the per-realisation CW source (ReplicaEngine.set_cw): the reference's single-source waveform
(deterministic.py:50-163) evaluated in np.longdouble in the conditioned form of pta_cw_hyper.h, and helpers that turn a source of the
cw_* parameterisation into add_cgw / oracle.cgw_dt arguments."""
import numpy as np

from pta_replicator_amd.constants import KPC2S, MPC2S, SOLAR2S

L = np.longdouble
PI_L = L("3.14159265358979323846264338327950288")
SRC = ("cos_gwtheta", "gwphi", "log10_mc", "log10_fgw", "amp", "phase0", "psi", "cos_inc")


def phi_rad(log10_mc, log10_fgw):
    """Phi = 1 / (32 (mc w0)^(5/3)) [rad]: the scale of the reference formula's cancellation."""
    return 1.0 / (32 * (10.0 ** log10_mc * SOLAR2S * np.pi * 10.0 ** log10_fgw) ** (5 / 3))


def _poly5(d):
    return d * (5 + d * (10 + d * (10 + d * (5 + d))))


def wave_ld(toa_s, ra, dec, src, amp_is_h, pdist, mode, psr_term, tref):
    """residual [s] (float64) of source `src` (8 values in SRC order, floats) for a pulsar at (ra, dec) at the float64 times
    toa_s = mjd * 86400; t = toa_s - tref rounded in float64 as the reference does, the pulsar's unit vector in float64 as the
    reference computes it, everything else in long double."""
    c, gwphi, lmc, lfgw, lamp, phase0, psi, ci = (L(float(x)) for x in src)
    s = np.sqrt((1 - c) * (1 + c))
    cgp, sgp = np.cos(gwphi), np.sin(gwphi)
    # the pulsar's unit vector is an input: float64, the reference's expression (deterministic.py:88), as the engine uploads it
    ptheta, pphi = np.pi / 2 - float(dec), float(ra)
    phat = np.array([np.sin(ptheta) * np.cos(pphi), np.sin(ptheta) * np.sin(pphi), np.cos(ptheta)]).astype(L)
    m = np.array([sgp, -cgp, L(0)])
    n = np.array([-c * cgp, -c * sgp, s])
    om = np.array([-s * cgp, -s * sgp, -c])
    mp, np_, op = np.sum(m * phat), np.sum(n * phat), np.sum(om * phat)
    fplus = L(0.5) * (mp ** 2 - np_ ** 2) / (1 + op)
    fcross = mp * np_ / (1 + op)
    cosmu = -op
    mc = L(10) ** lmc * L(SOLAR2S)
    w0 = PI_L * L(10) ** lfgw
    phase0 = phase0 / 2
    fac1 = L(256) / 5 * mc ** (L(5) / 3) * w0 ** (L(8) / 3)
    Phi = 1 / L(32) / mc ** (L(5) / 3) * w0 ** (L(-5) / 3)
    fac3 = (L(10) ** lamp / (2 * w0 ** (L(2) / 3))) if amp_is_h else mc ** (L(5) / 3) / (L(10) ** lamp * L(MPC2S))
    amp0 = fac3 * w0 ** (L(-1) / 3)
    pd = L(float(pdist)) * L(KPC2S)
    t = (np.asarray(toa_s, dtype=np.float64) - float(tref)).astype(L)
    tp = t - pd * (1 - cosmu)
    with np.errstate(invalid="ignore", divide="ignore"):
        if mode == 0:
            d = np.expm1(np.log1p(-fac1 * t) / 8)
            dp = np.expm1(np.log1p(-fac1 * tp) / 8)
            ph, ph_p = phase0 - Phi * _poly5(d), phase0 - Phi * _poly5(dp)
            al, al_p = amp0 * (1 + d), amp0 * (1 + dp)
        elif mode == 1:
            dq = np.expm1(np.log1p(fac1 * pd * (1 - cosmu)) / 8)
            ph, al = phase0 + w0 * t, amp0
            ph_p, al_p = phase0 - Phi * _poly5(dq) + w0 / (1 + dq) ** 3 * t, amp0 * (1 + dq)
        else:
            ph, al = phase0 + w0 * t, amp0
            ph_p, al_p = phase0 + w0 * tp, amp0
        c2p, s2p = np.cos(2 * psi), np.sin(2 * psi)
        if1, if2 = L(0.5) * (3 + (2 * ci * ci - 1)), 2 * ci

        def pol(phase, alpha):
            At, Bt = np.sin(2 * phase) * if1, np.cos(2 * phase) * if2
            return alpha * (At * c2p + Bt * s2p), alpha * (-At * s2p + Bt * c2p)
        rp, rc = pol(ph, al)
        if psr_term:
            rp_p, rc_p = pol(ph_p, al_p)
            r = fplus * (rp_p - rp) + fcross * (rc_p - rc)
        else:
            r = -fplus * rp - fcross * rc
    r = np.asarray(r, dtype=np.float64)
    return np.where(np.isfinite(r), r, 0.0)


def cgw_kwargs(src, amp_is_h):
    """add_cgw / oracle.cgw_dt keyword arguments of a source (angles from the cosines, mc / fgw / dist from the logs)."""
    c, gwphi, lmc, lfgw, lamp, phase0, psi, ci = (float(x) for x in src)
    if amp_is_h:   # dist = 2 mc^(5/3) (pi fgw)^(2/3) / h, in Mpc
        mc = 10.0 ** lmc * SOLAR2S
        dist = 2 * mc ** (5 / 3) * (np.pi * 10.0 ** lfgw) ** (2 / 3) / 10.0 ** lamp / MPC2S
    else:
        dist = 10.0 ** lamp
    return dict(gwtheta=float(np.arccos(c)), gwphi=gwphi, mc=10.0 ** lmc, dist=dist, fgw=10.0 ** lfgw, phase0=phase0, psi=psi,
                inc=float(np.arccos(ci)))


def corner_sources(R, seed=0, amp_is_h=True):
    """R sources [R, 8] spanning log10 mc in [7, 10], log10 fgw in [-9, -7] (the four corners first), with cos = +-1 edges."""
    rng = np.random.default_rng(seed)
    src = np.zeros((R, 8))
    src[:, 0] = rng.uniform(-1, 1, R)
    src[:, 1] = rng.uniform(0, 2 * np.pi, R)
    src[:, 2] = rng.uniform(7, 10, R)
    src[:, 3] = rng.uniform(-9, -7, R)
    src[:, 5] = rng.uniform(0, 2 * np.pi, R)
    src[:, 6] = rng.uniform(0, np.pi, R)
    src[:, 7] = rng.uniform(-1, 1, R)
    corners = [(7, -9), (7, -7), (10, -9), (10, -7), (8.5, -8.5), (7.0, -9.0), (9.5, -7.5)]
    for i, (m, f) in enumerate(corners[:R]):
        src[i, 2], src[i, 3] = m, f
    edges = [(0, 1.0), (1, -1.0), (2, 1.0), (3, -1.0)]
    for i, e in edges:
        if i < R:
            src[i, 0] = e
        if i + 4 < R:
            src[i + 4, 7] = e
    if amp_is_h:
        src[:, 4] = rng.uniform(-16, -13, R)
    else:
        src[:, 4] = rng.uniform(1, 3, R)
    return src


def theta_of(src, amp_is_h, pdist=None):
    """the cw_* theta dict of a [R, 8] source array (and an optional [R, P] pdist)."""
    th = {"cw_" + k: src[:, j].copy() for j, k in enumerate(SRC) if k != "amp"}
    th["cw_log10_h" if amp_is_h else "cw_log10_dist"] = src[:, 4].copy()
    if pdist is not None:
        th["cw_pdist"] = np.asarray(pdist, dtype=np.float64)
    return th
