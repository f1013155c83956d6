// One continuous-wave source per realisation in throughput / TD mode: the uniform prior map of the CW labels, the per-(realisation,
// pulsar) scalars of add_cgw (deterministic.py:51-109) and the per-TOA waveform (:111-163) in a well-conditioned form.
//
// The reference's evolving phase phase0 + fac2 (w0^(-5/3) - omega(t)^(-5/3)) subtracts two nearly equal powers scaled by
// Phi = fac2 w0^(-5/3) = 1 / (32 (mc w0)^(5/3)) rad (up to 1e10 rad over a usual CW prior: 1e-6 relative error in fp64).  With
// l = log1p(-fac1 t) and d = expm1(l / 8) = (1 - fac1 t)^(1/8) - 1 the same quantities are
//     omega = w0 (1 + d)^-3,   phase = phase0 - Phi ((1 + d)^5 - 1) = phase0 - Phi d (5 + d (10 + d (10 + d (5 + d)))),
//     alpha = fac3 omega^(-1/3) = fac3 w0^(-1/3) (1 + d)
// without cancellation, one log1p + one expm1 per term instead of three pow.  A TOA after the merger (1 - fac1 t < 0: NaN) contributes
// 0, the rule of add_catalog_of_cws (deterministic.py:435,556).
//
// Everything is __host__ __device__: tests/cw compiles this header with g++ (-ffp-contract=off) and checks it against a long-double
// evaluation of the reference's expressions.
#pragma once
#include <stdint.h>
#include <math.h>
#include "pta_rng.h"

// constants.py (scipy.constants G, c, parsec; the reference's solar mass), as exact binary64 values
#define PTA_SOLAR2S 0x1.4a9140e71f62fp-18   // 4.925838061995516e-06 s
#define PTA_KPC2S 0x1.7f6ef4a3e56c8p+36     // 102927125054.33899 s
#define PTA_MPC2S 0x1.76725ae80e0bfp+46     // 102927125054338.98 s

// columns of the per-realisation source table (the CW labels, and the pairs of stream (CW, 0) that draw them)
#define PTA_CW_COL_COS_GWTHETA 0
#define PTA_CW_COL_GWPHI 1
#define PTA_CW_COL_LOG10_MC 2    // [Msun]
#define PTA_CW_COL_LOG10_FGW 3   // [Hz]
#define PTA_CW_COL_LOG10_AMP 4   // log10 h (strain) or log10 dist [Mpc]
#define PTA_CW_COL_PHASE0 5
#define PTA_CW_COL_PSI 6
#define PTA_CW_COL_COS_INC 7
#define PTA_CW_COL_PDIST 8       // + pulsar: pdist [kpc] (optional columns)
#define PTA_CW_NSRC 8

// scalar table of one (realisation, pulsar): PTA_CW_ENGINE_NPAR doubles
#define PTA_CW_P_W0 0        // pi fgw [rad/s]
#define PTA_CW_P_PHASE0 1    // orbital phase0 = phase0 / 2
#define PTA_CW_P_PHI 2       // fac2 w0^(-5/3) = 1 / (32 (mc w0)^(5/3)) [rad]
#define PTA_CW_P_FAC1 3      // 256/5 mc^(5/3) w0^(8/3) [1/s]
#define PTA_CW_P_AMP 4       // fac3 w0^(-1/3) [s]
#define PTA_CW_P_INCFAC1 5
#define PTA_CW_P_INCFAC2 6
#define PTA_CW_P_COS2PSI 7
#define PTA_CW_P_SIN2PSI 8
#define PTA_CW_P_FPLUS 9
#define PTA_CW_P_FCROSS 10
#define PTA_CW_P_PDC 11      // pd (1 - cos mu) [s]
#define PTA_CW_P_OMEGA_P 12  // phase_approx: w0 (1 + fac1 pd (1 - cos mu))^(-3/8)
#define PTA_CW_P_PHASE_P 13  // phase_approx: phase0 + fac2 (w053 - omega_p^(-5/3))
#define PTA_CW_P_AMP_P 14    // phase_approx: fac3 omega_p^(-1/3)

// label column j of realisation `realisation` drawn uniformly from [lo, hi): stream (CW, 0), pair j, u2 (the map of pta_hyper_draw)
PTA_HD double pta_cw_draw(uint64_t seed, uint64_t realisation, uint32_t j, double lo, double hi) {
  return pta_box_draw(seed, realisation, pta_stream_id(PTA_STREAM_CW, 0u), j, lo, hi);
}

// (1 + d)^5 - 1
PTA_HD double pta_cw_poly5(double d) { return d * (5.0 + d * (10.0 + d * (10.0 + d * (5.0 + d)))); }

// h -> fac3 w0^(-1/3) = h / (2 w0);  dist [Mpc] -> mc^(5/3) w0^(-1/3) / dist = (mc w0)^(5/3) / (w0^2 dist)
PTA_HD double pta_cw_amp(double log10_amp, int amp_is_h, double w0, double mw53) {
  const double a = pow(10.0, log10_amp);
  return amp_is_h ? a / (2.0 * w0) : mw53 / (w0 * w0 * (a * PTA_MPC2S));
}

// the scalars of one source seen from one pulsar (unit vector phat, distance pdist [kpc]); mode 0 evolve, 1 phase_approx, 2 mono
PTA_HD void pta_cw_params(const double *src, int amp_is_h, const double *phat, double pdist, int mode, double *par) {
  const double c = src[PTA_CW_COL_COS_GWTHETA];
  const double s = sqrt((1.0 - c) * (1.0 + c));  // sin(gwtheta), accurate at c -> +-1
  double sgp, cgp, s2p, c2p;
  sincos(src[PTA_CW_COL_GWPHI], &sgp, &cgp);
  sincos(2.0 * src[PTA_CW_COL_PSI], &s2p, &c2p);
  const double mc = pow(10.0, src[PTA_CW_COL_LOG10_MC]) * PTA_SOLAR2S;
  const double w0 = 3.14159265358979323846 * pow(10.0, src[PTA_CW_COL_LOG10_FGW]);
  const double mw53 = pow(mc * w0, 5.0 / 3.0);
  const double Phi = 1.0 / (32.0 * mw53);
  const double fac1 = 51.2 * mw53 * w0;
  const double amp = pta_cw_amp(src[PTA_CW_COL_LOG10_AMP], amp_is_h, w0, mw53);
  const double ci = src[PTA_CW_COL_COS_INC];
  // m = (sin phi, -cos phi, 0), n = (-cos theta cos phi, -cos theta sin phi, sin theta), omhat = (-sin theta cos phi, -sin theta sin phi,
  // -cos theta) (deterministic.py:85-87)
  const double mp = sgp * phat[0] - cgp * phat[1];
  const double np_ = (-c * cgp * phat[0] - c * sgp * phat[1]) + s * phat[2];
  const double op = (-s * cgp * phat[0] - s * sgp * phat[1]) - c * phat[2];
  const double phase0 = 0.5 * src[PTA_CW_COL_PHASE0];
  par[PTA_CW_P_W0] = w0;
  par[PTA_CW_P_PHASE0] = phase0;
  par[PTA_CW_P_PHI] = Phi;
  par[PTA_CW_P_FAC1] = fac1;
  par[PTA_CW_P_AMP] = amp;
  par[PTA_CW_P_INCFAC1] = 0.5 * (3.0 + (2.0 * ci * ci - 1.0));  // cos 2 inc = 2 cos^2 inc - 1
  par[PTA_CW_P_INCFAC2] = 2.0 * ci;
  par[PTA_CW_P_COS2PSI] = c2p;
  par[PTA_CW_P_SIN2PSI] = s2p;
  par[PTA_CW_P_FPLUS] = 0.5 * (mp * mp - np_ * np_) / (1.0 + op);
  par[PTA_CW_P_FCROSS] = (mp * np_) / (1.0 + op);
  const double pdc = pdist * PTA_KPC2S * (1.0 + op);  // pd (1 - cos mu), cos mu = -omhat . phat
  par[PTA_CW_P_PDC] = pdc;
  double om_p = 0.0, ph_p = 0.0, amp_p = 0.0;
  if (mode == 1) {  // (1 + fac1 pd (1 - cos mu))^(1/8) = 1 + d
    const double d = expm1(0.125 * log1p(fac1 * pdc));
    const double q = 1.0 + d;
    om_p = w0 / (q * q * q);
    ph_p = phase0 - Phi * pta_cw_poly5(d);
    amp_p = amp * q;
  }
  par[PTA_CW_P_OMEGA_P] = om_p;
  par[PTA_CW_P_PHASE_P] = ph_p;
  par[PTA_CW_P_AMP_P] = amp_p;
  par[15] = 0.0;
}

// plus / cross polarisation residual of one term: alpha (A cos 2psi + B sin 2psi), alpha (-A sin 2psi + B cos 2psi)
PTA_HD void pta_cw_pol(const double *par, double phase, double alpha, double &rplus, double &rcross) {
  double s, c;
  sincos(2.0 * phase, &s, &c);
  const double At = s * par[PTA_CW_P_INCFAC1], Bt = c * par[PTA_CW_P_INCFAC2];
  const double c2p = par[PTA_CW_P_COS2PSI], s2p = par[PTA_CW_P_SIN2PSI];
  rplus = alpha * (At * c2p + Bt * s2p);
  rcross = alpha * (-At * s2p + Bt * c2p);
}

// phase and amplitude of the evolving waveform at time t [s] (t relative to tref)
PTA_HD void pta_cw_evolve(const double *par, double t, double &phase, double &alpha) {
  const double d = expm1(0.125 * log1p(-par[PTA_CW_P_FAC1] * t));
  phase = par[PTA_CW_P_PHASE0] - par[PTA_CW_P_PHI] * pta_cw_poly5(d);
  alpha = par[PTA_CW_P_AMP] * (1.0 + d);
}

// residual [s] of the source at t = mjd * 86400 - tref; 0 where it is not finite (after the merger)
template <int MODE, int PSR_TERM>
PTA_HD double pta_cw_wave(const double *par, double t) {
  double ph, al, ph_p = 0.0, al_p = 0.0;
  if (MODE == 0) {
    pta_cw_evolve(par, t, ph, al);
    if (PSR_TERM) pta_cw_evolve(par, t - par[PTA_CW_P_PDC], ph_p, al_p);
  } else {
    ph = par[PTA_CW_P_PHASE0] + par[PTA_CW_P_W0] * t;
    al = par[PTA_CW_P_AMP];
    if (PSR_TERM) {
      if (MODE == 1) {
        ph_p = par[PTA_CW_P_PHASE_P] + par[PTA_CW_P_OMEGA_P] * t;
        al_p = par[PTA_CW_P_AMP_P];
      } else {
        ph_p = par[PTA_CW_P_PHASE0] + par[PTA_CW_P_W0] * (t - par[PTA_CW_P_PDC]);
        al_p = al;
      }
    }
  }
  double rp, rc;
  pta_cw_pol(par, ph, al, rp, rc);
  double r;
  if (PSR_TERM) {
    double rp_p, rc_p;
    pta_cw_pol(par, ph_p, al_p, rp_p, rc_p);
    r = par[PTA_CW_P_FPLUS] * (rp_p - rp) + par[PTA_CW_P_FCROSS] * (rc_p - rc);
  } else {
    r = -par[PTA_CW_P_FPLUS] * rp - par[PTA_CW_P_FCROSS] * rc;
  }
  return isfinite(r) ? r : 0.0;
}

// runtime-mode form of pta_cw_wave (host checks)
PTA_HD double pta_cw_wave_rt(const double *par, double t, int mode, int psr_term) {
  if (mode == 0) return psr_term ? pta_cw_wave<0, 1>(par, t) : pta_cw_wave<0, 0>(par, t);
  if (mode == 1) return psr_term ? pta_cw_wave<1, 1>(par, t) : pta_cw_wave<1, 0>(par, t);
  return psr_term ? pta_cw_wave<2, 1>(par, t) : pta_cw_wave<2, 0>(par, t);
}
