// Sine-Gaussian wavelets per realisation in throughput / TD mode (ReplicaEngine.set_burst, set_transients): the reference's add_burst
// (deterministic.py:718-793) and add_noise_transient (:796-819) with the callables taken from one family,
//
//     wavelet(t) = g(t) cos(2 pi f (t - t0) + phi),   g = exp(-1/2 ((t - t0) / tau)^2),   t = mjd * 86400,  t0 = t0_mjd * 86400
//
// (the envelope convention of the reference's golden, tau = the Gaussian's standard deviation).  A GW burst is a coherent sum of W
// wavelets from one sky position: h+ = sum_w A+_w g_w cos(w_w dt_w + phi+_w), hx likewise with Ax_w, phix_w, and
// res_a = -F+_a (h+ c2psi - hx s2psi) - Fx_a (h+ s2psi + hx c2psi).  Per (realisation, pulsar, wavelet) this folds into
//
//     g (C cos(w dt) + S sin(w dt)),   k+ = -(F+ c2psi + Fx s2psi),  kx = F+ s2psi - Fx c2psi,
//     C = k+ A+ cos phi+ + kx Ax cos phix,   S = -(k+ A+ sin phi+ + kx Ax sin phix).
//
// A noise transient is one wavelet in one pulsar: C = A cos phi, S = -A sin phi.  The phase is taken in turns, u = f dt split into its
// rounded product and the product's rounding error (one fma), reduced to [0, 1) and fed to pta_sincos_2pi_poly: no radian sincos of an
// argument in the thousands, and no table (the function is the same instructions on the host).
//
// Everything is __host__ __device__: tests/burst compiles this header with g++ (-ffp-contract=off) and checks it against the golden
// output of the reference and against a long-double evaluation of its expression.
#pragma once
#include <stdint.h>
#include <math.h>
#include "pta_rng.h"
#include "pta_bwm.h"

#define PTA_STREAM_BURST 13u  // field 0: the burst's sky labels, pair = column; field 1 + w: wavelet w, pair = column (pta_burst.h)
#define PTA_STREAM_NT 14u     // field v: noise transient v of the realisation, pair = column (pta_burst.h)

// label columns of a burst: the sky row [3] and the wavelet rows [W, 7] (the pairs of the streams that draw them)
#define PTA_BURST_SKY_COS_GWTHETA 0
#define PTA_BURST_SKY_GWPHI 1
#define PTA_BURST_SKY_PSI 2
#define PTA_BURST_NSKY 3
#define PTA_BURST_COL_T0_MJD 0
#define PTA_BURST_COL_LOG10_TAU 1
#define PTA_BURST_COL_LOG10_F 2
#define PTA_BURST_COL_LOG10_A_PLUS 3
#define PTA_BURST_COL_PHASE_PLUS 4
#define PTA_BURST_COL_LOG10_A_CROSS 5
#define PTA_BURST_COL_PHASE_CROSS 6
#define PTA_BURST_NCOL 7
// label columns of a noise transient [V, 6]
#define PTA_NT_COL_PSR 0
#define PTA_NT_COL_T0_MJD 1
#define PTA_NT_COL_LOG10_TAU 2
#define PTA_NT_COL_LOG10_F 3
#define PTA_NT_COL_LOG10_A 4
#define PTA_NT_COL_PHASE 5
#define PTA_NT_NCOL 6
// rows of the tables the add kernels read
#define PTA_BURST_NTAB 7  // (t0_s, -1/2 / tau^2, f, A+ cos phi+, A+ sin phi+, Ax cos phix, Ax sin phix)
#define PTA_NT_NTAB 6     // (psr, t0_s, -1/2 / tau^2, f, A cos phi, -A sin phi)
#define PTA_BURST_WMAX 128

// envelope arguments below this give exp = 0 exactly in fp64 (2^-1074 = e^-744.44; the bound |dt| > 38.7 tau is arg < -748.8): a
// wavelet whose every lane of a wave is below it may be skipped without changing a bit
#define PTA_BURST_ARG_ZERO (-748.0)

PTA_HD double pta_burst_sky_draw(uint64_t seed, uint64_t realisation, uint32_t j, double lo, double hi) {
  return pta_box_draw(seed, realisation, pta_stream_id(PTA_STREAM_BURST, 0u), j, lo, hi);
}
PTA_HD double pta_burst_wavelet_draw(uint64_t seed, uint64_t realisation, uint32_t w, uint32_t j, double lo, double hi) {
  return pta_box_draw(seed, realisation, pta_stream_id(PTA_STREAM_BURST, 1u + w), j, lo, hi);
}
PTA_HD double pta_nt_draw(uint64_t seed, uint64_t realisation, uint32_t v, uint32_t j, double lo, double hi) {
  return pta_box_draw(seed, realisation, pta_stream_id(PTA_STREAM_NT, v), j, lo, hi);
}
// the pulsar of a drawn transient: the floor of the U(0, P) draw, kept below P where the draw lands on the box's upper edge
PTA_HD double pta_nt_psr(double x, int P) { return fmin(fmax(floor(x), 0.0), (double)(P - 1)); }

// (t0_s, -1/2 / tau^2, f) of a wavelet from (t0_mjd, log10_tau, log10_f)
PTA_HD void pta_wavelet_shape(double t0_mjd, double log10_tau, double log10_f, double *tab) {
  const double tau = pow(10.0, log10_tau);
  tab[0] = t0_mjd * 86400.0;
  tab[1] = -0.5 / (tau * tau);
  tab[2] = pow(10.0, log10_f);
}

// table row of one burst wavelet (src: its PTA_BURST_NCOL label columns)
PTA_HD void pta_burst_wavelet_row(const double *src, double *tab) {
  pta_wavelet_shape(src[PTA_BURST_COL_T0_MJD], src[PTA_BURST_COL_LOG10_TAU], src[PTA_BURST_COL_LOG10_F], tab);
  const double ap = pow(10.0, src[PTA_BURST_COL_LOG10_A_PLUS]), ac = pow(10.0, src[PTA_BURST_COL_LOG10_A_CROSS]);
  double sp, cp, sc, cc;
  sincos(src[PTA_BURST_COL_PHASE_PLUS], &sp, &cp);
  sincos(src[PTA_BURST_COL_PHASE_CROSS], &sc, &cc);
  tab[3] = ap * cp;
  tab[4] = ap * sp;
  tab[5] = ac * cc;
  tab[6] = ac * sc;
}

// (k+, kx) of one pulsar for the burst's sky row (cos_gwtheta, gwphi, psi): the antenna patterns of pta_bwm_antenna
PTA_HD void pta_burst_antenna(const double *sky, const double *phat, double &kp, double &kc) {
  double fp, fc, s2p, c2p;
  pta_bwm_antenna(sky[PTA_BURST_SKY_COS_GWTHETA], sky[PTA_BURST_SKY_GWPHI], phat, fp, fc);
  sincos(2.0 * sky[PTA_BURST_SKY_PSI], &s2p, &c2p);
  kp = -(fp * c2p + fc * s2p);
  kc = fp * s2p - fc * c2p;
}

// (C, S) of one (pulsar, wavelet) from the pulsar's (k+, kx) and the wavelet's table row
PTA_HD void pta_burst_fold(double kp, double kc, const double *tab, double &C, double &S) {
  C = kp * tab[3] + kc * tab[5];
  S = -(kp * tab[4] + kc * tab[6]);
}

// table row of one noise transient (src: its PTA_NT_NCOL label columns)
PTA_HD void pta_nt_row(const double *src, double *tab) {
  tab[0] = src[PTA_NT_COL_PSR];
  pta_wavelet_shape(src[PTA_NT_COL_T0_MJD], src[PTA_NT_COL_LOG10_TAU], src[PTA_NT_COL_LOG10_F], tab + 1);
  const double a = pow(10.0, src[PTA_NT_COL_LOG10_A]);
  double sp, cp;
  sincos(src[PTA_NT_COL_PHASE], &sp, &cp);
  tab[4] = a * cp;
  tab[5] = -(a * sp);
}

// the envelope's argument -1/2 (dt / tau)^2 at t (nh = -1/2 / tau^2)
PTA_HD double pta_wavelet_arg(double t0, double nh, double t) {
  const double dt = t - t0;
  return nh * (dt * dt);
}

// g (C cos(2 pi f dt) + S sin(2 pi f dt)) at t, arg = pta_wavelet_arg(t0, nh, t): one exp, one sin / cos pair, two FMAs' worth of sum
PTA_HD double pta_wavelet_value(double t0, double f, double C, double S, double arg, double t) {
  const double dt = t - t0;
  const double u = f * dt, ul = fma(f, dt, -u);  // f dt = u + ul exactly
  const double fr = (u - floor(u)) + ul;         // turns in [0, 1) up to a rounding at the ends, which the reduction below takes
  double sn, cs;
  pta_sincos_2pi_poly(fr, sn, cs);
  return exp(arg) * (C * cs + S * sn);
}
