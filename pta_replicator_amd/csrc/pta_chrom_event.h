// Chromatic events per realisation in throughput / TD mode (ReplicaEngine.set_chromatic_events): deterministic terms in one pulsar that
// scale with the radio frequency, the DM dips, cusps, bumps and the yearly DM sinusoid of real arrays' noise models.  An event lives in
// one pulsar a.  With t = mjd * 86400 of a TOA, nu_i its radio frequency [MHz], t0 = t0_mjd * 86400, A = 10^log10_a [s at nu_ref],
// s = -1 if sign < 0 else +1, chi the chromatic index, tau = 10^log10_tau [s]:
//
//     dt_i = s A (nu_ref / nu_i)^chi shape(t_i)
//
//     kind 0  decay    t >= t0: exp(-(t - t0) / tau)          t < t0: 0
//     kind 1  cusp     t >= t0: exp(-(t - t0) / tau)          t < t0: exp(-(t0 - t) / tau_pre)
//     kind 2  bump     exp(-1/2 ((t - t0) / tau)^2)           (the envelope convention of the wavelets, pta_burst.h)
//     kind 3  annual   sin(2 pi t / YEAR_IN_SEC + phase)      (YEAR_IN_SEC = 365.25 * 86400 s; t0, tau unused)
//
// A TOA at exactly t0 takes the t >= t0 side.  For kind 1, tau_pre = 10^log10_tau_pre, or tau if that label is NaN.  Conventions:
// every time in seconds, natural-exponent envelopes (tau is the e-folding time; for the bump the Gaussian's standard deviation), the
// sign in a column of its own (a DM dip advances the TOAs: sign = -1, the default).  From enterprise_extensions: chrom_exp_decay
// (log10_Amp, log10_tau [days], t0 [MJD], sign_param, idx) is kind 0 with log10_tau + log10(86400); chrom_exp_cusp adds
// log10_tau_pre the same way; chrom_gaussian_bump's sigma [days] is tau; chrom_yearly_sinusoid (log10_Amp, phase, idx) is kind 3.
//
// The chromatic weight is folded into the exponent: with the per-TOA table lnu_i = ln(nu_ref / nu_i) (host, long double, rounded to
// fp64 once per prepare()) a term of kinds 0 - 2 is
//
//     s exp(e),   e = fma(x, y, b),   b = fma(chi, lnu_i, ln A),
//
// (x, y) = (-(t - t0), 1 / tau) after t0, (t - t0, 1 / tau_pre) before it (cusp), (-1/2 / tau^2, (t - t0)^2) for the bump: one exp per
// (event, TOA), no pow per TOA and no weight table per chi.  A lane on which the term is 0 by definition (a decay before t0) takes
// e = -infinity, exp = +0.  Kind 3 is s exp(b) sin(2 pi (t / YEAR + phase / 2 pi)) with the sine taken in turns: t / YEAR is split into its
// rounded product and the product's error by one fma (and the second word of 1 / YEAR), reduced to [0, 1) and fed to
// pta_sincos_2pi_poly.
//
// Rounding of kinds 0 - 2 against an exact evaluation from the same table row, u = 2^-53, X = |ln A| + |chi lnu| + |envelope argument|:
//     lnu rounded to fp64                         |chi lnu| u
//     b, one fma                                  (|ln A| + |chi lnu|) u
//     t - t0                                      |arg| u          (bump: 2 |arg| u, it is squared; and (t - t0)^2 adds |arg| u)
//     e, one fma                                  X u
// so |e - exact| <= 3 X u (bump: 4 X u), and the term is within (c X + d) u |term|, c = 3 (bump 4), d = 3: 2 u for an exp within one
// ulp, and 1 u for the second-order terms of exp(delta) - 1 at X <= 800.
//
// Everything is __host__ __device__: tests/chrom_event compiles this header with g++ (-ffp-contract=off) and checks it against a
// long-double evaluation of the definition.
#pragma once
#include <stdint.h>
#include <math.h>
#include "pta_rng.h"
#include "pta_burst.h"

#define PTA_STREAM_CE 15u  // field e: chromatic event slot e of the realisation, pair = label column (pta_chrom_event.h)

// label columns of a chromatic event [E, 9] (the pairs of the stream that draws them)
#define PTA_CE_COL_PSR 0
#define PTA_CE_COL_KIND 1
#define PTA_CE_COL_T0_MJD 2
#define PTA_CE_COL_LOG10_TAU 3
#define PTA_CE_COL_LOG10_TAU_PRE 4
#define PTA_CE_COL_LOG10_A 5
#define PTA_CE_COL_SIGN 6
#define PTA_CE_COL_INDEX 7
#define PTA_CE_COL_PHASE 8
#define PTA_CE_NCOL 9
// columns of the table row the add kernel reads
#define PTA_CE_TAB_PSR 0          // the pulsar, an integer held as a double
#define PTA_CE_TAB_KIND 1         // 0 decay, 1 cusp, 2 bump, 3 annual
#define PTA_CE_TAB_T0 2           // t0 [s]
#define PTA_CE_TAB_INV_TAU 3      // 1 / tau
#define PTA_CE_TAB_INV_TAU_PRE 4  // 1 / tau_pre (1 / tau where the label is NaN)
#define PTA_CE_TAB_NH 5           // -1/2 / tau^2
#define PTA_CE_TAB_SIGN 6         // -1 or +1
#define PTA_CE_TAB_LNA 7          // ln A = log10_a ln 10
#define PTA_CE_TAB_CHI 8          // the chromatic index
#define PTA_CE_TAB_TURNS 9        // phase / (2 pi)
#define PTA_CE_NTAB 10
#define PTA_CE_EMAX 128
#define PTA_CE_KIND_DECAY 0
#define PTA_CE_KIND_CUSP 1
#define PTA_CE_KIND_BUMP 2
#define PTA_CE_KIND_ANNUAL 3

// exponents below this give exp = 0 exactly in fp64 (PTA_BURST_ARG_ZERO, pta_burst.h): an event whose exponent lies below it on every
// active lane of a wave may be passed over without changing a bit
#define PTA_CE_ARG_ZERO PTA_BURST_ARG_ZERO
// 1 / YEAR_IN_SEC = 1 / 31557600 in two words (the second is the first's rounding error), and the constants of the table row
#define PTA_CE_FYR_HI 3.168808781402895e-08
#define PTA_CE_FYR_LO 2.9912186282424574e-24
#define PTA_CE_LN10 2.302585092994046
#define PTA_CE_INV_2PI 0.15915494309189535

PTA_HD double pta_ce_draw(uint64_t seed, uint64_t realisation, uint32_t e, uint32_t j, double lo, double hi) {
  return pta_box_draw(seed, realisation, pta_stream_id(PTA_STREAM_CE, e), j, lo, hi);
}

// table row of one event (src: its PTA_CE_NCOL label columns)
PTA_HD void pta_ce_row(const double *src, double *tab) {
  const double tau = pow(10.0, src[PTA_CE_COL_LOG10_TAU]);
  const double pre = src[PTA_CE_COL_LOG10_TAU_PRE];
  tab[PTA_CE_TAB_PSR] = src[PTA_CE_COL_PSR];
  tab[PTA_CE_TAB_KIND] = src[PTA_CE_COL_KIND];
  tab[PTA_CE_TAB_T0] = src[PTA_CE_COL_T0_MJD] * 86400.0;
  tab[PTA_CE_TAB_INV_TAU] = 1.0 / tau;
  tab[PTA_CE_TAB_INV_TAU_PRE] = pre != pre ? 1.0 / tau : 1.0 / pow(10.0, pre);
  tab[PTA_CE_TAB_NH] = -0.5 / (tau * tau);
  tab[PTA_CE_TAB_SIGN] = src[PTA_CE_COL_SIGN] < 0.0 ? -1.0 : 1.0;
  tab[PTA_CE_TAB_LNA] = src[PTA_CE_COL_LOG10_A] * PTA_CE_LN10;
  tab[PTA_CE_TAB_CHI] = src[PTA_CE_COL_INDEX];
  tab[PTA_CE_TAB_TURNS] = src[PTA_CE_COL_PHASE] * PTA_CE_INV_2PI;
}

// the exponent e of an event of kind 0 - 2 at t with lnu = ln(nu_ref / nu): -infinity where the term is 0 by definition
PTA_HD double pta_ce_exponent(int kind, const double *row, double t, double lnu) {
  const double b = fma(row[PTA_CE_TAB_CHI], lnu, row[PTA_CE_TAB_LNA]);
  const double dt = t - row[PTA_CE_TAB_T0];
  if (kind == PTA_CE_KIND_BUMP) return fma(row[PTA_CE_TAB_NH], dt * dt, b);
  const double after = fma(-dt, row[PTA_CE_TAB_INV_TAU], b);
  const double before = kind == PTA_CE_KIND_CUSP ? fma(dt, row[PTA_CE_TAB_INV_TAU_PRE], b) : -INFINITY;
  return dt >= 0.0 ? after : before;
}

// s exp(e) for the exponent of pta_ce_exponent
PTA_HD double pta_ce_exp_value(const double *row, double e) { return row[PTA_CE_TAB_SIGN] * exp(e); }

// the annual term at t: s exp(ln A + chi lnu) sin(2 pi (t / YEAR + turns))
PTA_HD double pta_ce_annual_value(const double *row, double t, double lnu) {
  const double b = fma(row[PTA_CE_TAB_CHI], lnu, row[PTA_CE_TAB_LNA]);
  const double u = t * PTA_CE_FYR_HI, ul = fma(t, PTA_CE_FYR_HI, -u) + t * PTA_CE_FYR_LO;  // t / YEAR = u + ul
  double fr = ((u - floor(u)) + ul) + row[PTA_CE_TAB_TURNS];
  fr -= floor(fr);  // turns in [0, 1) up to a rounding at the ends, which the reduction below takes
  double sn, cs;
  pta_sincos_2pi_poly(fr, sn, cs);
  return (row[PTA_CE_TAB_SIGN] * exp(b)) * sn;
}

// one event at one TOA, as the add kernel evaluates it without its wave-uniform skip (the host twin's per-TOA term)
PTA_HD double pta_ce_value(const double *row, double t, double lnu) {
  const int kind = (int)row[PTA_CE_TAB_KIND];
  if (kind == PTA_CE_KIND_ANNUAL) return pta_ce_annual_value(row, t, lnu);
  return pta_ce_exp_value(row, pta_ce_exponent(kind, row, t, lnu));
}
