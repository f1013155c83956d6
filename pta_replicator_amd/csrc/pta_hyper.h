// Per-realisation hyperparameters of throughput mode: the uniform prior map and the two theta-dependent amplitudes.
//
// theta of realisation r is drawn from stream (PTA_STREAM_HYPER, 0), pair j = parameter column, uniform u2 in [0, 1), so it is a
// pure function of (seed, r) like the residuals.  Everything here is __host__ __device__: tests/hyper compiles this header with
// g++ (-ffp-contract=off) and checks it against NumPy; the explicit fma makes the uniform map agree bit for bit on both sides.
#pragma once
#include <stdint.h>
#include <math.h>
#include "pta_rng.h"

#define PTA_YEAR_IN_SEC (365.25 * 86400.0)  // constants.py YEAR_IN_SEC
#define PTA_GWB_F1YR (1.0 / 3.16e7)         // the GWB spectrum's f1yr (red_noise.py:247), not 1 / YEAR_IN_SEC

// lo + (hi - lo) u, one rounding (the map of pta_box_draw, pta_rng.h)
PTA_HD double pta_hyper_affine(double lo, double hi, double u) { return fma(hi - lo, u, lo); }

// parameter column j of realisation `realisation` drawn uniformly from [lo, hi)
PTA_HD double pta_hyper_draw(uint64_t seed, uint64_t realisation, uint32_t j, double lo, double hi) {
  return pta_box_draw(seed, realisation, pta_stream_id(PTA_STREAM_HYPER, 0u), j, lo, hi);
}

// parameter column j of a further field of the hyperparameter stream: stream (PTA_STREAM_HYPER, field), pair j.  Field 0 is
// pta_hyper_draw bit for bit; field 1 holds the nodes of a per-realisation GWB spectrum (gwb_log10_hc)
PTA_HD double pta_hyper_draw_field(uint64_t seed, uint64_t realisation, uint32_t field, uint32_t j, double lo, double hi) {
  return pta_box_draw(seed, realisation, pta_stream_id(PTA_STREAM_HYPER, field), j, lo, hi);
}

// characteristic strain hc(f) of the power-law GWB, with the optional turnover (red_noise.py:245-251): same operations in the
// same order as red_noise.gwb_spectrum_hcf
PTA_HD double pta_gwb_hcf(double f, double log10_A, double gamma, int turnover, double f0, double beta, double power) {
  const double amp = pow(10.0, log10_A);
  const double alpha = -0.5 * (gamma - 3.0);
  double hcf = amp * pow(f / PTA_GWB_F1YR, alpha);
  if (turnover) {
    const double si = alpha - beta;
    hcf = hcf / pow(1.0 + pow(f / f0, power * si), 1.0 / power);
  }
  return hcf;
}

// characteristic strain hc(f) of a user-supplied spectrum (red_noise.py:255-263): log10 hc linear in log10 f between the M nodes
// fp (sorted by frequency), constant outside them - the userSpec branch of red_noise.gwb_spectrum_hcf, with numpy.interp's
// operations in numpy.interp's order.  What does not depend on fp is tabulated per frequency by the host (_hyper.spec_tables):
// the segment j (xp[j] <= x < xp[j + 1], x = log10 f), dx = x - xp[j] and dxp = xp[j + 1] - xp[j]; dxp = 0 marks a frequency
// that takes fp[j] itself (below the first node, at or above the last, or exactly on a node).  j is clamped to the table.
PTA_HD double pta_gwb_hcf_user(const double *fp, int M, int j, double dx, double dxp) {
  j = j < 0 ? 0 : (j > M - 1 ? M - 1 : j);
  double y = fp[j];
  if (dxp != 0.0 && j + 1 < M) {
    const double slope = (fp[j + 1] - fp[j]) / dxp;
    y = slope * dx + fp[j];
  }
  return pow(10.0, y);
}

// sqrt(prior) of one red-noise coefficient at frequency f [Hz] (red_noise.py:126):
//   prior = A^2 (f / fyr)^-gamma / (12 pi^2 Tspan) yr^3,  fyr = 1 / yr
PTA_HD double pta_rn_amp(double f, double tspan, double log10_A, double gamma) {
  const double yr = PTA_YEAR_IN_SEC;
  const double fyr = 1.0 / yr;
  const double amp = pow(10.0, log10_A);
  const double pi = 3.14159265358979323846;
  const double prior = pow(amp, 2.0) * pow(f / fyr, -gamma) / (12.0 * pow(pi, 2.0) * tspan) * pow(yr, 3.0);
  return sqrt(prior);
}
