// Prior variances of the optimal statistic under per-realisation noise parameters: b of one (realisation, pulsar, column), the
// diagonal of the low-rank covariance over the pulsar's mean white-noise variance s.  __host__ __device__: tests/os_matched
// compiles this header with g++ (-ffp-contract=off) against optimal_statistic.matched_prior, which evaluates the same operations
// in the same order.
#pragma once
#include <math.h>
#include "pta_hyper.h"

// red-noise column at frequency f: pta_rn_amp^2 / s, or the configured variance phi_fixed / s when log10_A is NaN ("as configured")
PTA_HD double pta_osm_rn_b(double f, double tspan, double log10_A, double gamma, double phi_fixed, double s) {
  double phi = phi_fixed;
  if (!isnan(log10_A)) {
    const double amp = pta_rn_amp(f, tspan, log10_A, gamma);
    phi = amp * amp;
  }
  return phi / s;
}

// GW auto-term column at frequency f = k / T: A^2 S(gamma) / s with the unit spectrum of optimal_statistic.unit_spectrum
PTA_HD double pta_osm_gw_b(double f, double T, double log10_A, double gamma, double s) {
  const double fyr = 1.0 / PTA_YEAR_IN_SEC;
  const double pi = 3.14159265358979323846;
  const double S = pow(fyr, gamma - 3.0) * pow(f, -gamma) / (12.0 * pow(pi, 2.0) * T);
  return pow(10.0, 2.0 * log10_A) * S / s;
}

// GW auto-term column at frequency f = k / T for a characteristic strain hc given directly (a per-realisation spectrum):
// hc^2 / (12 pi^2 f^3 T) / s - pta_osm_gw_b with hc^2 = A^2 (f yr)^(3 - gamma)
PTA_HD double pta_osm_gw_b_hc(double f, double T, double hc, double s) {
  const double pi = 3.14159265358979323846;
  return pow(hc, 2.0) / (12.0 * pow(pi, 2.0) * pow(f, 3.0) * T) / s;
}
