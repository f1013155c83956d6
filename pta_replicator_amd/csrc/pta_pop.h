// Poisson counts of a binned binary population, per (realisation, cell) (ReplicaEngine.set_population, pta_pop_kernels.hip).
//
// N ~ Poisson(lambda) is a pure function of (seed, realisation, ORIGINAL cell index, lambda): stream kind PTA_STREAM_POP, the stream's
// 24-bit field = the attempt number j, pair = the cell, one Philox block per attempt through pta_uniform_pair -> u1 in (0, 1],
// u2 in [0, 1).  How the host orders or bins the cells moves no draw.
//   lambda == 0             0, no draw
//   0 < lambda < 10         inversion by sequential search on u2 of attempt 0 (at most 255 steps)
//   10 <= lambda < 2^20     Hoermann's PTRS (Insur. Math. Econ. 12, 39 (1993)) with the constants of NumPy's legacy poisson; attempt j
//                           uses U = u2 - 0.5, V = u1; at most 64 attempts, then floor(lambda + 0.5) - a bound no input reaches in
//                           practice (P(reject)^64 < 1e-30), there so that nothing can spin a wave
//   lambda >= 2^20          max(0, floor(lambda + sqrt(lambda) z + 0.5)), z = z0 of pta_normal_pair(stream (POP, 0), pair = cell), fp64 form.
//                           The fp64 log test of PTRS compares k log(lambda) with lgamma(k + 1): at 2^20 an ulp of it is 2e-9 and the
//                           test still resolves its margin, at 1e12 it is 4e-3 and rounding would decide.
// Every product and sum is written so that g++ -ffp-contract=off and the device agree (IEEE / and sqrt, no contraction): only exp, log
// and lgamma can differ between the two, which decides a draw only where a comparison is within rounding of equality.
#pragma once
#include "pta_rng.h"

#define PTA_STREAM_POP 11u  // field j: attempt j of the Poisson draw of a population cell, pair p = original cell index (pta_pop.h)

#define PTA_POP_INVERSION_BELOW 10.0
#define PTA_POP_NORMAL_FROM 1048576.0  // 2^20
#define PTA_POP_INVERSION_STEPS 255
#define PTA_POP_PTRS_ATTEMPTS 64

// regime of a rate: 0 none (lambda == 0), 1 inversion, 2 PTRS, 3 normal.  The host sorts a bin's cells by it.
PTA_HD int pta_pop_regime(double lam) {
  return lam >= PTA_POP_NORMAL_FROM ? 3 : (lam >= PTA_POP_INVERSION_BELOW ? 2 : (lam > 0.0 ? 1 : 0));
}

PTA_HD double pta_pop_inversion(double lam, double u2) {
  double p = exp(-lam), cdf = p;
  int n = 0;
  while (u2 > cdf && n < PTA_POP_INVERSION_STEPS) {
    n += 1;
    p *= lam / (double)n;
    cdf += p;
  }
  return (double)n;
}

// attempts (optional): the number of Philox blocks the draw consumed
PTA_HD double pta_pop_ptrs(uint64_t seed, uint64_t realisation, uint32_t cell, double lam, int *attempts) {
  const double slam = sqrt(lam), loglam = log(lam);
  const double b = 0.931 + 2.53 * slam;
  const double a = -0.059 + 0.02483 * b;
  const double invalpha = 1.1239 + 1.1328 / (b - 3.4);
  const double vr = 0.9277 - 3.6224 / (b - 2.0);
  const double log_invalpha = log(invalpha);
  for (int j = 0; j < PTA_POP_PTRS_ATTEMPTS; ++j) {
    double u1, u2;
    pta_uniform_pair(pta_philox_draw(seed, realisation, pta_stream_id(PTA_STREAM_POP, (uint32_t)j), cell), u1, u2);
    const double U = u2 - 0.5, V = u1;
    const double us = 0.5 - fabs(U);
    const double k = floor((2.0 * a / us + b) * U + lam + 0.43);
    if (attempts) *attempts = j + 1;
    if (us >= 0.07 && V <= vr) return k;
    if (k < 0.0 || (us < 0.013 && V > us)) continue;
    const double lhs = log(V) + log_invalpha - log(a / (us * us) + b);
    const double rhs = -lam + k * loglam - lgamma(k + 1.0);
    if (lhs <= rhs) return k;
  }
  return floor(lam + 0.5);
}

PTA_HD double pta_pop_normal(uint64_t seed, uint64_t realisation, uint32_t cell, double lam) {
  double z0, z1;
  pta_normal_pair(seed, realisation, pta_stream_id(PTA_STREAM_POP, 0u), cell, z0, z1, 0);
  return fmax(0.0, floor(lam + sqrt(lam) * z0 + 0.5));
}

// N of (realisation, cell) for the rate lam (finite, >= 0).  On the device the caller has staged the Box-Muller tables
// (pta_rng_stage_tables) when a rate can reach the normal regime.
PTA_HD double pta_pop_poisson(uint64_t seed, uint64_t realisation, uint32_t cell, double lam, int *attempts = nullptr) {
  if (attempts) *attempts = 0;
  if (!(lam > 0.0)) return 0.0;
  if (lam < PTA_POP_INVERSION_BELOW) {
    double u1, u2;
    pta_uniform_pair(pta_philox_draw(seed, realisation, pta_stream_id(PTA_STREAM_POP, 0u), cell), u1, u2);
    if (attempts) *attempts = 1;
    return pta_pop_inversion(lam, u2);
  }
  if (lam < PTA_POP_NORMAL_FROM) return pta_pop_ptrs(seed, realisation, cell, lam, attempts);
  if (attempts) *attempts = 1;
  return pta_pop_normal(seed, realisation, cell, lam);
}

// the reference's weighted h^2 of a cell (deterministic.py:651), in its operation order
PTA_HD double pta_pop_weight(double n, double hs2, double fo, double t_obs) { return ((n * hs2) * fo) * t_obs; }
