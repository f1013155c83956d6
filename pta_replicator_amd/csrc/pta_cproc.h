// Common red processes with an ORF of their own (ReplicaEngine.add_common_process: clock = monopole, ephemeris = dipole, CURN, HD,
// or a [P, P] array), on the array-wide Fourier basis f_k = k / T:
//   dt_{a,i} += sum_c F_ic y_ac,   y_ac = sum_p sqrt(phi_pc) sum_j B_p[a, j] z_pcj,   B_p B_p^T = Gamma_p  [P, rho_p]
// z = deviate n = c rho_p + j of stream (CPROC, p): pair n >> 1, branch n & 1.  Everything that fixes the order of a sum lives here as
// host / device functions with explicit fma, so that tests/cproc compiles the same sums with g++ (-ffp-contract=off).
// Struct: pta_cproc_engine (include/pta_replicator_amd.h).
#pragma once
#include <stdint.h>
#include <math.h>
#include "pta_rng.h"
#include "pta_hyper.h"

#define PTA_STREAM_CPROC 12u  // + process index: deviate n = c rho + j (column c, factor column j), pair n >> 1, branch n & 1 (11: pta_pop.h)

// realisations per workgroup of pta_engine_cproc_add: two half-workgroups of PTA_CPROC_RG / 2 rows each, whose accumulators (two TOAs
// per lane) and prefetched output pairs stay in registers
#define PTA_CPROC_RG 16

// frequency [Hz] of column c (sin column 2k, cos column 2k + 1 share f_k = (k + 1) / T)
PTA_HD double pta_cproc_freq(int c, double tspan) { return (double)((c >> 1) + 1) / tspan; }

// sqrt(prior) of column c of process p in one realisation: the configured table where log10_A is NaN ("as configured") or no theta is
// given, else pta_rn_amp at the column's frequency with tspan = T
PTA_HD double pta_cproc_amp(const double *amp_conf, double tspan, int p, int K, int c, bool theta, double log10_A, double gamma) {
  if (!theta || isnan(log10_A)) return amp_conf[(int64_t)p * K + c];
  return pta_rn_amp(pta_cproc_freq(c, tspan), tspan, log10_A, gamma);
}

// deviate j of column c of process p (rank rho) of one realisation
PTA_HD double pta_cproc_deviate(uint64_t seed, uint64_t realisation, int p, int rho, int c, int j, int fast) {
  return pta_normal_single(seed, realisation, pta_stream_id(PTA_STREAM_CPROC, (uint32_t)p), (uint32_t)(c * rho + j), fast);
}

// sum_j B[a, j] z_j in ascending j, one fma per term
PTA_HD double pta_cproc_mix(const double *Brow, const double *z, int rho) {
  double acc = 0.0;
  for (int j = 0; j < rho; ++j) acc = fma(Brow[j], z[j], acc);
  return acc;
}

// one process joins the coefficient: acc + amp * mix, one fma (processes in ascending p, from acc = 0)
PTA_HD double pta_cproc_join(double acc, double amp, double mix) { return fma(amp, mix, acc); }

// harmonic k + 1 from harmonic k by the rotation through (s1, c1) = (sin, cos)(2 pi x): two products, two fma
PTA_HD void pta_cproc_rot(double &s, double &c, double s1, double c1) {
  const double sn = fma(s, c1, c * s1), cn = fma(c, c1, -(s * s1));
  s = sn;
  c = cn;
}

// one harmonic joins a TOA's sum: acc + a s + b c, the sin column first
PTA_HD double pta_cproc_term(double acc, double a, double b, double s, double c) { return fma(b, c, fma(a, s, acc)); }

// sum_k coef[2k] s_k + coef[2k + 1] c_k of one TOA as pta_engine_cproc_add forms it (the host twin's whole loop; the kernel runs the same
// calls with the rotation shared by the rows of a group)
PTA_HD double pta_cproc_synth(const double *coef, int K, double s1, double c1) {
  double s = s1, c = c1, acc = 0.0;
  for (int k = 0; k < K / 2; ++k) {
    acc = pta_cproc_term(acc, coef[2 * k], coef[2 * k + 1], s, c);
    pta_cproc_rot(s, c, s1, c1);
  }
  return acc;
}
