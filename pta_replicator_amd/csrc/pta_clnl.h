// Likelihood ratio of a common process with inter-pulsar correlations on a (log10_A, gamma) grid: the pieces of pta_clnl_kernels.hip whose
// operation order is part of the contract with the NumPy twin (optimal_statistic.py: clnl_scale, clnl_from_rows).  __host__ __device__:
// tests/clnl compiles this header with g++ (-ffp-contract=off) and checks it against NumPy on the CPU.
#pragma once
#include <math.h>
#include <stdint.h>
#include "pta_hyper.h"

#define PTA_CLNL_CMAX 64   // C = 2 n_f columns of the array-wide Fourier basis (pta_os_project's PTA_OS_CMAX)
#define PTA_CLNL_BLK 64    // rows of one block of the blocked forward substitution (pta_clnl_solve)
#define PTA_CLNL_RT 64     // realisations of one workgroup of pta_clnl_solve's diagonal-block kernel: one column per thread

// d_g,k = 10^log10_A (f_k yr)^((gamma_ref - gamma) / 2), f_k = (k / 2 + 1) / T: the square root of the grid point's spectrum over the
// unit spectrum at gamma_ref, column k of the sin / cos basis - optimal_statistic.clnl_scale, same operations in the same order
PTA_HD double pta_clnl_scale(int k, double T, double gamma_ref, double log10_A, double gamma) {
  const double f = (double)(k / 2 + 1) / T;
  return pow(10.0, log10_A) * pow(f * PTA_YEAR_IN_SEC, (gamma_ref - gamma) / 2.0);
}

// element (i, j <= i) of M_g = I + D T D, D = I_rho (x) diag(d): (d_i T_ij) d_j, the order of NumPy's D[:, None] * T * D[None, :]
PTA_HD double pta_clnl_m_entry(double di, double tij, double dj, int diag) {
  const double v = (di * tij) * dj;
  return diag ? 1.0 + v : v;
}

// ln L(r | common process) - ln L(r | noise only) = quad / 2 - sum_i ln L_ii
PTA_HD double pta_clnl_value(double quad, double half_logdet) { return 0.5 * quad - half_logdet; }
