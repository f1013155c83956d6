// Marginalised Gaussian log-likelihood on a theta grid: the pieces of pta_lnl_kernels.hip whose operation order is part of the
// contract with the NumPy oracle (optimal_statistic.py: lnl_quad, lnl_solve).  __host__ __device__: tests/lnl compiles this header
// with g++ (-ffp-contract=off) and runs the same per-thread sums and the same reduction tree on the CPU.
#pragma once
#include <math.h>
#include <stdint.h>
#include "pta_hyper.h"

#define PTA_LNL_KMAX 128  // K = K_rn + C columns per pulsar (the LDS budget of the factorisation and of the staged operator)
#define PTA_LNL_MMAX 16   // timing-model rows appended to the projection operator
#define PTA_LNL_QT 256    // threads of one (realisation, pulsar) workgroup of pta_lnl_quad

// element (r, a, k) of the projections q = [V; G] r_a as pta_os_project leaves them when it is called once per block of q_block
// operator rows with Y = q + P * k0 (Kt = K + m rows in all; q_block >= Kt: plain [R, P, Kt])
PTA_HD int64_t pta_lnl_q_index(int64_t r, int a, int k, int P, int Kt, int64_t ld_q, int q_block) {
  const int k0 = (k / q_block) * q_block;
  const int cb = (Kt - k0 < q_block) ? Kt - k0 : q_block;
  return r * ld_q + (int64_t)P * k0 + (int64_t)a * cb + (k - k0);
}

// residual i of the generalised-least-squares fit of the timing model: x_i = r_i - sum_k Ht[k * ldh + i] y_k with y = G r the m
// projections and H = M (M^T N'^-1 M)^-1/2 (so H y = M beta_hat).  r^T P0' r = x^T N'^-1 x is then a sum of squares: subtracting
// || G r ||^2 from r^T N'^-1 r instead loses (|r| / |x|)^2 eps when the rows carry a large component inside the span of M.
PTA_HD double pta_lnl_fit_residual(const double *r, const double *Ht, int64_t ldh, const double *y, int m, int i) {
  double x = r[i];
  for (int k = 0; k < m; ++k) x = fma(-Ht[(int64_t)k * ldh + i], y[k], x);
  return x;
}

// thread t of nt: its share of  sum_i x_i^2 / d_i  -  sum_e g_e (sum_{i in e} x_i / d_i)^2  of one (realisation, pulsar):
// TOAs t, t + nt, ... and epochs t, t + nt, ... in ascending order, the TOAs of an epoch in the order of the host-built list
// (ep_ptr [E + 1] offsets into ep_idx, ep_idx TOA indices within the pulsar).  dinv = 1 / d.
PTA_HD double pta_lnl_quad_partial(const double *r, const double *Ht, int64_t ldh, const double *y, int m, const double *dinv, int n,
                                   const int32_t *ep_ptr, const int32_t *ep_idx, const double *ep_g, int E, int t, int nt) {
  double acc = 0.0;
  for (int i = t; i < n; i += nt) {
    const double x = pta_lnl_fit_residual(r, Ht, ldh, y, m, i);
    acc = fma(x, x * dinv[i], acc);
  }
  double corr = 0.0;
  for (int e = t; e < E; e += nt) {
    double se = 0.0;
    for (int p = ep_ptr[e]; p < ep_ptr[e + 1]; ++p) {
      const int i = ep_idx[p];
      se = fma(pta_lnl_fit_residual(r, Ht, ldh, y, m, i), dinv[i], se);
    }
    corr = fma(ep_g[e] * se, se, corr);
  }
  return acc - corr;
}

// ln L of one (grid point, pulsar, realisation): r0 = r^T P0' r, quad = || L^-1 D q ||^2, logdet = 2 sum ln L_kk
PTA_HD double pta_lnl_value(double r0, double quad, double s, double logdet, double c) { return -0.5 * ((r0 - quad) / s + logdet + c); }
