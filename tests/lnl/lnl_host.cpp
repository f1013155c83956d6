// TEST HARNESS (not product code): compiles pta_replicator_amd/csrc/pta_lnl.h with g++ so that the per-thread sums, the reduction
// tree and the epilogue of the likelihood kernels can be checked against NumPy on a machine without a GPU.  Loaded by
// tests/test_lnl_host.py via ctypes.  lh_quad walks k_lnl_quad: PTA_LNL_QT threads per (realisation, pulsar), each wave joined by
// the xor butterfly of pta_lnl_wave_sum, the four waves as (w0 + w1) + (w2 + w3).
#include <stdint.h>
#include "../../pta_replicator_amd/csrc/pta_lnl.h"

extern "C" void lh_quad(const double *rows, int64_t ld_rows, int R, const int32_t *psr_off, int P, const double *dinv, const int32_t *psr_ep,
                        const int32_t *ep_ptr, const int32_t *ep_idx, const double *ep_g, const double *q, int64_t ld_q, int q_block, int K,
                        int m, const double *Ht, int64_t ldh, double *r0) {
  for (int64_t r = 0; r < R; ++r)
    for (int a = 0; a < P; ++a) {
      const int i0 = psr_off[a], n = psr_off[a + 1] - i0;
      const int e0 = psr_ep ? psr_ep[a] : 0, E = psr_ep ? psr_ep[a + 1] - e0 : 0;
      double v[PTA_LNL_QT], ys[PTA_LNL_MMAX];
      for (int k = 0; k < m; ++k) ys[k] = q[pta_lnl_q_index(r, a, K + k, P, K + m, ld_q, q_block)];
      for (int t = 0; t < PTA_LNL_QT; ++t)
        v[t] = pta_lnl_quad_partial(rows + r * ld_rows + i0, m ? Ht + i0 : nullptr, ldh, ys, m, dinv + i0, n, ep_ptr + e0, ep_idx, ep_g + e0, E, t, PTA_LNL_QT);
      double part[PTA_LNL_QT / 64];
      for (int w = 0; w < PTA_LNL_QT / 64; ++w) {
        double *x = v + 64 * w;
        for (int o = 32; o > 0; o >>= 1) {
          double y[64];
          for (int l = 0; l < 64; ++l) y[l] = x[l] + x[l ^ o];
          for (int l = 0; l < 64; ++l) x[l] = y[l];
        }
        part[w] = x[0];
      }
      r0[r * P + a] = (part[0] + part[1]) + (part[2] + part[3]);
    }
}

extern "C" int64_t lh_q_index(int64_t r, int a, int k, int P, int Kt, int64_t ld_q, int q_block) {
  return pta_lnl_q_index(r, a, k, P, Kt, ld_q, q_block);
}

extern "C" double lh_value(double r0, double quad, double s, double logdet, double c) { return pta_lnl_value(r0, quad, s, logdet, c); }
