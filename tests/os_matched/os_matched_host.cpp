// TEST HARNESS (not product code): compiles pta_replicator_amd/csrc/pta_os_matched.h with g++ so that the prior variances the
// device evaluates per (realisation, pulsar, column) can be checked against NumPy on a machine without a GPU.  Loaded by
// tests/test_os_matched_host.py via ctypes.  The loop is the indexing of k_osm_prior.
#include <stdint.h>
#include "../../pta_replicator_amd/csrc/pta_os_matched.h"

extern "C" void omh_prior(int R, int P, int K_rn, int C, const double *rn_f, const double *rn_tspan, const double *rn_phi,
                          const double *rn_log10_A, const double *rn_gamma, double T, const double *gw_log10_A, const double *gw_gamma,
                          const double *s, double *b) {
  const int K = K_rn + C;
  for (int64_t r = 0; r < R; ++r)
    for (int a = 0; a < P; ++a)
      for (int k = 0; k < K; ++k) {
        const int64_t ra = r * P + a;
        double v;
        if (k < K_rn) {
          const double lA = rn_log10_A ? rn_log10_A[ra] : NAN;
          v = pta_osm_rn_b(rn_f[(int64_t)a * (K_rn / 2) + k / 2], rn_tspan[a], lA, rn_log10_A ? rn_gamma[ra] : 0.0, rn_phi[(int64_t)a * K_rn + k], s[a]);
        } else {
          v = gw_log10_A ? pta_osm_gw_b((double)((k - K_rn) / 2 + 1) / T, T, gw_log10_A[r], gw_gamma[r], s[a]) : 0.0;
        }
        b[ra * K + k] = v;
      }
}
