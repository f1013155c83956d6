// TEST HARNESS (not product code): compiles pta_replicator_amd/csrc/pta_hyper.h with g++ so that the per-realisation
// hyperparameter formulas of the device can be checked against NumPy on a machine without a GPU.  Loaded by
// tests/test_hyper_host.py via ctypes.
#include <stdint.h>
#include "../../pta_replicator_amd/csrc/pta_hyper.h"

extern "C" {

// out[r * n_par + j] for realisations r0 .. r0+R-1, as pta_hyper_uniform writes it
void hh_hyper_uniform(uint64_t seed, uint64_t r0, int R, int n_par, const double *lo, const double *hi, double *out) {
  for (int r = 0; r < R; ++r)
    for (int j = 0; j < n_par; ++j) out[(int64_t)r * n_par + j] = pta_hyper_draw(seed, r0 + (uint64_t)r, (uint32_t)j, lo[j], hi[j]);
}

void hh_gwb_hcf(const double *f, int n, double log10_A, double gamma, int turnover, double f0, double beta, double power, double *out) {
  for (int i = 0; i < n; ++i) out[i] = pta_gwb_hcf(f[i], log10_A, gamma, turnover, f0, beta, power);
}

void hh_rn_amp(const double *f, int n, double tspan, double log10_A, double gamma, double *out) {
  for (int i = 0; i < n; ++i) out[i] = pta_rn_amp(f[i], tspan, log10_A, gamma);
}

}
