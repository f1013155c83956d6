// TEST HARNESS (not product code): compiles pta_replicator_amd/csrc/pta_pop.h with g++ so that the Poisson sampler of the population path
// can be checked against its NumPy twin (tests/pop_reference.py) on a machine without a GPU, and so that the GPU tests have the host
// build of the very same code to compare the device's counts with.  Loaded by tests/test_pop_host.py and tests/test_gpu_pop.py via ctypes.
#include <stdint.h>
#include "../../pta_replicator_amd/csrc/pta_pop.h"

extern "C" {

// out[i] = N of (realisation rho[i], cell cell[i]) at rate lam[i]; attempts[i] (optional) = Philox blocks consumed
void ph_poisson(uint64_t seed, const uint64_t *rho, const uint32_t *cell, const double *lam, int64_t n, double *out, int32_t *attempts) {
  for (int64_t i = 0; i < n; ++i) {
    int a = 0;
    out[i] = pta_pop_poisson(seed, rho[i], cell[i], lam[i], &a);
    if (attempts) attempts[i] = a;
  }
}

// z[i] = z0 of the Box-Muller pair of stream (POP, 0), pair = cell[i]: the deviate of the normal regime
void ph_normal_z0(uint64_t seed, const uint64_t *rho, const uint32_t *cell, int64_t n, double *z) {
  for (int64_t i = 0; i < n; ++i) {
    double z0, z1;
    pta_normal_pair(seed, rho[i], pta_stream_id(PTA_STREAM_POP, 0u), cell[i], z0, z1, 0);
    z[i] = z0;
  }
}

int ph_regime(double lam) { return pta_pop_regime(lam); }

double ph_weight(double n, double hs2, double fo, double t_obs) { return pta_pop_weight(n, hs2, fo, t_obs); }
}
