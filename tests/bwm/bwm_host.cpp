// TEST HARNESS (not product code): compiles pta_replicator_amd/csrc/pta_bwm.h with g++ so that the per-realisation burst-with-memory
// formulas of the device can be checked against the reference's golden output and a long-double evaluation of its expression on a
// machine without a GPU.  Loaded by tests/test_bwm_host.py via ctypes.
#include <stdint.h>
#include "../../pta_replicator_amd/csrc/pta_bwm.h"

extern "C" {

// out[r * 5 + j] for realisations r0 .. r0+R-1, as pta_bwm_uniform writes it
void bh_uniform(uint64_t seed, uint64_t r0, int R, const double *lo, const double *hi, double *out) {
  for (int r = 0; r < R; ++r)
    for (int j = 0; j < PTA_BWM_NSRC; ++j) out[(int64_t)r * PTA_BWM_NSRC + j] = pta_bwm_draw(seed, r0 + (uint64_t)r, (uint32_t)j, lo[j], hi[j]);
}

// coef and t0 [s] of one (burst, pulsar), as pta_engine_bwm_params writes them
void bh_params(const double *src, const double *phat, double *coef, double *t0_s) {
  *coef = pta_bwm_coef(src, phat);
  *t0_s = pta_bwm_t0(src);
}

// out[i] = the ramp at t = toa_s[i], as pta_engine_bwm_add evaluates it
void bh_ramp(double coef, double t0_s, const double *toa_s, int n, double *out) {
  for (int i = 0; i < n; ++i) out[i] = pta_bwm_ramp(coef, t0_s, toa_s[i]);
}

int bh_stream_kind(void) { return (int)PTA_STREAM_BWM; }
}
