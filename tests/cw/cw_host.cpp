// TEST HARNESS (not product code): compiles pta_replicator_amd/csrc/pta_cw_hyper.h with g++ so that the per-realisation CW formulas of
// the device can be checked against a long-double evaluation of the reference on a machine without a GPU.  Loaded by
// tests/test_cw_host.py via ctypes.
#include <stdint.h>
#include "../../pta_replicator_amd/csrc/pta_cw_hyper.h"

extern "C" {

// out[r * n_par + j] for realisations r0 .. r0+R-1, as pta_cw_uniform writes it
void ch_uniform(uint64_t seed, uint64_t r0, int R, int n_par, const double *lo, const double *hi, double *out) {
  for (int r = 0; r < R; ++r)
    for (int j = 0; j < n_par; ++j) out[(int64_t)r * n_par + j] = pta_cw_draw(seed, r0 + (uint64_t)r, (uint32_t)j, lo[j], hi[j]);
}

// the 16 scalars of one (source, pulsar), as pta_engine_cw_params writes them
void ch_params(const double *src, int amp_is_h, const double *phat, double pdist, int mode, double *par) {
  pta_cw_params(src, amp_is_h, phat, pdist, mode, par);
}

// out[i] = waveform at t = toa_s[i] - tref, as pta_engine_cw_add evaluates it
void ch_wave(const double *par, const double *toa_s, int n, double tref, int mode, int psr_term, double *out) {
  for (int i = 0; i < n; ++i) out[i] = pta_cw_wave_rt(par, toa_s[i] - tref, mode, psr_term);
}

void ch_constants(double *out) {
  out[0] = PTA_SOLAR2S;
  out[1] = PTA_KPC2S;
  out[2] = PTA_MPC2S;
}
}
