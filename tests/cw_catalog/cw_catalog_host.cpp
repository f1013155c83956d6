// TEST HARNESS (not product code): compiles pta_replicator_amd/csrc/pta_cw_catalog.h with g++ so that the catalogue's label draw, its
// table rows (the folded non-evolving modes included) and its sum over the sources can be checked against a long-double evaluation of
// the reference on a machine without a GPU.  Loaded by tests/test_cw_catalog_host.py via ctypes.
#include <stdint.h>
#include "../../pta_replicator_amd/csrc/pta_cw_catalog.h"

extern "C" {

int cc_npar(int mode) { return pta_cw_catalog_npar(mode); }

// out[(r * S + s) * 8 + j] for realisations r0 .. r0+R-1, as pta_cw_catalog_uniform writes it
void cc_uniform(uint64_t seed, uint64_t r0, int R, int S, const double *lo, const double *hi, double *out) {
  for (int r = 0; r < R; ++r)
    for (int s = 0; s < S; ++s)
      for (int j = 0; j < PTA_CW_NSRC; ++j)
        out[((int64_t)r * S + s) * PTA_CW_NSRC + j] = pta_cw_catalog_draw(seed, r0 + (uint64_t)r, (uint32_t)s, (uint32_t)j, lo[j], hi[j]);
}

// the table rows par[s * NPAR ..] of S sources src[s * 8 ..] seen from one pulsar, as pta_engine_cw_catalog_params writes them
void cc_params(const double *src, int S, int amp_is_h, const double *phat, double pdist, int mode, int psr_term, double *par) {
  for (int s = 0; s < S; ++s)
    pta_cw_catalog_params(src + s * PTA_CW_NSRC, amp_is_h, phat, pdist, mode, psr_term, par + (int64_t)s * pta_cw_catalog_npar(mode));
}

// out[i] = the sum over the first n sources at t = toa_s[i] - tref, as pta_engine_cw_catalog_add forms it
void cc_sum(const double *par, int n, const double *toa_s, int n_toa, double tref, int mode, int psr_term, double *out) {
  for (int i = 0; i < n_toa; ++i) out[i] = pta_cw_catalog_sum_rt(par, n, toa_s[i] - tref, mode, psr_term);
}
}
