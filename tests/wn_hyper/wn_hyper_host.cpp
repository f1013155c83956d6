// TEST HARNESS (not product code): compiles pta_replicator_amd/csrc/pta_wn_hyper.h (and the prior map of pta_hyper.h) with g++ so that
// the per-realisation white-noise formulas of the device can be checked against NumPy and a long-double evaluation on a machine
// without a GPU.  Loaded by tests/test_wn_hyper_host.py via ctypes.
#include <stdint.h>
#include "../../pta_replicator_amd/csrc/pta_wn_hyper.h"
#include "../../pta_replicator_amd/csrc/pta_hyper.h"

extern "C" {

// ea, eb [n] as pta_engine_wn_params writes them for n (label, configured) pairs
void wh_amplitudes(int n, const double *efac_label, const double *log10_equad_label, const double *efac_conf, const double *equad_conf, int tnequad,
                   double *ea, double *eb) {
  for (int i = 0; i < n; ++i) pta_wn_amplitudes(efac_label[i], log10_equad_label[i], efac_conf[i], equad_conf[i], tnequad, ea[i], eb[i]);
}

// ec [n] as pta_engine_wn_params writes it
void wh_ecorr(int n, const double *log10_ecorr_label, const double *ecorr_conf, double *ec) {
  for (int i = 0; i < n; ++i) ec[i] = pta_wn_pow10(log10_ecorr_label[i], ecorr_conf[i]);
}

// out[i] = the element of pta_engine_wn_add
void wh_element(int n, const double *o, int has_wn, const double *ea, const double *sigma, const double *z1, const double *eb, const double *z2,
                int has_ec, const double *ec, const double *ze, double *out) {
  for (int i = 0; i < n; ++i) out[i] = pta_wn_element(o[i], has_wn != 0, ea[i], sigma[i], z1[i], eb[i], z2[i], has_ec != 0, ec[i], ze[i]);
}

// out[r * n + j] for realisations r0 .. r0+R-1, as pta_hyper_uniform_field writes it
void wh_draw_field(uint64_t seed, uint64_t r0, int R, int n, int field, const double *lo, const double *hi, double *out) {
  for (int r = 0; r < R; ++r)
    for (int j = 0; j < n; ++j) out[(int64_t)r * n + j] = pta_hyper_draw_field(seed, r0 + (uint64_t)r, (uint32_t)field, (uint32_t)j, lo[j], hi[j]);
}

int wh_gmax(void) { return PTA_WN_HYPER_GMAX; }
}
