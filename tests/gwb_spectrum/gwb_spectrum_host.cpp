// TEST HARNESS (not product code): compiles the per-realisation GWB spectrum formulas of pta_replicator_amd/csrc/pta_hyper.h and
// pta_os_matched.h with g++ so that they can be checked against NumPy on a machine without a GPU.  Loaded by
// tests/test_gwb_spectrum_host.py via ctypes.
#include <stdint.h>
#include "../../pta_replicator_amd/csrc/pta_os_matched.h"

extern "C" {

// out[r * n + k] = hc of realisation r's M sorted nodes at the n tabulated frequencies, as pta_gwb_spectrum_scale_user evaluates it
void gs_hcf_user(const int32_t *seg, const double *dx, const double *dxp, int n, int M, int R, const double *log10_hc, double *out) {
  for (int r = 0; r < R; ++r)
    for (int k = 0; k < n; ++k) out[(int64_t)r * n + k] = pta_gwb_hcf_user(log10_hc + (int64_t)r * M, M, seg[k], dx[k], dxp[k]);
}

void gs_gwb_hcf(const double *f, int n, double log10_A, double gamma, double *out) {
  for (int i = 0; i < n; ++i) out[i] = pta_gwb_hcf(f[i], log10_A, gamma, 0, 1e-9, 1.0, 1.0);
}

// out[r * n_par + j], as pta_hyper_uniform_field writes it; field < 0: pta_hyper_draw (what pta_hyper_uniform writes)
void gs_draw_field(uint64_t seed, uint64_t r0, int R, int n_par, int field, const double *lo, const double *hi, double *out) {
  for (int r = 0; r < R; ++r)
    for (int j = 0; j < n_par; ++j)
      out[(int64_t)r * n_par + j] = field < 0 ? pta_hyper_draw(seed, r0 + (uint64_t)r, (uint32_t)j, lo[j], hi[j])
                                              : pta_hyper_draw_field(seed, r0 + (uint64_t)r, (uint32_t)field, (uint32_t)j, lo[j], hi[j]);
}

// the GW columns of pta_os_matched_prior_spec: b[(r * P + a) * C + c], c < C = 2 nf
void gs_osm_gw_b_hc(int R, int P, int nf, double T, const int32_t *seg, const double *dx, const double *dxp, int M, const double *log10_hc,
                    const double *s, double *b) {
  const int C = 2 * nf;
  for (int r = 0; r < R; ++r)
    for (int a = 0; a < P; ++a)
      for (int c = 0; c < C; ++c)
        b[((int64_t)r * P + a) * C + c] =
            pta_osm_gw_b_hc((double)(c / 2 + 1) / T, T, pta_gwb_hcf_user(log10_hc + (int64_t)r * M, M, seg[c / 2], dx[c / 2], dxp[c / 2]), s[a]);
}

// the power-law form of the same columns (pta_os_matched_prior)
void gs_osm_gw_b(int R, int P, int nf, double T, const double *log10_A, const double *gamma, const double *s, double *b) {
  const int C = 2 * nf;
  for (int r = 0; r < R; ++r)
    for (int a = 0; a < P; ++a)
      for (int c = 0; c < C; ++c) b[((int64_t)r * P + a) * C + c] = pta_osm_gw_b((double)(c / 2 + 1) / T, T, log10_A[r], gamma[r], s[a]);
}

}
