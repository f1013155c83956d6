// TEST HARNESS (not product code): compiles pta_replicator_amd/csrc/pta_burst.h with g++ so that the per-realisation wavelet formulas of
// the device can be checked against the reference's golden output and a long-double evaluation of its expression on a machine without
// a GPU.  Loaded by tests/test_burst_host.py via ctypes.
#include <stdint.h>
#include "../../pta_replicator_amd/csrc/pta_burst.h"

extern "C" {

// sky[r * 3 + j] and wav[(r * W + w) * 7 + j] for realisations r0 .. r0+R-1, as pta_burst_uniform writes them (lo / hi [10])
void bu_uniform(uint64_t seed, uint64_t r0, int R, int W, const double *lo, const double *hi, double *sky, double *wav) {
  for (int r = 0; r < R; ++r) {
    for (int j = 0; j < PTA_BURST_NSKY; ++j) sky[(int64_t)r * PTA_BURST_NSKY + j] = pta_burst_sky_draw(seed, r0 + (uint64_t)r, (uint32_t)j, lo[j], hi[j]);
    for (int w = 0; w < W; ++w)
      for (int j = 0; j < PTA_BURST_NCOL; ++j)
        wav[((int64_t)r * W + w) * PTA_BURST_NCOL + j] =
            pta_burst_wavelet_draw(seed, r0 + (uint64_t)r, (uint32_t)w, (uint32_t)j, lo[PTA_BURST_NSKY + j], hi[PTA_BURST_NSKY + j]);
  }
}

// out[(r * V + v) * 6 + j], as pta_transient_uniform writes it (lo / hi [6], column 0 the box (0, P))
void bu_nt_uniform(uint64_t seed, uint64_t r0, int R, int V, int P, const double *lo, const double *hi, double *out) {
  for (int r = 0; r < R; ++r)
    for (int v = 0; v < V; ++v) {
      double *row = out + ((int64_t)r * V + v) * PTA_NT_NCOL;
      for (int j = 0; j < PTA_NT_NCOL; ++j) row[j] = pta_nt_draw(seed, r0 + (uint64_t)r, (uint32_t)v, (uint32_t)j, lo[j], hi[j]);
      row[PTA_NT_COL_PSR] = pta_nt_psr(row[PTA_NT_COL_PSR], P);
    }
}

// wav[W x 7] and kk[P x 2] of one realisation, as pta_engine_burst_params writes them
void bu_burst_tables(const double *sky, const double *src, int W, const double *phat, int P, double *wav, double *kk) {
  for (int w = 0; w < W; ++w) pta_burst_wavelet_row(src + w * PTA_BURST_NCOL, wav + w * PTA_BURST_NTAB);
  for (int a = 0; a < P; ++a) pta_burst_antenna(sky, phat + 3 * a, kk[2 * a], kk[2 * a + 1]);
}

// out[i] = the sum over the wavelets at t = toa_s[i] for a pulsar with (kp, kc), as pta_engine_burst_add accumulates it
void bu_burst_term(const double *wav, int W, double kp, double kc, const double *toa_s, int n, double *out) {
  for (int i = 0; i < n; ++i) {
    double acc = 0.0;
    for (int w = 0; w < W; ++w) {
      const double *row = wav + w * PTA_BURST_NTAB;
      double C, S;
      pta_burst_fold(kp, kc, row, C, S);
      acc += pta_wavelet_value(row[0], row[2], C, S, pta_wavelet_arg(row[0], row[1], toa_s[i]), toa_s[i]);
    }
    out[i] = acc;
  }
}

// tab[V x 6] of one realisation, as pta_engine_transient_params writes it
void bu_nt_tables(const double *src, int V, double *tab) {
  for (int v = 0; v < V; ++v) pta_nt_row(src + v * PTA_NT_NCOL, tab + v * PTA_NT_NTAB);
}

// out[i] = the sum over the transients of pulsar a at t = toa_s[i], as pta_engine_transient_add accumulates it
void bu_nt_term(const double *tab, int V, int a, const double *toa_s, int n, double *out) {
  for (int i = 0; i < n; ++i) {
    double acc = 0.0;
    for (int v = 0; v < V; ++v) {
      const double *row = tab + v * PTA_NT_NTAB;
      if ((int)row[0] != a) continue;
      acc += pta_wavelet_value(row[1], row[3], row[4], row[5], pta_wavelet_arg(row[1], row[2], toa_s[i]), toa_s[i]);
    }
    out[i] = acc;
  }
}

int bu_stream_burst(void) { return (int)PTA_STREAM_BURST; }
int bu_stream_nt(void) { return (int)PTA_STREAM_NT; }
double bu_arg_zero(void) { return PTA_BURST_ARG_ZERO; }
}
