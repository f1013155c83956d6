// TEST HARNESS (not product code): compiles pta_replicator_amd/csrc/pta_chrom_event.h with g++ so that the per-realisation chromatic-event
// formulas of the device can be checked against a long-double evaluation of their definition on a machine without a GPU.  Loaded by
// tests/chrom_event_reference.py via ctypes.
#include <stdint.h>
#include "../../pta_replicator_amd/csrc/pta_chrom_event.h"

extern "C" {

// out[(r * E + e) * 9 + j] for realisations r0 .. r0+R-1, as pta_chrom_event_uniform writes it (lo / hi [E x 9])
void ce_uniform(uint64_t seed, uint64_t r0, int R, int E, int P, const double *lo, const double *hi, double *out) {
  for (int r = 0; r < R; ++r)
    for (int e = 0; e < E; ++e) {
      double *row = out + ((int64_t)r * E + e) * PTA_CE_NCOL;
      for (int j = 0; j < PTA_CE_NCOL; ++j)
        row[j] = pta_ce_draw(seed, r0 + (uint64_t)r, (uint32_t)e, (uint32_t)j, lo[e * PTA_CE_NCOL + j], hi[e * PTA_CE_NCOL + j]);
      row[PTA_CE_COL_PSR] = pta_nt_psr(row[PTA_CE_COL_PSR], P);
    }
}

// tab[E x 10] of one realisation, as pta_engine_chrom_event_params writes it
void ce_tables(const double *src, int E, double *tab) {
  for (int e = 0; e < E; ++e) pta_ce_row(src + e * PTA_CE_NCOL, tab + e * PTA_CE_NTAB);
}

// out[i] = the sum over the events of pulsar a at (toa_s[i], lnu[i]), as pta_engine_chrom_event_add accumulates it
void ce_term(const double *tab, int E, int a, const double *toa_s, const double *lnu, int n, double *out) {
  for (int i = 0; i < n; ++i) {
    double acc = 0.0;
    for (int e = 0; e < E; ++e) {
      const double *row = tab + e * PTA_CE_NTAB;
      if ((int)row[PTA_CE_TAB_PSR] != a) continue;
      acc += pta_ce_value(row, toa_s[i], lnu[i]);
    }
    out[i] = acc;
  }
}

int ce_stream(void) { return (int)PTA_STREAM_CE; }
double ce_arg_zero(void) { return PTA_CE_ARG_ZERO; }
}
