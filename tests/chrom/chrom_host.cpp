// Host twin of the chromatic-process device formulas (csrc/pta_chrom.h compiled as plain C++): the coefficient of one (realisation,
// pulsar, column) as k_engine_chrom_coef forms it, and the prior draw of its two fields.  Test infrastructure, not product code.
#include <stdint.h>
#include "../../pta_replicator_amd/csrc/pta_chrom.h"

extern "C" {

int ch_stream_kind(void) { return (int)PTA_STREAM_CHROM; }
int ch_rg(void) { return PTA_CHROM_RG; }

// coef [K] of pulsar a in one realisation: amp(c) z_c, z_c = branch c & 1 of pair c >> 1 of stream (CHROM, a); theta = 0: configured
void ch_coef(uint64_t seed, uint64_t realisation, int a, int K, const double *amp_conf, const double *f, const double *tspan, int theta,
             double log10_A, double gamma, double *coef, double *z) {
  for (int p = 0; p < K / 2; ++p) {
    double z0, z1;
    pta_normal_pair(seed, realisation, pta_stream_id(PTA_STREAM_CHROM, (uint32_t)a), (uint32_t)p, z0, z1, 0);
    z[2 * p] = z0;
    z[2 * p + 1] = z1;
    coef[2 * p] = pta_chrom_amp(amp_conf, f, tspan, a, K, 2 * p, theta != 0, log10_A, gamma) * z0;
    coef[2 * p + 1] = pta_chrom_amp(amp_conf, f, tspan, a, K, 2 * p + 1, theta != 0, log10_A, gamma) * z1;
  }
}

void ch_draw_field(uint64_t seed, uint64_t r0, int R, int n, int field, const double *lo, const double *hi, double *out) {
  for (int r = 0; r < R; ++r)
    for (int j = 0; j < n; ++j) out[(int64_t)r * n + j] = pta_hyper_draw_field(seed, r0 + (uint64_t)r, (uint32_t)field, (uint32_t)j, lo[j], hi[j]);
}
}
