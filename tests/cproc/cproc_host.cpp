// Host twin of the common-process device formulas (csrc/pta_cproc.h compiled as plain C++): the coefficients of one realisation as
// k_engine_cproc_coef forms them, the synthesis of one TOA as k_engine_cproc_add forms it, and the prior draw of its two fields.  Test
// infrastructure, not product code.
#include <stdint.h>
#include "../../pta_replicator_amd/csrc/pta_cproc.h"

extern "C" {

int cp_stream_kind(void) { return (int)PTA_STREAM_CPROC; }
int cp_rg(void) { return PTA_CPROC_RG; }

// z [kp * rho] of process p in one realisation, column c major, factor column j minor
void cp_draws(uint64_t seed, uint64_t realisation, int p, int rho, int kp, double *z) {
  for (int c = 0; c < kp; ++c)
    for (int j = 0; j < rho; ++j) z[c * rho + j] = pta_cproc_deviate(seed, realisation, p, rho, c, j, 0);
}

// coef [P * K] of one realisation: the kernel's loop over the processes for every (pulsar, column).  B = the factors concatenated
// (process p at B + boff[p], [P x rho[p]] row-major); theta = 0: configured amplitudes; log10_A / gamma [n_proc] otherwise
void cp_coef(uint64_t seed, uint64_t realisation, int P, int n_proc, int K, const int *kp, const int *rho, const double *B, const int64_t *boff,
             const double *amp_conf, double tspan, int theta, const double *log10_A, const double *gamma, double *coef) {
  double z[4096];
  for (int c = 0; c < K; ++c)
    for (int a = 0; a < P; ++a) {
      double acc = 0.0;
      for (int p = 0; p < n_proc; ++p) {
        if (c >= kp[p]) continue;
        for (int j = 0; j < rho[p]; ++j) z[j] = pta_cproc_deviate(seed, realisation, p, rho[p], c, j, 0);
        const double amp = pta_cproc_amp(amp_conf, tspan, p, K, c, theta != 0, theta ? log10_A[p] : 0.0, theta ? gamma[p] : 0.0);
        acc = pta_cproc_join(acc, amp, pta_cproc_mix(B + boff[p] + (int64_t)a * rho[p], z, rho[p]));
      }
      coef[(int64_t)a * K + c] = acc;
    }
}

// sum_j Brow[j] z[j] as the kernel's threads form it
double cp_mix(const double *Brow, const double *z, int rho) { return pta_cproc_mix(Brow, z, rho); }

// out[i] = sum_k coef[2k] s_k(i) + coef[2k + 1] c_k(i) of n TOAs with (sin, cos)(2 pi x) in sc1 [n x 2]
void cp_synth(const double *coef, int K, const double *sc1, int n, double *out) {
  for (int i = 0; i < n; ++i) out[i] = pta_cproc_synth(coef, K, sc1[2 * i], sc1[2 * i + 1]);
}

void cp_draw_field(uint64_t seed, uint64_t r0, int R, int n, int field, const double *lo, const double *hi, double *out) {
  for (int r = 0; r < R; ++r)
    for (int j = 0; j < n; ++j) out[(int64_t)r * n + j] = pta_hyper_draw_field(seed, r0 + (uint64_t)r, (uint32_t)field, (uint32_t)j, lo[j], hi[j]);
}
}
