// Per-realisation hyperparameters in throughput mode (ReplicaEngine.generate(theta=...), generate_sampled):
//   pta_hyper_uniform          theta drawn on chip from uniform boxes, keyed by (seed, realisation) like the residuals: stream (HYPER, 0)
//                              through the shared box draw (pta_box_kernels.hip)
//   pta_gwb_spectrum_scale     hcf(f_k; A_r, gamma_r) / hcf0(f_k) per (realisation, bin): the factor the scaled GWB transforms apply
//   pta_gwb_spectrum_scale_user  the same factor for a spectrum given per realisation as M nodes of log10 hc (gwb_log10_hc)
//   pta_hyper_uniform_field    pta_hyper_uniform on stream (HYPER, field): the prior draws of those nodes (field 1), the same box draw
//   pta_engine_rn_coef_hyper   k_engine_rn_coef with sqrt(prior) evaluated per (realisation, pulsar, frequency)
// pta_engine_generate_hyper (pta_engine_kernels.hip) is pta_engine_generate with the last two stages above switched in, in the stage
// order of pta_engine_generate: pta_engine_rn_coef_hyper -> pta_gwb_spectrum_scale -> scaled GWB transform -> ORF mix -> synthesis.
// The fused synthesis kernel is unchanged: only its inputs (RN coefficients, mixed GWB grid series) depend on theta.
#include "pta_common.h"
#include "pta_rng.h"
#include "pta_hyper.h"

extern "C" int pta_hyper_uniform(uint64_t seed, uint64_t r0, int R, int n_par, const double *lo, const double *hi, double *out,
                                 void *stream) {
  PTA_REQUIRE(lo && hi && out, PTA_E_ARG, "pta_hyper_uniform: NULL argument");
  PTA_REQUIRE(R > 0 && n_par > 0, PTA_E_ARG, "pta_hyper_uniform: R=%d n_par=%d", R, n_par);
  const int64_t total = (int64_t)R * n_par;
  PTA_REQUIRE(total < (1LL << 31), PTA_E_ARG, "pta_hyper_uniform: problem too large");
  return pta_box_uniform_launch(seed, r0, R, 1, n_par, PTA_STREAM_HYPER, 0u, lo, hi, out, pta_stream(stream));
}

__global__ void k_gwb_spectrum_scale(const double *__restrict__ f, const double *__restrict__ hcf0, int Nf, int R,
                                     const double *__restrict__ log10_A, const double *__restrict__ gamma, int turnover, double f0,
                                     double beta, double power, double *__restrict__ scale, int64_t ld_scale) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)R * Nf) return;
  const int k = (int)(idx % Nf);
  const int64_t r = idx / Nf;
  scale[r * ld_scale + k] = pta_gwb_hcf(f[k], log10_A[r], gamma[r], turnover, f0, beta, power) / hcf0[k];
}

extern "C" int pta_gwb_spectrum_scale(const double *f, const double *hcf0, int Nf, int R, const double *log10_A, const double *gamma,
                                      int turnover, double f0, double beta, double power, double *scale, int64_t ld_scale,
                                      void *stream) {
  PTA_REQUIRE(f && hcf0 && log10_A && gamma && scale, PTA_E_ARG, "pta_gwb_spectrum_scale: NULL argument");
  PTA_REQUIRE(Nf >= 3 && R > 0 && ld_scale >= Nf, PTA_E_ARG, "pta_gwb_spectrum_scale: Nf=%d R=%d ld_scale=%lld", Nf, R,
              (long long)ld_scale);
  const int64_t total = (int64_t)R * Nf;
  PTA_REQUIRE(total < (1LL << 31), PTA_E_ARG, "pta_gwb_spectrum_scale: problem too large");
  hipLaunchKernelGGL(k_gwb_spectrum_scale, dim3(pta_cdiv(total, 256)), dim3(256), 0, pta_stream(stream), f, hcf0, Nf, R, log10_A, gamma,
                     turnover ? 1 : 0, f0, beta, power, scale, ld_scale);
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}

// coef[(r*P + a)*K + c] = sqrt(prior(f_a[c/2]; A_ra, gamma_ra)) * z, z = deviate c of stream (RN, a): the draws of k_engine_rn_coef;
// log10_A[r*P + a] = NaN takes amp_fixed[a*K + c] (pulsar not sampled, or without red noise: amp_fixed row zero)
__global__ void k_engine_rn_coef_hyper(uint64_t seed, uint64_t r0, int R, int P, int K, const double *__restrict__ rn_f,
                                       const double *__restrict__ rn_tspan, const double *__restrict__ log10_A,
                                       const double *__restrict__ gamma, const double *__restrict__ amp_fixed,
                                       double *__restrict__ coef, int fast) {
  pta_rng_stage_tables();  // Box-Muller tables -> LDS (pta_rng.h)
  __syncthreads();
  int idx = blockIdx.x * blockDim.x + threadIdx.x;  // (r, a, pair)
  int hp = K / 2;
  int total = R * P * hp;
  if (idx >= total) return;
  int p = idx % hp, ra = idx / hp;
  int a = ra % P, r = ra / P;
  double z0, z1;
  pta_normal_pair(seed, r0 + (uint64_t)r, pta_stream_id(PTA_STREAM_RN, (uint32_t)a), (uint32_t)p, z0, z1, fast);
  const double lA = log10_A[ra];
  double a0, a1;
  if (isnan(lA)) {
    a0 = amp_fixed[(int64_t)a * K + 2 * p];
    a1 = amp_fixed[(int64_t)a * K + 2 * p + 1];
  } else {
    a0 = a1 = pta_rn_amp(rn_f[(int64_t)a * hp + p], rn_tspan[a], lA, gamma[ra]);  // sin and cos column share f (np.repeat(f, 2))
  }
  int64_t o = (int64_t)ra * K + 2 * p;
  coef[o] = a0 * z0;
  coef[o + 1] = a1 * z1;
}

extern "C" int pta_engine_rn_coef_hyper(uint64_t seed, uint64_t r0, int R, int P, int K, const double *rn_f, const double *rn_tspan,
                                        const double *log10_A, const double *gamma, const double *amp_fixed, double *coef, int rng_fast,
                                        void *stream) {
  PTA_REQUIRE(rn_f && rn_tspan && log10_A && gamma && amp_fixed && coef, PTA_E_ARG, "pta_engine_rn_coef_hyper: NULL argument");
  PTA_REQUIRE(R > 0 && P > 0 && K > 0 && (K % 2) == 0, PTA_E_ARG, "pta_engine_rn_coef_hyper: R=%d P=%d K=%d (K must be even)", R, P,
              K);
  int64_t total = (int64_t)R * P * (K / 2);
  PTA_REQUIRE(total < (1LL << 31), PTA_E_ARG, "pta_engine_rn_coef_hyper: problem too large");
  hipLaunchKernelGGL(k_engine_rn_coef_hyper, dim3(pta_cdiv(total, 256)), dim3(256), 0, pta_stream(stream), seed, r0, R, P, K, rn_f,
                     rn_tspan, log10_A, gamma, amp_fixed, coef, rng_fast ? 1 : 0);
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}

extern "C" int pta_hyper_uniform_field(uint64_t seed, uint64_t r0, int R, int n_par, int field, const double *lo, const double *hi,
                                       double *out, void *stream) {
  PTA_REQUIRE(lo && hi && out, PTA_E_ARG, "pta_hyper_uniform_field: NULL argument");
  PTA_REQUIRE(R > 0 && n_par > 0, PTA_E_ARG, "pta_hyper_uniform_field: R=%d n_par=%d", R, n_par);
  PTA_REQUIRE(field >= 0 && field <= 0xFFFFFF, PTA_E_ARG, "pta_hyper_uniform_field: field=%d does not fit the 24-bit stream field", field);
  const int64_t total = (int64_t)R * n_par;
  PTA_REQUIRE(total < (1LL << 31), PTA_E_ARG, "pta_hyper_uniform_field: problem too large");
  return pta_box_uniform_launch(seed, r0, R, 1, n_par, PTA_STREAM_HYPER, (uint32_t)field, lo, hi, out, pta_stream(stream));
}

#define PTA_GWB_SPEC_MMAX 4096  // nodes of one spectrum: 32 KiB of LDS
#define PTA_GWB_SPEC_BINS 1024  // bins per workgroup: 4 per thread, so the M nodes are staged once per 1024 bins

// One workgroup = PTA_GWB_SPEC_BINS consecutive bins of ONE realisation: its M node values go to LDS once, every thread then
// evaluates its bins from the per-bin tables (no bracket search).  Lanes read and write consecutive doubles.
__global__ __launch_bounds__(256) void k_gwb_spectrum_scale_user(const int32_t *__restrict__ seg, const double *__restrict__ dx,
                                                                 const double *__restrict__ dxp, const double *__restrict__ hcf0, int Nf,
                                                                 int M, int nb, const double *__restrict__ log10_hc, int64_t ld_hc,
                                                                 double *__restrict__ scale, int64_t ld_scale) {
  extern __shared__ __attribute__((aligned(16))) double fp[];
  const int64_t r = blockIdx.x / nb;
  const int k0 = (int)(blockIdx.x % nb) * PTA_GWB_SPEC_BINS;
  const double *row = log10_hc + r * ld_hc;
  for (int j = threadIdx.x; j < M; j += 256) fp[j] = row[j];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < PTA_GWB_SPEC_BINS / 256; ++i) {
    const int k = k0 + i * 256 + (int)threadIdx.x;
    if (k < Nf) scale[r * ld_scale + k] = pta_gwb_hcf_user(fp, M, seg[k], dx[k], dxp[k]) / hcf0[k];
  }
}

extern "C" int pta_gwb_spectrum_scale_user(const int32_t *seg, const double *dx, const double *dxp, const double *hcf0, int Nf, int M, int R,
                                           const double *log10_hc, int64_t ld_hc, double *scale, int64_t ld_scale, void *stream) {
  PTA_REQUIRE(seg && dx && dxp && hcf0 && log10_hc && scale, PTA_E_ARG, "pta_gwb_spectrum_scale_user: NULL argument");
  PTA_REQUIRE(M >= 2 && M <= PTA_GWB_SPEC_MMAX, PTA_E_ARG, "pta_gwb_spectrum_scale_user: M=%d (2..%d nodes)", M, PTA_GWB_SPEC_MMAX);
  PTA_REQUIRE(Nf >= 3 && R > 0 && ld_scale >= Nf && ld_hc >= M, PTA_E_ARG, "pta_gwb_spectrum_scale_user: Nf=%d R=%d ld_scale=%lld ld_hc=%lld", Nf,
              R, (long long)ld_scale, (long long)ld_hc);
  const int nb = (int)pta_cdiv(Nf, PTA_GWB_SPEC_BINS);
  PTA_REQUIRE((int64_t)R * ld_scale < (1LL << 31) && (int64_t)R * ld_hc < (1LL << 31) && (int64_t)R * nb < (1LL << 31), PTA_E_ARG,
              "pta_gwb_spectrum_scale_user: problem too large");
  hipLaunchKernelGGL(k_gwb_spectrum_scale_user, dim3((unsigned)((int64_t)R * nb)), dim3(256), (size_t)M * sizeof(double), pta_stream(stream), seg,
                     dx, dxp, hcf0, Nf, M, nb, log10_hc, ld_hc, scale, ld_scale);
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}
