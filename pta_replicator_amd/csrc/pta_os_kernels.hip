// Cross-correlation optimal statistic of whole ensembles (pta_replicator_amd/optimal_statistic.py holds the definitions and the
// realisation-independent preparation).  Two launches per batch:
//
//   pta_os_project   Y[r, a, c] = sum_i W[c, off_a + i] rows[r, off_a + i]     ragged skinny projection, fp64 MFMA
//   pta_os_pairs     num[r, p] = Y[r, a_p, :] . Y[r, b_p, :],  A2[r, o] = sum_p wt[o, p] num[r, p]     one workgroup per realisation
//
// pta_os_project reads every residual once: at 68 x 5000 TOAs it is 2.79 GB per 1024 realisations against 76 MB of W.  One
// workgroup = one pulsar x (64 RW) realisations: each of its four waves owns RW tiles of 16 realisations and accumulates a 16 x C
// block with v_mfma_f64_16x16x4_f64 (A = 16 realisations x 4 TOAs straight from global memory, B = 4 TOAs x 16 columns of W from
// LDS), K running over the pulsar's TOAs in chunks of 64.  The W chunk is staged once in LDS for the four waves, and the next
// chunk's residuals and W values are loaded into registers while the current chunk's MFMAs run.
//
// Bit-identity: a realisation's Y is the same MFMA chain over the same TOA order whatever R, the launch geometry or the row slot
// of its tile (MFMA output rows are independent; rows past R are clamped reads that are never stored; TOAs past the pulsar's end
// enter as exact zeros in both operands).  No cross-realisation split, no atomics.
#include "pta_common.h"
#include "pta_mfma.h"

#define PTA_OS_KC 64     // TOAs per K chunk
#define PTA_OS_CMAX 64   // columns of W (2 n_f)
#define PTA_OS_NORF 8    // ORFs of one pta_os_pairs call

template <int CT, int RW>
__global__ __launch_bounds__(256) void k_os_project(const double *__restrict__ Wt, int64_t ldw, int C, const int32_t *__restrict__ psr_off,
                                                    const double *__restrict__ rows, int64_t ld_rows, int R, double *__restrict__ Y,
                                                    int64_t ld_y) {
  constexpr int S = (16 * CT) | 16;  // LDS row stride in doubles: rows 4j + g and 4j + g + 1 of a half-wave read land 32 banks apart
  constexpr int NW = CT * 4;         // W values staged per thread and chunk (64 TOAs x 16 CT columns / 256 threads)
  __shared__ double wl[PTA_OS_KC * S];
  const int a = blockIdx.y;
  const int i0 = psr_off[a], n = psr_off[a + 1] - i0;
  const int t = threadIdx.x, l = t & 63, w = t >> 6, g = l >> 4, m = l & 15;
  const int rbase = (blockIdx.x * 4 + w) * 16 * RW;
  const double *rp[RW];
#pragma unroll
  for (int q = 0; q < RW; ++q) rp[q] = rows + (int64_t)min(rbase + 16 * q + m, R - 1) * ld_rows + i0;
  const int wk = t & 63, wc = t >> 6;  // staging: TOA wk of the chunk, columns wc + 4 u
  pta_f64x4 acc[RW][CT];
#pragma unroll
  for (int q = 0; q < RW; ++q)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[q][ct] = pta_f64x4{0.0, 0.0, 0.0, 0.0};
  double av[RW][16], wv[NW];
  auto load = [&](int k0, double (&A)[RW][16], double (&V)[NW]) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int k = k0 + 4 * j + g;  // lane l of MFMA step j holds TOA 4 j + (l >> 4) of realisation l & 15
#pragma unroll
      for (int q = 0; q < RW; ++q) A[q][j] = k < n ? rp[q][k] : 0.0;
    }
    const int k = k0 + wk;
#pragma unroll
    for (int u = 0; u < NW; ++u) {
      const int c = wc + 4 * u;
      V[u] = (k < n && c < C) ? Wt[(int64_t)c * ldw + i0 + k] : 0.0;
    }
  };
  load(0, av, wv);
  for (int k0 = 0; k0 < n; k0 += PTA_OS_KC) {
    __syncthreads();  // the previous chunk's B reads are done
#pragma unroll
    for (int u = 0; u < NW; ++u) wl[wk * S + wc + 4 * u] = wv[u];
    __syncthreads();
    double an[RW][16], wn[NW];
    const bool more = k0 + PTA_OS_KC < n;
    if (more) load(k0 + PTA_OS_KC, an, wn);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        const double b = wl[(4 * j + g) * S + 16 * ct + m];
#pragma unroll
        for (int q = 0; q < RW; ++q) acc[q][ct] = pta_mfma_f64(av[q][j], b, acc[q][ct]);
      }
    }
    if (more) {
#pragma unroll
      for (int q = 0; q < RW; ++q)
#pragma unroll
        for (int j = 0; j < 16; ++j) av[q][j] = an[q][j];
#pragma unroll
      for (int u = 0; u < NW; ++u) wv[u] = wn[u];
    }
  }
#pragma unroll
  for (int q = 0; q < RW; ++q)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = rbase + 16 * q + pta_mfma_row(l, e), c = 16 * ct + pta_mfma_col(l);
        if (r < R && c < C) Y[(int64_t)r * ld_y + (int64_t)a * C + c] = acc[q][ct][e];
      }
}

__device__ __forceinline__ double pta_os_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void k_os_pairs(const double *__restrict__ Y, int64_t ld_y, int PC, int C, const int32_t *__restrict__ pa,
                                                  const int32_t *__restrict__ pb, int np, const double *__restrict__ wt, int n_orf,
                                                  double *__restrict__ A2, int64_t ld_a2, const double *__restrict__ den,
                                                  double *__restrict__ pout, int64_t ld_p) {
  extern __shared__ double ys[];  // Y of this realisation, [P * C]
  __shared__ double part[4][PTA_OS_NORF];
  const int64_t r = blockIdx.x;
  const int t = threadIdx.x, l = t & 63, w = t >> 6;
  for (int i = t; i < PC; i += 256) ys[i] = Y[r * ld_y + i];
  __syncthreads();
  double s[PTA_OS_NORF];
#pragma unroll
  for (int o = 0; o < PTA_OS_NORF; ++o) s[o] = 0.0;
  for (int p = t; p < np; p += 256) {  // fixed pair -> thread assignment: the same sums in the same order for every realisation
    const double *ya = ys + pa[p] * C, *yb = ys + pb[p] * C;
    double num = 0.0;
    for (int c = 0; c < C; ++c) num = fma(ya[c], yb[c], num);
    if (pout) pout[r * ld_p + p] = den ? num / den[p] : num;
#pragma unroll
    for (int o = 0; o < PTA_OS_NORF; ++o)
      if (o < n_orf) s[o] = fma(wt[(int64_t)o * np + p], num, s[o]);
  }
#pragma unroll
  for (int o = 0; o < PTA_OS_NORF; ++o) {
    if (o < n_orf) {
      const double v = pta_os_wave_sum(s[o]);
      if (l == 0) part[w][o] = v;
    }
  }
  __syncthreads();
  if (t < n_orf) A2[r * ld_a2 + t] = (part[0][t] + part[1][t]) + (part[2][t] + part[3][t]);
}

// The launch plan of pta_os_project, the one place it is decided: rw 16-realisation tiles per wave, ct 16-column tiles of W, ng
// workgroups along the realisations.  `who` names the entry in the refusals.
static int pta_os_project_choose(const char *who, int C, int P, int R, int &rw, int &ct, unsigned &ng) {
  PTA_REQUIRE(C >= 1 && C <= PTA_OS_CMAX && P > 0 && P <= 65535 && R > 0, PTA_E_ARG, "%s: C=%d (1..%d) P=%d R=%d", who, C, PTA_OS_CMAX, P, R);
  // two 16-realisation tiles per wave when that still leaves every CU a few workgroups (halves the W re-reads); the choice only
  // regroups realisations, the per-realisation sums are the same
  rw = ((long long)pta_cdiv(R, 128) * P >= 1024) ? 2 : 1;
  ng = pta_cdiv(R, 64 * rw);
  PTA_REQUIRE(ng <= 0x7fffffffu, PTA_E_ARG, "%s: R=%d exceeds one launch", who, R);
  ct = (C + 15) / 16;
  return PTA_OK;
}

extern "C" int pta_os_project_plan(int C, int P, int R, int32_t *plan) {
  PTA_REQUIRE(plan, PTA_E_ARG, "pta_os_project_plan: NULL argument");
  int rw, ct;
  unsigned ng;
  const int rc = pta_os_project_choose("pta_os_project_plan", C, P, R, rw, ct, ng);
  if (rc != PTA_OK) return rc;
  plan[0] = rw, plan[1] = ct, plan[2] = (int32_t)ng;
  return PTA_OK;
}

extern "C" int pta_os_project(const double *Wt, int64_t ldw, int C, const int32_t *psr_off, int P, const double *rows, int64_t ld_rows, int R,
                              double *Y, int64_t ld_y, void *stream) {
  PTA_REQUIRE(Wt && psr_off && rows && Y, PTA_E_ARG, "pta_os_project: NULL argument");
  int rw, ct;
  unsigned ng;
  const int rc = pta_os_project_choose("pta_os_project", C, P, R, rw, ct, ng);
  if (rc != PTA_OK) return rc;
  PTA_REQUIRE(ld_y >= (int64_t)P * C && ldw >= 1 && ld_rows >= 1, PTA_E_ARG, "pta_os_project: ld_y=%lld < P*C=%d or ldw / ld_rows < 1",
              (long long)ld_y, P * C);
  dim3 grid(ng, P), block(256);
  hipStream_t s = pta_stream(stream);
#define PTA_OS_CASE(CT_)                                                                                                  \
  case CT_:                                                                                                               \
    if (rw == 2)                                                                                                          \
      hipLaunchKernelGGL((k_os_project<CT_, 2>), grid, block, 0, s, Wt, ldw, C, psr_off, rows, ld_rows, R, Y, ld_y);     \
    else                                                                                                                  \
      hipLaunchKernelGGL((k_os_project<CT_, 1>), grid, block, 0, s, Wt, ldw, C, psr_off, rows, ld_rows, R, Y, ld_y);     \
    break;
  switch (ct) {
    PTA_OS_CASE(1) PTA_OS_CASE(2) PTA_OS_CASE(3) PTA_OS_CASE(4)
  }
#undef PTA_OS_CASE
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}

extern "C" int pta_os_pairs(const double *Y, int64_t ld_y, int P, int C, int R, const int32_t *pair_a, const int32_t *pair_b, int n_pairs,
                            const double *wt, int n_orf, double *A2, int64_t ld_a2, const double *den, double *pair_out, int64_t ld_pair,
                            void *stream) {
  PTA_REQUIRE(Y && pair_a && pair_b && wt && A2, PTA_E_ARG, "pta_os_pairs: NULL argument");
  PTA_REQUIRE(P >= 2 && C >= 1 && C <= PTA_OS_CMAX && R > 0 && n_pairs >= 1 && n_orf >= 1 && n_orf <= PTA_OS_NORF, PTA_E_ARG,
              "pta_os_pairs: P=%d C=%d R=%d n_pairs=%d n_orf=%d (1..%d)", P, C, R, n_pairs, n_orf, PTA_OS_NORF);
  PTA_REQUIRE((int64_t)P * C * 8 <= 65536, PTA_E_ARG, "pta_os_pairs: P*C=%d doubles exceed the 64 KiB of one workgroup's LDS", P * C);
  PTA_REQUIRE(ld_y >= (int64_t)P * C && ld_a2 >= n_orf && (!pair_out || ld_pair >= n_pairs), PTA_E_ARG, "pta_os_pairs: leading dimension too small");
  hipLaunchKernelGGL(k_os_pairs, dim3(R), dim3(256), (size_t)P * C * 8, pta_stream(stream), Y, ld_y, P * C, C, pair_a, pair_b, n_pairs, wt, n_orf,
                     A2, ld_a2, den, pair_out, ld_pair);
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}
