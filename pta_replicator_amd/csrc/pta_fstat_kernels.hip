// Continuous-wave F-statistics of whole ensembles (pta_replicator_amd/f_statistic.py holds the definitions and the
// realisation-independent preparation).  Three launches per batch (four with sky_max):
//
//   pta_fstat_project   Q[r, a, c] = sum_i W[c, off_a + i] rows[r, off_a + i], c < 2 J       ragged grouped GEMM, fp64 MFMA
//   pta_fstat_fp        Fp[r, j] = 1/2 sum_a q_raj^T G_aj^-1 q_raj                            one thread per (r, j), pulsars ascending
//   pta_fstat_fe        N_rjs = sum_a phi_as (x) q_raj on the matrix cores, Fe = 1/2 N^T M_js^-1 N in registers; the full map or
//                       the per-tile maxima, which k_fstat_fe_reduce folds over the sky tiles in ascending order
//
// pta_fstat_project: one workgroup = one pulsar x 32 TM realisations x 32 TN columns (128 x 128 when the launch is large, down to
// 64 x 64 when it has few workgroups), four waves as 2 x 2, each TM x TN MFMA tiles.  K runs over the pulsar's own TOAs in slabs of 16, double-buffered in LDS ([row][k], row stride
// 17 doubles), the next slab fetched into registers under the current slab's MFMAs: one barrier per slab.  Both operands are
// fetched with 16 lanes on 16 consecutive TOAs of one row (128 contiguous bytes; the pulsars' offsets are arbitrary, so no wider
// vector load is aligned).  TOAs past the pulsar's end enter as zeros in both operands, realisations past R are clamped reads that
// are never stored.  Every output is one MFMA chain over the TOAs in ascending slabs: no split-K, no atomics, so a realisation's Q
// is bit-identical whatever R, the chunk or its row slot (MFMA output rows are independent).
//
// pta_fstat_fe: k_sky_stat (pta_sky_stat.h, shared with pta_bwm_stat) under the policy fe_stat below - 8 frequencies x (sin, cos) as
// the 16 rows of a wave's A tile, the 10 unique entries of the 4 x 4 M_js^-1 per cell, pta_fstat_quad as the form - and the fold of the
// per-tile maxima, k_fstat_fe_reduce, which both statistics use.
#include "pta_sky_stat.h"

#define FS_BK 16   // TOAs per K slab
#define FS_LD 17   // LDS row stride in doubles (odd: the 16 rows of a fragment read fall into 16 different bank pairs)
#define FS_FILL 2048  // workgroups of pta_fstat_project below which it takes a smaller tile (eight per compute unit of 256)

template <int TM, int TN>
__global__ __launch_bounds__(256) void k_fstat_project(const double *__restrict__ Wt, int64_t ldw, int C, const int32_t *__restrict__ psr_off,
                                                       const double *__restrict__ rows, int64_t ld_rows, int R, double *__restrict__ Q,
                                                       int64_t ld_q) {
  constexpr int BM = 32 * TM, BN = 32 * TN;  // realisations and columns per workgroup
  __shared__ double As[2][BM * FS_LD];
  __shared__ double Bs[2][BN * FS_LD];
  const int a = blockIdx.z;
  const int i0 = psr_off[a], n = psr_off[a + 1] - i0;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const int t = threadIdx.x, l = t & 63, w = t >> 6, wm = w >> 1, wn = w & 1;
  const int kx = t & 15, rr = t >> 4;  // staging: TOA kx of the slab, rows / columns rr + 16 u
  const double *ap[2 * TM], *bp[2 * TN];
  bool bok[2 * TN];
#pragma unroll
  for (int u = 0; u < 2 * TM; ++u) ap[u] = rows + (int64_t)min(m0 + rr + 16 * u, R - 1) * ld_rows + i0;
#pragma unroll
  for (int u = 0; u < 2 * TN; ++u) {
    const int c = n0 + rr + 16 * u;
    bok[u] = c < C;
    bp[u] = Wt + (int64_t)min(c, C - 1) * ldw + i0;
  }
  pta_f64x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = pta_f64x4{0.0, 0.0, 0.0, 0.0};
  double ra[2 * TM], rb[2 * TN];
  auto fetch = [&](int k0) {
    const int k = k0 + kx;
    const bool in = k < n;
#pragma unroll
    for (int u = 0; u < 2 * TM; ++u) ra[u] = in ? ap[u][k] : 0.0;
#pragma unroll
    for (int u = 0; u < 2 * TN; ++u) rb[u] = (in && bok[u]) ? bp[u][k] : 0.0;
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int u = 0; u < 2 * TM; ++u) As[buf][(rr + 16 * u) * FS_LD + kx] = ra[u];
#pragma unroll
    for (int u = 0; u < 2 * TN; ++u) Bs[buf][(rr + 16 * u) * FS_LD + kx] = rb[u];
  };
  const int nslab = (n + FS_BK - 1) / FS_BK;
  if (nslab > 0) {
    fetch(0);
    stash(0);
  }
  __syncthreads();
  const int fr = (l & 15) * FS_LD + (l >> 4);  // fragment element of lane l: row l & 15, k = l >> 4 of an MFMA step
  for (int s = 0; s < nslab; ++s) {
    const int cur = s & 1;
    const bool more = s + 1 < nslab;
    if (more) fetch((s + 1) * FS_BK);
    const double *Ab = As[cur] + wm * 16 * TM * FS_LD + fr, *Bb = Bs[cur] + wn * 16 * TN * FS_LD + fr;
#pragma unroll
    for (int kk = 0; kk < FS_BK; kk += 4) {
      double fa[TM], fb[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) fa[i] = Ab[i * 16 * FS_LD + kk];
#pragma unroll
      for (int j = 0; j < TN; ++j) fb[j] = Bb[j * 16 * FS_LD + kk];
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = pta_mfma_f64(fa[i], fb[j], acc[i][j]);
    }
    if (more) stash(cur ^ 1);
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = m0 + wm * 16 * TM + i * 16 + pta_mfma_row(l, e), c = n0 + wn * 16 * TN + j * 16 + pta_mfma_col(l);
        if (r < R && c < C) Q[(int64_t)r * ld_q + (int64_t)a * C + c] = acc[i][j][e];
      }
}

__global__ __launch_bounds__(256) void k_fstat_fp(const double *__restrict__ Q, int64_t ld_q, int P, int J, int R, const double *__restrict__ Ginv,
                                                  double *__restrict__ fp, int64_t ld_fp) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)R * J) return;
  const int64_t r = idx / J;
  const int j = (int)(idx - r * J);
  const double *q = Q + r * ld_q + 2 * j;
  double s = 0.0;
  for (int a = 0; a < P; ++a) {  // ascending pulsars, one fma chain: the same sum for a realisation whatever the launch
    const double2 v = *reinterpret_cast<const double2 *>(q + (int64_t)a * 2 * J);
    const double *g = Ginv + ((int64_t)a * J + j) * 3;
    const double u = fma(g[2], v.y * v.y, fma(2.0 * g[1], v.x * v.y, g[0] * (v.x * v.x)));
    s += u;
  }
  fp[r * ld_fp + j] = 0.5 * s;
}

// 1/2 n^T M^-1 n, m = the packed upper triangle of M^-1; one fixed fma chain
__device__ __forceinline__ double pta_fstat_quad(const double (&m)[10], double n0, double n1, double n2, double n3) {
  double d = m[0] * (n0 * n0);
  d = fma(m[4], n1 * n1, d);
  d = fma(m[7], n2 * n2, d);
  d = fma(m[9], n3 * n3, d);
  double o = m[1] * (n0 * n1);
  o = fma(m[2], n0 * n2, o);
  o = fma(m[3], n0 * n3, o);
  o = fma(m[5], n1 * n2, o);
  o = fma(m[6], n1 * n3, o);
  o = fma(m[8], n2 * n3, o);
  return fma(0.5, d, o);
}

// pta_fstat_fe's policy of k_sky_stat (pta_sky_stat.h): 8 frequencies x (sin, cos) per workgroup.  Row rho of the A tile is frequency
// (rho & 3) + 4 (rho >> 3), sin / cos (rho >> 2) & 1, so that accumulator registers (2 e, 2 e + 1) of a lane are the sin / cos sums of its
// cell e (frequency j0 + g + 4 e): both chains together hold the whole 4-vector N_rjs of the lane's two cells.
struct fe_stat {
  static constexpr int JB = 8, NC = 2, NM = 10, QPJ = 2;
  static constexpr bool AMP = false;
  static __device__ __forceinline__ int64_t qoff(int a, int, int J) { return (int64_t)a * 2 * J; }
  static __device__ __forceinline__ int acol(int m) { return 2 * ((m & 3) + 4 * (m >> 3)) + ((m >> 2) & 1); }
  static __device__ __forceinline__ double value(const double (&mi)[10], const pta_f64x4 &np_, const pta_f64x4 &nc_, int cell, double &, double &) {
    return pta_fstat_quad(mi, np_[2 * cell], np_[2 * cell + 1], nc_[2 * cell], nc_[2 * cell + 1]);
  }
};

// fold the sub-tile maxima in ascending sky order: strictly greater wins, so the lowest index is kept on ties
__global__ __launch_bounds__(256) void k_fstat_fe_reduce(const double *__restrict__ pval, const int32_t *__restrict__ parg, int64_t n, int ntile,
                                                         int J, double *__restrict__ fe_max, int64_t ld_max, int32_t *__restrict__ fe_arg,
                                                         int64_t ld_arg) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  const int64_t r = idx / J;
  const int j = (int)(idx - r * J);
  const double *v = pval + r * ntile * J + j;
  const int32_t *ix = parg + r * ntile * J + j;
  double best = v[0];
  int32_t bi = ix[0];
  for (int k = 1; k < ntile; ++k)
    if (v[(int64_t)k * J] > best) best = v[(int64_t)k * J], bi = ix[(int64_t)k * J];
  fe_max[r * ld_max + j] = best;
  fe_arg[r * ld_arg + j] = bi;
}

// internal launcher of the fold over the sub-tile maxima (declared in pta_common.h): pta_sky_stat_launch calls it for both statistics
int pta_fstat_reduce_launch(const double *part_val, const int32_t *part_arg, int64_t n, int ntile, int J, double *vmax, int64_t ld_max,
                            int32_t *varg, int64_t ld_arg, hipStream_t stream) {
  hipLaunchKernelGGL(k_fstat_fe_reduce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, part_val, part_arg, n, ntile, J, vmax, ld_max, varg,
                     ld_arg);
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}

// The launch plan of pta_fstat_project, the one place it is decided: the bm x bn (realisations x columns) tile of a workgroup.  `who`
// names the entry in the refusals.
static int pta_fstat_project_choose(const char *who, int C, int P, int R, int &bm, int &bn) {
  PTA_REQUIRE(C >= 2 && C % 2 == 0 && C <= PTA_FSTAT_CMAX && P > 0 && P <= 65535 && R > 0, PTA_E_ARG,
              "%s: C=%d (even, 2..%d) P=%d (1..65535) R=%d", who, C, PTA_FSTAT_CMAX, P, R);
  PTA_REQUIRE(pta_cdiv(R, 64) <= 65535u, PTA_E_ARG, "%s: R=%d exceeds one launch (64 * 65535 realisations)", who, R);
  // The tile follows the launch's size alone - a realisation's Q does not depend on it (every output is its own MFMA chain over
  // ascending slabs).  128 x 128 while that leaves FS_FILL workgroups; else 64 rows, then 64 columns: a workgroup walks its whole
  // pulsar, so with few workgroups the longest pulsar of a ragged array sets the launch's time, and a smaller tile shortens that walk.
  bm = 128, bn = C > 64 ? 128 : (C > 32 ? 64 : 32);
  auto wgs = [&]() { return (long long)P * pta_cdiv(R, bm) * pta_cdiv(C, bn); };
  if (wgs() < FS_FILL) bm = 64;
  if (wgs() < FS_FILL && bn == 128) bn = 64;
  return PTA_OK;
}

extern "C" int pta_fstat_project_plan(int C, int P, int R, int32_t *plan) {
  PTA_REQUIRE(plan, PTA_E_ARG, "pta_fstat_project_plan: NULL argument");
  int bm, bn;
  const int rc = pta_fstat_project_choose("pta_fstat_project_plan", C, P, R, bm, bn);
  if (rc != PTA_OK) return rc;
  plan[0] = bm, plan[1] = bn;
  return PTA_OK;
}

extern "C" int pta_fstat_project(const double *Wt, int64_t ldw, int C, const int32_t *psr_off, int P, const double *rows, int64_t ld_rows, int R,
                                 double *Q, int64_t ld_q, void *stream) {
  PTA_REQUIRE(Wt && psr_off && rows && Q, PTA_E_ARG, "pta_fstat_project: NULL argument");
  int bm, bn;
  const int rc = pta_fstat_project_choose("pta_fstat_project", C, P, R, bm, bn);
  if (rc != PTA_OK) return rc;
  PTA_REQUIRE(ld_q >= (int64_t)P * C && ldw >= 1 && ld_rows >= 1, PTA_E_ARG, "pta_fstat_project: ld_q=%lld < P*C=%lld or ldw / ld_rows < 1",
              (long long)ld_q, (long long)P * C);
  hipStream_t s = pta_stream(stream);
  dim3 block(256);
  const dim3 grid(pta_cdiv(C, bn), pta_cdiv(R, bm), P);
#define PTA_FS_PROJ(TM_, TN_) \
  hipLaunchKernelGGL((k_fstat_project<TM_, TN_>), grid, block, 0, s, Wt, ldw, C, psr_off, rows, ld_rows, R, Q, ld_q)
  if (bm == 128) {
    if (bn == 128) PTA_FS_PROJ(4, 4);
    else if (bn == 64) PTA_FS_PROJ(4, 2);
    else PTA_FS_PROJ(4, 1);
  } else {
    if (bn == 128) PTA_FS_PROJ(2, 4);
    else if (bn == 64) PTA_FS_PROJ(2, 2);
    else PTA_FS_PROJ(2, 1);
  }
#undef PTA_FS_PROJ
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}

extern "C" int pta_fstat_fp(const double *Q, int64_t ld_q, int P, int J, int R, const double *Ginv, double *fp, int64_t ld_fp, void *stream) {
  PTA_REQUIRE(Q && Ginv && fp, PTA_E_ARG, "pta_fstat_fp: NULL argument");
  PTA_REQUIRE(P > 0 && J >= 1 && 2 * J <= PTA_FSTAT_CMAX && R > 0, PTA_E_ARG, "pta_fstat_fp: P=%d J=%d (1..%d) R=%d", P, J, PTA_FSTAT_CMAX / 2, R);
  PTA_REQUIRE(ld_q >= (int64_t)P * 2 * J && ld_q % 2 == 0 && ld_fp >= J, PTA_E_ARG, "pta_fstat_fp: ld_q=%lld (even, >= 2*P*J=%lld) ld_fp=%lld (>= J)",
              (long long)ld_q, (long long)P * 2 * J, (long long)ld_fp);
  PTA_REQUIRE(((uintptr_t)Q & 15) == 0, PTA_E_ARG, "pta_fstat_fp: Q must be 16-byte aligned");
  const long long nb = ((long long)R * J + 255) / 256;
  PTA_REQUIRE(nb <= 0x7fffffffLL, PTA_E_ARG, "pta_fstat_fp: R*J=%lld exceeds one launch", (long long)R * J);
  hipLaunchKernelGGL(k_fstat_fp, dim3((unsigned)nb), dim3(256), 0, pta_stream(stream), Q, ld_q, P, J, R, Ginv, fp, ld_fp);
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}

extern "C" int64_t pta_fstat_fe_tiles(int S) { return S < 1 ? 0 : (int64_t)((S + SKY_ST - 1) / SKY_ST) * (SKY_ST / 16); }

extern "C" int pta_fstat_fe_plan(int P, int J, int R, int S, int32_t *plan) { return pta_sky_stat_plan<fe_stat>("pta_fstat_fe_plan", P, J, R, S, plan); }

extern "C" int pta_fstat_fe(const double *Q, int64_t ld_q, int P, int J, int R, const double *phi, int S, const double *Minv, double *fe,
                            int64_t ld_fe, double *fe_max, int64_t ld_max, int32_t *fe_arg, int64_t ld_arg, double *part_val, int32_t *part_arg,
                            void *stream) {
  PTA_REQUIRE(Q && phi && Minv, PTA_E_ARG, "pta_fstat_fe: NULL argument");
  PTA_REQUIRE(P >= 2 && P <= PTA_FSTAT_PMAX && J >= 1 && 2 * J <= PTA_FSTAT_CMAX && R > 0 && S >= 1, PTA_E_ARG,
              "pta_fstat_fe: P=%d (2..%d) J=%d (1..%d) R=%d S=%d", P, PTA_FSTAT_PMAX, J, PTA_FSTAT_CMAX / 2, R, S);
  PTA_REQUIRE(ld_q >= (int64_t)P * 2 * J, PTA_E_ARG, "pta_fstat_fe: ld_q=%lld < 2*P*J=%lld", (long long)ld_q, (long long)P * 2 * J);
  return pta_sky_stat_launch<fe_stat>("pta_fstat_fe", "fe", Q, ld_q, P, 2 * J, J, R, phi, S, Minv, fe, ld_fe, nullptr, 0, fe_max, ld_max, fe_arg, ld_arg,
                                      part_val, part_arg, stream);
}
