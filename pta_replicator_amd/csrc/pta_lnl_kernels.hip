// Timing-model-marginalised Gaussian log-likelihood of every realisation on a grid of noise parameters
// (pta_replicator_amd/optimal_statistic.py holds the algebra, the theta-independent preparation and the NumPy oracle).  Per pulsar a,
// with q = V r_a (pta_os_project over the rows of [V; G]), b(theta_g) the prior variances (pta_os_matched_prior with the grid in
// place of the realisations), D = diag(sqrt b) and Mc = I + D A D = L L^T:
//
//     ln L[g, a, r] = -1/2 [ (r^T P0' r - || L^-1 D q ||^2) / s_a + 2 sum_k ln L_kk + c_a ]
//
//   pta_lnl_quad     r0[r, a] = r^T P0' r              one workgroup per (realisation, pulsar): a streaming pass over the residuals, as the
//                                                      N'^-1 norm of the timing-model fit's residual x = r - H y (pta_lnl.h)
//   pta_lnl_factor   Lt[g, a], logdet[g, a]            one workgroup per (grid point, pulsar): Cholesky in LDS, diagonal blocks inverted
//   pta_lnl_apply    ln L[g, a, r]                     L^-1 D q on the fp64 matrix cores, sum of squares and epilogue fused
//   pta_lnl_reduce   ln L[g, r] = sum_a ln L[g, a, r]  ascending a
//
// The factorisation depends on (grid point, pulsar) alone, so it is done once and applied to every realisation: the per-realisation
// work is the blocked forward substitution y = L^-1 (D q) of the K x R block of projections, in blocks of 16 rows, with the 16 x 16
// diagonal blocks of L inverted once by the factorisation (across blocks it stays a substitution, whose error does not grow with the
// condition number of L as that of an explicit T = L^-1 D can; the near-collinear red-noise and common-process columns that make Mc
// ill-conditioned lie in different blocks).
//
// pta_lnl_factor keeps the packed lower triangle column by column in LDS, E[start(k) + (m - k)] = L[m, k], start(k) = k K - k (k - 1) / 2
// (lanes read and write consecutive doubles).  The left-looking sweep is pta_os_matched_solve's: at step j thread t owns row m = j + t,
// every thread accumulates the pivot from the same broadcast reads, one barrier per step.  Then every 16 x 16 diagonal block is
// inverted in place, all blocks at once, from its last column to its first: X[j, j] = 1 / L[j, j], X[i, j] = -X[j, j] sum_{k = j + 1 .. i}
// X[i, k] L[k, j].  The operator leaves as Lt[k * K + i] = L[i, k] (X[i, k] inside the diagonal blocks, zeros above the diagonal), the
// layout pta_lnl_apply stages.
//
// pta_lnl_apply: one workgroup = one pulsar x 128 realisations x a run of grid points.  Each wave keeps the projections of its 2 x 16
// realisations in registers for the whole run, in the B-operand layout of v_mfma_f64_16x16x4_f64 (lane l holds q[r = l & 15][k = 4 step +
// (l >> 4)]); per grid point the operator is staged in LDS as [k][i] with a row stride = 16 mod 32 doubles, so the A-operand read of a
// half-wave (16 rows i x 2 columns k) covers 32 distinct 8-byte slots.  Block row `it`: acc = sum_{jt < it} L[it, jt] y_jt (4 it MFMAs per
// tile), rhs = D q_it - acc, y_it = X[it, it] rhs (4 MFMAs).  The f64 accumulator layout (register e of lane l = row (l >> 4) + 4 e) is the
// B-operand layout of k-step e, so y_jt and rhs feed the next MFMAs from the registers they were produced in.  The squares of y are
// summed per lane in ascending block order and the four lanes of a realisation are joined by two xor shuffles.
//
// Bit-identity: every (g, a, r) value is one fixed sequence of operations on A_a, b[g, a], q[r, a] and r0[r, a]: MFMA output columns
// are independent, rows past R are clamped reads that are never stored, there is no split across workgroups and there are no atomics.
// A value therefore does not depend on R, G, the chunks or the slots it is computed in.
#include "pta_common.h"
#include "pta_lnl.h"
#include "pta_mfma.h"

#define PTA_LNL_RW 2  // 16-realisation tiles per wave of pta_lnl_apply

__device__ __forceinline__ double pta_lnl_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(PTA_LNL_QT) void k_lnl_quad(const double *__restrict__ rows, int64_t ld_rows, const int32_t *__restrict__ psr_off,
                                                         int P, const double *__restrict__ dinv, const int32_t *__restrict__ psr_ep,
                                                         const int32_t *__restrict__ ep_ptr, const int32_t *__restrict__ ep_idx,
                                                         const double *__restrict__ ep_g, const double *__restrict__ q, int64_t ld_q,
                                                         int q_block, int K, int m, const double *__restrict__ Ht, int64_t ldh,
                                                         double *__restrict__ r0) {
  __shared__ double part[PTA_LNL_QT / 64];
  __shared__ double ys[PTA_LNL_MMAX];  // y = G r of this (realisation, pulsar)
  const int a = blockIdx.x % P;
  const int64_t r = blockIdx.x / P;
  const int i0 = psr_off[a], n = psr_off[a + 1] - i0;
  const int e0 = psr_ep ? psr_ep[a] : 0, E = psr_ep ? psr_ep[a + 1] - e0 : 0;
  const int t = threadIdx.x;
  if (t < m) ys[t] = q[pta_lnl_q_index(r, a, K + t, P, K + m, ld_q, q_block)];
  __syncthreads();
  double v = pta_lnl_quad_partial(rows + r * ld_rows + i0, m ? Ht + i0 : nullptr, ldh, ys, m, dinv + i0, n, ep_ptr + e0, ep_idx, ep_g + e0, E, t, PTA_LNL_QT);
  v = pta_lnl_wave_sum(v);
  if ((t & 63) == 0) part[t >> 6] = v;
  __syncthreads();
  if (t == 0) r0[r * P + a] = (part[0] + part[1]) + (part[2] + part[3]);
}

__global__ __launch_bounds__(128) void k_lnl_factor(const double *__restrict__ A, int P, int K, const double *__restrict__ b,
                                                    double *__restrict__ Lt, double *__restrict__ logdet) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  double *E = lds, *d = lds + K * (K + 1) / 2;
  const int64_t ga = blockIdx.x;
  const int a = (int)(ga % P);
  const double *Aa = A + (int64_t)a * K * K;
  const int t = threadIdx.x;
  if (t < K) d[t] = sqrt(b[ga * K + t]);
  __syncthreads();
  // ---- Mc = I + D A D = L L^T, column by column
  double nxt = Aa[min(t, K - 1)], nxt_diag = Aa[0], lsum = 0.0;
  int sj = 0;
  for (int j = 0; j < K; ++j) {
    const int m = j + t, mm = min(m, K - 1);
    const double cur = nxt, ajj = nxt_diag;
    if (j + 1 < K) {  // row j + 1 of the symmetric A, in flight during this step's dot product
      nxt = Aa[(int64_t)(j + 1) * K + min(j + 1 + t, K - 1)];
      nxt_diag = Aa[(int64_t)(j + 1) * K + j + 1];
    }
    double acc = 0.0, dd = 0.0;
    int sk = 0;
#pragma unroll 4
    for (int k = 0; k < j; ++k) {
      const double ejk = E[sk + (j - k)];
      const double emk = E[sk + (mm - k)];
      acc = fma(emk, ejk, acc);
      dd = fma(ejk, ejk, dd);
      sk += K - k;
    }
    const double dj = d[j];
    const double root = sqrt((1.0 + dj * ajj * dj) - dd);
    lsum += log(root);
    if (m < K) E[sj + t] = t == 0 ? root : (dj * cur * d[m] - acc) * (1.0 / root);
    sj += K - j;
    __syncthreads();
  }
  // ---- the 16 x 16 diagonal blocks inverted in place, all blocks at once, from a block's last column to its first
  const int i = t, j0 = (t >> 4) << 4;
  for (int jj = 15; jj >= 0; --jj) {
    const int j = j0 + jj;
    const bool on = i < K && j <= i;
    const int cj = j * K - j * (j - 1) / 2;  // start(j)
    double xjj = 0.0, acc = 0.0;
    if (on) {
      xjj = 1.0 / E[cj];
      int ck = cj + (K - j);  // start(j + 1)
      for (int k = j + 1; k <= i; ++k) {
        acc = fma(E[ck + (i - k)], E[cj + (k - j)], acc);
        ck += K - k;
      }
    }
    __syncthreads();  // column j of the block has been read as L by its threads
    if (on) E[cj + (i - j)] = i == j ? xjj : -acc * xjj;
    __syncthreads();
  }
  // ---- Lt[k][i] = L[i, k] (X[i, k] inside the diagonal blocks), zeros above the diagonal
  double *out = Lt + ga * K * K;
  for (int e = t; e < K * K; e += 128) {
    const int k = e / K, r = e - k * K;
    out[e] = r >= k ? E[k * K - k * (k - 1) / 2 + (r - k)] : 0.0;
  }
  if (t == 0) logdet[ga] = 2.0 * lsum;
}

template <int KT>
__global__ __launch_bounds__(256) void k_lnl_apply(const double *__restrict__ Lt, const double *__restrict__ logdet, const double *__restrict__ b,
                                                   int P, int K, int G, int g_per, const double *__restrict__ q, int64_t ld_q, int q_block, int Kt,
                                                   int R, const double *__restrict__ r0, const double *__restrict__ s, const double *__restrict__ c,
                                                   double *__restrict__ lp, int64_t ld_g, int64_t ld_a) {
  constexpr int KP = 16 * KT, S = KP | 16, RW = PTA_LNL_RW;
  extern __shared__ __attribute__((aligned(16))) double tl[];  // [4 ceil(K / 4)][S]: tl[k * S + i] = L[i, k]; then d [KP]
  const int a = blockIdx.y;
  const int t = threadIdx.x, l = t & 63, w = t >> 6, g4 = l >> 4, m = l & 15;
  const int rbase = (blockIdx.x * 4 + w) * 16 * RW;
  const int nks = (K + 3) / 4;
  double *dl = tl + 4 * nks * S;
  double qv[RW][KP / 4];
#pragma unroll
  for (int u = 0; u < RW; ++u) {
    const int64_t r = min(rbase + 16 * u + m, R - 1);
#pragma unroll
    for (int ks = 0; ks < KP / 4; ++ks) {
      const int k = 4 * ks + g4;
      qv[u][ks] = k < K ? q[pta_lnl_q_index(r, a, k, P, Kt, ld_q, q_block)] : 0.0;
    }
  }
  const double sa = s[a], ca = c[a];
  double r0v[RW];
#pragma unroll
  for (int u = 0; u < RW; ++u) r0v[u] = r0[(int64_t)min(rbase + 16 * u + m, R - 1) * P + a];
  const int g_lo = blockIdx.z * g_per, g_hi = min(G, g_lo + g_per);
  for (int g = g_lo; g < g_hi; ++g) {
    const double *Lg = Lt + ((int64_t)g * P + a) * K * K;
    __syncthreads();  // the previous grid point's operand reads are done
    for (int e = t; e < 4 * nks * KP; e += 256) {
      const int k = e / KP, i = e - k * KP;
      tl[k * S + i] = (k < K && i < K) ? Lg[(int64_t)k * K + i] : 0.0;
    }
    if (t < KP) dl[t] = t < K ? sqrt(b[((int64_t)g * P + a) * K + t]) : 0.0;
    __syncthreads();
    double ss[RW], y[RW][KP / 4];
#pragma unroll
    for (int u = 0; u < RW; ++u) ss[u] = 0.0;
#pragma unroll
    for (int it = 0; it < KT; ++it) {
      if (16 * it < K) {
        pta_f64x4 acc[RW], yy[RW];
#pragma unroll
        for (int u = 0; u < RW; ++u) acc[u] = yy[u] = pta_f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int ks = 0; ks < 4 * it; ++ks) {  // the blocks left of the diagonal: L[it, jt] y_jt
          const double av = tl[(4 * ks + g4) * S + 16 * it + m];
#pragma unroll
          for (int u = 0; u < RW; ++u) acc[u] = pta_mfma_f64(av, y[u][ks], acc[u]);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {  // the diagonal block's inverse times D q_it - acc; accumulator register e = B operand of k-step e
          if (4 * it + e < nks) {
            const double av = tl[(16 * it + 4 * e + g4) * S + 16 * it + m];
            const double dk = dl[16 * it + 4 * e + g4];
#pragma unroll
            for (int u = 0; u < RW; ++u) yy[u] = pta_mfma_f64(av, dk * qv[u][4 * it + e] - acc[u][e], yy[u]);
          }
        }
#pragma unroll
        for (int u = 0; u < RW; ++u)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            y[u][4 * it + e] = yy[u][e];
            ss[u] = fma(yy[u][e], yy[u][e], ss[u]);
          }
      }
    }
    const double ld = logdet[(int64_t)g * P + a];
#pragma unroll
    for (int u = 0; u < RW; ++u) {
      double v = ss[u];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      const int r = rbase + 16 * u + m;
      if (g4 == 0 && r < R) lp[(int64_t)g * ld_g + (int64_t)a * ld_a + r] = pta_lnl_value(r0v[u], v, sa, ld, ca);
    }
  }
}

__global__ void k_lnl_reduce(const double *__restrict__ lp, int64_t ld_g, int64_t ld_a, int P, int G, int R, double *__restrict__ lnl,
                             int64_t ld_lnl) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)G * R) return;
  const int64_t g = idx / R, r = idx - g * R;
  double v = 0.0;
  for (int a = 0; a < P; ++a) v += lp[g * ld_g + a * ld_a + r];  // ascending pulsars
  lnl[g * ld_lnl + r] = v;
}

extern "C" int pta_lnl_quad(const double *rows, int64_t ld_rows, int R, const int32_t *psr_off, int P, const double *dinv,
                            const int32_t *psr_ep, const int32_t *ep_ptr, const int32_t *ep_idx, const double *ep_g, const double *q,
                            int64_t ld_q, int q_block, int K, int m, const double *Ht, int64_t ldh, double *r0, void *stream) {
  PTA_REQUIRE(rows && psr_off && dinv && r0, PTA_E_ARG, "pta_lnl_quad: NULL argument");
  PTA_REQUIRE(!psr_ep || (ep_ptr && ep_idx && ep_g), PTA_E_ARG, "pta_lnl_quad: psr_ep without the epoch lists");
  PTA_REQUIRE(P > 0 && R > 0 && (int64_t)R * P <= 0x7fffffffLL && ld_rows >= 1, PTA_E_ARG, "pta_lnl_quad: P=%d R=%d ld_rows=%lld", P, R,
              (long long)ld_rows);
  PTA_REQUIRE(K >= 0 && K <= PTA_LNL_KMAX && m >= 0 && m <= PTA_LNL_MMAX, PTA_E_ARG, "pta_lnl_quad: K=%d (0..%d) m=%d (0..%d)", K, PTA_LNL_KMAX, m,
              PTA_LNL_MMAX);
  PTA_REQUIRE(m == 0 || (q && Ht && ldh >= 1 && q_block >= 1 && ld_q >= (int64_t)P * (K + m)), PTA_E_ARG,
              "pta_lnl_quad: m=%d timing-model rows need q and Ht with q_block >= 1 and ld_q >= P * (K + m)", m);
  hipLaunchKernelGGL(k_lnl_quad, dim3((unsigned)((int64_t)R * P)), dim3(PTA_LNL_QT), 0, pta_stream(stream), rows, ld_rows, psr_off, P, dinv, psr_ep,
                     ep_ptr, ep_idx, ep_g, q, ld_q, q_block, K, m, Ht, ldh, r0);
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}

extern "C" int pta_lnl_factor(const double *A, int P, int K, int C, int G, const double *b, double *Lt, double *logdet, void *stream) {
  PTA_REQUIRE(A && b && Lt && logdet, PTA_E_ARG, "pta_lnl_factor: NULL argument");
  PTA_REQUIRE(K >= 1 && K <= PTA_LNL_KMAX && C >= 0 && C <= K, PTA_E_ARG, "pta_lnl_factor: K=%d (1..%d) C=%d (0..K)", K, PTA_LNL_KMAX, C);
  PTA_REQUIRE(P > 0 && G > 0 && (int64_t)G * P <= 0x7fffffffLL, PTA_E_ARG, "pta_lnl_factor: P=%d G=%d", P, G);
  const size_t shmem = ((size_t)K * (K + 1) / 2 + K) * sizeof(double);
  if (shmem > 65536) PTA_HIP(hipFuncSetAttribute((const void *)k_lnl_factor, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
  hipLaunchKernelGGL(k_lnl_factor, dim3((unsigned)((int64_t)G * P)), dim3(128), shmem, pta_stream(stream), A, P, K, b, Lt, logdet);
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}

template <int KT>
static int pta_lnl_apply_launch(dim3 grid, size_t shmem, hipStream_t st, const double *Lt, const double *logdet, const double *b, int P, int K, int G,
                                int g_per, const double *q, int64_t ld_q, int q_block, int Kt, int R, const double *r0, const double *s, const double *c,
                                double *lp, int64_t ld_g, int64_t ld_a) {
  if (shmem > 65536) PTA_HIP(hipFuncSetAttribute((const void *)k_lnl_apply<KT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
  hipLaunchKernelGGL((k_lnl_apply<KT>), grid, dim3(256), shmem, st, Lt, logdet, b, P, K, G, g_per, q, ld_q, q_block, Kt, R, r0, s, c, lp, ld_g, ld_a);
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}

// The launch plan of pta_lnl_apply, the one place it is decided: the k_lnl_apply<kt> instance, g_per grid points per workgroup and gz
// workgroups along the grid.  `who` names the entry in the refusals.
static int pta_lnl_apply_choose(const char *who, int P, int K, int G, int R, int &kt, int &g_per, unsigned &gz) {
  PTA_REQUIRE(K >= 1 && K <= PTA_LNL_KMAX, PTA_E_ARG, "%s: K=%d (1..%d)", who, K, PTA_LNL_KMAX);
  PTA_REQUIRE(P > 0 && P <= 65535 && G > 0 && R > 0, PTA_E_ARG, "%s: P=%d G=%d R=%d", who, P, G, R);
  kt = (K + 15) / 16;
  const unsigned rb = pta_cdiv(R, 64 * PTA_LNL_RW);
  // grid points per workgroup (they share the projections held in registers): as many as leave the device a few thousand workgroups
  long long gp = (long long)G * P * rb / 4096;
  gp = gp < 1 ? 1 : (gp > 16 ? 16 : gp);
  g_per = (int)gp;
  gz = pta_cdiv(G, gp);
  PTA_REQUIRE(gz <= 65535u, PTA_E_ARG, "%s: G=%d exceeds one launch", who, G);
  return PTA_OK;
}

extern "C" int pta_lnl_apply_plan(int P, int K, int G, int R, int32_t *plan) {
  PTA_REQUIRE(plan, PTA_E_ARG, "pta_lnl_apply_plan: NULL argument");
  int kt, g_per;
  unsigned gz;
  const int rc = pta_lnl_apply_choose("pta_lnl_apply_plan", P, K, G, R, kt, g_per, gz);
  if (rc != PTA_OK) return rc;
  plan[0] = kt, plan[1] = g_per, plan[2] = (int32_t)gz;
  return PTA_OK;
}

extern "C" int pta_lnl_apply(const double *Lt, const double *logdet, const double *b, int P, int K, int C, int G, const double *q, int64_t ld_q, int q_block, int Kt,
                             int R, const double *r0, const double *s, const double *c, double *lnl_pulsar, int64_t ld_g, int64_t ld_a,
                             void *stream) {
  PTA_REQUIRE(Lt && logdet && b && q && r0 && s && c && lnl_pulsar, PTA_E_ARG, "pta_lnl_apply: NULL argument");
  PTA_REQUIRE(K >= 1 && K <= PTA_LNL_KMAX && C >= 0 && C <= K && Kt >= K && Kt <= K + PTA_LNL_MMAX, PTA_E_ARG,
              "pta_lnl_apply: K=%d (1..%d) C=%d (0..K) Kt=%d (K..K+%d)", K, PTA_LNL_KMAX, C, Kt, PTA_LNL_MMAX);
  PTA_REQUIRE(P > 0 && P <= 65535 && G > 0 && R > 0, PTA_E_ARG, "pta_lnl_apply: P=%d G=%d R=%d", P, G, R);
  PTA_REQUIRE(q_block >= 1 && ld_q >= (int64_t)P * Kt && ld_a >= R && ld_g >= 1, PTA_E_ARG,
              "pta_lnl_apply: q_block=%d ld_q=%lld (>= P * Kt) ld_a=%lld (>= R)", q_block, (long long)ld_q, (long long)ld_a);
  int kt, g_per;
  unsigned gz;
  const int rc = pta_lnl_apply_choose("pta_lnl_apply", P, K, G, R, kt, g_per, gz);
  if (rc != PTA_OK) return rc;
  const int kp = 16 * kt, S = kp | 16;
  const unsigned rb = pta_cdiv(R, 64 * PTA_LNL_RW);
  const size_t shmem = ((size_t)4 * ((K + 3) / 4) * S + kp) * sizeof(double);
  dim3 grid(rb, P, gz);
  hipStream_t st = pta_stream(stream);
#define PTA_LNL_CASE(KT_) \
  case KT_:               \
    return pta_lnl_apply_launch<KT_>(grid, shmem, st, Lt, logdet, b, P, K, G, g_per, q, ld_q, q_block, Kt, R, r0, s, c, lnl_pulsar, ld_g, ld_a);
  switch (kt) {
    PTA_LNL_CASE(1) PTA_LNL_CASE(2) PTA_LNL_CASE(3) PTA_LNL_CASE(4) PTA_LNL_CASE(5) PTA_LNL_CASE(6) PTA_LNL_CASE(7) PTA_LNL_CASE(8)
  }
#undef PTA_LNL_CASE
  return PTA_E_ARG;
}

extern "C" int pta_lnl_reduce(const double *lnl_pulsar, int64_t ld_g, int64_t ld_a, int P, int G, int R, double *lnl, int64_t ld_lnl, void *stream) {
  PTA_REQUIRE(lnl_pulsar && lnl, PTA_E_ARG, "pta_lnl_reduce: NULL argument");
  PTA_REQUIRE(P > 0 && G > 0 && R > 0 && ld_a >= R && ld_lnl >= R && ld_g >= 1, PTA_E_ARG, "pta_lnl_reduce: P=%d G=%d R=%d ld_a=%lld ld_lnl=%lld", P, G,
              R, (long long)ld_a, (long long)ld_lnl);
  const int64_t total = (int64_t)G * R;
  PTA_REQUIRE(total < (1LL << 31) * 256, PTA_E_ARG, "pta_lnl_reduce: problem too large");
  hipLaunchKernelGGL(k_lnl_reduce, dim3(pta_cdiv(total, 256)), dim3(256), 0, pta_stream(stream), lnl_pulsar, ld_g, ld_a, P, G, R, lnl, ld_lnl);
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}
