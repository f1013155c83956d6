// Optimal statistic under per-realisation noise parameters (pta_replicator_amd/optimal_statistic.py holds the algebra and the
// theta-independent preparation: V = U^T P0', A = U^T P0' U per pulsar, U = [F_rn | F]).  Per batch:
//
//   pta_os_project         q[r, a, :] = V_a r_a                       the existing projection, once per block of <= 64 rows of V
//   pta_os_matched_prior   b[r, a, k] = prior variance / s            elementwise (pta_os_matched.h)
//   pta_os_matched_prior_spec   the same with the GW columns from a per-realisation spectrum (M nodes of log10 hc)
//   pta_os_matched_solve   X[r, a, :], Z[r, a, :, :]                  one workgroup per (realisation, pulsar), everything in LDS
//   pta_os_matched_pairs   num, den, A2, sigma per realisation        one workgroup per realisation, one wave per pair
//
// pta_os_matched_solve factors Mc = I + D A D (D = diag sqrt b) and substitutes the 1 + C right-hand sides D [q | A[:, F]] in one
// left-looking sweep over the augmented matrix [Mc | D q | D A_F].  LDS row k holds what step k produced, contiguous in m:
//     E[k][m] = L[m, k] for k < m < K,    E[k][K + c] = H[k, c] for c <= C          (K + C - k doubles; the diagonal is not kept)
// At step j thread t owns m = j + 1 + t:  E[j][m] = (init(j, m) - sum_{k<j} E[k][m] E[k][j]) / sqrt(p_j),  p_j = Mc[j, j] - sum_{k<j} E[k][j]^2.
// Every thread reads row j of L (E[k][j], a broadcast) for its own dot product, so it accumulates p_j from the same reads: one
// barrier per step.  Lanes read and write consecutive doubles (no bank conflicts); init(j, .) comes from row j of the symmetric A
// (L2-resident, coalesced), fetched one step ahead.  X and Z then are K-long dot products of columns of H.
//
// Bit-identity: a workgroup sees one (realisation, pulsar) and sums over k in ascending order; pta_os_matched_pairs gives pair p to
// wave p mod 4 of its realisation's workgroup, sums each wave's pairs in ascending order and joins the four waves in a fixed
// tree.  No atomics, no split across realisations: a result does not depend on R, the chunk or the row slot.
#include "pta_common.h"
#include "pta_os_matched.h"

#define PTA_OSM_KMAX 128  // K = K_rn + C
#define PTA_OSM_CMAX 64   // C = 2 n_f
#define PTA_OSM_NORF 8

__global__ void k_osm_prior(int R, int P, int K_rn, int C, const double *__restrict__ rn_f, const double *__restrict__ rn_tspan,
                            const double *__restrict__ rn_phi, const double *__restrict__ rn_log10_A, const double *__restrict__ rn_gamma,
                            double T, const double *__restrict__ gw_log10_A, const double *__restrict__ gw_gamma,
                            const double *__restrict__ s, double *__restrict__ b) {
  const int K = K_rn + C;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)R * P * K) return;
  const int k = (int)(idx % K);
  const int64_t ra = idx / K;
  const int a = (int)(ra % P);
  const int64_t r = ra / P;
  double v;
  if (k < K_rn) {
    const double lA = rn_log10_A ? rn_log10_A[ra] : NAN;
    v = pta_osm_rn_b(rn_f[(int64_t)a * (K_rn / 2) + k / 2], rn_tspan[a], lA, rn_log10_A ? rn_gamma[ra] : 0.0, rn_phi[(int64_t)a * K_rn + k], s[a]);
  } else {
    v = gw_log10_A ? pta_osm_gw_b((double)((k - K_rn) / 2 + 1) / T, T, gw_log10_A[r], gw_gamma[r], s[a]) : 0.0;
  }
  b[idx] = v;
}

// k_osm_prior with the GW columns hc_r(f_k)^2 / (12 pi^2 f_k^3 T) / s_a: hc_r interpolated from realisation r's M nodes with the
// tables of the n_f = C / 2 frequencies k / T (pta_gwb_hcf_user); the node rows are a few hundred bytes, read through the cache
__global__ void k_osm_prior_spec(int R, int P, int K_rn, int C, const double *__restrict__ rn_f, const double *__restrict__ rn_tspan,
                                 const double *__restrict__ rn_phi, const double *__restrict__ rn_log10_A, const double *__restrict__ rn_gamma,
                                 double T, const int32_t *__restrict__ seg, const double *__restrict__ dx, const double *__restrict__ dxp, int M,
                                 const double *__restrict__ log10_hc, int64_t ld_hc, const double *__restrict__ s, double *__restrict__ b) {
  const int K = K_rn + C;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)R * P * K) return;
  const int k = (int)(idx % K);
  const int64_t ra = idx / K;
  const int a = (int)(ra % P);
  const int64_t r = ra / P;
  double v;
  if (k < K_rn) {
    const double lA = rn_log10_A ? rn_log10_A[ra] : NAN;
    v = pta_osm_rn_b(rn_f[(int64_t)a * (K_rn / 2) + k / 2], rn_tspan[a], lA, rn_log10_A ? rn_gamma[ra] : 0.0, rn_phi[(int64_t)a * K_rn + k], s[a]);
  } else {
    const int c = (k - K_rn) / 2;
    v = pta_osm_gw_b_hc((double)(c + 1) / T, T, pta_gwb_hcf_user(log10_hc + r * ld_hc, M, seg[c], dx[c], dxp[c]), s[a]);
  }
  b[idx] = v;
}

__device__ __forceinline__ int64_t pta_osm_q_index(int64_t r, int a, int k, int P, int K, int64_t ld_q, int q_block) {
  const int k0 = (k / q_block) * q_block;
  const int cb = min(q_block, K - k0);
  return r * ld_q + (int64_t)P * k0 + (int64_t)a * cb + (k - k0);
}

__global__ __launch_bounds__(256) void k_osm_solve(const double *__restrict__ A, int P, int K, int C, const double *__restrict__ b,
                                                   const double *__restrict__ q, int64_t ld_q, int q_block, const double *__restrict__ S,
                                                   const double *__restrict__ s, double *__restrict__ X, double *__restrict__ Z) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int W = K + C;                      // row k of E holds m = k + 1 .. W
  const int nE = K * W - K * (K - 1) / 2;
  double *E = lds, *d = lds + nE, *qs = d + K;
  const int64_t ra = blockIdx.x;
  const int a = (int)(ra % P);
  const int64_t r = ra / P;
  const double *Aa = A + (int64_t)a * K * K;
  const int t = threadIdx.x;
  if (t < K) {
    d[t] = sqrt(b[ra * K + t]);
    qs[t] = q[pta_osm_q_index(r, a, t, P, K, ld_q, q_block)];
  }
  __syncthreads();
  const int F0 = K - C;
  // raw (unscaled) entry (j, m) of [A | q | A_F]; m is clamped by the caller to <= W
  auto raw = [&](int j, int m) { return m < K ? Aa[(int64_t)j * K + m] : (m == K ? qs[j] : Aa[(int64_t)j * K + F0 + (m - K - 1)]); };
  double nxt = raw(0, min(1 + t, W)), nxt_diag = Aa[0];
  int sj = 0;                               // start of row j in E
  for (int j = 0; j < K; ++j) {
    const int m = j + 1 + t, mm = min(m, W);
    const double cur = nxt, ajj = nxt_diag;
    if (j + 1 < K) {                        // next step's operands, in flight during this step's dot product
      nxt = raw(j + 1, min(j + 2 + t, W));
      nxt_diag = Aa[(int64_t)(j + 1) * K + j + 1];
    }
    double acc = 0.0, dd = 0.0;
    int sk = 0;
#pragma unroll 4
    for (int k = 0; k < j; ++k) {
      const double ejk = E[sk + (j - k - 1)];
      const double emk = E[sk + (mm - k - 1)];
      acc = fma(emk, ejk, acc);
      dd = fma(ejk, ejk, dd);
      sk += W - k;
    }
    const double dj = d[j];
    const double p = (1.0 + dj * ajj * dj) - dd;
    const double inv = 1.0 / sqrt(p);
    if (m <= W) E[sj + t] = ((m < K ? dj * cur * d[m] : dj * cur) - acc) * inv;
    sj += W - j;
    __syncthreads();
  }
  // H[k, c] = E[k][K + c] at E[start(k) + K + c - k - 1]
  const int nz = C * (C + 1) / 2;
  const double sa = s[a];
  for (int e = t; e < C + nz; e += 256) {
    int c1, c2;                             // columns of H: c1 of A_F (1 + c), c2 = 0 (q) for X or a second column of A_F
    if (e < C) {
      c1 = e;
      c2 = -1;
    } else {
      const int z = e - C;
      c1 = (int)((sqrt(8.0 * z + 1.0) - 1.0) * 0.5);
      while (c1 * (c1 + 1) / 2 > z) --c1;
      while ((c1 + 1) * (c1 + 2) / 2 <= z) ++c1;
      c2 = z - c1 * (c1 + 1) / 2;
    }
    double acc = 0.0;
    int hk = K - 1;                         // start(k) + K - k - 1: H[k, 0]
    for (int k = 0; k < K; ++k) {
      acc = fma(E[hk + 1 + c1], E[hk + 1 + c2], acc);
      hk += W - k - 1;
    }
    if (e < C) {
      X[ra * C + c1] = sqrt(S[c1]) * (qs[F0 + c1] - acc) / sa;
    } else {
      Z[ra * nz + (e - C)] = sqrt(S[c1]) * (Aa[(int64_t)(F0 + c1) * K + F0 + c2] - acc) * sqrt(S[c2]) / sa;
    }
  }
}

__device__ __forceinline__ double pta_osm_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void k_osm_pairs(const double *__restrict__ X, const double *__restrict__ Z, int P, int C,
                                                   const int32_t *__restrict__ pa, const int32_t *__restrict__ pb, int np,
                                                   const double *__restrict__ G, const double *__restrict__ G2, int n_orf,
                                                   double *__restrict__ A2, int64_t ld_a2, double *__restrict__ sigma, int64_t ld_sigma,
                                                   double *__restrict__ rho, double *__restrict__ sigma_pair, int64_t ld_p) {
  __shared__ double wz[PTA_OSM_CMAX * (PTA_OSM_CMAX + 1) / 2];  // 1 on the diagonal of the packed lower triangle, 2 off it
  __shared__ double part[2][4][PTA_OSM_NORF];
  const int nz = C * (C + 1) / 2;
  const int64_t r = blockIdx.x;
  const int t = threadIdx.x, l = t & 63, w = t >> 6;
  for (int e = t; e < nz; e += 256) wz[e] = 2.0;
  __syncthreads();
  if (t < C) wz[t * (t + 1) / 2 + t] = 1.0;
  __syncthreads();
  const double *Xr = X + r * P * C, *Zr = Z + r * P * nz;
  double sn[PTA_OSM_NORF], sd[PTA_OSM_NORF];
#pragma unroll
  for (int o = 0; o < PTA_OSM_NORF; ++o) sn[o] = sd[o] = 0.0;
  for (int p = w; p < np; p += 4) {         // fixed pair -> wave assignment, ascending within the wave
    const int a = pa[p], bq = pb[p];
    const double *xa = Xr + (int64_t)a * C, *xb = Xr + (int64_t)bq * C, *za = Zr + (int64_t)a * nz, *zb = Zr + (int64_t)bq * nz;
    double num = 0.0, den = 0.0;
    for (int c = l; c < C; c += 64) num = fma(xa[c], xb[c], num);
    for (int e = l; e < nz; e += 64) den = fma(wz[e] * za[e], zb[e], den);
    num = pta_osm_wave_sum(num);
    den = pta_osm_wave_sum(den);
    if (rho && l == 0) {
      rho[r * ld_p + p] = num / den;
      sigma_pair[r * ld_p + p] = 1.0 / sqrt(den);
    }
#pragma unroll
    for (int o = 0; o < PTA_OSM_NORF; ++o)
      if (o < n_orf) {
        sn[o] = fma(G[(int64_t)o * np + p], num, sn[o]);
        sd[o] = fma(G2[(int64_t)o * np + p], den, sd[o]);
      }
  }
#pragma unroll
  for (int o = 0; o < PTA_OSM_NORF; ++o)
    if (o < n_orf && l == 0) {
      part[0][w][o] = sn[o];
      part[1][w][o] = sd[o];
    }
  __syncthreads();
  if (t < n_orf) {
    const double n = (part[0][0][t] + part[0][1][t]) + (part[0][2][t] + part[0][3][t]);
    const double dn = (part[1][0][t] + part[1][1][t]) + (part[1][2][t] + part[1][3][t]);
    A2[r * ld_a2 + t] = n / dn;
    sigma[r * ld_sigma + t] = 1.0 / sqrt(dn);
  }
}

extern "C" int pta_os_matched_prior(int R, int P, int K_rn, int C, const double *rn_f, const double *rn_tspan, const double *rn_phi,
                                    const double *rn_log10_A, const double *rn_gamma, double T, const double *gw_log10_A,
                                    const double *gw_gamma, const double *s, double *b, void *stream) {
  PTA_REQUIRE(s && b, PTA_E_ARG, "pta_os_matched_prior: NULL argument");
  PTA_REQUIRE(R > 0 && P > 0 && K_rn >= 0 && (K_rn % 2) == 0 && C >= 2 && (C % 2) == 0 && C <= PTA_OSM_CMAX && K_rn + C <= PTA_OSM_KMAX, PTA_E_ARG,
              "pta_os_matched_prior: R=%d P=%d K_rn=%d C=%d (K_rn, C even, C <= %d, K_rn + C <= %d)", R, P, K_rn, C, PTA_OSM_CMAX, PTA_OSM_KMAX);
  PTA_REQUIRE(K_rn == 0 || (rn_f && rn_tspan && rn_phi), PTA_E_ARG, "pta_os_matched_prior: red-noise tables missing");
  PTA_REQUIRE(!rn_log10_A == !rn_gamma && !gw_log10_A == !gw_gamma, PTA_E_ARG, "pta_os_matched_prior: amplitude and index come together");
  PTA_REQUIRE(T > 0, PTA_E_ARG, "pta_os_matched_prior: T=%g", T);
  const int64_t total = (int64_t)R * P * (K_rn + C);
  PTA_REQUIRE(total < (1LL << 31) * 256, PTA_E_ARG, "pta_os_matched_prior: problem too large");
  hipLaunchKernelGGL(k_osm_prior, dim3(pta_cdiv(total, 256)), dim3(256), 0, pta_stream(stream), R, P, K_rn, C, rn_f, rn_tspan, rn_phi,
                     rn_log10_A, rn_gamma, T, gw_log10_A, gw_gamma, s, b);
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}

extern "C" int pta_os_matched_prior_spec(int R, int P, int K_rn, int C, const double *rn_f, const double *rn_tspan, const double *rn_phi,
                                         const double *rn_log10_A, const double *rn_gamma, double T, const int32_t *seg, const double *dx,
                                         const double *dxp, int M, const double *log10_hc, int64_t ld_hc, const double *s, double *b,
                                         void *stream) {
  PTA_REQUIRE(s && b && seg && dx && dxp && log10_hc, PTA_E_ARG, "pta_os_matched_prior_spec: NULL argument");
  PTA_REQUIRE(R > 0 && P > 0 && K_rn >= 0 && (K_rn % 2) == 0 && C >= 2 && (C % 2) == 0 && C <= PTA_OSM_CMAX && K_rn + C <= PTA_OSM_KMAX, PTA_E_ARG,
              "pta_os_matched_prior_spec: R=%d P=%d K_rn=%d C=%d (K_rn, C even, C <= %d, K_rn + C <= %d)", R, P, K_rn, C, PTA_OSM_CMAX,
              PTA_OSM_KMAX);
  PTA_REQUIRE(M >= 2 && ld_hc >= M, PTA_E_ARG, "pta_os_matched_prior_spec: M=%d (>= 2 nodes) ld_hc=%lld", M, (long long)ld_hc);
  PTA_REQUIRE(K_rn == 0 || (rn_f && rn_tspan && rn_phi), PTA_E_ARG, "pta_os_matched_prior_spec: red-noise tables missing");
  PTA_REQUIRE(!rn_log10_A == !rn_gamma, PTA_E_ARG, "pta_os_matched_prior_spec: amplitude and index come together");
  PTA_REQUIRE(T > 0, PTA_E_ARG, "pta_os_matched_prior_spec: T=%g", T);
  const int64_t total = (int64_t)R * P * (K_rn + C);
  PTA_REQUIRE(total < (1LL << 31) * 256 && (int64_t)R * ld_hc < (1LL << 31), PTA_E_ARG, "pta_os_matched_prior_spec: problem too large");
  hipLaunchKernelGGL(k_osm_prior_spec, dim3(pta_cdiv(total, 256)), dim3(256), 0, pta_stream(stream), R, P, K_rn, C, rn_f, rn_tspan, rn_phi,
                     rn_log10_A, rn_gamma, T, seg, dx, dxp, M, log10_hc, ld_hc, s, b);
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}

extern "C" int pta_os_matched_solve(const double *A, int P, int K, int C, int R, const double *b, const double *q, int64_t ld_q, int q_block,
                                    const double *S, const double *s, double *X, double *Z, void *stream) {
  PTA_REQUIRE(A && b && q && S && s && X && Z, PTA_E_ARG, "pta_os_matched_solve: NULL argument");
  PTA_REQUIRE(K >= 1 && K <= PTA_OSM_KMAX && C >= 1 && C <= PTA_OSM_CMAX && C <= K, PTA_E_ARG,
              "pta_os_matched_solve: K=%d (1..%d) C=%d (1..%d, <= K)", K, PTA_OSM_KMAX, C, PTA_OSM_CMAX);
  PTA_REQUIRE(P > 0 && R > 0 && (int64_t)R * P <= 0x7fffffffLL, PTA_E_ARG, "pta_os_matched_solve: P=%d R=%d", P, R);
  PTA_REQUIRE(q_block >= 1 && ld_q >= (int64_t)P * K, PTA_E_ARG, "pta_os_matched_solve: q_block=%d ld_q=%lld < P*K=%d", q_block, (long long)ld_q,
              P * K);
  const size_t shmem = ((size_t)K * (K + C) - (size_t)K * (K - 1) / 2 + 2 * (size_t)K) * sizeof(double);
  if (shmem > 65536) PTA_HIP(hipFuncSetAttribute((const void *)k_osm_solve, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
  hipLaunchKernelGGL(k_osm_solve, dim3((unsigned)((int64_t)R * P)), dim3(256), shmem, pta_stream(stream), A, P, K, C, b, q, ld_q, q_block, S, s, X,
                     Z);
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}

extern "C" int pta_os_matched_pairs(const double *X, const double *Z, int P, int C, int R, const int32_t *pair_a, const int32_t *pair_b, int n_pairs,
                                    const double *G, const double *G2, int n_orf, double *A2, int64_t ld_a2, double *sigma, int64_t ld_sigma,
                                    double *rho, double *sigma_pair, int64_t ld_pair, void *stream) {
  PTA_REQUIRE(X && Z && pair_a && pair_b && G && G2 && A2 && sigma, PTA_E_ARG, "pta_os_matched_pairs: NULL argument");
  PTA_REQUIRE(P >= 2 && C >= 1 && C <= PTA_OSM_CMAX && R > 0 && n_pairs >= 1 && n_orf >= 1 && n_orf <= PTA_OSM_NORF, PTA_E_ARG,
              "pta_os_matched_pairs: P=%d C=%d R=%d n_pairs=%d n_orf=%d (1..%d)", P, C, R, n_pairs, n_orf, PTA_OSM_NORF);
  PTA_REQUIRE(!rho == !sigma_pair, PTA_E_ARG, "pta_os_matched_pairs: rho and sigma_pair come together");
  PTA_REQUIRE(ld_a2 >= n_orf && ld_sigma >= n_orf && (!rho || ld_pair >= n_pairs), PTA_E_ARG, "pta_os_matched_pairs: leading dimension too small");
  hipLaunchKernelGGL(k_osm_pairs, dim3(R), dim3(256), 0, pta_stream(stream), X, Z, P, C, pair_a, pair_b, n_pairs, G, G2, n_orf, A2, ld_a2, sigma,
                     ld_sigma, rho, sigma_pair, ld_pair);
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}
