// Likelihood ratio of a common process with inter-pulsar correlations (Hellings-Downs, monopole, dipole, none, or a user ORF) against
// noise only, per realisation on a grid of (log10_A, gamma) - pta_replicator_amd/optimal_statistic.py holds the algebra, the host
// preparation (clnl_plan) and the NumPy twin (clnl_from_rows).  The intrinsic noise is the configured one, so with Gamma = B B^T
// (B [P, rho]), Y = W r (pta_os_project), T = (B^T (x) I) blockdiag(Z_a) (B (x) I) and D_g = I_rho (x) diag(d_g):
//
//     M_g = I + D_g T D_g = L_g L_g^T        n = rho C rows, eigenvalues >= 1
//     ratio[g, r] = 1/2 || L_g^-1 D_g Y'_r ||^2 - sum_i ln L_g,ii,    Y'_r = (B^T (x) I) Y_r
//
//   pta_clnl_mix        Y'[r, i, :] = sum_a B^T[i, a] Y[r, a, :]     one workgroup per realisation, its Y in LDS, pulsars ascending
//   pta_clnl_assemble   M_g (lower triangle and diagonal, zeros above)  one workgroup per (grid point, 4 rows), d_g in LDS
//   (pta_potrf_batched_ex factors the grid chunk in place)
//   pta_clnl_rhs        V[g][i, r] = d_g,i Y'[r, i]                   32 x 32 tiles of Y' transposed through LDS, every grid point
//   pta_clnl_solve      V <- L_g^-1 V, quad[g, r] = sum_i V[i, r]^2   blocked forward substitution: pta_dgemm + the diagonal block, per 64 rows
//   pta_clnl_finish     ratio[g, r] = quad / 2 - sum_i ln L_ii        one workgroup per grid point
//
// pta_clnl_solve: blocked forward substitution over blocks of 64 rows.  For block j (rows j0 = 64 j ..) the update V_j -= L[j, < j0] V[< j0]
// is pta_dgemm (transB = 0, beta = 1, batch = grid points): its operands have at most 64 rows, which selects the 64 x 64-tile kernel
// whatever R, and that kernel forms every element as one chain of v_mfma_f64_16x16x4_f64 over k in ascending order.  Then
// k_clnl_solve_diag finishes the block: the packed diagonal block L_jj (16.6 KB) is staged in LDS, every thread of a one-wave workgroup keeps one
// column of V_j in LDS slots of its own and substitutes in ascending row order, adding the squares to quad in that order.  V[< j0] was written by earlier
// launches, so no workgroup re-reads its own stores.
//
// Bit-identity: a value (g, r) is one fixed sequence of operations on L_g and column r: MFMA output columns are independent, rows past
// n and columns past R are clamped reads that are never stored, no reduction is split across workgroups and there are no atomics.  It
// does not depend on R, G, the leading dimensions or the chunks and slots it is computed in.
#include "pta_common.h"
#include "pta_clnl.h"

__global__ __launch_bounds__(256) void k_clnl_mix(const double *__restrict__ Y, int64_t ld_y, int P, int C, const double *__restrict__ Bt,
                                                  int rho, double *__restrict__ Yp, int64_t ld_yp) {
  extern __shared__ __attribute__((aligned(16))) double ys[];  // Y of this realisation [P, C]
  const int64_t r = blockIdx.x;
  const int t = threadIdx.x;
  for (int e = t; e < P * C; e += 256) ys[e] = Y[r * ld_y + e];
  __syncthreads();
  for (int e = t; e < rho * C; e += 256) {
    const int i = e / C, k = e - i * C;
    double acc = 0.0;
    for (int a = 0; a < P; ++a) acc = fma(Bt[(int64_t)i * P + a], ys[a * C + k], acc);  // ascending pulsars
    Yp[r * ld_yp + e] = acc;
  }
}

__global__ __launch_bounds__(256) void k_clnl_assemble(const double *__restrict__ T, int n, int C, double gamma_ref, double Tspan,
                                                       const double *__restrict__ log10_A, const double *__restrict__ gamma,
                                                       double *__restrict__ M) {
  __shared__ double d[PTA_CLNL_CMAX];
  const int g = blockIdx.y, t = threadIdx.x;
  if (t < C) d[t] = pta_clnl_scale(t, Tspan, gamma_ref, log10_A[g], gamma[g]);
  __syncthreads();
  double *Mg = M + (int64_t)g * n * n;
  const int i0 = blockIdx.x * 4;
  for (int ii = 0; ii < 4; ++ii) {
    const int i = i0 + ii;
    if (i >= n) break;
    const double di = d[i % C];
    const double *Ti = T + (int64_t)i * n;
    double *Mi = Mg + (int64_t)i * n;
    for (int j = t; j < n; j += 256) Mi[j] = j <= i ? pta_clnl_m_entry(di, Ti[j], d[j % C], j == i) : 0.0;
  }
}

__global__ __launch_bounds__(256) void k_clnl_rhs(const double *__restrict__ Yp, int64_t ld_yp, int n, int C, int R, double gamma_ref,
                                                  double Tspan, const double *__restrict__ log10_A, const double *__restrict__ gamma, int G,
                                                  double *__restrict__ V, int64_t ld_v) {
  __shared__ double tile[32][33];  // tile[realisation][row]
  __shared__ double d[32];
  const int t = threadIdx.x, lx = t & 31, ly = t >> 5;
  const int i0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
  for (int s = 0; s < 4; ++s) {
    const int rl = ly + 8 * s;
    tile[rl][lx] = Yp[(int64_t)min(r0 + rl, R - 1) * ld_yp + min(i0 + lx, n - 1)];
  }
  for (int g = 0; g < G; ++g) {
    __syncthreads();  // the tile is loaded; the previous grid point's d has been read
    if (t < 32) d[t] = pta_clnl_scale(min(i0 + t, n - 1) % C, Tspan, gamma_ref, log10_A[g], gamma[g]);
    __syncthreads();
    double *Vg = V + (int64_t)g * n * ld_v;
    for (int s = 0; s < 4; ++s) {
      const int il = ly + 8 * s, i = i0 + il, r = r0 + lx;
      if (i < n && r < R) Vg[(int64_t)i * ld_v + r] = d[il] * tile[lx][il];
    }
  }
}

__global__ __launch_bounds__(PTA_CLNL_RT) void k_clnl_solve_diag(const double *__restrict__ L, int n, double *__restrict__ V, int64_t ld_v, int R,
                                                                 double *__restrict__ quad, int64_t ld_quad, int j0) {
  constexpr int BLK = PTA_CLNL_BLK;
  __shared__ double Ls[BLK * (BLK + 1) / 2];  // packed rows of the diagonal block: Ls[i (i + 1) / 2 + k] = L[j0 + i, j0 + k], k <= i
  __shared__ double ys[BLK * PTA_CLNL_RT];    // ys[i * RT + t]: row j0 + i of thread t's column, right-hand side then solution
  const int g = blockIdx.y, t = threadIdx.x;
  const double *Lg = L + (int64_t)g * n * n;
  double *Vg = V + (int64_t)g * n * ld_v;
  const int rows = min(BLK, n - j0);
  for (int e = t; e < BLK * BLK; e += PTA_CLNL_RT) {  // rows past n: identity rows, whose right-hand sides are zero
    const int i = e / BLK, k = e - i * BLK;
    if (k <= i) Ls[i * (i + 1) / 2 + k] = i < rows ? Lg[(int64_t)(j0 + i) * n + j0 + k] : (i == k ? 1.0 : 0.0);
  }
  // one column per thread, kept in its own LDS slots (no other thread reads them)
  const int r = blockIdx.x * PTA_CLNL_RT + t;
  const int64_t rc = min(r, R - 1);
  double *yc = ys + t;
  for (int i = 0; i < BLK; ++i) yc[i * PTA_CLNL_RT] = i < rows ? Vg[(int64_t)(j0 + i) * ld_v + rc] : 0.0;
  __syncthreads();
  // four rows at a time: four independent chains over k < i0 share one read of y_k, then the 4 x 4 triangle in sequence.  Every row's
  // sum still runs over k in ascending order, and the squares are added in ascending row order
  double ss = 0.0;
  for (int i0 = 0; i0 < rows; i0 += 4) {
    const double *L0 = Ls + i0 * (i0 + 1) / 2, *L1 = L0 + i0 + 1, *L2 = L1 + i0 + 2, *L3 = L2 + i0 + 3;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll 4
    for (int k = 0; k < i0; ++k) {
      const double yk = yc[k * PTA_CLNL_RT];
      s0 = fma(L0[k], yk, s0);
      s1 = fma(L1[k], yk, s1);
      s2 = fma(L2[k], yk, s2);
      s3 = fma(L3[k], yk, s3);
    }
    const double y0 = (yc[i0 * PTA_CLNL_RT] - s0) / L0[i0];
    s1 = fma(L1[i0], y0, s1);
    const double y1 = (yc[(i0 + 1) * PTA_CLNL_RT] - s1) / L1[i0 + 1];
    s2 = fma(L2[i0], y0, s2);
    s2 = fma(L2[i0 + 1], y1, s2);
    const double y2 = (yc[(i0 + 2) * PTA_CLNL_RT] - s2) / L2[i0 + 2];
    s3 = fma(L3[i0], y0, s3);
    s3 = fma(L3[i0 + 1], y1, s3);
    s3 = fma(L3[i0 + 2], y2, s3);
    const double y3 = (yc[(i0 + 3) * PTA_CLNL_RT] - s3) / L3[i0 + 3];
    const double yv[4] = {y0, y1, y2, y3};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      yc[(i0 + e) * PTA_CLNL_RT] = yv[e];
      ss = fma(yv[e], yv[e], ss);
      if (r < R && i0 + e < rows) Vg[(int64_t)(j0 + i0 + e) * ld_v + r] = yv[e];
    }
  }
  if (r < R) {
    double *q = quad + (int64_t)g * ld_quad + r;
    *q = j0 == 0 ? ss : *q + ss;
  }
}

__global__ __launch_bounds__(256) void k_clnl_finish(const double *__restrict__ L, int n, const double *__restrict__ quad, int64_t ld_quad,
                                                     int R, double *__restrict__ out, int64_t ld_g) {
  __shared__ double part[4];
  const int g = blockIdx.x, t = threadIdx.x;
  const double *Lg = L + (int64_t)g * n * n;
  double v = 0.0;
  for (int i = t; i < n; i += 256) v += log(Lg[(int64_t)i * n + i]);  // thread t: rows t, t + 256, ... ascending
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((t & 63) == 0) part[t >> 6] = v;
  __syncthreads();
  const double hl = (part[0] + part[1]) + (part[2] + part[3]);
  for (int r = t; r < R; r += 256) out[(int64_t)g * ld_g + r] = pta_clnl_value(quad[(int64_t)g * ld_quad + r], hl);
}

extern "C" int pta_clnl_mix(const double *Y, int64_t ld_y, int P, int C, int R, const double *Bt, int rho, double *Yp, int64_t ld_yp,
                            void *stream) {
  PTA_REQUIRE(Y && Bt && Yp, PTA_E_ARG, "pta_clnl_mix: NULL argument");
  PTA_REQUIRE(P >= 1 && C >= 1 && C <= PTA_CLNL_CMAX && (int64_t)P * C <= 8192 && rho >= 1 && rho <= P && R >= 1, PTA_E_ARG,
              "pta_clnl_mix: P=%d C=%d (1..%d, P C <= 8192) rho=%d (1..P) R=%d", P, C, PTA_CLNL_CMAX, rho, R);
  PTA_REQUIRE(ld_y >= (int64_t)P * C && ld_yp >= (int64_t)rho * C, PTA_E_ARG, "pta_clnl_mix: ld_y=%lld (>= P C) ld_yp=%lld (>= rho C)",
              (long long)ld_y, (long long)ld_yp);
  hipLaunchKernelGGL(k_clnl_mix, dim3((unsigned)R), dim3(256), sizeof(double) * (size_t)P * C, pta_stream(stream), Y, ld_y, P, C, Bt, rho, Yp, ld_yp);
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}

// the checks the grid-point entries share: n = rho C rows, G grid points in one launch
#define PTA_CLNL_REQUIRE_SHAPE(who)                                                                                                         \
  PTA_REQUIRE(rho >= 1 && C >= 1 && C <= PTA_CLNL_CMAX && (int64_t)rho * C <= 65535 && G >= 1 && G <= 65535, PTA_E_ARG,                      \
              who ": rho=%d C=%d (1..%d, rho C <= 65535) G=%d (1..65535)", rho, C, PTA_CLNL_CMAX, G)

extern "C" int pta_clnl_assemble(const double *T, int rho, int C, double gamma_ref, double Tspan, const double *log10_A, const double *gamma,
                                 int G, double *M, void *stream) {
  PTA_REQUIRE(T && log10_A && gamma && M, PTA_E_ARG, "pta_clnl_assemble: NULL argument");
  PTA_CLNL_REQUIRE_SHAPE("pta_clnl_assemble");
  PTA_REQUIRE(Tspan > 0.0 && isfinite(Tspan) && isfinite(gamma_ref), PTA_E_ARG, "pta_clnl_assemble: Tspan=%g gamma_ref=%g", Tspan, gamma_ref);
  const int n = rho * C;
  hipLaunchKernelGGL(k_clnl_assemble, dim3(pta_cdiv(n, 4), (unsigned)G), dim3(256), 0, pta_stream(stream), T, n, C, gamma_ref, Tspan, log10_A, gamma, M);
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}

extern "C" int pta_clnl_rhs(const double *Yp, int64_t ld_yp, int rho, int C, int R, double gamma_ref, double Tspan, const double *log10_A,
                            const double *gamma, int G, double *V, int64_t ld_v, void *stream) {
  PTA_REQUIRE(Yp && log10_A && gamma && V, PTA_E_ARG, "pta_clnl_rhs: NULL argument");
  PTA_CLNL_REQUIRE_SHAPE("pta_clnl_rhs");
  PTA_REQUIRE(Tspan > 0.0 && isfinite(Tspan) && isfinite(gamma_ref), PTA_E_ARG, "pta_clnl_rhs: Tspan=%g gamma_ref=%g", Tspan, gamma_ref);
  const int n = rho * C;
  PTA_REQUIRE(R >= 1 && R <= 65535 * 32 && ld_yp >= n && ld_v >= R, PTA_E_ARG, "pta_clnl_rhs: R=%d ld_yp=%lld (>= rho C) ld_v=%lld (>= R)", R,
              (long long)ld_yp, (long long)ld_v);
  hipLaunchKernelGGL(k_clnl_rhs, dim3(pta_cdiv(n, 32), pta_cdiv(R, 32)), dim3(256), 0, pta_stream(stream), Yp, ld_yp, n, C, R, gamma_ref, Tspan,
                     log10_A, gamma, G, V, ld_v);
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}

extern "C" int pta_clnl_solve(const double *L, int n, int G, double *V, int64_t ld_v, int R, double *quad, int64_t ld_quad, void *stream) {
  PTA_REQUIRE(L && V && quad, PTA_E_ARG, "pta_clnl_solve: NULL argument");
  PTA_REQUIRE(n >= 1 && n <= 65535 && G >= 1 && G <= 65535 && R >= 1, PTA_E_ARG, "pta_clnl_solve: n=%d (1..65535) G=%d (1..65535) R=%d", n, G, R);
  PTA_REQUIRE(ld_v >= R && ld_quad >= R, PTA_E_ARG, "pta_clnl_solve: ld_v=%lld ld_quad=%lld (>= R)", (long long)ld_v, (long long)ld_quad);
  hipStream_t s = pta_stream(stream);
  for (int j0 = 0; j0 < n; j0 += PTA_CLNL_BLK) {
    if (j0) {  // V_j -= L[j, < j] V[< j]: at most 64 rows, so pta_dgemm's 64 x 64-tile kernel whatever R - one chain of MFMAs over k per element
      const int rc = pta_dgemm_launch(0, n - j0 < PTA_CLNL_BLK ? n - j0 : PTA_CLNL_BLK, R, j0, -1.0, L + (int64_t)j0 * n, n, 1, V, ld_v, 1.0,
                                      V + (int64_t)j0 * ld_v, ld_v, 0, G, (int64_t)n * n, (int64_t)n * ld_v, (int64_t)n * ld_v, 1, s);
      if (rc != PTA_OK) return rc;
    }
    hipLaunchKernelGGL(k_clnl_solve_diag, dim3(pta_cdiv(R, PTA_CLNL_RT), (unsigned)G), dim3(PTA_CLNL_RT), 0, s, L, n, V, ld_v, R, quad, ld_quad, j0);
    PTA_LAUNCH_CHECK();
  }
  return PTA_OK;
}

extern "C" int pta_clnl_finish(const double *L, int n, int G, const double *quad, int64_t ld_quad, int R, double *lnl_ratio, int64_t ld_g,
                               void *stream) {
  PTA_REQUIRE(L && quad && lnl_ratio, PTA_E_ARG, "pta_clnl_finish: NULL argument");
  PTA_REQUIRE(n >= 1 && n <= 65535 && G >= 1 && R >= 1, PTA_E_ARG, "pta_clnl_finish: n=%d (1..65535) G=%d R=%d", n, G, R);
  PTA_REQUIRE(ld_quad >= R && ld_g >= R, PTA_E_ARG, "pta_clnl_finish: ld_quad=%lld ld_g=%lld (>= R)", (long long)ld_quad, (long long)ld_g);
  hipLaunchKernelGGL(k_clnl_finish, dim3((unsigned)G), dim3(256), 0, pta_stream(stream), L, n, quad, ld_quad, R, lnl_ratio, ld_g);
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}
