// Per-frequency optimal statistic (pta_replicator_amd/optimal_statistic.py holds the derivation): per realisation and ORF o the
// cross-correlated power of every Fourier bin, a2_o = F_o^-1 b_o, instead of one broadband amplitude.  With X_a [C] the weighted
// projection of pulsar a, Z_a [C, C] its weighted Gram matrix (C = 2 n_f, column 2 k / 2 k + 1 = sin / cos of bin k) and G_o,p the
// ORF value of pair p = (a < b):
//
//     n_p[k]    = X_a[2k] X_b[2k] + X_a[2k+1] X_b[2k+1]
//     D_p[k, j] = sum_{i in {2k, 2k+1}} sum_{l in {2j, 2j+1}} Z_a[i, l] Z_b[i, l]
//     b_o = sum_p G_o,p n_p,     F_o = sum_p G_o,p^2 D_p,     a2_o = F_o^-1 b_o,     sigma_o[k] = sqrt((F_o^-1)_kk)
//
// ("full"), or a2_o[k] = b_o[k] / F_o[k, k], sigma_o[k] = F_o[k, k]^-1/2 ("narrowband").
//
//   pta_os_pairs_pf          fixed noise: F_o does not depend on the realisation, the host hands in F_o^-1 (or 1 / diag F_o); the
//                            kernel forms b_o and applies it.  One workgroup per realisation, Y_r in LDS as in k_os_pairs; lane
//                            (k, s) walks the pairs s, s + NS, ... in ascending order with n_orf accumulators.
//   pta_os_matched_pairs_pf  per-realisation noise: X, packed Z of pta_os_matched_solve.  One workgroup per realisation; a thread
//                            owns blocks (k, j <= k) of F (four products of packed entries each, pta_os_spectrum.h) and walks its
//                            group's pairs g, g + NG, ... in ascending order - no cross-lane reduction per pair.  The groups are
//                            joined through LDS in ascending g, then each ORF is solved by one wave in LDS: Jacobi scaling
//                            d^-1/2 F d^-1/2, Cholesky, M = L^-1, a2 = d^-1/2 M^T M d^-1/2 b, sigma_k = d_k^-1/2 |M[:, k]|.
//
// Bit-identity: a workgroup sees one realisation; every sum runs in an order fixed by (n_f, n_orf, n_pairs) alone.  No atomics, no
// split of a realisation across workgroups: a result does not depend on R, the chunk or the row slot.
#include "pta_common.h"
#include "pta_os_spectrum.h"

#define PTA_OSP_CMAX 64   // C = 2 n_f
#define PTA_OSP_NORF 8
#define PTA_OSP_BPT 3     // blocks per thread when n_f (n_f + 1) / 2 > 256 (at most 528 blocks)

__global__ __launch_bounds__(256) void k_osp_pairs(const double *__restrict__ Y, int64_t ld_y, int PC, int C, const int32_t *__restrict__ pa,
                                                   const int32_t *__restrict__ pb, int np, const double *__restrict__ G, int n_orf,
                                                   const double *__restrict__ op, int full, double *__restrict__ a2, int64_t ld_a2) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int nf = C / 2, NS = 256 / nf;     // NS pair slices of n_f lanes
  const int nA = max(PC, n_orf * NS * nf);
  double *ys = lds;                        // Y of this realisation [P * C]; afterwards the slices' partial sums [n_orf][NS][n_f]
  double *bs = lds + ((nA + 1) & ~1);      // b [n_orf][n_f]
  const int64_t r = blockIdx.x;
  const int t = threadIdx.x;
  for (int i = t; i < PC; i += 256) ys[i] = Y[r * ld_y + i];
  __syncthreads();
  const int k = t % nf, s = t / nf;
  double acc[PTA_OSP_NORF];
#pragma unroll
  for (int o = 0; o < PTA_OSP_NORF; ++o) acc[o] = 0.0;
  if (s < NS) {
    for (int p = s; p < np; p += NS) {     // fixed pair -> lane assignment, ascending
      const double *ya = ys + pa[p] * C + 2 * k, *yb = ys + pb[p] * C + 2 * k;
      const double n = fma(ya[1], yb[1], ya[0] * yb[0]);
#pragma unroll
      for (int o = 0; o < PTA_OSP_NORF; ++o)
        if (o < n_orf) acc[o] = fma(G[(int64_t)o * np + p], n, acc[o]);
    }
  }
  __syncthreads();                         // every lane is done with Y
  if (s < NS) {
#pragma unroll
    for (int o = 0; o < PTA_OSP_NORF; ++o)
      if (o < n_orf) ys[(o * NS + s) * nf + k] = acc[o];
  }
  __syncthreads();
  const int o = t / nf;
  if (o < n_orf) {
    double v = 0.0;
    for (int q = 0; q < NS; ++q) v += ys[(o * NS + q) * nf + k];
    bs[t] = v;
  }
  __syncthreads();
  if (o < n_orf) {
    double v;
    if (full) {
      const double *row = op + (int64_t)t * nf;   // row k of F_o^-1
      v = 0.0;
      for (int j = 0; j < nf; ++j) v = fma(row[j], bs[o * nf + j], v);
    } else {
      v = bs[t] * op[t];
    }
    a2[r * ld_a2 + t] = v;
  }
}

template <int BPT>
__global__ __launch_bounds__(256) void k_osp_matched(const double *__restrict__ X, const double *__restrict__ Z, int P, int C,
                                                     const int32_t *__restrict__ pa, const int32_t *__restrict__ pb, int np,
                                                     const double *__restrict__ G, const double *__restrict__ G2, int n_orf, int full,
                                                     double *__restrict__ a2, int64_t ld_a2, double *__restrict__ sigma, int64_t ld_sigma,
                                                     double *__restrict__ fisher, int64_t ld_f) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int nf = C / 2, nb = pta_osp_nblocks(nf), nz = C * (C + 1) / 2;
  const int NG = BPT > 1 ? 1 : 256 / nb;   // pair groups of nb threads (one group of 256 threads with up to BPT blocks each)
  const int W = nb + nf;                   // a group's partial sums per ORF: the blocks of F, then b
  double *part = lds;                      // [NG][n_orf][W]; after the join M = L^-1 [n_orf][nb]
  double *Fp = part + NG * n_orf * W;      // [n_orf][nb] packed F, scaled and factored in place
  double *bv = Fp + n_orf * nb;            // [n_orf][n_f] b
  double *dinv = bv + n_orf * nf;          // [n_orf][n_f] diag(F)^-1/2
  double *yv = dinv + n_orf * nf;          // [n_orf][n_f] M d^-1/2 b
  const int64_t r = blockIdx.x;
  const int t = threadIdx.x, l = t & 63, w = t >> 6;
  const double *Xr = X + r * P * C, *Zr = Z + r * P * nz;
  const int g = BPT > 1 ? 0 : t / nb;
  const bool offdiag = full || fisher;     // narrowband without F written out needs the diagonal blocks alone
  int e[BPT], bk[BPT], idx[BPT][4];
  bool own[BPT], diag[BPT];
#pragma unroll
  for (int u = 0; u < BPT; ++u) {
    e[u] = BPT > 1 ? t + 256 * u : t % nb;
    own[u] = g < NG && e[u] < nb;
    int k = 0, j = 0;
    if (own[u]) pta_osp_block_kj(e[u], k, j);
    own[u] = own[u] && (k == j || offdiag);
    pta_osp_block_entries(k, j, idx[u]);
    bk[u] = k;
    diag[u] = own[u] && k == j;
  }
  double acc[BPT][PTA_OSP_NORF], accb[BPT][PTA_OSP_NORF];
#pragma unroll
  for (int u = 0; u < BPT; ++u)
#pragma unroll
    for (int o = 0; o < PTA_OSP_NORF; ++o) acc[u][o] = accb[u][o] = 0.0;
  if (g < NG) {
    int a_cur = -1;
    double za[BPT][4], xa[BPT][2];
#pragma unroll
    for (int u = 0; u < BPT; ++u) {
      za[u][0] = za[u][1] = za[u][2] = za[u][3] = 0.0;
      xa[u][0] = xa[u][1] = 0.0;
    }
    for (int p = g; p < np; p += NG) {     // fixed pair -> group assignment, ascending within the group
      const int a = pa[p], b = pb[p];
      const double *zb = Zr + (int64_t)b * nz, *xb = Xr + (int64_t)b * C;
      if (a != a_cur) {                    // pairs come sorted by a: its entries stay in registers
        const double *zap = Zr + (int64_t)a * nz, *xap = Xr + (int64_t)a * C;
#pragma unroll
        for (int u = 0; u < BPT; ++u) {
          if (own[u]) {
#pragma unroll
            for (int q = 0; q < 4; ++q) za[u][q] = zap[idx[u][q]];
          }
          if (diag[u]) {
            xa[u][0] = xap[2 * bk[u]];
            xa[u][1] = xap[2 * bk[u] + 1];
          }
        }
        a_cur = a;
      }
#pragma unroll
      for (int u = 0; u < BPT; ++u) {
        if (own[u]) {
          double d = za[u][0] * zb[idx[u][0]];
          d = fma(za[u][1], zb[idx[u][1]], d);
          d = fma(za[u][2], zb[idx[u][2]], d);
          d = fma(za[u][3], zb[idx[u][3]], d);
#pragma unroll
          for (int o = 0; o < PTA_OSP_NORF; ++o)
            if (o < n_orf) acc[u][o] = fma(G2[(int64_t)o * np + p], d, acc[u][o]);
        }
        if (diag[u]) {
          const double n = fma(xa[u][1], xb[2 * bk[u] + 1], xa[u][0] * xb[2 * bk[u]]);
#pragma unroll
          for (int o = 0; o < PTA_OSP_NORF; ++o)
            if (o < n_orf) accb[u][o] = fma(G[(int64_t)o * np + p], n, accb[u][o]);
        }
      }
    }
  }
#pragma unroll
  for (int u = 0; u < BPT; ++u)
#pragma unroll
    for (int o = 0; o < PTA_OSP_NORF; ++o) {
      if (o < n_orf && own[u]) part[(g * n_orf + o) * W + e[u]] = acc[u][o];
      if (o < n_orf && diag[u]) part[(g * n_orf + o) * W + nb + bk[u]] = accb[u][o];
    }
  __syncthreads();
  for (int i = t; i < n_orf * W; i += 256) {   // join the groups in ascending g
    const int o = i / W, c = i - o * W;
    double v = 0.0;
    if (c >= nb || offdiag || pta_osp_is_diagonal(c))   // blocks nobody accumulated are never read
      for (int q = 0; q < NG; ++q) v += part[(q * n_orf + o) * W + c];
    if (c < nb)
      Fp[o * nb + c] = v;
    else
      bv[o * nf + c - nb] = v;
  }
  __syncthreads();
  if (fisher) {
    for (int i = t; i < n_orf * nf * nf; i += 256) {
      const int o = i / (nf * nf), kj = i - o * nf * nf, k = kj / nf, j = kj - k * nf;
      fisher[r * ld_f + i] = Fp[o * nb + pta_osp_block(max(k, j), min(k, j))];
    }
  }
  const int ok = t / nf, kk = t - ok * nf;     // (ORF, bin) of thread t < n_orf n_f <= 256
  if (!full) {
    if (ok < n_orf) {
      bool bad = false;
      for (int q = 0; q < nf; ++q) bad |= !(Fp[ok * nb + pta_osp_block(q, q)] > 0.0);
      const double d = Fp[ok * nb + pta_osp_block(kk, kk)];
      a2[r * ld_a2 + t] = bad ? NAN : bv[t] / d;
      sigma[r * ld_sigma + t] = bad ? NAN : 1.0 / sqrt(d);
    }
    return;
  }
  if (ok < n_orf) dinv[t] = 1.0 / sqrt(Fp[ok * nb + pta_osp_block(kk, kk)]);
  __syncthreads();
  for (int i = t; i < n_orf * nb; i += 256) {  // Jacobi scaling: unit diagonal
    const int o = i / nb;
    int k, j;
    pta_osp_block_kj(i - o * nb, k, j);
    Fp[i] = dinv[o * nf + k] * Fp[i] * dinv[o * nf + j];
  }
  __syncthreads();
  double *M = part;
  for (int ob = 0; ob < n_orf; ob += 4) {      // one wave per ORF, lane = row; every wave keeps the barriers
    const int o = ob + w;
    const bool act = o < n_orf && l < nf;
    double *A = Fp + (act ? o : 0) * nb, *Mo = M + (act ? o : 0) * nb;
    bool bad = false;
    for (int j = 0; j < nf; ++j) {             // left-looking Cholesky, column j
      double s = 0.0;
      if (act && l >= j) {
        s = A[pta_osp_block(l, j)];
        for (int k = 0; k < j; ++k) s = fma(-A[pta_osp_block(l, k)], A[pta_osp_block(j, k)], s);
      }
      const double p = __shfl(s, j, 64);       // the pivot
      bad |= !(p > 0.0);                       // also NaN; nothing below indexes by a value, so a bad pivot only spreads NaN
      const double rp = sqrt(p);
      if (act && l >= j) A[pta_osp_block(l, j)] = (l == j) ? rp : s / rp;
      __syncthreads();
    }
    if (act) {                                 // column l of M = L^-1 by forward substitution; a lane re-reads only its own writes
      for (int i = l; i < nf; ++i) {
        double s = (i == l) ? 1.0 : 0.0;
        for (int k = l; k < i; ++k) s = fma(-A[pta_osp_block(i, k)], Mo[pta_osp_block(k, l)], s);
        Mo[pta_osp_block(i, l)] = s / A[pta_osp_block(i, i)];
      }
    }
    __syncthreads();
    if (act) {
      double y = 0.0;
      for (int k = 0; k <= l; ++k) y = fma(Mo[pta_osp_block(l, k)], dinv[o * nf + k] * bv[o * nf + k], y);
      yv[o * nf + l] = y;
    }
    __syncthreads();
    if (act) {
      double v = 0.0, q = 0.0;
      for (int i = l; i < nf; ++i) {
        const double m = Mo[pta_osp_block(i, l)];
        v = fma(m, yv[o * nf + i], v);
        q = fma(m, m, q);
      }
      a2[r * ld_a2 + o * nf + l] = bad ? NAN : dinv[o * nf + l] * v;
      sigma[r * ld_sigma + o * nf + l] = bad ? NAN : dinv[o * nf + l] * sqrt(q);
    }
  }
}

extern "C" int pta_os_pairs_pf(const double *Y, int64_t ld_y, int P, int C, int R, const int32_t *pair_a, const int32_t *pair_b, int n_pairs,
                               const double *G, int n_orf, const double *op, int mode, double *a2, int64_t ld_a2, void *stream) {
  PTA_REQUIRE(Y && pair_a && pair_b && G && op && a2, PTA_E_ARG, "pta_os_pairs_pf: NULL argument");
  PTA_REQUIRE(P >= 2 && C >= 2 && (C % 2) == 0 && C <= PTA_OSP_CMAX && R > 0 && n_pairs >= 1 && n_orf >= 1 && n_orf <= PTA_OSP_NORF, PTA_E_ARG,
              "pta_os_pairs_pf: P=%d C=%d (even, 2..%d) R=%d n_pairs=%d n_orf=%d (1..%d)", P, C, PTA_OSP_CMAX, R, n_pairs, n_orf, PTA_OSP_NORF);
  PTA_REQUIRE(mode == 0 || mode == 1, PTA_E_ARG, "pta_os_pairs_pf: mode=%d (0 full, 1 narrowband)", mode);
  PTA_REQUIRE((int64_t)P * C * 8 <= 65536, PTA_E_ARG, "pta_os_pairs_pf: P*C=%d doubles exceed the 64 KiB of Y in one workgroup's LDS", P * C);
  const int nf = C / 2;
  PTA_REQUIRE(ld_y >= (int64_t)P * C && ld_a2 >= (int64_t)n_orf * nf, PTA_E_ARG, "pta_os_pairs_pf: leading dimension too small");
  const int nA = P * C > n_orf * (256 / nf) * nf ? P * C : n_orf * (256 / nf) * nf;
  const size_t shmem = ((size_t)((nA + 1) & ~1) + (size_t)n_orf * nf) * sizeof(double);
  if (shmem > 65536) PTA_HIP(hipFuncSetAttribute((const void *)k_osp_pairs, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
  hipLaunchKernelGGL(k_osp_pairs, dim3(R), dim3(256), shmem, pta_stream(stream), Y, ld_y, P * C, C, pair_a, pair_b, n_pairs, G, n_orf, op,
                     mode == 0, a2, ld_a2);
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}

extern "C" int pta_os_matched_pairs_pf(const double *X, const double *Z, int P, int C, int R, const int32_t *pair_a, const int32_t *pair_b,
                                       int n_pairs, const double *G, const double *G2, int n_orf, int mode, double *a2, int64_t ld_a2,
                                       double *sigma, int64_t ld_sigma, double *fisher, int64_t ld_fisher, void *stream) {
  PTA_REQUIRE(X && Z && pair_a && pair_b && G && G2 && a2 && sigma, PTA_E_ARG, "pta_os_matched_pairs_pf: NULL argument");
  PTA_REQUIRE(P >= 2 && C >= 2 && (C % 2) == 0 && C <= PTA_OSP_CMAX && R > 0 && n_pairs >= 1 && n_orf >= 1 && n_orf <= PTA_OSP_NORF, PTA_E_ARG,
              "pta_os_matched_pairs_pf: P=%d C=%d (even, 2..%d) R=%d n_pairs=%d n_orf=%d (1..%d)", P, C, PTA_OSP_CMAX, R, n_pairs, n_orf,
              PTA_OSP_NORF);
  PTA_REQUIRE(mode == 0 || mode == 1, PTA_E_ARG, "pta_os_matched_pairs_pf: mode=%d (0 full, 1 narrowband)", mode);
  const int nf = C / 2, nb = nf * (nf + 1) / 2;
  PTA_REQUIRE(ld_a2 >= (int64_t)n_orf * nf && ld_sigma >= (int64_t)n_orf * nf && (!fisher || ld_fisher >= (int64_t)n_orf * nf * nf), PTA_E_ARG,
              "pta_os_matched_pairs_pf: leading dimension too small");
  const int ng = nb > 256 ? 1 : 256 / nb;
  const size_t shmem = ((size_t)ng * n_orf * (nb + nf) + (size_t)n_orf * nb + 3 * (size_t)n_orf * nf) * sizeof(double);
  hipStream_t s = pta_stream(stream);
  if (nb > 256) {
    if (shmem > 65536)
      PTA_HIP(hipFuncSetAttribute((const void *)k_osp_matched<PTA_OSP_BPT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
    hipLaunchKernelGGL(k_osp_matched<PTA_OSP_BPT>, dim3(R), dim3(256), shmem, s, X, Z, P, C, pair_a, pair_b, n_pairs, G, G2, n_orf, mode == 0, a2,
                       ld_a2, sigma, ld_sigma, fisher, ld_fisher);
  } else {
    if (shmem > 65536) PTA_HIP(hipFuncSetAttribute((const void *)k_osp_matched<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
    hipLaunchKernelGGL(k_osp_matched<1>, dim3(R), dim3(256), shmem, s, X, Z, P, C, pair_a, pair_b, n_pairs, G, G2, n_orf, mode == 0, a2, ld_a2,
                       sigma, ld_sigma, fisher, ld_fisher);
  }
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}
