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
// pta_fstat_fe: the product over pulsars (K = P) of Q against phi.  One wave owns 8 frequencies x 16 sky points: the 16 rows of its
// A tile are (frequency, sin / cos) ordered so that accumulator registers (0, 1) and (2, 3) of a lane are the sin / cos sums of
// frequencies g and g + 4 (g = lane >> 4); two MFMA chains, one against F+ and one against Fx of the same 16 sky points, leave the
// whole 4-vector N_rjs of two (j, s) in one lane.  phi of the wave's sky points (2 KS doubles, KS = ceil(P / 4))
// and the 10 unique entries of M_js^-1 of its two (j, s) stay in registers for the whole launch; the workgroup (4 waves = 64 sky
// points) walks its realisations, staging Q[r, :, 16 columns] once per realisation in LDS (double-buffered, one barrier per
// realisation).  N never leaves the registers.  Pulsars are summed in ascending groups of four by the MFMA, the quadratic form is
// one fixed fma chain, the maximum over a tile is an ascending scan of its 16 sky points (strictly greater wins: the lower index on ties), and
// the tiles are folded in ascending order: an (r, j, s) value is the same in either mode and in any chunk.
#include "pta_common.h"
#include "pta_mfma.h"

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

#define FS_RB 8  // realisations per scan of the sky_max reduction: 8 x 8 frequencies = one (realisation, frequency) per lane
#define FS_ST PTA_FSTAT_SKY_TILE  // sky points per workgroup of k_fstat_fe: four waves x 16
static_assert(FS_ST == 64, "k_fstat_fe: a workgroup is four waves of 16 sky points");

template <int KS, bool MAXMODE>
__global__ __launch_bounds__(256) void k_fstat_fe(const double *__restrict__ Q, int64_t ld_q, int P, int J, int R, int rchunk,
                                                  const double *__restrict__ phi, int S, const double *__restrict__ Minv,
                                                  double *__restrict__ fe, int64_t ld_fe, double *__restrict__ pval,
                                                  int32_t *__restrict__ parg, int ntile) {
  __shared__ double Al[2][4 * KS * 16];  // Q[r, a, 2 j0 .. 2 j0 + 15] of one realisation, a < 4 KS (zeros past P)
  __shared__ double Mx[MAXMODE ? 4 * FS_RB * 8 * FS_LD : 1];  // sky_max: Fe of FS_RB realisations x 8 frequencies x 16 sky points per wave
  constexpr int NL = (4 * KS * 16 + 255) / 256;
  const int t = threadIdx.x, l = t & 63, w = t >> 6, g = l >> 4, m = l & 15;
  const int j0 = blockIdx.y * 8, st = blockIdx.x;
  const int s = st * FS_ST + w * 16 + m;  // this lane's sky point
  const int ja = j0 + g, jb = j0 + g + 4;   // and its two frequencies
  const int r_lo = blockIdx.z * rchunk, r_hi = min(R, r_lo + rchunk);
  // B operand: lane l of step k supplies phi[a = 4 k + (l >> 4)][s][+ / x]
  double bplus[KS], bcross[KS];
#pragma unroll
  for (int k = 0; k < KS; ++k) {
    const int a = 4 * k + g;
    const bool ok = a < P && s < S;
    bplus[k] = ok ? phi[((int64_t)a * S + s) * 2] : 0.0;
    bcross[k] = ok ? phi[((int64_t)a * S + s) * 2 + 1] : 0.0;
  }
  double ma[10], mb[10];
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    ma[i] = (ja < J && s < S) ? Minv[((int64_t)ja * S + s) * 10 + i] : 0.0;
    mb[i] = (jb < J && s < S) ? Minv[((int64_t)jb * S + s) * 10 + i] : 0.0;
  }
  // A operand: row rho = l & 15 of the tile is frequency (rho & 3) + 4 (rho >> 3), sin / cos (rho >> 2) & 1
  const int acol = 2 * ((m & 3) + 4 * (m >> 3)) + ((m >> 2) & 1);
  double qv[NL];
  auto fetch = [&](int r) {
#pragma unroll
    for (int u = 0; u < NL; ++u) {
      const int idx = t + 256 * u, a = idx >> 4, c = 2 * j0 + (idx & 15);
      qv[u] = (idx < 4 * KS * 16 && a < P && c < 2 * J) ? Q[(int64_t)r * ld_q + (int64_t)a * 2 * J + c] : 0.0;
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int u = 0; u < NL; ++u) {
      const int idx = t + 256 * u;
      if (idx < 4 * KS * 16) Al[buf][idx] = qv[u];
    }
  };
  if (r_lo < r_hi) fetch(r_lo);
  for (int r = r_lo; r < r_hi; ++r) {
    const int cur = (r - r_lo) & 1;
    stash(cur);
    __syncthreads();  // the buffer written two realisations ago was last read before the previous barrier
    if (r + 1 < r_hi) fetch(r + 1);
    pta_f64x4 np_ = pta_f64x4{0.0, 0.0, 0.0, 0.0}, nc_ = pta_f64x4{0.0, 0.0, 0.0, 0.0};
    const double *Ab = Al[cur] + g * 16 + acol;
#pragma unroll
    for (int k = 0; k < KS; ++k) {
      const double av = Ab[k * 64];
      np_ = pta_mfma_f64(av, bplus[k], np_);
      nc_ = pta_mfma_f64(av, bcross[k], nc_);
    }
    // accumulator e of lane l: tile row (l >> 4) + 4 e = frequency g + 4 (e >> 1), sin / cos e & 1; column = sky point l & 15
    const double fa = pta_fstat_quad(ma, np_[0], np_[1], nc_[0], nc_[1]);
    const double fb = pta_fstat_quad(mb, np_[2], np_[3], nc_[2], nc_[3]);
    if (!MAXMODE) {
      if (s < S) {
        if (ja < J) fe[(int64_t)r * ld_fe + (int64_t)ja * S + s] = fa;
        if (jb < J) fe[(int64_t)r * ld_fe + (int64_t)jb * S + s] = fb;
      }
    } else {
      // maximum over the 16 sky points of the wave, FS_RB realisations at a time through the wave's own LDS block [realisation]
      // [frequency][sky point]: a lane then scans the 16 sky points of one (realisation, frequency) in ascending order, strictly
      // greater winning (the lower index on ties), and eight lanes write eight consecutive frequencies.  Sky points past S never win.
      const int q = (r - r_lo) % FS_RB;
      double *mw = Mx + w * (FS_RB * 8 * FS_LD);
      mw[(q * 8 + g) * FS_LD + m] = s < S ? fa : -INFINITY;
      mw[(q * 8 + g + 4) * FS_LD + m] = s < S ? fb : -INFINITY;
      if (q == FS_RB - 1 || r + 1 == r_hi) {  // uniform over the workgroup
        __syncthreads();
        const int qq = l >> 3, jj = j0 + (l & 7);
        if (qq <= q && jj < J) {
          const double *v = mw + l * FS_LD;
          double best = v[0];
          int bk = 0;
#pragma unroll
          for (int k = 1; k < 16; ++k)
            if (v[k] > best) best = v[k], bk = k;
          const int64_t slot = ((int64_t)(r - q + qq) * ntile + st * 4 + w) * J;  // [r][16-point sub-tile, ascending in s][j]
          pval[slot + jj] = best;
          parg[slot + jj] = st * FS_ST + w * 16 + bk;
        }
      }
    }
  }
}

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

// internal launcher of the fold over the sub-tile maxima (declared in pta_common.h): shared with pta_bwm_stat, whose per-tile layout is the same
int pta_fstat_reduce_launch(const double *part_val, const int32_t *part_arg, int64_t n, int ntile, int J, double *vmax, int64_t ld_max,
                            int32_t *varg, int64_t ld_arg, hipStream_t stream) {
  hipLaunchKernelGGL(k_fstat_fe_reduce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, part_val, part_arg, n, ntile, J, vmax, ld_max, varg,
                     ld_arg);
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}

extern "C" int pta_fstat_project(const double *Wt, int64_t ldw, int C, const int32_t *psr_off, int P, const double *rows, int64_t ld_rows, int R,
                                 double *Q, int64_t ld_q, void *stream) {
  PTA_REQUIRE(Wt && psr_off && rows && Q, PTA_E_ARG, "pta_fstat_project: NULL argument");
  PTA_REQUIRE(C >= 2 && C % 2 == 0 && C <= PTA_FSTAT_CMAX && P > 0 && P <= 65535 && R > 0, PTA_E_ARG,
              "pta_fstat_project: C=%d (even, 2..%d) P=%d (1..65535) R=%d", C, PTA_FSTAT_CMAX, P, R);
  PTA_REQUIRE(ld_q >= (int64_t)P * C && ldw >= 1 && ld_rows >= 1, PTA_E_ARG, "pta_fstat_project: ld_q=%lld < P*C=%lld or ldw / ld_rows < 1",
              (long long)ld_q, (long long)P * C);
  PTA_REQUIRE(pta_cdiv(R, 64) <= 65535u, PTA_E_ARG, "pta_fstat_project: R=%d exceeds one launch (64 * 65535 realisations)", R);
  hipStream_t s = pta_stream(stream);
  dim3 block(256);
  // The tile follows the launch's size alone - a realisation's Q does not depend on it (every output is its own MFMA chain over
  // ascending slabs).  128 x 128 while that leaves FS_FILL workgroups; else 64 rows, then 64 columns: a workgroup walks its whole
  // pulsar, so with few workgroups the longest pulsar of a ragged array sets the launch's time, and a smaller tile shortens that walk.
  int bm = 128, bn = C > 64 ? 128 : (C > 32 ? 64 : 32);
  auto wgs = [&]() { return (long long)P * pta_cdiv(R, bm) * pta_cdiv(C, bn); };
  if (wgs() < FS_FILL) bm = 64;
  if (wgs() < FS_FILL && bn == 128) bn = 64;
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

extern "C" int64_t pta_fstat_fe_tiles(int S) { return S < 1 ? 0 : (int64_t)((S + FS_ST - 1) / FS_ST) * (FS_ST / 16); }

extern "C" int pta_fstat_fe(const double *Q, int64_t ld_q, int P, int J, int R, const double *phi, int S, const double *Minv, double *fe,
                            int64_t ld_fe, double *fe_max, int64_t ld_max, int32_t *fe_arg, int64_t ld_arg, double *part_val, int32_t *part_arg,
                            void *stream) {
  PTA_REQUIRE(Q && phi && Minv, PTA_E_ARG, "pta_fstat_fe: NULL argument");
  PTA_REQUIRE(P >= 2 && P <= PTA_FSTAT_PMAX && J >= 1 && 2 * J <= PTA_FSTAT_CMAX && R > 0 && S >= 1, PTA_E_ARG,
              "pta_fstat_fe: P=%d (2..%d) J=%d (1..%d) R=%d S=%d", P, PTA_FSTAT_PMAX, J, PTA_FSTAT_CMAX / 2, R, S);
  PTA_REQUIRE(ld_q >= (int64_t)P * 2 * J, PTA_E_ARG, "pta_fstat_fe: ld_q=%lld < 2*P*J=%lld", (long long)ld_q, (long long)P * 2 * J);
  const bool maxmode = fe == nullptr;
  if (maxmode) {
    PTA_REQUIRE(fe_max && fe_arg && part_val && part_arg, PTA_E_ARG,
                "pta_fstat_fe: without the full map (fe NULL) fe_max, fe_arg and the workspaces part_val, part_arg are needed");
    PTA_REQUIRE(ld_max >= J && ld_arg >= J, PTA_E_ARG, "pta_fstat_fe: ld_max=%lld or ld_arg=%lld < J=%d", (long long)ld_max, (long long)ld_arg, J);
  } else {
    PTA_REQUIRE(!fe_max && !fe_arg, PTA_E_ARG, "pta_fstat_fe: one output mode per call: the full map (fe) or the maxima (fe_max, fe_arg)");
    PTA_REQUIRE(ld_fe >= (int64_t)J * S, PTA_E_ARG, "pta_fstat_fe: ld_fe=%lld < J*S=%lld", (long long)ld_fe, (long long)J * S);
  }
  const unsigned nst = pta_cdiv(S, FS_ST), njb = pta_cdiv(J, 8);
  // realisations per workgroup: enough workgroups to fill the chip, never fewer than 8 realisations per walk (phi and M^-1 are
  // loaded once per workgroup); the split only regroups realisations
  long long nz = 4096 / ((long long)nst * njb);
  if (nz < 1) nz = 1;
  if (nz > (R + 7) / 8) nz = (R + 7) / 8;
  if (nz > 65535) nz = 65535;
  const int rchunk = (int)((R + nz - 1) / nz);
  const unsigned ngz = pta_cdiv(R, rchunk);
  const int ntile = (int)pta_fstat_fe_tiles(S);
  dim3 grid(nst, njb, ngz), block(256);
  hipStream_t s = pta_stream(stream);
  const int ks = (P + 3) / 4;  // MFMA steps of four pulsars
#define PTA_FS_CASE(KS_)                                                                                                              \
  case KS_:                                                                                                                           \
    if (maxmode)                                                                                                                      \
      hipLaunchKernelGGL((k_fstat_fe<KS_, true>), grid, block, 0, s, Q, ld_q, P, J, R, rchunk, phi, S, Minv, fe, ld_fe, part_val, \
                         part_arg, ntile);                                                                                            \
    else                                                                                                                              \
      hipLaunchKernelGGL((k_fstat_fe<KS_, false>), grid, block, 0, s, Q, ld_q, P, J, R, rchunk, phi, S, Minv, fe, ld_fe, part_val, \
                         part_arg, ntile);                                                                                            \
    break;
  switch (ks) {
    PTA_FS_CASE(1) PTA_FS_CASE(2) PTA_FS_CASE(3) PTA_FS_CASE(4) PTA_FS_CASE(5) PTA_FS_CASE(6) PTA_FS_CASE(7) PTA_FS_CASE(8)
    PTA_FS_CASE(9) PTA_FS_CASE(10) PTA_FS_CASE(11) PTA_FS_CASE(12) PTA_FS_CASE(13) PTA_FS_CASE(14) PTA_FS_CASE(15) PTA_FS_CASE(16)
    PTA_FS_CASE(17) PTA_FS_CASE(18) PTA_FS_CASE(19) PTA_FS_CASE(20) PTA_FS_CASE(21) PTA_FS_CASE(22) PTA_FS_CASE(23) PTA_FS_CASE(24)
    PTA_FS_CASE(25) PTA_FS_CASE(26) PTA_FS_CASE(27) PTA_FS_CASE(28) PTA_FS_CASE(29) PTA_FS_CASE(30) PTA_FS_CASE(31) PTA_FS_CASE(32)
  }
#undef PTA_FS_CASE
  PTA_LAUNCH_CHECK();
  if (maxmode) {
    return pta_fstat_reduce_launch(part_val, part_arg, (int64_t)R * J, ntile, J, fe_max, ld_max, fe_arg, ld_arg, s);
  }
  return PTA_OK;
}
