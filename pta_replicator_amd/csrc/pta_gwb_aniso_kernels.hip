// Anisotropic GWB per realisation: an ORF factor per realisation and the mix that reads it.
//
//   pta_gwb_orf_factor   M_r = chol(2 sum_k clm[r, k] basis[k])   (red_noise.py:225-226, 235 with a clm per realisation)
//   pta_gwb_mix_batched  G[r] = M_r G0[r]                         (red_noise.py:268; pta_gwb_mix with a factor per realisation)
//
// pta_gwb_orf_factor, P <= 80: one workgroup = PTA_ORF_RB realisations, one per wave.  The workgroup walks the lower triangle of the
// basis once - every basis element is read once per workgroup and feeds all its realisations, a thread's elements accumulate in
// registers so that the reads of one k are all in flight together - and leaves the packed lower triangles
// of the ORFs in LDS, column by column, E[start(k) + (m - k)] = ORF[m, k], start(k) = k P - k (k - 1) / 2 (the layout of pta_lnl_factor).
// The sum over k is pta_orf_combine's (ascending k, product then sum, times two last), so a row of clm equal to the configured one
// gives the configured ORF bit for bit.  Each wave then factors its own matrix with the left-looking sweep of pta_os_matched_solve /
// pta_lnl_factor: at step j lane l owns rows j + l and j + l + 64, every lane accumulates the pivot from the same broadcast reads
// (rows past j + 63 only exist for the first P - 64 steps).  A
// pivot that is not positive or not finite sets info[r] = j + 1 (LAPACK's convention) and the whole of M_r becomes NaN: a realisation
// with a sky that is not positive definite never comes out as plausible numbers.  No atomics, nothing shared between realisations: M_r
// is a function of (basis, clm[r]) alone, whatever R or the workgroup it is computed in.
// P > 80: clm . basis by the batched GEMM, pta_potrf_batched_ex with forward-substitution panel solves, and the same NaN fill.
//
// pta_gwb_mix_batched, P <= 80: k_gwb_mix_small (pta_gwb_kernels.hip) with blockIdx.y = realisation: the factor is staged K-major in
// LDS once per workgroup and reused over `tpw` 64-sample tiles of that realisation; MFMA layout, bounds handling and HBM traffic per
// (r, a, sample) are that kernel's.  Every output is one fixed sequence of operations, whatever tpw.
#include <math.h>
#include <atomic>
#include "pta_common.h"
#include "pta_mfma.h"

#define PTA_ORF_RB 4     // realisations per workgroup of k_gwb_orf_factor (one per wave)
#define PTA_ORF_PMAX 80  // largest P of the LDS kernels (4 packed triangles: 104 KB; the mix's square: 51 KB)
#define PTA_ORF_EPT 13    // lower-triangle elements per thread of k_gwb_orf_factor: ceil(80 * 81 / 2 / 256)
#define PTA_ORF_LMMAX 81 // (lmax + 1)^2 at lmax = 8 (pta_orf_basis)

__global__ __launch_bounds__(256) void k_gwb_orf_factor(const double *__restrict__ basis, int n_lm, int P, const double *__restrict__ clm,
                                                        int64_t ld_clm, int R, double *__restrict__ Mchol, int32_t *__restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int T = P * (P + 1) / 2;
  double *cs = lds + PTA_ORF_RB * T;  // [PTA_ORF_RB][n_lm]
  const int t = threadIdx.x, l = t & 63, w = t >> 6;
  const int64_t rbase = (int64_t)blockIdx.x * PTA_ORF_RB;
  for (int i = t; i < PTA_ORF_RB * n_lm; i += 256) {
    const int q = i / n_lm, k = i - q * n_lm;
    const int64_t r = rbase + q < R ? rbase + q : R - 1;  // a wave past R repeats the last realisation and stores nothing
    cs[i] = clm[r * ld_clm + k];
  }
  __syncthreads();
  // ---- ORF_q = 2 sum_k clm[q, k] basis[k], lower triangle: thread t owns elements t, t + 256, .. of the row-major lower triangle and
  // keeps their sums in registers, so that one step of k has all its basis reads in flight at once
  const int64_t PP = (int64_t)P * P;
  int boff[PTA_ORF_EPT], at[PTA_ORF_EPT];
  double sum[PTA_ORF_EPT][PTA_ORF_RB];
#pragma unroll
  for (int u = 0; u < PTA_ORF_EPT; ++u) {
    const int i = t + 256 * u;
    int m = (int)((sqrt(8.0 * i + 1.0) - 1.0) * 0.5);
    while (m * (m + 1) / 2 > i) --m;
    while ((m + 1) * (m + 2) / 2 <= i) ++m;
    const int k = i - m * (m + 1) / 2;
    boff[u] = i < T ? m * P + k : -1;
    at[u] = k * P - k * (k - 1) / 2 + (m - k);
#pragma unroll
    for (int q = 0; q < PTA_ORF_RB; ++q) sum[u][q] = 0.0;
  }
  for (int kk = 0; kk < n_lm; ++kk) {
    double c[PTA_ORF_RB], b[PTA_ORF_EPT];
#pragma unroll
    for (int q = 0; q < PTA_ORF_RB; ++q) c[q] = cs[q * n_lm + kk];
#pragma unroll
    for (int u = 0; u < PTA_ORF_EPT; ++u) b[u] = boff[u] >= 0 ? basis[kk * PP + boff[u]] : 0.0;
#pragma unroll
    for (int u = 0; u < PTA_ORF_EPT; ++u)
#pragma unroll
      for (int q = 0; q < PTA_ORF_RB; ++q) sum[u][q] = sum[u][q] + c[q] * b[u];
  }
#pragma unroll
  for (int u = 0; u < PTA_ORF_EPT; ++u)
    if (boff[u] >= 0) {
#pragma unroll
      for (int q = 0; q < PTA_ORF_RB; ++q) lds[q * T + at[u]] = sum[u][q] * 2.0;
    }
  __syncthreads();
  // ---- ORF_w = L L^T, column by column; wave w owns matrix w.  A matrix is private to its wave, whose LDS accesses complete in program
  // order: column j is read as ORF before it is written as L without a barrier in between; the barrier closes the step
  double *E = lds + w * T;
  int bad = 0, sj = 0;
  for (int j = 0; j < P; ++j) {
    const int m0 = j + l, m1 = m0 + 64;
    const int mm0 = min(m0, P - 1), mm1 = min(m1, P - 1);
    const bool two = j + 64 < P;  // uniform: rows past j + 63 exist
    double acc0 = 0.0, acc1 = 0.0, dd = 0.0;
    int sk = 0;
    if (two) {
#pragma unroll 4
      for (int k = 0; k < j; ++k) {
        const double ejk = E[sk + (j - k)];
        acc0 = fma(E[sk + (mm0 - k)], ejk, acc0);
        acc1 = fma(E[sk + (mm1 - k)], ejk, acc1);
        dd = fma(ejk, ejk, dd);
        sk += P - k;
      }
    } else {
#pragma unroll 4
      for (int k = 0; k < j; ++k) {
        const double ejk = E[sk + (j - k)];
        acc0 = fma(E[sk + (mm0 - k)], ejk, acc0);
        dd = fma(ejk, ejk, dd);
        sk += P - k;
      }
    }
    const double piv = E[sj] - dd;
    const double a0 = E[sj + (mm0 - j)], a1 = E[sj + (mm1 - j)];
    const bool ok = piv > 0.0 && piv <= 1.79769313486231570815e308;
    if (!ok && !bad) bad = j + 1;
    const double root = ok ? sqrt(piv) : nan("");
    if (m0 < P) E[sj + (m0 - j)] = l == 0 ? root : (a0 - acc0) / root;
    if (m1 < P) E[sj + (m1 - j)] = (a1 - acc1) / root;
    sj += P - j;
    __syncthreads();
  }
  // ---- M_r, its upper triangle zero (the mix reads the full square); all NaN where the ORF was not positive definite
  const int64_t r = rbase + w;
  if (r >= R) return;
  double *out = Mchol + r * PP;
  const double qnan = nan("");
  for (int e = l; e < P * P; e += 64) {
    const int m = e / P, k = e - m * P;
    out[e] = bad ? qnan : (k <= m ? E[k * P - k * (k - 1) / 2 + (m - k)] : 0.0);
  }
  if (l == 0) info[r] = bad;
}

__global__ void k_gwb_orf_nan_fill(double *__restrict__ Mchol, int64_t PP, const int32_t *__restrict__ info) {
  const int64_t r = blockIdx.x;
  if (info[r] == 0) return;
  const double qnan = nan("");
  for (int64_t e = threadIdx.x; e < PP; e += blockDim.x) Mchol[r * PP + e] = qnan;
}

extern "C" int pta_gwb_orf_factor(const double *basis, int n_lm, int P, const double *clm, int64_t ld_clm, int R, double *Mchol,
                                  int32_t *info, void *stream) {
  PTA_REQUIRE(basis && clm && Mchol && info, PTA_E_ARG, "pta_gwb_orf_factor: NULL argument");
  PTA_REQUIRE(n_lm >= 1 && n_lm <= PTA_ORF_LMMAX && P > 0 && P <= 4096 && R > 0 && ld_clm >= n_lm, PTA_E_ARG,
              "pta_gwb_orf_factor: n_lm=%d (1..%d) P=%d (1..4096) R=%d ld_clm=%lld", n_lm, PTA_ORF_LMMAX, P, R, (long long)ld_clm);
  hipStream_t s = pta_stream(stream);
  if (P <= PTA_ORF_PMAX) {
    const size_t shmem = (size_t)PTA_ORF_RB * (P * (P + 1) / 2 + n_lm) * sizeof(double);
    if (shmem > 65536) {  // once per device: the largest request the kernel can make (P = 80, n_lm = 81)
      static std::atomic<uint64_t> raised{0};
      int dev = 0;
      PTA_HIP(hipGetDevice(&dev));
      const uint64_t bit = 1ull << (dev & 63);
      if (!(raised.load() & bit)) {
        const int most = PTA_ORF_RB * (PTA_ORF_PMAX * (PTA_ORF_PMAX + 1) / 2 + PTA_ORF_LMMAX) * (int)sizeof(double);
        PTA_HIP(hipFuncSetAttribute((const void *)k_gwb_orf_factor, hipFuncAttributeMaxDynamicSharedMemorySize, most));
        raised.fetch_or(bit);
      }
    }
    hipLaunchKernelGGL(k_gwb_orf_factor, dim3(pta_cdiv(R, PTA_ORF_RB)), dim3(256), shmem, s, basis, n_lm, P, clm, ld_clm, R, Mchol, info);
    PTA_LAUNCH_CHECK();
    return PTA_OK;
  }
  const int PP = P * P;
  int rc = pta_dgemm_launch(0, R, PP, n_lm, 2.0, clm, ld_clm, 1, basis, PP, 0.0, Mchol, PP, 0, 1, 0, 0, 0, 1, s);
  if (rc != PTA_OK) return rc;
  rc = pta_potrf_batched_ex(Mchol, P, P, PP, R, info, PTA_POTRF_SUBSTITUTION | PTA_POTRF_ZERO_UPPER, stream);
  if (rc != PTA_OK) return rc;
  hipLaunchKernelGGL(k_gwb_orf_nan_fill, dim3(R), dim3(256), 0, s, Mchol, (int64_t)PP, info);
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}

#define MIXB_JT 64
template <int NTA>
__global__ __launch_bounds__(256) void k_gwb_mix_batched(const double *__restrict__ Mchol, int64_t ld_m, int P, const double *__restrict__ G0,
                                                         int npts, int64_t ldg, double *__restrict__ G, int tpw) {
  extern __shared__ double Ms[];  // [KP][MP]: Ms[b * MP + a] = M_r[a][b], zero padded
  constexpr int MP = NTA * 16;
  const int KP = (P + 3) & ~3;
  const int t = threadIdx.x, l = t & 63, wv = t >> 6;
  const int64_t r = blockIdx.y;
  const double *__restrict__ Mr = Mchol + r * ld_m;
  for (int idx = t; idx < KP * MP; idx += 256) {
    const int b = idx / MP, a = idx - b * MP;
    Ms[idx] = (a < P && b < P) ? Mr[(int64_t)a * P + b] : 0.0;
  }
  __syncthreads();
  const int col = l & 15, quad = l >> 4;
  const double *__restrict__ g0 = G0 + r * P * ldg;
  for (int tt = 0; tt < tpw; ++tt) {
    const int j0 = (blockIdx.x * tpw + tt) * MIXB_JT;
    if (j0 >= npts) break;
    const int jj = j0 + wv * 16 + col;
    const bool jin = jj < npts;
    pta_f64x4 acc[NTA];
#pragma unroll
    for (int i = 0; i < NTA; ++i) acc[i] = pta_f64x4{0.0, 0.0, 0.0, 0.0};
    double bv[NTA * 4];  // all K-steps' G0 samples of this tile in flight at once (KP / 4 <= NTA * 4)
#pragma unroll
    for (int s4 = 0; s4 < NTA * 4; ++s4) {
      const int b = 4 * s4 + quad;
      bv[s4] = (b < P && jin) ? g0[(int64_t)b * ldg + jj] : 0.0;
    }
#pragma unroll
    for (int s4 = 0; s4 < NTA * 4; ++s4) {
      if (4 * s4 < KP) {  // uniform
        const int b = 4 * s4 + quad;
#pragma unroll
        for (int i = 0; i < NTA; ++i) acc[i] = pta_mfma_f64(Ms[b * MP + i * 16 + col], bv[s4], acc[i]);
      }
    }
    if (jin) {
#pragma unroll
      for (int i = 0; i < NTA; ++i)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
          const int a = i * 16 + pta_mfma_row(l, rg);
          if (a < P) G[(r * P + a) * ldg + jj] = acc[i][rg];
        }
    }
  }
}

// The launch plan of pta_gwb_mix_batched, the one place it is decided: the k_gwb_mix_batched<nta> instance, tpw 64-sample tiles per
// workgroup and gx workgroups per realisation; nta = 0: the batched GEMM (variant != 0 or P > PTA_ORF_PMAX), which has no such choice.
// `who` names the entry in the refusals.
static int pta_gwb_mix_batched_choose(const char *who, int P, int R, int npts, int variant, int &nta, int &tpw, unsigned &gx) {
  PTA_REQUIRE(P > 0 && R > 0 && npts > 0, PTA_E_ARG, "%s: P=%d R=%d npts=%d", who, P, R, npts);
  nta = tpw = 0, gx = 0;
  if (variant != 0 || P > PTA_ORF_PMAX) return PTA_OK;
  nta = (P + 15) / 16;
  const int ntile = (int)pta_cdiv(npts, MIXB_JT);
  // a workgroup keeps its factor for all tiles of the realisation once the realisations alone fill the chip, else for four
  tpw = (R >= 512 || ntile <= 4) ? ntile : 4;
  gx = pta_cdiv(ntile, tpw);
  PTA_REQUIRE(R <= 65535, PTA_E_ARG, "%s: R=%d too large for one launch", who, R);
  return PTA_OK;
}

extern "C" int pta_gwb_mix_batched_plan(int P, int R, int npts, int variant, int32_t *plan) {
  PTA_REQUIRE(plan, PTA_E_ARG, "pta_gwb_mix_batched_plan: NULL argument");
  int nta, tpw;
  unsigned gx;
  const int rc = pta_gwb_mix_batched_choose("pta_gwb_mix_batched_plan", P, R, npts, variant, nta, tpw, gx);
  if (rc != PTA_OK) return rc;
  plan[0] = nta, plan[1] = tpw, plan[2] = (int32_t)gx;
  return PTA_OK;
}

// variant: as pta_gwb_mix (0 = the LDS kernel when P <= 80, else the batched MFMA GEMM; 1 = always that GEMM; 2 = the VALU reference GEMM)
extern "C" int pta_gwb_mix_batched(const double *Mchol, int64_t ld_m, int P, const double *G0, int R, int npts, int64_t ldg, double *G,
                                   int variant, void *stream) {
  PTA_REQUIRE(Mchol && G0 && G, PTA_E_ARG, "pta_gwb_mix_batched: NULL argument");
  PTA_REQUIRE(P > 0 && R > 0 && npts > 0 && ldg >= npts && ld_m >= (int64_t)P * P, PTA_E_ARG,
              "pta_gwb_mix_batched: P=%d R=%d npts=%d ldg=%lld ld_m=%lld", P, R, npts, (long long)ldg, (long long)ld_m);
  const int64_t sr = (int64_t)P * ldg;
  int nta, tpw;
  unsigned gx;
  const int rc0 = pta_gwb_mix_batched_choose("pta_gwb_mix_batched", P, R, npts, variant, nta, tpw, gx);
  if (rc0 != PTA_OK) return rc0;
  if (nta) {
    const int kp = (P + 3) & ~3;
    const size_t shmem = (size_t)kp * nta * 16 * sizeof(double);
    dim3 g(gx, R);
#define PTA_MIXB(N) hipLaunchKernelGGL(k_gwb_mix_batched<N>, g, dim3(256), shmem, pta_stream(stream), Mchol, ld_m, P, G0, npts, ldg, G, tpw)
    switch (nta) {
      case 1: PTA_MIXB(1); break;
      case 2: PTA_MIXB(2); break;
      case 3: PTA_MIXB(3); break;
      case 4: PTA_MIXB(4); break;
      default: PTA_MIXB(5); break;
    }
#undef PTA_MIXB
    PTA_LAUNCH_CHECK();
    return PTA_OK;
  }
  for (int rb = 0; rb < R; rb += 32768) {
    const int rc_ = (R - rb < 32768) ? (R - rb) : 32768;
    int rc = pta_dgemm_launch(0, P, npts, P, 1.0, Mchol + rb * ld_m, P, 1, G0 + rb * sr, ldg, 0.0, G + rb * sr, ldg, 0, rc_, ld_m, sr, sr,
                              variant == 2 ? 0 : 1, pta_stream(stream));
    if (rc != PTA_OK) return rc;
  }
  return PTA_OK;
}
