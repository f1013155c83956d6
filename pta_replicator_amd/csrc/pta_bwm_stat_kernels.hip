// Earth-term burst-with-memory matched filter of whole ensembles (pta_replicator_amd/bwm_statistic.py holds the definitions and the
// realisation-independent preparation).  The projection Q[r, a, j] = W_a[j] . r_a is pta_fstat_project (csrc/pta_fstat_kernels.hip),
// unchanged; this file holds what follows it:
//
//   pta_bwm_stat   N_rjs = sum_a phi_as q_raj (a 2-vector) on the matrix cores, Fb = 1/2 N^T M_js^-1 N and A = M_js^-1 N in registers; the
//                  full map (and the amplitudes), or the per-tile maxima, which pta_fstat_fe's fold (pta_fstat_reduce_launch) takes over the sky tiles in ascending order
//
// The structure is pta_fstat_fe's.  The product over pulsars (K = P) of Q against phi: one wave owns 16 epochs x 16 sky points; the 16
// rows of its A tile are the epochs j0 .. j0 + 15 in their order, so accumulator register e of a lane is epoch j0 + (lane >> 4) + 4 e at
// sky point lane & 15.  Two MFMA chains, one against F+ and one against Fx of the same 16 sky points, leave both components of N_rjs of
// four (j, s) cells in one lane: the 2 x 2 form needs no cross-lane step.  phi of the wave's sky points (2 KS doubles, KS = ceil(P / 4))
// and the 3 unique entries of M_js^-1 of its four cells stay in registers for the whole launch; the workgroup (4 waves = 64 sky points)
// walks its realisations, staging Q[r, :, 16 epochs] once per realisation in LDS (double-buffered, one barrier per realisation).  N
// never leaves the registers.  Pulsars are summed in ascending groups of four by the MFMA in one chain per output (no split over
// pulsars, no atomics), the quadratic form is one fixed fma chain, the maximum over a tile is an ascending scan of its 16 sky points
// (strictly greater wins: the lower index on ties), and the tiles are folded in ascending order: an (r, j, s) value is the same in every
// output mode, chunk and row slot.
#include "pta_common.h"
#include "pta_mfma.h"

#define BS_LD 17   // LDS row stride in doubles of the sky_max block (odd: 16 rows fall into 16 different bank pairs)
#define BS_RB 4    // realisations per scan of the sky_max reduction: 4 x 16 epochs = one (realisation, epoch) per lane
#define BS_JB 16   // epochs per workgroup
#define BS_ST PTA_FSTAT_SKY_TILE  // sky points per workgroup: four waves x 16 (the tiling pta_fstat_fe_tiles counts)
static_assert(BS_ST == 64, "k_bwm_stat: a workgroup is four waves of 16 sky points");

template <int KS, bool MAXMODE>
__global__ __launch_bounds__(256) void k_bwm_stat(const double *__restrict__ Q, int64_t ld_q, int P, int C, int J, int R, int rchunk,
                                                  const double *__restrict__ phi, int S, const double *__restrict__ Minv,
                                                  double *__restrict__ fb, int64_t ld_fb, double *__restrict__ amp, int64_t ld_amp,
                                                  double *__restrict__ pval, int32_t *__restrict__ parg, int ntile) {
  __shared__ double Al[2][4 * KS * BS_JB];  // Q[r, a, j0 .. j0 + 15] of one realisation, a < 4 KS (zeros past P and past J)
  __shared__ double Mx[MAXMODE ? 4 * BS_RB * BS_JB * BS_LD : 1];  // sky_max: Fb of BS_RB realisations x 16 epochs x 16 sky points per wave
  constexpr int NL = (4 * KS * BS_JB + 255) / 256;
  const int t = threadIdx.x, l = t & 63, w = t >> 6, g = l >> 4, m = l & 15;
  const int j0 = blockIdx.y * BS_JB, st = blockIdx.x;
  const int s = st * BS_ST + w * 16 + m;  // this lane's sky point
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
  // M^-1 of the lane's four cells: epochs j0 + g + 4 e at sky point s, packed (00, 01, 11)
  double mi[4][3];
  bool live[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int j = j0 + g + 4 * e;
    live[e] = j < J && s < S;
#pragma unroll
    for (int i = 0; i < 3; ++i) mi[e][i] = live[e] ? Minv[((int64_t)j * S + s) * 3 + i] : 0.0;
  }
  double qv[NL];
  auto fetch = [&](int r) {
#pragma unroll
    for (int u = 0; u < NL; ++u) {
      const int idx = t + 256 * u, a = idx >> 4, c = j0 + (idx & 15);
      qv[u] = (idx < 4 * KS * BS_JB && a < P && c < J) ? Q[(int64_t)r * ld_q + (int64_t)a * C + c] : 0.0;
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int u = 0; u < NL; ++u) {
      const int idx = t + 256 * u;
      if (idx < 4 * KS * BS_JB) Al[buf][idx] = qv[u];
    }
  };
  if (r_lo < r_hi) fetch(r_lo);
  for (int r = r_lo; r < r_hi; ++r) {
    const int cur = (r - r_lo) & 1;
    stash(cur);
    __syncthreads();  // the buffer written two realisations ago was last read before the previous barrier
    if (r + 1 < r_hi) fetch(r + 1);
    pta_f64x4 np_ = pta_f64x4{0.0, 0.0, 0.0, 0.0}, nc_ = pta_f64x4{0.0, 0.0, 0.0, 0.0};
    // A operand: lane l of step k supplies Q[r, a = 4 k + (l >> 4), j0 + (l & 15)]
    const double *Ab = Al[cur] + g * BS_JB + m;
#pragma unroll
    for (int k = 0; k < KS; ++k) {
      const double av = Ab[k * 4 * BS_JB];
      np_ = pta_mfma_f64(av, bplus[k], np_);
      nc_ = pta_mfma_f64(av, bcross[k], nc_);
    }
    // accumulator e of lane l: tile row (l >> 4) + 4 e = epoch j0 + g + 4 e; column = sky point l & 15
    double f[4], a0[4], a1[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      a0[e] = fma(mi[e][1], nc_[e], mi[e][0] * np_[e]);  // A = M^-1 N
      a1[e] = fma(mi[e][2], nc_[e], mi[e][1] * np_[e]);
      f[e] = 0.5 * fma(nc_[e], a1[e], np_[e] * a0[e]);   // 1/2 N^T A
    }
    if (!MAXMODE) {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (live[e]) {
          const int64_t cell = (int64_t)(j0 + g + 4 * e) * S + s;
          fb[(int64_t)r * ld_fb + cell] = f[e];
          if (amp) *reinterpret_cast<double2 *>(amp + (int64_t)r * ld_amp + 2 * cell) = double2{a0[e], a1[e]};
        }
    } else {
      // maximum over the 16 sky points of the wave, BS_RB realisations at a time through the wave's own LDS block [realisation][epoch]
      // [sky point]: a lane then scans the 16 sky points of one (realisation, epoch) in ascending order, strictly greater winning (the
      // lower index on ties), and 16 lanes write 16 consecutive epochs.  Sky points past S never win.
      const int q = (r - r_lo) % BS_RB;
      double *mw = Mx + w * (BS_RB * BS_JB * BS_LD);
#pragma unroll
      for (int e = 0; e < 4; ++e) mw[(q * BS_JB + g + 4 * e) * BS_LD + m] = s < S ? f[e] : -INFINITY;
      if (q == BS_RB - 1 || r + 1 == r_hi) {  // uniform over the workgroup
        __syncthreads();
        const int qq = l >> 4, jj = j0 + (l & 15);
        if (qq <= q && jj < J) {
          const double *v = mw + l * BS_LD;
          double best = v[0];
          int bk = 0;
#pragma unroll
          for (int k = 1; k < 16; ++k)
            if (v[k] > best) best = v[k], bk = k;
          const int64_t slot = ((int64_t)(r - q + qq) * ntile + st * 4 + w) * J;  // [r][16-point sub-tile, ascending in s][j]
          pval[slot + jj] = best;
          parg[slot + jj] = st * BS_ST + w * 16 + bk;
        }
      }
    }
  }
}

extern "C" int pta_bwm_stat(const double *Q, int64_t ld_q, int P, int C, int J, int R, const double *phi, int S, const double *Minv, double *fb,
                            int64_t ld_fb, double *amp, int64_t ld_amp, double *fb_max, int64_t ld_max, int32_t *fb_arg, int64_t ld_arg,
                            double *part_val, int32_t *part_arg, void *stream) {
  PTA_REQUIRE(Q && phi && Minv, PTA_E_ARG, "pta_bwm_stat: NULL argument");
  PTA_REQUIRE(P >= 2 && P <= PTA_FSTAT_PMAX && J >= 1 && C >= J && C <= PTA_FSTAT_CMAX && R > 0 && S >= 1, PTA_E_ARG,
              "pta_bwm_stat: P=%d (2..%d) J=%d C=%d (J <= C <= %d) R=%d S=%d", P, PTA_FSTAT_PMAX, J, C, PTA_FSTAT_CMAX, R, S);
  PTA_REQUIRE(ld_q >= (int64_t)P * C, PTA_E_ARG, "pta_bwm_stat: ld_q=%lld < P*C=%lld", (long long)ld_q, (long long)P * C);
  const bool maxmode = fb == nullptr;
  if (maxmode) {
    PTA_REQUIRE(fb_max && fb_arg && part_val && part_arg, PTA_E_ARG,
                "pta_bwm_stat: without the full map (fb NULL) fb_max, fb_arg and the workspaces part_val, part_arg are needed");
    PTA_REQUIRE(!amp, PTA_E_ARG, "pta_bwm_stat: the amplitudes come with the full map only (amp needs fb)");
    PTA_REQUIRE(ld_max >= J && ld_arg >= J, PTA_E_ARG, "pta_bwm_stat: ld_max=%lld or ld_arg=%lld < J=%d", (long long)ld_max, (long long)ld_arg, J);
  } else {
    PTA_REQUIRE(!fb_max && !fb_arg, PTA_E_ARG, "pta_bwm_stat: one output mode per call: the full map (fb) or the maxima (fb_max, fb_arg)");
    PTA_REQUIRE(ld_fb >= (int64_t)J * S, PTA_E_ARG, "pta_bwm_stat: ld_fb=%lld < J*S=%lld", (long long)ld_fb, (long long)J * S);
    if (amp) {
      PTA_REQUIRE(ld_amp >= (int64_t)2 * J * S && ld_amp % 2 == 0 && ((uintptr_t)amp & 15) == 0, PTA_E_ARG,
                  "pta_bwm_stat: ld_amp=%lld (even, >= 2*J*S=%lld), amp 16-byte aligned", (long long)ld_amp, (long long)2 * J * S);
    }
  }
  const unsigned nst = pta_cdiv(S, BS_ST), njb = pta_cdiv(J, BS_JB);
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
#define PTA_BS_CASE(KS_)                                                                                                                 \
  case KS_:                                                                                                                              \
    if (maxmode)                                                                                                                         \
      hipLaunchKernelGGL((k_bwm_stat<KS_, true>), grid, block, 0, s, Q, ld_q, P, C, J, R, rchunk, phi, S, Minv, fb, ld_fb, amp, ld_amp, \
                         part_val, part_arg, ntile);                                                                                     \
    else                                                                                                                                 \
      hipLaunchKernelGGL((k_bwm_stat<KS_, false>), grid, block, 0, s, Q, ld_q, P, C, J, R, rchunk, phi, S, Minv, fb, ld_fb, amp, ld_amp, \
                         part_val, part_arg, ntile);                                                                                     \
    break;
  switch (ks) {
    PTA_BS_CASE(1) PTA_BS_CASE(2) PTA_BS_CASE(3) PTA_BS_CASE(4) PTA_BS_CASE(5) PTA_BS_CASE(6) PTA_BS_CASE(7) PTA_BS_CASE(8)
    PTA_BS_CASE(9) PTA_BS_CASE(10) PTA_BS_CASE(11) PTA_BS_CASE(12) PTA_BS_CASE(13) PTA_BS_CASE(14) PTA_BS_CASE(15) PTA_BS_CASE(16)
    PTA_BS_CASE(17) PTA_BS_CASE(18) PTA_BS_CASE(19) PTA_BS_CASE(20) PTA_BS_CASE(21) PTA_BS_CASE(22) PTA_BS_CASE(23) PTA_BS_CASE(24)
    PTA_BS_CASE(25) PTA_BS_CASE(26) PTA_BS_CASE(27) PTA_BS_CASE(28) PTA_BS_CASE(29) PTA_BS_CASE(30) PTA_BS_CASE(31) PTA_BS_CASE(32)
  }
#undef PTA_BS_CASE
  PTA_LAUNCH_CHECK();
  if (maxmode) {
    // the fold over the sub-tile maxima in ascending sky order is pta_fstat_fe's (k_fstat_fe_reduce): the same [r][tile][j] layout
    return pta_fstat_reduce_launch(part_val, part_arg, (int64_t)R * J, ntile, J, fb_max, ld_max, fb_arg, ld_arg, s);
  }
  return PTA_OK;
}
