// The kernel and the launcher the sky-grid statistics share (pta_fstat_fe in pta_fstat_kernels.hip, pta_bwm_stat in
// pta_bwm_stat_kernels.hip): the product over pulsars (K = P) of the projections Q against the antenna patterns phi on the matrix cores,
// a quadratic form per (realisation, grid point j, sky point s) in registers, and either the full map or its maximum over the sky.
//
// One wave owns 16 rows of Q (Stat::JB grid points x Stat::QPJ columns each) x 16 sky points.  Two MFMA chains, one against F+ and one
// against Fx of the same 16 sky points, leave every component of N_rjs of Stat::NC cells in one lane - cell e of a lane is grid point
// j0 + (lane >> 4) + 4 e at sky point lane & 15 - so the form needs no cross-lane step.  phi of the wave's sky points (2 KS doubles, KS =
// ceil(P / 4)) and the Stat::NM unique entries of M_js^-1 of its cells stay in registers for the whole launch; the workgroup (4 waves = 64
// sky points) walks its realisations, staging Q[r, :, 16 columns] once per realisation in LDS (double-buffered, one barrier per
// realisation).  N never leaves the registers.  Pulsars are summed in ascending groups of four by the MFMA in one chain per output (no
// split over pulsars, no atomics), the quadratic form is one fixed fma chain, the maximum over a tile is an ascending scan of its 16 sky
// points (strictly greater wins: the lower index on ties), and the tiles are folded in ascending order: an (r, j, s) value is the same
// in every output mode, chunk and row slot.
//
// Stat, the statistic's policy (no data members):
//   JB, NC     grid points per workgroup (8 or 16) and cells per lane, JB = 4 NC
//   NM         packed entries of M_js^-1 per cell
//   QPJ        columns of Q per grid point: the workgroup stages columns QPJ j0 .. QPJ j0 + 15, below QPJ J
//   AMP        whether the amplitude output exists
//   qoff(a, C, J)  offset of pulsar a in a row of Q
//   acol(m)        staged column of row m of the A tile
//   value(mi, np_, nc_, cell, a0, a1)   the statistic of cell `cell` from its M^-1 entries and both accumulators; a0, a1: the amplitudes
#pragma once
#include "pta_common.h"
#include "pta_mfma.h"

#define SKY_LD 17  // LDS row stride in doubles of the sky_max block (odd: 16 rows fall into 16 different bank pairs)
#define SKY_ST PTA_FSTAT_SKY_TILE  // sky points per workgroup: four waves x 16 (the tiling pta_fstat_fe_tiles counts)
static_assert(SKY_ST == 64, "k_sky_stat: a workgroup is four waves of 16 sky points");

template <class Stat, int KS, bool MAXMODE>
__global__ __launch_bounds__(256) void k_sky_stat(const double *__restrict__ Q, int64_t ld_q, int P, int C, int J, int R, int rchunk,
                                                  const double *__restrict__ phi, int S, const double *__restrict__ Minv,
                                                  double *__restrict__ out, int64_t ld_out, double *__restrict__ amp, int64_t ld_amp,
                                                  double *__restrict__ pval, int32_t *__restrict__ parg, int ntile) {
  constexpr int JB = Stat::JB, NC = Stat::NC, NM = Stat::NM, RB = 64 / JB;  // RB realisations per scan: one (realisation, j) per lane
  static_assert(JB == 4 * NC && JB * Stat::QPJ == 16, "k_sky_stat: a wave's A tile is 16 rows, four cells apart per lane");
  __shared__ double Al[2][4 * KS * 16];  // Q[r, a, QPJ j0 .. QPJ j0 + 15] of one realisation, a < 4 KS (zeros past P and past QPJ J)
  __shared__ double Mx[MAXMODE ? 4 * RB * JB * SKY_LD : 1];  // sky_max: the values of RB realisations x JB grid points x 16 sky points per wave
  constexpr int NL = (4 * KS * 16 + 255) / 256;
  const int t = threadIdx.x, l = t & 63, w = t >> 6, g = l >> 4, m = l & 15;
  const int j0 = blockIdx.y * JB, st = blockIdx.x;
  const int s = st * SKY_ST + w * 16 + m;  // this lane's sky point
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
  // M^-1 of the lane's cells: grid points j0 + g + 4 e at sky point s, packed
  double mi[NC][NM];
  bool live[NC];
#pragma unroll
  for (int e = 0; e < NC; ++e) {
    const int j = j0 + g + 4 * e;
    live[e] = j < J && s < S;
#pragma unroll
    for (int i = 0; i < NM; ++i) mi[e][i] = live[e] ? Minv[((int64_t)j * S + s) * NM + i] : 0.0;
  }
  const int acol = Stat::acol(m);
  double qv[NL];
  auto fetch = [&](int r) {
#pragma unroll
    for (int u = 0; u < NL; ++u) {
      const int idx = t + 256 * u, a = idx >> 4, c = Stat::QPJ * j0 + (idx & 15);
      qv[u] = (idx < 4 * KS * 16 && a < P && c < Stat::QPJ * J) ? Q[(int64_t)r * ld_q + Stat::qoff(a, C, J) + c] : 0.0;
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
    // A operand: lane l of step k supplies Q[r, a = 4 k + (l >> 4), staged column acol(l & 15)]
    const double *Ab = Al[cur] + g * 16 + acol;
#pragma unroll
    for (int k = 0; k < KS; ++k) {
      const double av = Ab[k * 64];
      np_ = pta_mfma_f64(av, bplus[k], np_);
      nc_ = pta_mfma_f64(av, bcross[k], nc_);
    }
    // accumulator i of lane l: tile row (l >> 4) + 4 i; column = sky point l & 15
    double f[NC], a0[NC], a1[NC];
#pragma unroll
    for (int e = 0; e < NC; ++e) f[e] = Stat::value(mi[e], np_, nc_, e, a0[e], a1[e]);
    if (!MAXMODE) {
      if (s < S) {  // the sky point first, then each cell's grid point: one mask per cell costs Fe 4 VGPRs from KS = 16 on (a wave per SIMD)
#pragma unroll
        for (int e = 0; e < NC; ++e)
          if (j0 + g + 4 * e < J) {
            const int64_t cell = (int64_t)(j0 + g + 4 * e) * S + s;
            out[(int64_t)r * ld_out + cell] = f[e];
            if (Stat::AMP && amp) *reinterpret_cast<double2 *>(amp + (int64_t)r * ld_amp + 2 * cell) = double2{a0[e], a1[e]};
          }
      }
    } else {
      // maximum over the 16 sky points of the wave, RB realisations at a time through the wave's own LDS block [realisation][grid point]
      // [sky point]: a lane then scans the 16 sky points of one (realisation, grid point) in ascending order, strictly greater winning
      // (the lower index on ties), and JB lanes write JB consecutive grid points.  Sky points past S never win.
      const int q = (r - r_lo) % RB;
      double *mw = Mx + w * (RB * JB * SKY_LD);
#pragma unroll
      for (int e = 0; e < NC; ++e) mw[(q * JB + g + 4 * e) * SKY_LD + m] = s < S ? f[e] : -INFINITY;
      if (q == RB - 1 || r + 1 == r_hi) {  // uniform over the workgroup
        __syncthreads();
        const int qq = l / JB, jj = j0 + l % JB;
        if (qq <= q && jj < J) {
          const double *v = mw + l * SKY_LD;
          double best = v[0];
          int bk = 0;
#pragma unroll
          for (int k = 1; k < 16; ++k)
            if (v[k] > best) best = v[k], bk = k;
          const int64_t slot = ((int64_t)(r - q + qq) * ntile + st * 4 + w) * J;  // [r][16-point sub-tile, ascending in s][j]
          pval[slot + jj] = best;
          parg[slot + jj] = st * SKY_ST + w * 16 + bk;
        }
      }
    }
  }
}

// The launch plan of a sky statistic, the one place it is decided: ks MFMA steps of four pulsars (the k_sky_stat<Stat, ks, mode>
// instance), rchunk realisations per workgroup, and the grid nst x njb x ngz.  `who` names the entry in the refusals.
template <class Stat>
static int pta_sky_stat_choose(const char *who, int P, int J, int R, int S, int &ks, int &rchunk, unsigned &nst, unsigned &njb, unsigned &ngz) {
  PTA_REQUIRE(P >= 2 && P <= PTA_FSTAT_PMAX && J >= 1 && Stat::QPJ * J <= PTA_FSTAT_CMAX && R > 0 && S >= 1, PTA_E_ARG,
              "%s: P=%d (2..%d) J=%d (1..%d) R=%d S=%d", who, P, PTA_FSTAT_PMAX, J, PTA_FSTAT_CMAX / Stat::QPJ, R, S);
  nst = pta_cdiv(S, SKY_ST), njb = pta_cdiv(J, Stat::JB);
  // realisations per workgroup: enough workgroups to fill the chip, never fewer than 8 realisations per walk (phi and M^-1 are
  // loaded once per workgroup); the split only regroups realisations
  long long nz = 4096 / ((long long)nst * njb);
  if (nz < 1) nz = 1;
  if (nz > (R + 7) / 8) nz = (R + 7) / 8;
  if (nz > 65535) nz = 65535;
  rchunk = (int)((R + nz - 1) / nz);
  ngz = pta_cdiv(R, rchunk);
  ks = (P + 3) / 4;  // MFMA steps of four pulsars
  return PTA_OK;
}

// plan[0..2] = ks, rchunk, ngz: what the pta_*_plan entry of a sky statistic returns
template <class Stat>
static int pta_sky_stat_plan(const char *who, int P, int J, int R, int S, int32_t *plan) {
  PTA_REQUIRE(plan, PTA_E_ARG, "%s: NULL argument", who);
  int ks, rchunk;
  unsigned nst, njb, ngz;
  const int rc = pta_sky_stat_choose<Stat>(who, P, J, R, S, ks, rchunk, nst, njb, ngz);
  if (rc != PTA_OK) return rc;
  plan[0] = ks, plan[1] = rchunk, plan[2] = (int32_t)ngz;
  return PTA_OK;
}

// The output-mode refusals, the grid, the KS = ceil(P / 4) x mode dispatch and the fold of the maxima.  The entry has checked Q, phi,
// Minv, the sizes and ld_q; `entry` and `map` are its name and the name of its map argument, for the wording.  out != NULL: the full
// map (and amp); out == NULL: vmax / varg through the workspaces part_val / part_arg [R * J * pta_fstat_fe_tiles(S)].
template <class Stat>
static int pta_sky_stat_launch(const char *entry, const char *map, const double *Q, int64_t ld_q, int P, int C, int J, int R, const double *phi,
                               int S, const double *Minv, double *out, int64_t ld_out, double *amp, int64_t ld_amp, double *vmax, int64_t ld_max,
                               int32_t *varg, int64_t ld_arg, double *part_val, int32_t *part_arg, void *stream) {
  const bool maxmode = out == nullptr;
  if (maxmode) {
    PTA_REQUIRE(vmax && varg && part_val && part_arg, PTA_E_ARG,
                "%s: without the full map (%s NULL) %s_max, %s_arg and the workspaces part_val, part_arg are needed", entry, map, map, map);
    PTA_REQUIRE(!amp, PTA_E_ARG, "%s: the amplitudes come with the full map only (amp needs %s)", entry, map);
    PTA_REQUIRE(ld_max >= J && ld_arg >= J, PTA_E_ARG, "%s: ld_max=%lld or ld_arg=%lld < J=%d", entry, (long long)ld_max, (long long)ld_arg, J);
  } else {
    PTA_REQUIRE(!vmax && !varg, PTA_E_ARG, "%s: one output mode per call: the full map (%s) or the maxima (%s_max, %s_arg)", entry, map, map, map);
    PTA_REQUIRE(ld_out >= (int64_t)J * S, PTA_E_ARG, "%s: ld_%s=%lld < J*S=%lld", entry, map, (long long)ld_out, (long long)J * S);
    if (amp) {
      PTA_REQUIRE(ld_amp >= (int64_t)2 * J * S && ld_amp % 2 == 0 && ((uintptr_t)amp & 15) == 0, PTA_E_ARG,
                  "%s: ld_amp=%lld (even, >= 2*J*S=%lld), amp 16-byte aligned", entry, (long long)ld_amp, (long long)2 * J * S);
    }
  }
  int ks, rchunk;
  unsigned nst, njb, ngz;
  const int rc = pta_sky_stat_choose<Stat>(entry, P, J, R, S, ks, rchunk, nst, njb, ngz);
  if (rc != PTA_OK) return rc;
  const int ntile = (int)pta_fstat_fe_tiles(S);
  dim3 grid(nst, njb, ngz), block(256);
  hipStream_t s = pta_stream(stream);
#define PTA_SKY_CASE(KS_)                                                                                                                    \
  case KS_:                                                                                                                                  \
    if (maxmode)                                                                                                                             \
      hipLaunchKernelGGL((k_sky_stat<Stat, KS_, true>), grid, block, 0, s, Q, ld_q, P, C, J, R, rchunk, phi, S, Minv, out, ld_out, amp, ld_amp, \
                         part_val, part_arg, ntile);                                                                                         \
    else                                                                                                                                     \
      hipLaunchKernelGGL((k_sky_stat<Stat, KS_, false>), grid, block, 0, s, Q, ld_q, P, C, J, R, rchunk, phi, S, Minv, out, ld_out, amp, ld_amp, \
                         part_val, part_arg, ntile);                                                                                         \
    break;
  switch (ks) {
    PTA_SKY_CASE(1) PTA_SKY_CASE(2) PTA_SKY_CASE(3) PTA_SKY_CASE(4) PTA_SKY_CASE(5) PTA_SKY_CASE(6) PTA_SKY_CASE(7) PTA_SKY_CASE(8)
    PTA_SKY_CASE(9) PTA_SKY_CASE(10) PTA_SKY_CASE(11) PTA_SKY_CASE(12) PTA_SKY_CASE(13) PTA_SKY_CASE(14) PTA_SKY_CASE(15) PTA_SKY_CASE(16)
    PTA_SKY_CASE(17) PTA_SKY_CASE(18) PTA_SKY_CASE(19) PTA_SKY_CASE(20) PTA_SKY_CASE(21) PTA_SKY_CASE(22) PTA_SKY_CASE(23) PTA_SKY_CASE(24)
    PTA_SKY_CASE(25) PTA_SKY_CASE(26) PTA_SKY_CASE(27) PTA_SKY_CASE(28) PTA_SKY_CASE(29) PTA_SKY_CASE(30) PTA_SKY_CASE(31) PTA_SKY_CASE(32)
  }
#undef PTA_SKY_CASE
  PTA_LAUNCH_CHECK();
  // the fold over the sub-tile maxima in ascending sky order (k_fstat_fe_reduce): part_val / part_arg are [r][tile][j]
  return maxmode ? pta_fstat_reduce_launch(part_val, part_arg, (int64_t)R * J, ntile, J, vmax, ld_max, varg, ld_arg, s) : PTA_OK;
}
