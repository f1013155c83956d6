// One chromatic Gaussian process per pulsar (ReplicaEngine.set_chromatic_noise, theta chrom_* keys), added after the fused launch:
//   pta_engine_chrom_coef  coef[R, P, K] = sqrt(prior) z, z = deviate c of stream (CHROM, a): pair c >> 1, branch c & 1, as k_engine_rn_coef
//                          maps stream RN; sqrt(prior) configured, or pta_rn_amp per (realisation, pulsar) from theta
//   pta_engine_chrom_add   out[r, i] (+)= sum_c Ft_chrom[c, i] coef[r, a(i), c] over the engine's tiles, the product on the fp64 matrix cores
// Formulas: pta_chrom.h.  No atomics; the sum over c runs in one fixed order: a realisation's term is the same bits in every batch,
// row slot, chunk and view.
#include "pta_common.h"
#include "pta_rng.h"
#include "pta_mfma.h"
#include "pta_chrom.h"

__global__ void k_engine_chrom_coef(pta_chrom_engine ch, uint64_t seed, uint64_t r0, int R) {
  pta_rng_stage_tables();  // Box-Muller tables -> LDS (pta_rng.h)
  __syncthreads();
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;  // (r, a, pair)
  const int P = ch.n_psr, K = ch.k, hp = K / 2;
  if (idx >= R * P * hp) return;
  const int p = idx % hp, ra = idx / hp;
  const int a = ra % P, r = ra / P;
  double z0, z1;
  pta_normal_pair(seed, r0 + (uint64_t)r, pta_stream_id(PTA_STREAM_CHROM, (uint32_t)a), (uint32_t)p, z0, z1, ch.rng_fast);
  const bool theta = ch.log10_A != nullptr;
  const double lA = theta ? ch.log10_A[(int64_t)r * ch.ld_theta + a] : 0.0, g = theta ? ch.gamma[(int64_t)r * ch.ld_theta + a] : 0.0;
  const int64_t o = (int64_t)ra * K + 2 * p;
  ch.coef[o] = pta_chrom_amp(ch.amp, ch.f, ch.tspan, a, K, 2 * p, theta, lA, g) * z0;
  ch.coef[o + 1] = pta_chrom_amp(ch.amp, ch.f, ch.tspan, a, K, 2 * p + 1, theta, lA, g) * z1;
}

extern "C" int pta_engine_chrom_coef(const pta_chrom_engine *chrom_host, uint64_t seed, uint64_t r0, int R, void *stream) {
  PTA_REQUIRE(chrom_host, PTA_E_ARG, "pta_engine_chrom_coef: NULL argument");
  const pta_chrom_engine &ch = *chrom_host;
  PTA_REQUIRE(ch.amp && ch.coef, PTA_E_ARG, "pta_engine_chrom_coef: NULL table (amp / coef)");
  PTA_REQUIRE(R > 0 && ch.n_psr > 0 && ch.k > 0 && (ch.k % 2) == 0, PTA_E_ARG, "pta_engine_chrom_coef: R=%d n_psr=%d k=%d (k must be even)", R,
              ch.n_psr, ch.k);
  if (ch.log10_A) {
    PTA_REQUIRE(ch.gamma && ch.f && ch.tspan, PTA_E_ARG, "pta_engine_chrom_coef: gamma / f / tspan missing beside log10_A");
    PTA_REQUIRE(ch.ld_theta >= ch.n_psr, PTA_E_ARG, "pta_engine_chrom_coef: ld_theta=%lld too small", (long long)ch.ld_theta);
  }
  const int64_t total = (int64_t)R * ch.n_psr * (ch.k / 2);
  PTA_REQUIRE(total < (1LL << 31), PTA_E_ARG, "pta_engine_chrom_coef: problem too large");
  hipLaunchKernelGGL(k_engine_chrom_coef, dim3(pta_cdiv(total, 256)), dim3(256), 0, pta_stream(stream), ch, seed, r0, R);
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}

#define CHROM_U 4  // rows a lane has in flight in the read-modify-write: 4 x 16 bytes per lane, as k_engine_bwm_add

// workgroup = one engine tile (<= PTA_ENGINE_TILE consecutive TOAs of one pulsar) x PTA_CHROM_RG realisations, in two phases.
// Product: a wave owns 64 TOAs of the tile and all RG rows - RG / 16 row tiles x 4 column tiles of v_mfma_f64_16x16x4_f64, one K-step per
// four bins, operand and accumulator maps those of k_engine_synth_mfma (its WIDE form: column c of MFMA tile j stands for TOA 64 wv +
// 32 (j >> 1) + 2 c + (j & 1), so a lane ends with pairs of adjacent TOAs).  The same hazards, the same answers: every load is
// unconditional, from a clamped address; a bin >= K enters with a zero coefficient; a TOA beyond the tile's count reads the tile's last
// one and lands in a column of the staged tile that is never read; a row beyond R reads row R - 1 and is never stored.  The design-matrix
// entries of a K-step are loaded once and feed every row tile.  The sums go to LDS as 16-byte pairs, sres[row][TOA].
// Read-modify-write: k_engine_bwm_add's, the value read from sres instead of computed - a half-workgroup owns a row, lane p two
// adjacent TOAs and one 16-byte access; a row that starts on an odd 8-byte slot has its pairs one element later, its head moved by
// lane 0 and an odd element left at the end by the lane it falls to; CHROM_U rows in flight, all loads issued before the first store.
// Every element is added once or written: the same value on the pair, head and tail paths.
// 1-D launch, XCD-aware as the fused kernel: workgroup `lin` takes item (lin % 8) * chunk + lin / 8, the realisation groups of a tile
// adjacent, so a tile's design-matrix slab is read from HBM into ONE L2.
template <bool ACC>
__global__ __launch_bounds__(PTA_ENGINE_TILE) void k_engine_chrom_add(const int32_t *__restrict__ tile_psr, const int32_t *__restrict__ tile_start,
                                                                      const int32_t *__restrict__ tile_count, int n_tiles,
                                                                      const double *__restrict__ Ft, int64_t ldf, const double *__restrict__ coef,
                                                                      int K, int P, int R, double *__restrict__ out, int64_t ld_out) {
  static_assert(PTA_ENGINE_TILE == 256, "k_engine_chrom_add: four waves of 64 TOAs, a half-workgroup of 128 lanes covers a tile in pairs");
  static_assert(PTA_CHROM_RG % 16 == 0 && PTA_CHROM_RG >= 16 && PTA_CHROM_RG <= 64, "PTA_CHROM_RG: 16, 32, 48 or 64");
  constexpr int RG = PTA_CHROM_RG, MT = RG / 16, PITCH = PTA_CHROM_PITCH;
  extern __shared__ __attribute__((aligned(16))) double sres[];  // [RG][PITCH]
  const int nrg = (R + RG - 1) / RG;
  const int64_t total = (int64_t)nrg * n_tiles, chunk = (total + 7) >> 3;
  const int64_t item = (int64_t)(blockIdx.x & 7) * chunk + (blockIdx.x >> 3);
  if (item >= total) return;  // workgroup-uniform, ahead of the barrier
  const int tile = (int)(item / nrg);
  const int r_lo = (int)(item - (int64_t)tile * nrg) * RG, r_hi = min(R, r_lo + RG);
  const int cnt = tile_count[tile];
  const int a = tile_psr[tile];
  const int64_t c0 = tile_start[tile];
  const int t = threadIdx.x;
  {
    const int l = t & 63, wv = __builtin_amdgcn_readfirstlane(t >> 6);
    const int col = l & 15, quad = l >> 4;
    const int t2 = wv * 64 + 2 * col;  // this lane's first TOA (inside the tile) of each half of the wave's 64
    if (wv * 64 < cnt) {               // wave-uniform: a wave beyond the tile's count has no column that is read
      int tcl[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) tcl[j] = min(t2 + 32 * (j >> 1) + (j & 1), cnt - 1);
      const double *__restrict__ cf[MT];
#pragma unroll
      for (int m = 0; m < MT; ++m) cf[m] = coef + ((int64_t)min(r_lo + 16 * m + col, R - 1) * P + a) * K;
      const double *__restrict__ Fb = Ft + c0;
      pta_f64x4 acc[MT][4];
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[m][j] = pta_f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 2
      for (int k0 = 0; k0 < K; k0 += 4) {
        const int k = k0 + quad, kc = min(k, K - 1);
        const double *__restrict__ Fk = Fb + (int64_t)kc * ldf;
        double bv[4], av[MT];
#pragma unroll
        for (int j = 0; j < 4; ++j) bv[j] = Fk[tcl[j]];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          const double a_ld = cf[m][kc];
          av[m] = (k < K) ? a_ld : 0.0;
        }
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[m][j] = pta_mfma_f64(av[m], bv[j], acc[m][j]);
      }
      // accumulator register g of row tile m is realisation 16 m + quad + 4 g; column tiles 2 h, 2 h + 1 are TOAs t2 + 32 h, + 1
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
          for (int h = 0; h < 2; ++h)
            *reinterpret_cast<double2 *>(sres + (16 * m + quad + 4 * g) * PITCH + t2 + 32 * h) = double2{acc[m][2 * h][g], acc[m][2 * h + 1][g]};
    }
  }
  __syncthreads();
  const int p = t & 127;
  const int hb = __builtin_amdgcn_readfirstlane(t >> 7);  // uniform over the wave
  for (int rb = r_lo + hb; rb < r_hi; rb += 2 * CHROM_U) {
    double oh[CHROM_U];
    double *row[CHROM_U];
    const double *sv[CHROM_U];
    double2 o[CHROM_U];
    int kind[CHROM_U], head[CHROM_U];  // kind: 0 nothing, 1 a pair, 2 a single element at head + 2 p
#pragma unroll
    for (int u = 0; u < CHROM_U; ++u) {
      const int r = rb + 2 * u;
      const bool live = r < r_hi;
      const int rr = live ? r : r_hi - 1;  // a clamped read that is never used
      sv[u] = sres + (rr - r_lo) * PITCH;
      row[u] = out + (int64_t)rr * ld_out + c0;
      head[u] = (int)(((uintptr_t)row[u] >> 3) & 1);
      const int i = head[u] + 2 * p;
      kind[u] = !live ? 0 : (i + 1 < cnt ? 1 : (i < cnt ? 2 : 0));
      head[u] = (live && p == 0) ? head[u] : 0;  // from here on: this lane moves the row's unaligned first element
      o[u] = double2{0.0, 0.0};
      oh[u] = 0.0;
      if (ACC) {
        if (kind[u] == 1) o[u] = *reinterpret_cast<const double2 *>(row[u] + i);
        else if (kind[u] == 2) o[u].x = row[u][i];
        if (head[u]) oh[u] = row[u][0];
      }
    }
#pragma unroll
    for (int u = 0; u < CHROM_U; ++u) {
      const int sh = (int)(((uintptr_t)row[u] >> 3) & 1);
      const int i = sh + 2 * p;  // <= 255: sv[i + 1] stays inside the row's pitch
      const double vx = sv[u][i], vy = sv[u][i + 1];
      if (kind[u] == 1) *reinterpret_cast<double2 *>(row[u] + i) = ACC ? double2{o[u].x + vx, o[u].y + vy} : double2{vx, vy};
      else if (kind[u] == 2) row[u][i] = ACC ? o[u].x + vx : vx;
      if (head[u]) {
        const double vh = sv[u][0];
        row[u][0] = ACC ? oh[u] + vh : vh;
      }
    }
  }
}

extern "C" int pta_engine_chrom_add(const pta_engine_plan *plan_host, const pta_chrom_engine *chrom_host, int R, double *out, int64_t ld_out,
                                    int accumulate, void *stream) {
  PTA_REQUIRE(plan_host && chrom_host && out, PTA_E_ARG, "pta_engine_chrom_add: NULL argument");
  const pta_engine_plan &p = *plan_host;
  const pta_chrom_engine &ch = *chrom_host;
  PTA_REQUIRE(p.tile_psr && p.tile_start && p.tile_count && ch.Ft && ch.coef, PTA_E_ARG, "pta_engine_chrom_add: tiles / design matrix / coef missing");
  PTA_REQUIRE(ch.k > 0 && (ch.k % 2) == 0, PTA_E_ARG, "pta_engine_chrom_add: k=%d (k must be even)", ch.k);
  PTA_REQUIRE(R > 0 && p.n_tiles > 0 && ch.n_psr == p.n_psr && ld_out >= p.n_toa && ch.ldf >= p.n_toa, PTA_E_ARG,
              "pta_engine_chrom_add: R=%d n_tiles=%d n_psr=%d/%d ld_out=%lld ldf=%lld", R, p.n_tiles, ch.n_psr, p.n_psr, (long long)ld_out,
              (long long)ch.ldf);
  PTA_REQUIRE(((uintptr_t)out & 7) == 0, PTA_E_ARG, "pta_engine_chrom_add: out must be 8-byte aligned");
  const int64_t total = (int64_t)pta_cdiv(R, PTA_CHROM_RG) * p.n_tiles, nwg = ((total + 7) >> 3) << 3;
  PTA_REQUIRE(nwg < (1LL << 31), PTA_E_ARG, "pta_engine_chrom_add: R=%d too large for one launch (%lld workgroups)", R, (long long)nwg);
  const size_t shmem = (size_t)PTA_CHROM_RG * PTA_CHROM_PITCH * sizeof(double);
  const dim3 grid((unsigned)nwg), block(PTA_ENGINE_TILE);
  hipStream_t s = pta_stream(stream);
  if (accumulate) {
    if (shmem > 65536) PTA_HIP(hipFuncSetAttribute((const void *)k_engine_chrom_add<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
    hipLaunchKernelGGL((k_engine_chrom_add<true>), grid, block, shmem, s, p.tile_psr, p.tile_start, p.tile_count, p.n_tiles, ch.Ft, ch.ldf, ch.coef,
                       ch.k, p.n_psr, R, out, ld_out);
  } else {
    if (shmem > 65536) PTA_HIP(hipFuncSetAttribute((const void *)k_engine_chrom_add<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
    hipLaunchKernelGGL((k_engine_chrom_add<false>), grid, block, shmem, s, p.tile_psr, p.tile_start, p.tile_count, p.n_tiles, ch.Ft, ch.ldf, ch.coef,
                       ch.k, p.n_psr, R, out, ld_out);
  }
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}
