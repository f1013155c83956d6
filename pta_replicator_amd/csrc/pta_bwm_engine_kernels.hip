// One burst with memory per realisation (ReplicaEngine.set_bwm + theta bwm_* keys, set_bwm_prior + generate_sampled):
//   pta_bwm_uniform        burst labels drawn on chip from uniform boxes, stream (BWM, 0), pair = label column: keyed by (seed, realisation);
//                          the shared box draw (pta_box_kernels.hip)
//   pta_engine_bwm_params  coef[R, P] = pol * strain, one thread per (realisation, pulsar), and t0_s[R]
//   pta_engine_bwm_add     the ramp over the engine's TOA tiles x groups of realisations, added into (or written to) out[R, n_toa]
// Formulas: pta_bwm.h.  No atomics and one fixed operation per element: a realisation's term is the same in every batch.
#include "pta_common.h"
#include "pta_rng.h"
#include "pta_bwm.h"

#define BWM_ADD_RG 16  // realisations per workgroup of the ramp kernel: two half-workgroups x two batches of BWM_ADD_U rows
#define BWM_ADD_U 4    // rows a lane has in flight: 4 x 16 bytes per lane, 16 KiB per workgroup

extern "C" int pta_bwm_uniform(uint64_t seed, uint64_t r0, int R, const double *lo, const double *hi, double *out, void *stream) {
  PTA_REQUIRE(lo && hi && out, PTA_E_ARG, "pta_bwm_uniform: NULL argument");
  PTA_REQUIRE(R > 0, PTA_E_ARG, "pta_bwm_uniform: R=%d", R);
  const int64_t total = (int64_t)R * PTA_BWM_NSRC;
  PTA_REQUIRE(total < (1LL << 31), PTA_E_ARG, "pta_bwm_uniform: problem too large");
  return pta_box_uniform_launch(seed, r0, R, 1, PTA_BWM_NSRC, PTA_STREAM_BWM, 0u, lo, hi, out, pta_stream(stream));
}

__global__ void k_engine_bwm_params(pta_bwm_engine bw, int R) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // (r, a)
  if (idx >= (int64_t)R * bw.n_psr) return;
  const int a = (int)(idx % bw.n_psr);
  const int64_t r = idx / bw.n_psr;
  const double *src = bw.src + r * bw.ld_src;
  bw.coef[idx] = pta_bwm_coef(src, bw.phat + 3 * a);
  if (a == 0) bw.t0_s[r] = pta_bwm_t0(src);
}

extern "C" int pta_engine_bwm_params(const pta_bwm_engine *bwm_host, int R, void *stream) {
  PTA_REQUIRE(bwm_host, PTA_E_ARG, "pta_engine_bwm_params: NULL argument");
  const pta_bwm_engine &bw = *bwm_host;
  PTA_REQUIRE(bw.src && bw.phat && bw.coef && bw.t0_s, PTA_E_ARG, "pta_engine_bwm_params: NULL table");
  PTA_REQUIRE(R > 0 && bw.n_psr > 0, PTA_E_ARG, "pta_engine_bwm_params: R=%d n_psr=%d", R, bw.n_psr);
  PTA_REQUIRE(bw.ld_src >= PTA_BWM_NSRC, PTA_E_ARG, "pta_engine_bwm_params: ld_src=%lld too small", (long long)bw.ld_src);
  const int64_t total = (int64_t)R * bw.n_psr;
  PTA_REQUIRE(total < (1LL << 31), PTA_E_ARG, "pta_engine_bwm_params: problem too large");
  hipLaunchKernelGGL(k_engine_bwm_params, dim3(pta_cdiv(total, 128)), dim3(128), 0, pta_stream(stream), bw, R);
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}

// workgroup = one engine tile (<= PTA_ENGINE_TILE consecutive TOAs of one pulsar) x BWM_ADD_RG realisations.  A half-workgroup (two
// waves, 128 lanes) owns a row of the tile: lane p holds two adjacent TOAs and moves them with one 16-byte access.  Pulsar offsets,
// ld_out and out itself are arbitrary, so a row's first element may sit on an odd 8-byte slot: its pairs then start one element
// later (lane p takes elements 2 p + 1, 2 p + 2), lane 0 moves the head alone, and an odd element left at the end is moved alone
// by the lane it falls to.  The three TOAs a lane can need stay in registers; coef[r, a] and t0[r] are uniform over the half
// (scalar loads).  The rows of a half are walked BWM_ADD_U at a time, all loads issued before the first store.  Every element is
// ramp(coef, t0, t) (pta_bwm.h), added once or written: the same value on the pair, head and tail paths.
template <bool ACC>
__global__ __launch_bounds__(PTA_ENGINE_TILE) void k_engine_bwm_add(const int32_t *__restrict__ tile_psr, const int32_t *__restrict__ tile_start,
                                                                    const int32_t *__restrict__ tile_count, const double *__restrict__ toa_s,
                                                                    const double *__restrict__ coef, const double *__restrict__ t0_s, int P, int R,
                                                                    double *__restrict__ out, int64_t ld_out) {
  static_assert(PTA_ENGINE_TILE == 256, "k_engine_bwm_add: a half-workgroup of 128 lanes covers a tile in pairs");
  const int tile = blockIdx.x;
  const int cnt = tile_count[tile];
  const int a = tile_psr[tile];
  const int64_t c0 = tile_start[tile];
  const int p = threadIdx.x & 127;
  const int hb = __builtin_amdgcn_readfirstlane(threadIdx.x >> 7);  // uniform over the wave
  const double *ts = toa_s + c0;
  const double ta = 2 * p < cnt ? ts[2 * p] : 0.0, tb = 2 * p + 1 < cnt ? ts[2 * p + 1] : 0.0, tc = 2 * p + 2 < cnt ? ts[2 * p + 2] : 0.0;
  const int r_lo = blockIdx.y * BWM_ADD_RG, r_hi = min(R, r_lo + BWM_ADD_RG);
  for (int rb = r_lo + hb; rb < r_hi; rb += 2 * BWM_ADD_U) {
    double cf[BWM_ADD_U], t0[BWM_ADD_U], oh[BWM_ADD_U];
    double *row[BWM_ADD_U];
    double2 o[BWM_ADD_U];
    int kind[BWM_ADD_U], head[BWM_ADD_U];  // kind: 0 nothing, 1 a pair, 2 a single element at head + 2 p
#pragma unroll
    for (int u = 0; u < BWM_ADD_U; ++u) {
      const int r = rb + 2 * u;
      const bool live = r < r_hi;
      const int rr = live ? r : r_hi - 1;  // a clamped read that is never used
      cf[u] = coef[(int64_t)rr * P + a];
      t0[u] = t0_s[rr];
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
    for (int u = 0; u < BWM_ADD_U; ++u) {
      const int sh = (int)(((uintptr_t)row[u] >> 3) & 1);
      const int i = sh + 2 * p;
      const double vx = pta_bwm_ramp(cf[u], t0[u], sh ? tb : ta), vy = pta_bwm_ramp(cf[u], t0[u], sh ? tc : tb);
      if (kind[u] == 1) *reinterpret_cast<double2 *>(row[u] + i) = ACC ? double2{o[u].x + vx, o[u].y + vy} : double2{vx, vy};
      else if (kind[u] == 2) row[u][i] = ACC ? o[u].x + vx : vx;
      if (head[u]) {
        const double vh = pta_bwm_ramp(cf[u], t0[u], ta);
        row[u][0] = ACC ? oh[u] + vh : vh;
      }
    }
  }
}

extern "C" int pta_engine_bwm_add(const pta_engine_plan *plan_host, const pta_bwm_engine *bwm_host, int R, double *out, int64_t ld_out,
                                  int accumulate, void *stream) {
  PTA_REQUIRE(plan_host && bwm_host && out, PTA_E_ARG, "pta_engine_bwm_add: NULL argument");
  const pta_engine_plan &p = *plan_host;
  const pta_bwm_engine &bw = *bwm_host;
  PTA_REQUIRE(p.tile_psr && p.tile_start && p.tile_count && bw.toa_s && bw.coef && bw.t0_s, PTA_E_ARG,
              "pta_engine_bwm_add: tiles / TOAs / table missing");
  PTA_REQUIRE(R > 0 && p.n_tiles > 0 && bw.n_psr == p.n_psr && ld_out >= p.n_toa, PTA_E_ARG,
              "pta_engine_bwm_add: R=%d n_tiles=%d n_psr=%d/%d ld_out=%lld", R, p.n_tiles, bw.n_psr, p.n_psr, (long long)ld_out);
  PTA_REQUIRE(((uintptr_t)out & 7) == 0, PTA_E_ARG, "pta_engine_bwm_add: out must be 8-byte aligned");
  const unsigned groups = pta_cdiv(R, BWM_ADD_RG);
  PTA_REQUIRE(groups <= 65535, PTA_E_ARG, "pta_engine_bwm_add: R=%d too large for one launch", R);
  const dim3 grid(p.n_tiles, groups), block(PTA_ENGINE_TILE);
  hipStream_t s = pta_stream(stream);
  if (accumulate)
    hipLaunchKernelGGL((k_engine_bwm_add<true>), grid, block, 0, s, p.tile_psr, p.tile_start, p.tile_count, bw.toa_s, bw.coef, bw.t0_s, p.n_psr, R,
                       out, ld_out);
  else
    hipLaunchKernelGGL((k_engine_bwm_add<false>), grid, block, 0, s, p.tile_psr, p.tile_start, p.tile_count, bw.toa_s, bw.coef, bw.t0_s, p.n_psr, R,
                       out, ld_out);
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}
