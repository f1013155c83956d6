// One continuous-wave source per realisation (ReplicaEngine.set_cw + theta cw_* keys, set_cw_prior + generate_sampled):
//   pta_cw_uniform        CW labels drawn on chip from uniform boxes, stream (CW, 0), pair = label column: keyed by (seed, realisation)
//   pta_engine_cw_params  [R, P, PTA_CW_ENGINE_NPAR] scalar table, one thread per (realisation, pulsar)
//   pta_engine_cw_add     the waveform over the engine's TOA tiles x groups of realisations, added into (or written to) out[R, n_toa]
// Formulas: pta_cw_hyper.h.  No atomics and a fixed operation order per element: a realisation's CW term is the same in every batch.
#include "pta_common.h"
#include "pta_rng.h"
#include "pta_cw_hyper.h"

#define CW_ADD_RG 16  // realisations per workgroup of the waveform kernel

__global__ void k_cw_uniform(uint64_t seed, uint64_t r0, int R, int n_par, const double *__restrict__ lo, const double *__restrict__ hi,
                             double *__restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)R * n_par) return;
  const int j = (int)(idx % n_par);
  const int64_t r = idx / n_par;
  out[idx] = pta_cw_draw(seed, r0 + (uint64_t)r, (uint32_t)j, lo[j], hi[j]);
}

extern "C" int pta_cw_uniform(uint64_t seed, uint64_t r0, int R, int n_par, const double *lo, const double *hi, double *out, void *stream) {
  PTA_REQUIRE(lo && hi && out, PTA_E_ARG, "pta_cw_uniform: NULL argument");
  PTA_REQUIRE(R > 0 && n_par > 0, PTA_E_ARG, "pta_cw_uniform: R=%d n_par=%d", R, n_par);
  const int64_t total = (int64_t)R * n_par;
  PTA_REQUIRE(total < (1LL << 31), PTA_E_ARG, "pta_cw_uniform: problem too large");
  hipLaunchKernelGGL(k_cw_uniform, dim3(pta_cdiv(total, 256)), dim3(256), 0, pta_stream(stream), seed, r0, R, n_par, lo, hi, out);
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}

__global__ void k_engine_cw_params(pta_cw_engine cw, int R) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // (r, a)
  if (idx >= (int64_t)R * cw.n_psr) return;
  const int a = (int)(idx % cw.n_psr);
  const int64_t r = idx / cw.n_psr;
  const double *src = cw.src + r * cw.ld_src;
  const double pd = cw.has_pdist ? src[PTA_CW_COL_PDIST + a] : cw.pdist[a];
  pta_cw_params(src, cw.amp_is_h, cw.phat + 3 * a, pd, cw.mode, cw.par + idx * PTA_CW_ENGINE_NPAR);
}

extern "C" int pta_engine_cw_params(const pta_cw_engine *cw_host, int R, void *stream) {
  PTA_REQUIRE(cw_host, PTA_E_ARG, "pta_engine_cw_params: NULL argument");
  const pta_cw_engine &cw = *cw_host;
  PTA_REQUIRE(cw.src && cw.phat && cw.par && (cw.has_pdist || cw.pdist), PTA_E_ARG, "pta_engine_cw_params: NULL table");
  PTA_REQUIRE(R > 0 && cw.n_psr > 0 && cw.mode >= 0 && cw.mode <= 2, PTA_E_ARG, "pta_engine_cw_params: R=%d n_psr=%d mode=%d", R,
              cw.n_psr, cw.mode);
  PTA_REQUIRE(cw.ld_src >= PTA_CW_NSRC + (cw.has_pdist ? cw.n_psr : 0), PTA_E_ARG, "pta_engine_cw_params: ld_src=%lld too small",
              (long long)cw.ld_src);
  const int64_t total = (int64_t)R * cw.n_psr;
  PTA_REQUIRE(total < (1LL << 31), PTA_E_ARG, "pta_engine_cw_params: problem too large");
  hipLaunchKernelGGL(k_engine_cw_params, dim3(pta_cdiv(total, 128)), dim3(128), 0, pta_stream(stream), cw, R);
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}

// workgroup = one engine tile (<= PTA_ENGINE_TILE consecutive TOAs of one pulsar) x CW_ADD_RG realisations; lanes run over the TOAs,
// the (r, a) scalars are the same for the whole workgroup (scalar loads)
template <int MODE, int PSR_TERM>
__global__ __launch_bounds__(PTA_ENGINE_TILE) void k_engine_cw_add(const int32_t *__restrict__ tile_psr, const int32_t *__restrict__ tile_start,
                                                                   const int32_t *__restrict__ tile_count, const double *__restrict__ toa_s,
                                                                   double tref, const double *__restrict__ par, int P, int R,
                                                                   double *__restrict__ out, int64_t ld_out, int accumulate) {
  const int tile = blockIdx.x;
  const int i = threadIdx.x;
  if (i >= tile_count[tile]) return;  // no barriers below
  const int a = tile_psr[tile];
  const int64_t col = (int64_t)tile_start[tile] + i;
  const double t = toa_s[col] - tref;  // mjd * 86400 - tref, rounded as deterministic.py:98 rounds it
  const int r0 = blockIdx.y * CW_ADD_RG, r1 = min(R, r0 + CW_ADD_RG);
  for (int r = r0; r < r1; ++r) {
    const double v = pta_cw_wave<MODE, PSR_TERM>(par + ((int64_t)r * P + a) * PTA_CW_ENGINE_NPAR, t);
    double *o = out + (int64_t)r * ld_out + col;
    *o = accumulate ? *o + v : v;
  }
}

extern "C" int pta_engine_cw_add(const pta_engine_plan *plan_host, const pta_cw_engine *cw_host, int R, double *out, int64_t ld_out,
                                 int accumulate, void *stream) {
  PTA_REQUIRE(plan_host && cw_host && out, PTA_E_ARG, "pta_engine_cw_add: NULL argument");
  const pta_engine_plan &p = *plan_host;
  const pta_cw_engine &cw = *cw_host;
  PTA_REQUIRE(p.tile_psr && p.tile_start && p.tile_count && cw.toa_s && cw.par, PTA_E_ARG, "pta_engine_cw_add: tiles / TOAs / table missing");
  PTA_REQUIRE(R > 0 && p.n_tiles > 0 && cw.n_psr == p.n_psr && ld_out >= p.n_toa && cw.mode >= 0 && cw.mode <= 2, PTA_E_ARG,
              "pta_engine_cw_add: R=%d n_tiles=%d n_psr=%d/%d ld_out=%lld mode=%d", R, p.n_tiles, cw.n_psr, p.n_psr, (long long)ld_out,
              cw.mode);
  const unsigned groups = pta_cdiv(R, CW_ADD_RG);
  PTA_REQUIRE(groups <= 65535, PTA_E_ARG, "pta_engine_cw_add: R=%d too large for one launch", R);
  const dim3 grid(p.n_tiles, groups), block(PTA_ENGINE_TILE);
  hipStream_t s = pta_stream(stream);
  const int acc = accumulate ? 1 : 0;
#define CW_LAUNCH(M, T)                                                                                                                 \
  hipLaunchKernelGGL((k_engine_cw_add<M, T>), grid, block, 0, s, p.tile_psr, p.tile_start, p.tile_count, cw.toa_s, cw.tref, cw.par, \
                     p.n_psr, R, out, ld_out, acc)
  const int pt = cw.psr_term ? 1 : 0;
  if (cw.mode == 0) {
    if (pt) CW_LAUNCH(0, 1); else CW_LAUNCH(0, 0);
  } else if (cw.mode == 1) {
    if (pt) CW_LAUNCH(1, 1); else CW_LAUNCH(1, 0);
  } else {
    if (pt) CW_LAUNCH(2, 1); else CW_LAUNCH(2, 0);
  }
#undef CW_LAUNCH
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}
