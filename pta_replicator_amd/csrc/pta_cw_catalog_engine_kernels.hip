// A catalogue of S continuous-wave sources per realisation (theta's cw_* keys of shape [R, S], set_cw_prior(n_sources=S)):
//   pta_cw_catalog_uniform        labels [R, S, 8] drawn on chip, source s from stream (CW, s), pair = label column
//   pta_engine_cw_catalog_params  table [R][P][S][NPAR], one thread per (realisation, pulsar, source) below the realisation's count
//   pta_engine_cw_catalog_add     the catalogue's sum over the engine's TOA tiles x groups of realisations: a register accumulator over
//                                 the sources in ascending order, then ONE read-modify-write of out[R, n_toa]
// Formulas and table layout: pta_cw_catalog.h.  No atomics, no split over the sources and a fixed operation order per element: a
// realisation's catalogue term is the same in every batch.
#include "pta_common.h"
#include "pta_rng.h"
#include "pta_cw_catalog.h"

#define CWC_ADD_RG 4  // realisations per workgroup of the sum kernel (each walks up to S sources)

static_assert(PTA_CW_CATALOG_NPAR_EVOLVE == PTA_CW_ENGINE_NPAR, "the evolving table row is pta_cw_params' row");

__global__ void k_cw_catalog_uniform(uint64_t seed, uint64_t r0, int R, int S, const double *__restrict__ lo, const double *__restrict__ hi,
                                     double *__restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // (r, s, j)
  if (idx >= (int64_t)R * S * PTA_CW_NSRC) return;
  const int j = (int)(idx % PTA_CW_NSRC);
  const int64_t rs = idx / PTA_CW_NSRC;
  const uint32_t s = (uint32_t)(rs % S);
  const int64_t r = rs / S;
  out[idx] = pta_cw_catalog_draw(seed, r0 + (uint64_t)r, s, (uint32_t)j, lo[j], hi[j]);
}

extern "C" int pta_cw_catalog_uniform(uint64_t seed, uint64_t r0, int R, int S, const double *lo, const double *hi, double *out, void *stream) {
  PTA_REQUIRE(lo && hi && out, PTA_E_ARG, "pta_cw_catalog_uniform: NULL argument");
  PTA_REQUIRE(R > 0 && S > 0 && (int64_t)S - 1 <= 0xFFFFFF, PTA_E_ARG, "pta_cw_catalog_uniform: R=%d S=%d", R, S);
  const int64_t total = (int64_t)R * S * PTA_CW_NSRC;
  PTA_REQUIRE(total < (1LL << 31), PTA_E_ARG, "pta_cw_catalog_uniform: problem too large");
  hipLaunchKernelGGL(k_cw_catalog_uniform, dim3(pta_cdiv(total, 256)), dim3(256), 0, pta_stream(stream), seed, r0, R, S, lo, hi, out);
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}

// the number of sources of realisation r that are evaluated: count[r] clamped to 0 .. S (the host validates it; the clamp keeps a
// table walk inside the table whatever the array holds), S without a count array
__device__ __forceinline__ int cwc_count(const int32_t *__restrict__ count, int64_t r, int S) {
  return count ? min(max(count[r], 0), S) : S;
}

__global__ void k_engine_cw_catalog_params(pta_cw_catalog_engine cw, int R) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // (r, a, s): the table's own order
  const int S = cw.n_src, P = cw.n_psr;
  if (idx >= (int64_t)R * P * S) return;
  const int s = (int)(idx % S);
  const int64_t ra = idx / S;
  const int a = (int)(ra % P);
  const int64_t r = ra / P;
  if (s >= cwc_count(cw.count, r, S)) return;  // entries past the count are never read
  const double *src = cw.src + r * cw.ld_src + (int64_t)s * PTA_CW_NSRC;
  const double pd = cw.has_pdist ? cw.pdist[r * cw.ld_pdist + a] : cw.pdist[a];
  pta_cw_catalog_params(src, cw.amp_is_h, cw.phat + 3 * a, pd, cw.mode, cw.psr_term, cw.par + idx * pta_cw_catalog_npar(cw.mode));
}

// the argument classes shared by the two engine entries
static int cwc_check(const pta_cw_catalog_engine &cw, int R, const char *who) {
  PTA_REQUIRE(R > 0 && cw.n_psr > 0 && cw.n_src > 0 && cw.mode >= 0 && cw.mode <= 2, PTA_E_ARG, "%s: R=%d n_psr=%d n_src=%d mode=%d", who, R,
              cw.n_psr, cw.n_src, cw.mode);
  PTA_REQUIRE((int64_t)cw.n_src - 1 <= 0xFFFFFF, PTA_E_ARG, "%s: n_src=%d does not fit the 24-bit stream field", who, cw.n_src);
  PTA_REQUIRE((int64_t)R * cw.n_psr * cw.n_src < (1LL << 31), PTA_E_ARG, "%s: problem too large", who);
  return PTA_OK;
}

extern "C" int pta_engine_cw_catalog_params(const pta_cw_catalog_engine *cw_host, int R, void *stream) {
  PTA_REQUIRE(cw_host, PTA_E_ARG, "pta_engine_cw_catalog_params: NULL argument");
  const pta_cw_catalog_engine &cw = *cw_host;
  PTA_REQUIRE(cw.src && cw.phat && cw.par && cw.pdist, PTA_E_ARG, "pta_engine_cw_catalog_params: NULL table");
  const int rc = cwc_check(cw, R, "pta_engine_cw_catalog_params");
  if (rc != PTA_OK) return rc;
  PTA_REQUIRE(cw.ld_src >= (int64_t)PTA_CW_NSRC * cw.n_src, PTA_E_ARG, "pta_engine_cw_catalog_params: ld_src=%lld too small",
              (long long)cw.ld_src);
  PTA_REQUIRE(!cw.has_pdist || cw.ld_pdist >= cw.n_psr, PTA_E_ARG, "pta_engine_cw_catalog_params: ld_pdist=%lld too small",
              (long long)cw.ld_pdist);
  const int64_t total = (int64_t)R * cw.n_psr * cw.n_src;
  hipLaunchKernelGGL(k_engine_cw_catalog_params, dim3(pta_cdiv(total, 128)), dim3(128), 0, pta_stream(stream), cw, R);
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}

// workgroup = one engine tile (<= PTA_ENGINE_TILE consecutive TOAs of one pulsar) x CWC_ADD_RG realisations; lanes run over the TOAs,
// the (r, a, s) scalars are the same for the whole workgroup (scalar loads).  A lane's value depends on its own (r, a, TOA, sources)
// alone.
template <int MODE, int PSR_TERM>
__global__ __launch_bounds__(PTA_ENGINE_TILE) void k_engine_cw_catalog_add(
    const int32_t *__restrict__ tile_psr, const int32_t *__restrict__ tile_start, const int32_t *__restrict__ tile_count,
    const double *__restrict__ toa_s, double tref, const double *__restrict__ par, const int32_t *__restrict__ count, int P, int S, int R,
    double *__restrict__ out, int64_t ld_out, int accumulate) {
  const int tile = blockIdx.x;
  const int i = threadIdx.x;
  if (i >= tile_count[tile]) return;  // no barriers below
  const int a = tile_psr[tile];
  const int64_t col = (int64_t)tile_start[tile] + i;
  const double t = toa_s[col] - tref;  // mjd * 86400 - tref, rounded as deterministic.py:98 rounds it
  constexpr int NPAR = MODE == 0 ? PTA_CW_CATALOG_NPAR_EVOLVE : PTA_CW_CATALOG_NPAR_FOLDED;
  const int r0 = blockIdx.y * CWC_ADD_RG, r1 = min(R, r0 + CWC_ADD_RG);
  for (int r = r0; r < r1; ++r) {
    const int n = cwc_count(count, r, S);
    const double v = pta_cw_catalog_sum<MODE, PSR_TERM>(par + ((int64_t)r * P + a) * S * NPAR, n, t);
    double *o = out + (int64_t)r * ld_out + col;
    *o = accumulate ? *o + v : v;
  }
}

extern "C" int pta_engine_cw_catalog_add(const pta_engine_plan *plan_host, const pta_cw_catalog_engine *cw_host, int R, double *out,
                                         int64_t ld_out, int accumulate, void *stream) {
  PTA_REQUIRE(plan_host && cw_host && out, PTA_E_ARG, "pta_engine_cw_catalog_add: NULL argument");
  const pta_engine_plan &p = *plan_host;
  const pta_cw_catalog_engine &cw = *cw_host;
  PTA_REQUIRE(p.tile_psr && p.tile_start && p.tile_count && cw.toa_s && cw.par, PTA_E_ARG,
              "pta_engine_cw_catalog_add: tiles / TOAs / table missing");
  const int rc = cwc_check(cw, R, "pta_engine_cw_catalog_add");
  if (rc != PTA_OK) return rc;
  PTA_REQUIRE(p.n_tiles > 0 && cw.n_psr == p.n_psr && ld_out >= p.n_toa, PTA_E_ARG,
              "pta_engine_cw_catalog_add: n_tiles=%d n_psr=%d/%d ld_out=%lld n_toa=%d", p.n_tiles, cw.n_psr, p.n_psr, (long long)ld_out,
              p.n_toa);
  const unsigned groups = pta_cdiv(R, CWC_ADD_RG);
  PTA_REQUIRE(groups <= 65535, PTA_E_ARG, "pta_engine_cw_catalog_add: R=%d too large for one launch", R);
  const dim3 grid(p.n_tiles, groups), block(PTA_ENGINE_TILE);
  hipStream_t s = pta_stream(stream);
  const int acc = accumulate ? 1 : 0;
#define CWC_LAUNCH(M, T)                                                                                                            \
  hipLaunchKernelGGL((k_engine_cw_catalog_add<M, T>), grid, block, 0, s, p.tile_psr, p.tile_start, p.tile_count, cw.toa_s, cw.tref, \
                     cw.par, cw.count, p.n_psr, cw.n_src, R, out, ld_out, acc)
  const int pt = cw.psr_term ? 1 : 0;
  if (cw.mode == 0) {
    if (pt) CWC_LAUNCH(0, 1); else CWC_LAUNCH(0, 0);
  } else if (cw.mode == 1) {
    if (pt) CWC_LAUNCH(1, 1); else CWC_LAUNCH(1, 0);
  } else {
    if (pt) CWC_LAUNCH(2, 1); else CWC_LAUNCH(2, 0);
  }
#undef CWC_LAUNCH
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}
