// A catalogue of S continuous-wave sources per realisation (theta's cw_* keys of shape [R, S], set_cw_prior(n_sources=S)):
//   pta_cw_catalog_uniform        labels [R, S, 8] drawn on chip, source s from stream (CW, s), pair = label column: the shared box draw
//                                 (pta_box_kernels.hip) with S sources
//   pta_engine_cw_catalog_params  table [R][P][S][NPAR], one thread per (realisation, pulsar, source) below the realisation's count
//   pta_engine_cw_catalog_add     the catalogue's sum over the engine's TOA tiles x groups of realisations: a register accumulator over
//                                 the sources in ascending order, then ONE read-modify-write of out[R, n_toa]: k_engine_term_add
//                                 (pta_engine_term.h) with cwc_term
// Formulas and table layout: pta_cw_catalog.h.  No atomics, no split over the sources and a fixed operation order per element: a
// realisation's catalogue term is the same in every batch.
#include "pta_common.h"
#include "pta_rng.h"
#include "pta_cw_catalog.h"
#include "pta_engine_term.h"

#define CWC_ADD_RG 4  // realisations per workgroup of the sum kernel (each walks up to S sources)

static_assert(PTA_CW_CATALOG_NPAR_EVOLVE == PTA_CW_ENGINE_NPAR, "the evolving table row is pta_cw_params' row");

extern "C" int pta_cw_catalog_uniform(uint64_t seed, uint64_t r0, int R, int S, const double *lo, const double *hi, double *out, void *stream) {
  PTA_REQUIRE(lo && hi && out, PTA_E_ARG, "pta_cw_catalog_uniform: NULL argument");
  PTA_REQUIRE(R > 0 && S > 0 && (int64_t)S - 1 <= 0xFFFFFF, PTA_E_ARG, "pta_cw_catalog_uniform: R=%d S=%d", R, S);
  const int64_t total = (int64_t)R * S * PTA_CW_NSRC;
  PTA_REQUIRE(total < (1LL << 31), PTA_E_ARG, "pta_cw_catalog_uniform: problem too large");
  return pta_box_uniform_launch(seed, r0, R, S, PTA_CW_NSRC, PTA_STREAM_CW, 0u, lo, hi, out, pta_stream(stream));
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

// the term of k_engine_term_add (pta_engine_term.h): the sum over the evaluated sources of realisation r at pulsar a, a register
// accumulator in ascending source order.  A lane's value depends on its own (r, a, TOA, sources) alone.
template <int MODE, int PSR_TERM>
struct cwc_term {
  const double *__restrict__ par;
  const int32_t *__restrict__ count;
  int P, S;
  __device__ double value(int r, int a, double t) const {
    constexpr int NPAR = MODE == 0 ? PTA_CW_CATALOG_NPAR_EVOLVE : PTA_CW_CATALOG_NPAR_FOLDED;
    return pta_cw_catalog_sum<MODE, PSR_TERM>(par + ((int64_t)r * P + a) * S * NPAR, cwc_count(count, r, S), t);
  }
};

extern "C" int pta_engine_cw_catalog_add(const pta_engine_plan *plan_host, const pta_cw_catalog_engine *cw_host, int R, double *out,
                                         int64_t ld_out, int accumulate, void *stream) {
  PTA_REQUIRE(plan_host && cw_host && out, PTA_E_ARG, "pta_engine_cw_catalog_add: NULL argument");
  const pta_engine_plan &p = *plan_host;
  const pta_cw_catalog_engine &cw = *cw_host;
  const int bad = pta_term_add_refusal(p, cw.toa_s, cw.par, cw.n_psr, ld_out, cw.mode, R, CWC_ADD_RG);
  PTA_REQUIRE(bad != 1, PTA_E_ARG, "pta_engine_cw_catalog_add: tiles / TOAs / table missing");
  const int rc = cwc_check(cw, R, "pta_engine_cw_catalog_add");
  if (rc != PTA_OK) return rc;
  PTA_REQUIRE(bad != 2, PTA_E_ARG, "pta_engine_cw_catalog_add: n_tiles=%d n_psr=%d/%d ld_out=%lld n_toa=%d", p.n_tiles, cw.n_psr, p.n_psr,
              (long long)ld_out, p.n_toa);
  PTA_REQUIRE(bad != 3, PTA_E_ARG, "pta_engine_cw_catalog_add: R=%d too large for one launch", R);
  return pta_term_add_launch<cwc_term, CWC_ADD_RG>(p, cw.toa_s, cw.tref, cw.mode, cw.psr_term, R, out, ld_out, accumulate, stream, cw.par, cw.count,
                                                   p.n_psr, cw.n_src);
}
