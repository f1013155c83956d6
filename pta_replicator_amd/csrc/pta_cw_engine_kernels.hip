// One continuous-wave source per realisation (ReplicaEngine.set_cw + theta cw_* keys, set_cw_prior + generate_sampled):
//   pta_cw_uniform        CW labels drawn on chip from uniform boxes, stream (CW, 0), pair = label column: keyed by (seed, realisation);
//                         the shared box draw (pta_box_kernels.hip)
//   pta_engine_cw_params  [R, P, PTA_CW_ENGINE_NPAR] scalar table, one thread per (realisation, pulsar)
//   pta_engine_cw_add     the waveform over the engine's TOA tiles x groups of realisations, added into (or written to) out[R, n_toa]:
//                         k_engine_term_add (pta_engine_term.h) with cw_term
// Formulas: pta_cw_hyper.h.  No atomics and a fixed operation order per element: a realisation's CW term is the same in every batch.
#include "pta_common.h"
#include "pta_rng.h"
#include "pta_cw_hyper.h"
#include "pta_engine_term.h"

#define CW_ADD_RG 16  // realisations per workgroup of the waveform kernel

extern "C" int pta_cw_uniform(uint64_t seed, uint64_t r0, int R, int n_par, const double *lo, const double *hi, double *out, void *stream) {
  PTA_REQUIRE(lo && hi && out, PTA_E_ARG, "pta_cw_uniform: NULL argument");
  PTA_REQUIRE(R > 0 && n_par > 0, PTA_E_ARG, "pta_cw_uniform: R=%d n_par=%d", R, n_par);
  const int64_t total = (int64_t)R * n_par;
  PTA_REQUIRE(total < (1LL << 31), PTA_E_ARG, "pta_cw_uniform: problem too large");
  return pta_box_uniform_launch(seed, r0, R, 1, n_par, PTA_STREAM_CW, 0u, lo, hi, out, pta_stream(stream));
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

// the term of k_engine_term_add (pta_engine_term.h): the waveform of the one source of realisation r at pulsar a, from row (r, a) of the
// scalar table
template <int MODE, int PSR_TERM>
struct cw_term {
  const double *__restrict__ par;
  int P;
  __device__ double value(int r, int a, double t) const { return pta_cw_wave<MODE, PSR_TERM>(par + ((int64_t)r * P + a) * PTA_CW_ENGINE_NPAR, t); }
};

extern "C" int pta_engine_cw_add(const pta_engine_plan *plan_host, const pta_cw_engine *cw_host, int R, double *out, int64_t ld_out,
                                 int accumulate, void *stream) {
  PTA_REQUIRE(plan_host && cw_host && out, PTA_E_ARG, "pta_engine_cw_add: NULL argument");
  const pta_engine_plan &p = *plan_host;
  const pta_cw_engine &cw = *cw_host;
  const int bad = pta_term_add_refusal(p, cw.toa_s, cw.par, cw.n_psr, ld_out, cw.mode, R, CW_ADD_RG);
  PTA_REQUIRE(bad != 1, PTA_E_ARG, "pta_engine_cw_add: tiles / TOAs / table missing");
  PTA_REQUIRE(R > 0 && bad != 2, PTA_E_ARG, "pta_engine_cw_add: R=%d n_tiles=%d n_psr=%d/%d ld_out=%lld mode=%d", R, p.n_tiles, cw.n_psr,
              p.n_psr, (long long)ld_out, cw.mode);
  PTA_REQUIRE(bad != 3, PTA_E_ARG, "pta_engine_cw_add: R=%d too large for one launch", R);
  return pta_term_add_launch<cw_term, CW_ADD_RG>(p, cw.toa_s, cw.tref, cw.mode, cw.psr_term, R, out, ld_out, accumulate, stream, cw.par, p.n_psr);
}
