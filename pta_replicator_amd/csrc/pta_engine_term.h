// The tile walk the per-realisation waveform terms share (pta_engine_cw_add: one source, RG = 16; pta_engine_cw_catalog_add: the sum of
// a catalogue, RG = 4), the checks their entries have in common and the (mode, psr_term) dispatch.
#pragma once
#include "pta_common.h"

// workgroup = one engine tile (<= PTA_ENGINE_TILE consecutive TOAs of one pulsar) x RG realisations; lanes run over the TOAs, the
// scalars term.value(r, a, .) reads are the same for the whole workgroup (scalar loads).  Term: a trivially copyable struct, value(r, a,
// t) = the term of realisation r (row of out) for pulsar a at t.  No atomics, one read-modify-write per element.
template <class Term, int RG>
__global__ __launch_bounds__(PTA_ENGINE_TILE) void k_engine_term_add(const int32_t *__restrict__ tile_psr, const int32_t *__restrict__ tile_start,
                                                                     const int32_t *__restrict__ tile_count, const double *__restrict__ toa_s,
                                                                     double tref, Term term, int R, double *__restrict__ out, int64_t ld_out,
                                                                     int accumulate) {
  const int tile = blockIdx.x;
  const int i = threadIdx.x;
  if (i >= tile_count[tile]) return;  // no barriers below
  const int a = tile_psr[tile];
  const int64_t col = (int64_t)tile_start[tile] + i;
  const double t = toa_s[col] - tref;  // mjd * 86400 - tref, rounded as deterministic.py:98 rounds it
  const int r0 = blockIdx.y * RG, r1 = min(R, r0 + RG);
  for (int r = r0; r < r1; ++r) {
    const double v = term.value(r, a, t);
    double *o = out + (int64_t)r * ld_out + col;
    *o = accumulate ? *o + v : v;
  }
}

// the first check of a term's add entry that fails, 0 = none; the entry words the refusal: 1 = tiles / TOAs / table missing, 2 = the
// plan has no tiles, another pulsar count or more TOAs than a row of out, or mode is none of 0 .. 2, 3 = too many groups for one launch
static inline int pta_term_add_refusal(const pta_engine_plan &p, const double *toa_s, const double *par, int n_psr, int64_t ld_out, int mode,
                                       int R, int RG) {
  if (!(p.tile_psr && p.tile_start && p.tile_count && toa_s && par)) return 1;
  if (!(p.n_tiles > 0 && n_psr == p.n_psr && ld_out >= p.n_toa && mode >= 0 && mode <= 2)) return 2;
  return pta_cdiv(R, RG) <= 65535 ? 0 : 3;
}

// k_engine_term_add<Term<mode, psr_term>, RG> over the plan's tiles x groups of RG realisations, Term<.,.>{fields...}
template <template <int, int> class Term, int RG, class... Fields>
static int pta_term_add_launch(const pta_engine_plan &p, const double *toa_s, double tref, int mode, int psr_term, int R, double *out,
                               int64_t ld_out, int accumulate, void *stream, Fields... fields) {
  const dim3 grid(p.n_tiles, pta_cdiv(R, RG)), block(PTA_ENGINE_TILE);
  hipStream_t s = pta_stream(stream);
  const int acc = accumulate ? 1 : 0;
#define PTA_TERM_LAUNCH(M, T)                                                                                                       \
  hipLaunchKernelGGL((k_engine_term_add<Term<M, T>, RG>), grid, block, 0, s, p.tile_psr, p.tile_start, p.tile_count, toa_s, tref, \
                     (Term<M, T>{fields...}), R, out, ld_out, acc)
  if (mode == 0) {
    if (psr_term) PTA_TERM_LAUNCH(0, 1); else PTA_TERM_LAUNCH(0, 0);
  } else if (mode == 1) {
    if (psr_term) PTA_TERM_LAUNCH(1, 1); else PTA_TERM_LAUNCH(1, 0);
  } else {
    if (psr_term) PTA_TERM_LAUNCH(2, 1); else PTA_TERM_LAUNCH(2, 0);
  }
#undef PTA_TERM_LAUNCH
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}
