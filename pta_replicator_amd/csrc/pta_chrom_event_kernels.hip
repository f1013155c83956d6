// Chromatic events per realisation (ReplicaEngine.set_chromatic_events + theta ce_* keys, set_chromatic_event_prior + generate_sampled):
//   pta_chrom_event_uniform         labels drawn on chip: column j of slot e from stream (CE, e), pair j, in the slot's own box
//                                   (lo / hi [E, 9]); the pulsar column floored as pta_nt_psr floors it
//   pta_engine_chrom_event_params   tab[R, E, 10] per event from the label rows, one thread per row
//   pta_engine_chrom_event_add      per (realisation, pulsar) the sum over the realisation's live events in that pulsar, over the engine's
//                                   TOA tiles x groups of realisations
// Formulas, the exponent fold and its rounding: pta_chrom_event.h.  No atomics; a register accumulator over the events in ascending
// order, then one read-modify-write: a realisation's term is the same bits in every batch and row slot.
#include "pta_common.h"
#include "pta_rng.h"
#include "pta_chrom_event.h"

#define CE_ADD_RG 4  // realisations per workgroup of the add kernel (BURST_ADD_RG: a lane's TOA and ln(nu_ref / nu) stay in registers)

static_assert(PTA_CE_NCOL == 9 && PTA_CE_NTAB == 10 && PTA_CE_EMAX == 128, "layouts of include/pta_replicator_amd.h");

// ---------------------------------------------------------------- label draws
__global__ void k_chrom_event_uniform(uint64_t seed, uint64_t r0, int R, int E, int P, const double *__restrict__ lo,
                                      const double *__restrict__ hi, double *__restrict__ out) {
  const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;  // (r, e, j): R E 9 < 2^31, so 32-bit index arithmetic
  if (idx >= (uint32_t)R * E * PTA_CE_NCOL) return;
  const uint32_t j = idx % PTA_CE_NCOL, re = idx / PTA_CE_NCOL;
  const uint32_t e = re % E, r = re / E;
  const double x = pta_ce_draw(seed, r0 + r, e, j, lo[e * PTA_CE_NCOL + j], hi[e * PTA_CE_NCOL + j]);
  out[idx] = j == PTA_CE_COL_PSR ? pta_nt_psr(x, P) : x;
}

extern "C" int pta_chrom_event_uniform(uint64_t seed, uint64_t r0, int R, int E, int P, const double *lo, const double *hi, double *out,
                                       void *stream) {
  PTA_REQUIRE(lo && hi && out, PTA_E_ARG, "pta_chrom_event_uniform: NULL argument");
  PTA_REQUIRE(R > 0 && E >= 1 && E <= PTA_CE_EMAX && P > 0, PTA_E_ARG, "pta_chrom_event_uniform: R=%d E=%d P=%d", R, E, P);
  PTA_REQUIRE((int64_t)R * E * PTA_CE_NCOL < (1LL << 31), PTA_E_ARG, "pta_chrom_event_uniform: problem too large");
  hipLaunchKernelGGL(k_chrom_event_uniform, dim3(pta_cdiv((int64_t)R * E * PTA_CE_NCOL, 256)), dim3(256), 0, pta_stream(stream), seed, r0, R, E,
                     P, lo, hi, out);
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}

// ---------------------------------------------------------------- table
// events at or past the realisation's count are neither read nor written
__device__ __forceinline__ int ce_count(const int32_t *count, int r, int E) { return count ? min(max(count[r], 0), E) : E; }

__global__ void k_engine_chrom_event_params(pta_chrom_event_engine c, int R) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // (r, e)
  if (idx >= (int64_t)R * c.n_ev) return;
  if ((int)(idx % c.n_ev) >= ce_count(c.count, (int)(idx / c.n_ev), c.n_ev)) return;
  pta_ce_row(c.src + idx * PTA_CE_NCOL, c.tab + idx * PTA_CE_NTAB);
}

extern "C" int pta_engine_chrom_event_params(const pta_chrom_event_engine *ce_host, int R, void *stream) {
  PTA_REQUIRE(ce_host, PTA_E_ARG, "pta_engine_chrom_event_params: NULL argument");
  const pta_chrom_event_engine &c = *ce_host;
  PTA_REQUIRE(c.src && c.tab, PTA_E_ARG, "pta_engine_chrom_event_params: NULL table");
  PTA_REQUIRE(R > 0 && c.n_ev >= 1 && c.n_ev <= PTA_CE_EMAX, PTA_E_ARG, "pta_engine_chrom_event_params: R=%d n_ev=%d", R, c.n_ev);
  const int64_t total = (int64_t)R * c.n_ev;
  PTA_REQUIRE(total * PTA_CE_NTAB < (1LL << 31), PTA_E_ARG, "pta_engine_chrom_event_params: problem too large");
  hipLaunchKernelGGL(k_engine_chrom_event_params, dim3(pta_cdiv(total, 128)), dim3(128), 0, pta_stream(stream), c, R);
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}

// ---------------------------------------------------------------- the term
// workgroup = one engine tile (<= PTA_ENGINE_TILE consecutive TOAs of one pulsar a) x CE_ADD_RG realisations, a lane per TOA.  The table
// row, the test on the pulsar and the branch on the kind are uniform over the workgroup (scalar loads and branches).  An event whose
// exponent is below PTA_CE_ARG_ZERO (or -infinity: a decay before its t0) on every active lane of the wave is passed over; its term would
// be s * (+0), and acc starts at +0.0, so the sum is the same bits with and without the branch.  Accumulating, a (tile, realisation) whose
// pulsar holds no live event of the realisation is neither read nor written.
__global__ __launch_bounds__(PTA_ENGINE_TILE) void k_engine_chrom_event_add(const int32_t *__restrict__ tile_psr, const int32_t *__restrict__ tile_start,
                                                                            const int32_t *__restrict__ tile_count, const double *__restrict__ toa_s,
                                                                            const double *__restrict__ lnu, const double *__restrict__ tab,
                                                                            const int32_t *__restrict__ count, int E, int R,
                                                                            double *__restrict__ out, int64_t ld_out, int accumulate) {
  const int tile = blockIdx.x;
  const int i = threadIdx.x;
  if (i >= tile_count[tile]) return;  // no barriers below
  const int a = tile_psr[tile];
  const int64_t col = (int64_t)tile_start[tile] + i;
  const double t = toa_s[col], l = lnu[col];
  const int r_lo = blockIdx.y * CE_ADD_RG, r_hi = min(R, r_lo + CE_ADD_RG);
  for (int r = r_lo; r < r_hi; ++r) {
    const int ne = ce_count(count, r, E);
    double acc = 0.0;
    bool hit = false;
    for (int e = 0; e < ne; ++e) {
      const double *row = tab + ((int64_t)r * E + e) * PTA_CE_NTAB;
      if ((int)row[PTA_CE_TAB_PSR] != a) continue;
      hit = true;
      const int kind = (int)row[PTA_CE_TAB_KIND];
      if (kind == PTA_CE_KIND_ANNUAL) {
        acc += pta_ce_annual_value(row, t, l);
      } else {
        const double ex = pta_ce_exponent(kind, row, t, l);
        if (__all(ex < PTA_CE_ARG_ZERO)) continue;
        acc += pta_ce_exp_value(row, ex);
      }
    }
    if (accumulate && !hit) continue;
    double *o = out + (int64_t)r * ld_out + col;
    *o = accumulate ? *o + acc : acc;
  }
}

extern "C" int pta_engine_chrom_event_add(const pta_engine_plan *plan_host, const pta_chrom_event_engine *ce_host, int R, double *out,
                                          int64_t ld_out, int accumulate, void *stream) {
  PTA_REQUIRE(plan_host && ce_host && out, PTA_E_ARG, "pta_engine_chrom_event_add: NULL argument");
  const pta_engine_plan &p = *plan_host;
  const pta_chrom_event_engine &c = *ce_host;
  PTA_REQUIRE(p.tile_psr && p.tile_start && p.tile_count && c.toa_s && c.lnu && c.tab, PTA_E_ARG,
              "pta_engine_chrom_event_add: tiles / TOAs / table missing");
  PTA_REQUIRE(R > 0 && p.n_tiles > 0 && c.n_psr == p.n_psr && ld_out >= p.n_toa && c.n_ev >= 1 && c.n_ev <= PTA_CE_EMAX, PTA_E_ARG,
              "pta_engine_chrom_event_add: R=%d n_tiles=%d n_psr=%d/%d ld_out=%lld n_ev=%d", R, p.n_tiles, c.n_psr, p.n_psr, (long long)ld_out,
              c.n_ev);
  PTA_REQUIRE(((uintptr_t)out & 7) == 0, PTA_E_ARG, "pta_engine_chrom_event_add: out must be 8-byte aligned");
  const unsigned groups = pta_cdiv(R, CE_ADD_RG);
  PTA_REQUIRE(groups <= 65535, PTA_E_ARG, "pta_engine_chrom_event_add: R=%d too large for one launch", R);
  hipLaunchKernelGGL(k_engine_chrom_event_add, dim3(p.n_tiles, groups), dim3(PTA_ENGINE_TILE), 0, pta_stream(stream), p.tile_psr, p.tile_start,
                     p.tile_count, c.toa_s, c.lnu, c.tab, c.count, c.n_ev, R, out, ld_out, accumulate ? 1 : 0);
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}
