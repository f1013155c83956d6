// White-noise parameters per realisation (theta's wn_efac, wn_log10_equad, wn_log10_ecorr; set_hyper_prior + generate_sampled):
//   pta_engine_wn_params  amplitude tables ea, eb [R, G_wn] and ec [R, G_ec], one thread per (realisation, group); every pow is here
//   pta_engine_wn_add     the EFAC / EQUAD and ECORR terms over the engine's TOA tiles x groups of realisations, added into (or written
//                         to) out[R, n_toa] with the deviates of the fused synthesis kernel: same stream, same counter
// Formulas: pta_wn_hyper.h.  No atomics and one fixed operation order per element: a realisation's terms are the same in every batch.
#include "pta_common.h"
#include "pta_rng.h"
#include "pta_wn_hyper.h"

#define WN_ADD_RG 8  // realisations per workgroup of the add kernel: two half-workgroups x four rows each

__global__ void k_engine_wn_params(pta_engine_wn_hyper w, int R) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // (r, column): the EFAC / EQUAD groups, then the ECORR groups
  const int nw = w.ea ? w.n_wn : 0, ne = w.ec ? w.n_ec : 0;
  if (idx >= (int64_t)R * (nw + ne)) return;
  const int64_t r = idx / (nw + ne);
  const int c = (int)(idx - r * (nw + ne));
  const double nan = pta_bits_to_double(0x7FF8000000000000ull);
  if (c < nw) {
    const double le = w.efac ? w.efac[r * w.ld_efac + c] : nan, lq = w.log10_equad ? w.log10_equad[r * w.ld_equad + c] : nan;
    double ea, eb;
    pta_wn_amplitudes(le, lq, w.efac_conf[c], w.equad_conf[c], w.tnequad, ea, eb);
    w.ea[r * w.n_wn + c] = ea;
    w.eb[r * w.n_wn + c] = eb;
  } else {
    const int g = c - nw;
    w.ec[r * w.n_ec + g] = pta_wn_pow10(w.log10_ecorr ? w.log10_ecorr[r * w.ld_ecorr + g] : nan, w.ecorr_conf[g]);
  }
}

extern "C" int pta_engine_wn_params(const pta_engine_wn_hyper *wn_host, int R, void *stream) {
  PTA_REQUIRE(wn_host, PTA_E_ARG, "pta_engine_wn_params: NULL argument");
  const pta_engine_wn_hyper &w = *wn_host;
  PTA_REQUIRE(w.ea || w.ec, PTA_E_ARG, "pta_engine_wn_params: NULL tables (neither ea / eb nor ec)");
  PTA_REQUIRE(!w.ea == !w.eb, PTA_E_ARG, "pta_engine_wn_params: ea and eb go together");
  PTA_REQUIRE(R > 0, PTA_E_ARG, "pta_engine_wn_params: R=%d", R);
  PTA_REQUIRE(!w.ea || (w.n_wn > 0 && w.efac_conf && w.equad_conf), PTA_E_ARG, "pta_engine_wn_params: n_wn=%d or the configured efac / equad missing",
              w.n_wn);
  PTA_REQUIRE(!w.ec || (w.n_ec > 0 && w.ecorr_conf), PTA_E_ARG, "pta_engine_wn_params: n_ec=%d or the configured ecorr missing", w.n_ec);
  PTA_REQUIRE(!w.ea || ((!w.efac || w.ld_efac >= w.n_wn) && (!w.log10_equad || w.ld_equad >= w.n_wn)), PTA_E_ARG,
              "pta_engine_wn_params: ld_efac=%lld / ld_equad=%lld too small", (long long)w.ld_efac, (long long)w.ld_equad);
  PTA_REQUIRE(!w.ec || !w.log10_ecorr || w.ld_ecorr >= w.n_ec, PTA_E_ARG, "pta_engine_wn_params: ld_ecorr=%lld too small", (long long)w.ld_ecorr);
  const int64_t total = (int64_t)R * ((w.ea ? w.n_wn : 0) + (w.ec ? w.n_ec : 0));
  PTA_REQUIRE(total < (1LL << 31), PTA_E_ARG, "pta_engine_wn_params: problem too large");
  hipLaunchKernelGGL(k_engine_wn_params, dim3(pta_cdiv(total, 128)), dim3(128), 0, pta_stream(stream), w, R);
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}

// what a lane keeps of one TOA of its tile
struct wn_toa {
  double sigma;
  uint32_t pair;  // idx_in_psr: the Box-Muller pair of stream (WN, a)
  int e;          // ECORR: the offset of the epoch's deviate in the staged range, or (tile_epn == 0) the epoch itself
  int gw, ge;     // slot of the TOA's groups in the staged amplitude rows; slot PTA_WN_HYPER_GMAX holds 0 (no group)
};

// workgroup = one engine tile (<= PTA_ENGINE_TILE consecutive TOAs of one pulsar) x WN_ADD_RG realisations.  Staged once per workgroup:
// the Box-Muller tables, the amplitude rows of the tile's pulsar (its groups are contiguous columns of ea / eb / ec; slot
// PTA_WN_HYPER_GMAX is the zero of a TOA without a group) and - tile_epn > 0 - the ECORR deviates of the pair range the tile's epochs
// cover, one Box-Muller pair per (realisation, epoch pair), as the fused kernel stages them.  Then a half-workgroup (two waves, 128
// lanes) owns a row of the tile: lane p holds two adjacent TOAs and moves them with one 16-byte access.  Pulsar offsets, ld_out and
// out itself are arbitrary, so a row's first element may sit on an odd 8-byte slot: its pairs then start one element later (lane p
// takes elements 2 p + 1, 2 p + 2), lane 0 moves the head alone, and an odd element left at the end is moved alone by the lane it
// falls to (the scheme of k_engine_bwm_add).  The three TOAs a lane can need stay in registers.  Every element is pta_wn_element
// (pta_wn_hyper.h) of the same operands on the pair, head and tail paths; the row's loads are issued ahead of its draws.
template <bool FAST, bool ACC>
__global__ __launch_bounds__(PTA_ENGINE_TILE) void k_engine_wn_add(const int32_t *__restrict__ tile_psr, const int32_t *__restrict__ tile_start,
                                                                   const int32_t *__restrict__ tile_count, const int32_t *__restrict__ tile_ep0,
                                                                   const int32_t *__restrict__ tile_epn, const int32_t *__restrict__ idx_in_psr,
                                                                   const int32_t *__restrict__ epoch_of, pta_engine_wn_hyper w, uint64_t seed,
                                                                   uint64_t r0, int R, double *__restrict__ out, int64_t ld_out) {
  static_assert(PTA_ENGINE_TILE == 256, "k_engine_wn_add: a half-workgroup of 128 lanes covers a tile in pairs");
  constexpr int fast = FAST ? 1 : 0;
  constexpr int GM = PTA_WN_HYPER_GMAX;
  __shared__ double zec[WN_ADD_RG][2 * PTA_ENGINE_EPMAX];
  __shared__ double amp[3][WN_ADD_RG][GM + 1];  // ea, eb, ec of the tile's pulsar
  pta_rng_stage_tables();  // Box-Muller tables -> LDS (pta_rng.h)
  const int tile = blockIdx.x;
  const int cnt = tile_count[tile];
  const int a = tile_psr[tile];
  const int64_t c0 = tile_start[tile];
  const int t = threadIdx.x;
  const bool has_wn = w.ea != nullptr, has_ec = w.ec != nullptr;
  const int r_lo = blockIdx.y * WN_ADD_RG, nrow = min(WN_ADD_RG, R - r_lo);
  const int gw0 = has_wn ? w.wn_psr0[a] : 0, ngw = has_wn ? min(w.wn_psr0[a + 1] - gw0, GM) : 0;
  const int ge0 = has_ec ? w.ec_psr0[a] : 0, nge = has_ec ? min(w.ec_psr0[a + 1] - ge0, GM) : 0;
  for (int idx = t; idx < WN_ADD_RG * (GM + 1); idx += PTA_ENGINE_TILE) {
    const int q = idx / (GM + 1), j = idx - q * (GM + 1);
    const int64_t r = r_lo + min(q, nrow - 1);  // rows past R: a clamped read that is never used
    amp[0][q][j] = j < ngw ? w.ea[r * w.n_wn + gw0 + j] : 0.0;
    amp[1][q][j] = j < ngw ? w.eb[r * w.n_wn + gw0 + j] : 0.0;
    amp[2][q][j] = j < nge ? w.ec[r * w.n_ec + ge0 + j] : 0.0;
  }
  __syncthreads();
  const uint32_t strm_wn = pta_stream_id(PTA_STREAM_WN, (uint32_t)a), strm_ec = pta_stream_id(PTA_STREAM_ECORR, (uint32_t)a);
  const int epn = has_ec ? min(tile_epn[tile], PTA_ENGINE_EPMAX) : 0;
  const int ep0 = has_ec ? tile_ep0[tile] : 0;
  if (epn > 0) {  // the tile's ECORR deviates -> LDS
    for (int idx = t; idx < epn * nrow; idx += PTA_ENGINE_TILE) {
      const int q = idx / epn, p = idx - q * epn;
      double z0, z1;
      pta_normal_pair(seed, r0 + (uint64_t)(r_lo + q), strm_ec, (uint32_t)(ep0 + p), z0, z1, fast);
      zec[q][2 * p] = z0;
      zec[q][2 * p + 1] = z1;
    }
    __syncthreads();
  }
  const int p = t & 127;
  const int hb = __builtin_amdgcn_readfirstlane(t >> 7);  // uniform over the wave
  wn_toa T[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int64_t i = c0 + min(2 * p + j, cnt - 1);  // past the tile's count: a clamped read that is never used
    T[j].sigma = has_wn ? w.sigma[i] : 0.0;
    T[j].pair = (uint32_t)idx_in_psr[i];
    const int gw = has_wn ? w.wn_group[i] - gw0 : -1, ge = has_ec ? w.ec_group[i] - ge0 : -1;
    T[j].gw = (gw >= 0 && gw < ngw) ? gw : GM;
    T[j].ge = (ge >= 0 && ge < nge) ? ge : GM;
    const int e = has_ec ? epoch_of[i] : 0;
    T[j].e = epn > 0 ? min(max(e - 2 * ep0, 0), 2 * epn - 1) : e;
  }
  auto element = [&](double o, const wn_toa &x, int q) {
    const uint64_t r = r0 + (uint64_t)(r_lo + q);
    double z1 = 0.0, z2 = 0.0, ze = 0.0;
    if (has_wn) pta_normal_pair(seed, r, strm_wn, x.pair, z1, z2, fast);
    if (has_ec) ze = epn > 0 ? zec[q][x.e] : pta_normal_single(seed, r, strm_ec, (uint32_t)x.e, fast);
    return pta_wn_element(o, has_wn, amp[0][q][x.gw], x.sigma, z1, amp[1][q][x.gw], z2, has_ec, amp[2][q][x.ge], ze);
  };
  for (int q = hb; q < nrow; q += 2) {
    double *row = out + (int64_t)(r_lo + q) * ld_out + c0;
    const int sh = (int)(((uintptr_t)row >> 3) & 1);
    const int i = sh + 2 * p;
    const int kind = i + 1 < cnt ? 1 : (i < cnt ? 2 : 0);  // 0 nothing, 1 a pair, 2 a single element at i
    const bool head = sh && p == 0;                        // this lane moves the row's unaligned first element
    double2 o = double2{0.0, 0.0};
    double oh = 0.0;
    if (ACC) {
      if (kind == 1) o = *reinterpret_cast<const double2 *>(row + i);
      else if (kind == 2) o.x = row[i];
      if (head) oh = row[0];
    }
    const wn_toa &xa = sh ? T[1] : T[0], &xb = sh ? T[2] : T[1];
    if (kind == 1) {
      const double vx = element(o.x, xa, q), vy = element(o.y, xb, q);
      *reinterpret_cast<double2 *>(row + i) = double2{vx, vy};
    } else if (kind == 2) {
      row[i] = element(o.x, xa, q);
    }
    if (head) row[0] = element(oh, T[0], q);
  }
}

typedef void (*pta_wn_add_fn)(const int32_t *, const int32_t *, const int32_t *, const int32_t *, const int32_t *, const int32_t *, const int32_t *,
                              pta_engine_wn_hyper, uint64_t, uint64_t, int, double *, int64_t);

extern "C" int pta_engine_wn_add(const pta_engine_plan *plan_host, const pta_engine_wn_hyper *wn_host, uint64_t seed, uint64_t r0, int R, double *out,
                                 int64_t ld_out, int accumulate, void *stream) {
  PTA_REQUIRE(plan_host && wn_host && out, PTA_E_ARG, "pta_engine_wn_add: NULL argument");
  const pta_engine_plan &p = *plan_host;
  const pta_engine_wn_hyper &w = *wn_host;
  PTA_REQUIRE(p.tile_psr && p.tile_start && p.tile_count && p.tile_ep0 && p.tile_epn && p.idx_in_psr, PTA_E_ARG,
              "pta_engine_wn_add: tile table / idx_in_psr missing");
  PTA_REQUIRE(w.ea || w.ec, PTA_E_ARG, "pta_engine_wn_add: NULL tables (neither ea / eb nor ec): nothing to add");
  PTA_REQUIRE(!w.ea == !w.eb, PTA_E_ARG, "pta_engine_wn_add: ea and eb go together");
  PTA_REQUIRE(!w.ea || (w.n_wn > 0 && w.sigma && w.wn_group && w.wn_psr0), PTA_E_ARG, "pta_engine_wn_add: n_wn=%d or sigma / wn_group / wn_psr0 missing",
              w.n_wn);
  PTA_REQUIRE(!w.ec || (w.n_ec > 0 && w.ec_group && w.ec_psr0 && p.epoch_of), PTA_E_ARG,
              "pta_engine_wn_add: n_ec=%d or ec_group / ec_psr0 / the plan's epoch_of missing", w.n_ec);
  PTA_REQUIRE(R > 0 && p.n_tiles > 0 && w.n_psr == p.n_psr && ld_out >= p.n_toa, PTA_E_ARG,
              "pta_engine_wn_add: R=%d n_tiles=%d n_psr=%d/%d ld_out=%lld", R, p.n_tiles, w.n_psr, p.n_psr, (long long)ld_out);
  PTA_REQUIRE(w.max_per_psr >= 1 && w.max_per_psr <= PTA_WN_HYPER_GMAX, PTA_E_ARG, "pta_engine_wn_add: max_per_psr=%d (1 .. %d groups of one pulsar)",
              w.max_per_psr, PTA_WN_HYPER_GMAX);
  PTA_REQUIRE(((uintptr_t)out & 7) == 0, PTA_E_ARG, "pta_engine_wn_add: out must be 8-byte aligned");
  const unsigned groups = pta_cdiv(R, WN_ADD_RG);
  PTA_REQUIRE(groups <= 65535, PTA_E_ARG, "pta_engine_wn_add: R=%d too large for one launch", R);
  static const pta_wn_add_fn kern[2][2] = {{k_engine_wn_add<false, false>, k_engine_wn_add<false, true>},
                                           {k_engine_wn_add<true, false>, k_engine_wn_add<true, true>}};
  hipLaunchKernelGGL(kern[p.rng_fast != 0][accumulate != 0], dim3(p.n_tiles, groups), dim3(PTA_ENGINE_TILE), 0, pta_stream(stream), p.tile_psr,
                     p.tile_start, p.tile_count, p.tile_ep0, p.tile_epn, p.idx_in_psr, p.epoch_of, w, seed, r0, R, out, ld_out);
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}
