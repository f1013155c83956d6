// Common red processes with an ORF of their own (ReplicaEngine.add_common_process, theta cp_* keys), added after the fused launch:
//   pta_engine_cproc_coef  coef[R, P, K] = sum_p sqrt(phi_pc) sum_j B_p[a, j] z_pcj, the deviates of a (realisation, column) drawn once
//                          into LDS and mixed by one thread per pulsar; sqrt(phi) configured, or pta_rn_amp per (realisation, process)
//   pta_engine_cproc_add   out[r, i] (+)= sum_k coef[r, a, 2k] s_k(i) + coef[r, a, 2k + 1] c_k(i) over the engine's tiles, the harmonics
//                          built in registers by rotation from two tabulated doubles per TOA - no design matrix is read
// Formulas and the order of every sum: pta_cproc.h.  No atomics: a thread owns its outputs, so a realisation's term is the same bits in
// every batch, row slot, chunk and view.
#include "pta_common.h"
#include "pta_rng.h"
#include "pta_cproc.h"

#define CPROC_COEF_THREADS 128

// workgroup = one (realisation, column c): the deviates z_pcj of every process that has the column -> LDS, then thread a mixes them
// with row a of each factor in ascending j and joins the processes in ascending p
__global__ __launch_bounds__(CPROC_COEF_THREADS) void k_engine_cproc_coef(pta_cproc_engine cp, uint64_t seed, uint64_t r0, int R) {
  extern __shared__ __attribute__((aligned(16))) double zs[];  // [sum_p rho_p]
  pta_rng_stage_tables();  // Box-Muller tables -> LDS (pta_rng.h)
  __syncthreads();
  const int K = cp.k, P = cp.n_psr;
  const int c = (int)(blockIdx.x % (unsigned)K), r = (int)(blockIdx.x / (unsigned)K);
  int off = 0;
  for (int p = 0; p < cp.n_proc; ++p) {
    const int rho = cp.rho[p];
    if (c < cp.kp[p])
      for (int j = threadIdx.x; j < rho; j += CPROC_COEF_THREADS)
        zs[off + j] = pta_cproc_deviate(seed, r0 + (uint64_t)r, p, rho, c, j, cp.rng_fast);
    off += rho;
  }
  __syncthreads();
  const bool theta = cp.log10_A != nullptr;
  for (int a = threadIdx.x; a < P; a += CPROC_COEF_THREADS) {
    double acc = 0.0;
    off = 0;
    for (int p = 0; p < cp.n_proc; ++p) {
      const int rho = cp.rho[p];
      if (c < cp.kp[p]) {
        const double lA = theta ? cp.log10_A[(int64_t)r * cp.ld_theta + p] : 0.0, g = theta ? cp.gamma[(int64_t)r * cp.ld_theta + p] : 0.0;
        const double amp = pta_cproc_amp(cp.amp, cp.tspan, p, K, c, theta, lA, g);
        acc = pta_cproc_join(acc, amp, pta_cproc_mix(cp.B[p] + (int64_t)a * rho, zs + off, rho));
      }
      off += rho;
    }
    cp.coef[((int64_t)r * P + a) * K + c] = acc;
  }
}

static int cproc_check(const pta_cproc_engine &cp, const char *who) {
  PTA_REQUIRE(cp.n_psr > 0 && cp.n_proc >= 1 && cp.n_proc <= PTA_CPROC_MAX, PTA_E_ARG, "%s: n_psr=%d n_proc=%d (1 .. %d processes)", who, cp.n_psr,
              cp.n_proc, PTA_CPROC_MAX);
  PTA_REQUIRE(cp.k > 0 && (cp.k % 2) == 0 && cp.k <= PTA_CPROC_KMAX, PTA_E_ARG, "%s: k=%d (k must be even, 2 .. %d)", who, cp.k, PTA_CPROC_KMAX);
  return PTA_OK;
}

extern "C" int pta_engine_cproc_coef(const pta_cproc_engine *cproc_host, uint64_t seed, uint64_t r0, int R, void *stream) {
  PTA_REQUIRE(cproc_host, PTA_E_ARG, "pta_engine_cproc_coef: NULL argument");
  const pta_cproc_engine &cp = *cproc_host;
  PTA_REQUIRE(cp.amp && cp.coef, PTA_E_ARG, "pta_engine_cproc_coef: NULL table (amp / coef)");
  PTA_REQUIRE(R > 0, PTA_E_ARG, "pta_engine_cproc_coef: R=%d", R);
  if (int rc = cproc_check(cp, "pta_engine_cproc_coef")) return rc;
  int64_t nz = 0;
  for (int p = 0; p < cp.n_proc; ++p) {
    PTA_REQUIRE(cp.B[p], PTA_E_ARG, "pta_engine_cproc_coef: NULL factor of process %d", p);
    PTA_REQUIRE(cp.rho[p] >= 1 && cp.rho[p] <= cp.n_psr, PTA_E_ARG, "pta_engine_cproc_coef: rho[%d]=%d (1 .. n_psr=%d)", p, cp.rho[p], cp.n_psr);
    PTA_REQUIRE(cp.kp[p] >= 2 && (cp.kp[p] % 2) == 0 && cp.kp[p] <= cp.k, PTA_E_ARG, "pta_engine_cproc_coef: kp[%d]=%d (even, 2 .. k=%d)", p, cp.kp[p],
                cp.k);
    nz += cp.rho[p];
  }
  PTA_REQUIRE(nz * 8 <= 65536, PTA_E_ARG, "pta_engine_cproc_coef: %lld deviates per column exceed the staging buffer", (long long)nz);
  PTA_REQUIRE(cp.tspan > 0 && cp.tspan < INFINITY, PTA_E_ARG, "pta_engine_cproc_coef: tspan=%g", cp.tspan);
  if (cp.log10_A) {
    PTA_REQUIRE(cp.gamma, PTA_E_ARG, "pta_engine_cproc_coef: gamma missing beside log10_A");
    PTA_REQUIRE(cp.ld_theta >= cp.n_proc, PTA_E_ARG, "pta_engine_cproc_coef: ld_theta=%lld too small", (long long)cp.ld_theta);
  }
  const int64_t total = (int64_t)R * cp.k;
  PTA_REQUIRE(total < (1LL << 31) && total * cp.n_psr < (1LL << 40), PTA_E_ARG, "pta_engine_cproc_coef: problem too large");
  hipLaunchKernelGGL(k_engine_cproc_coef, dim3((unsigned)total), dim3(CPROC_COEF_THREADS), (size_t)nz * sizeof(double), pta_stream(stream), cp, seed,
                     r0, R);
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}

// workgroup = one engine tile (<= PTA_ENGINE_TILE consecutive TOAs of one pulsar) x PTA_CPROC_RG realisations.  A half-workgroup (two
// waves, 128 lanes) owns every second row of the group, so all its rows start on the same 8-byte parity `sh` whatever ld_out is, and a
// lane owns the same two TOAs in all of them: elements sh + 2 p and sh + 2 p + 1, one 16-byte access (k_engine_bwm_add's pairs).  With
// sh = 1 the row's first element has no pair; lane 127, whose second element would lie past any tile, takes it instead.  The lane reads
// (sin, cos)(2 pi x) of its two TOAs once, builds harmonic k + 1 from harmonic k by rotation (pta_cproc_rot) and feeds it to the
// accumulators of its NR rows; the rows' coefficient pairs are uniform over the half (scalar loads).  With ACC the rows' old values are
// requested before the harmonic loop and added after it.  Every element is pta_cproc_synth of its (row, TOA), added once or written:
// the same value whichever lane and slot carry it.  No LDS, no barrier: a wave without an element leaves at once.
template <bool ACC>
__global__ __launch_bounds__(PTA_ENGINE_TILE) void k_engine_cproc_add(const int32_t *__restrict__ tile_psr, const int32_t *__restrict__ tile_start,
                                                                      const int32_t *__restrict__ tile_count, const double2 *__restrict__ sc1,
                                                                      const double *__restrict__ coef, int K, int P, int R,
                                                                      double *__restrict__ out, int64_t ld_out) {
  static_assert(PTA_ENGINE_TILE == 256, "k_engine_cproc_add: a half-workgroup of 128 lanes covers a tile in pairs");
  static_assert(PTA_CPROC_RG % 2 == 0 && PTA_CPROC_RG >= 2, "PTA_CPROC_RG: two half-workgroups");
  constexpr int NR = PTA_CPROC_RG / 2;
  const int tile = blockIdx.x;
  const int cnt = tile_count[tile];
  const int a = tile_psr[tile];
  const int64_t c0 = tile_start[tile];
  const int p = threadIdx.x & 127;
  const int hb = __builtin_amdgcn_readfirstlane(threadIdx.x >> 7);        // uniform over the wave
  const int wv = __builtin_amdgcn_readfirstlane((threadIdx.x >> 6) & 1);  // the wave of the half: lanes 64 wv .. 64 wv + 63
  const int r_hi = min(R, (int)(blockIdx.y + 1) * PTA_CPROC_RG), r_first = blockIdx.y * PTA_CPROC_RG + hb;
  if (r_first >= r_hi || cnt < 1) return;
  double *__restrict__ row0 = out + (int64_t)r_first * ld_out + c0;  // rows r_first + 2 u: row0 + 2 u ld_out, the same parity
  const int sh = __builtin_amdgcn_readfirstlane((int)(((uintptr_t)row0 >> 3) & 1));
  if (sh + 128 * wv >= cnt && !(sh && wv)) return;  // no element in this wave (the wave of lane 127 carries the head when sh = 1)
  const bool wrap = sh && p == 127;                 // this lane's second slot is the row's unaligned first element
  const int ix = sh + 2 * p, iy = wrap ? 0 : ix + 1;
  const bool pair = ix + 1 < cnt && !wrap, single = ix < cnt && !pair;
  const double2 bx = sc1[c0 + min(ix, cnt - 1)], by = sc1[c0 + min(iy, cnt - 1)];  // (sin, cos)(2 pi x); a clamped read is never used
  const double *__restrict__ cf[NR];
  double2 o[NR];
#pragma unroll
  for (int u = 0; u < NR; ++u) {
    const int r = min(r_first + 2 * u, r_hi - 1);  // a clamped row is computed and never stored
    cf[u] = coef + ((int64_t)r * P + a) * K;
    o[u] = double2{0.0, 0.0};
    if (ACC && r_first + 2 * u < r_hi) {
      const double *rw = row0 + (int64_t)(2 * u) * ld_out;
      if (pair) o[u] = *reinterpret_cast<const double2 *>(rw + ix);
      else {
        if (single) o[u].x = rw[ix];
        if (wrap) o[u].y = rw[0];
      }
    }
  }
  double ax[NR], ay[NR];
#pragma unroll
  for (int u = 0; u < NR; ++u) ax[u] = ay[u] = 0.0;
  double sx = bx.x, cx = bx.y, sy = by.x, cy = by.y;
#pragma unroll 2
  for (int k = 0; k < K; k += 2) {
#pragma unroll
    for (int u = 0; u < NR; ++u) {
      const double ca = cf[u][k], cb = cf[u][k + 1];
      ax[u] = pta_cproc_term(ax[u], ca, cb, sx, cx);
      ay[u] = pta_cproc_term(ay[u], ca, cb, sy, cy);
    }
    pta_cproc_rot(sx, cx, bx.x, bx.y);
    pta_cproc_rot(sy, cy, by.x, by.y);
  }
#pragma unroll
  for (int u = 0; u < NR; ++u) {
    if (r_first + 2 * u >= r_hi) break;  // uniform
    double *rw = row0 + (int64_t)(2 * u) * ld_out;
    const double vx = ACC ? o[u].x + ax[u] : ax[u], vy = ACC ? o[u].y + ay[u] : ay[u];
    if (pair) *reinterpret_cast<double2 *>(rw + ix) = double2{vx, vy};
    else {
      if (single) rw[ix] = vx;
      if (wrap) rw[0] = vy;
    }
  }
}

extern "C" int pta_engine_cproc_add(const pta_engine_plan *plan_host, const pta_cproc_engine *cproc_host, int R, double *out, int64_t ld_out,
                                    int accumulate, void *stream) {
  PTA_REQUIRE(plan_host && cproc_host && out, PTA_E_ARG, "pta_engine_cproc_add: NULL argument");
  const pta_engine_plan &p = *plan_host;
  const pta_cproc_engine &cp = *cproc_host;
  PTA_REQUIRE(p.tile_psr && p.tile_start && p.tile_count && cp.sc1 && cp.coef, PTA_E_ARG, "pta_engine_cproc_add: tiles / basis table / coef missing");
  if (int rc = cproc_check(cp, "pta_engine_cproc_add")) return rc;
  PTA_REQUIRE(R > 0 && p.n_tiles > 0 && cp.n_psr == p.n_psr && ld_out >= p.n_toa, PTA_E_ARG,
              "pta_engine_cproc_add: R=%d n_tiles=%d n_psr=%d/%d ld_out=%lld", R, p.n_tiles, cp.n_psr, p.n_psr, (long long)ld_out);
  PTA_REQUIRE(((uintptr_t)out & 7) == 0 && ((uintptr_t)cp.sc1 & 15) == 0 && ((uintptr_t)cp.coef & 15) == 0, PTA_E_ARG,
              "pta_engine_cproc_add: out must be 8-byte aligned, sc1 and coef 16-byte aligned");
  const unsigned groups = pta_cdiv(R, PTA_CPROC_RG);
  PTA_REQUIRE(groups <= 65535, PTA_E_ARG, "pta_engine_cproc_add: R=%d too large for one launch", R);
  const dim3 grid(p.n_tiles, groups), block(PTA_ENGINE_TILE);
  hipStream_t s = pta_stream(stream);
  const double2 *sc1 = reinterpret_cast<const double2 *>(cp.sc1);
  if (accumulate)
    hipLaunchKernelGGL((k_engine_cproc_add<true>), grid, block, 0, s, p.tile_psr, p.tile_start, p.tile_count, sc1, cp.coef, cp.k, p.n_psr, R, out,
                       ld_out);
  else
    hipLaunchKernelGGL((k_engine_cproc_add<false>), grid, block, 0, s, p.tile_psr, p.tile_start, p.tile_count, sc1, cp.coef, cp.k, p.n_psr, R, out,
                       ld_out);
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}
