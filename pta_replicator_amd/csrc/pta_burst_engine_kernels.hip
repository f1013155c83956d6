// Sine-Gaussian wavelets per realisation (ReplicaEngine.set_burst / set_transients + theta burst_* / nt_* keys, set_burst_prior /
// set_transient_prior + generate_sampled):
//   pta_burst_uniform            burst labels drawn on chip from uniform boxes: the sky row from stream (BURST, 0), wavelet w from stream
//                                (BURST, 1 + w), pair = label column; the shared box draw (pta_box_kernels.hip)
//   pta_transient_uniform        transient v from stream (NT, v), pair = label column; the pulsar column floored
//   pta_engine_burst_params      wav[R, W, 7] per wavelet and kk[R, P, 2] = (k+, kx) per pulsar, one thread per table row
//   pta_engine_burst_quad        c[R, P, 3] = Q_a^T term (remove_quad), a workgroup per (pulsar, realisation), fixed reduction order
//   pta_engine_burst_add         the sum over the wavelets over the engine's TOA tiles x groups of realisations, minus Q_i . c with
//                                remove_quad, added into (or written to) out[R, n_toa]
//   pta_engine_transient_params  tab[R, V, 6] per transient
//   pta_engine_transient_add     the sum over the realisation's transients that live in the tile's pulsar
// Formulas: pta_burst.h.  No atomics; a register accumulator over the wavelets in ascending order, then one read-modify-write: a
// realisation's term is the same bits in every batch and row slot.
#include "pta_common.h"
#include "pta_rng.h"
#include "pta_burst.h"

#define BURST_ADD_RG 4  // realisations per workgroup of the add kernels (the catalogue kernel's choice: a lane's TOA stays in a register)

static_assert(PTA_BURST_NSKY == 3 && PTA_BURST_NCOL == 7 && PTA_NT_NCOL == 6, "label layouts of include/pta_replicator_amd.h");

// ---------------------------------------------------------------- label draws
extern "C" int pta_burst_uniform(uint64_t seed, uint64_t r0, int R, int W, const double *lo, const double *hi, double *sky, double *wav,
                                 void *stream) {
  PTA_REQUIRE(lo && hi && sky && wav, PTA_E_ARG, "pta_burst_uniform: NULL argument");
  PTA_REQUIRE(R > 0 && W >= 1 && W <= PTA_BURST_WMAX, PTA_E_ARG, "pta_burst_uniform: R=%d W=%d", R, W);
  PTA_REQUIRE((int64_t)R * W * PTA_BURST_NCOL < (1LL << 31), PTA_E_ARG, "pta_burst_uniform: problem too large");
  int rc = pta_box_uniform_launch(seed, r0, R, 1, PTA_BURST_NSKY, PTA_STREAM_BURST, 0u, lo, hi, sky, pta_stream(stream));
  if (rc != PTA_OK) return rc;
  return pta_box_uniform_launch(seed, r0, R, W, PTA_BURST_NCOL, PTA_STREAM_BURST, 1u, lo + PTA_BURST_NSKY, hi + PTA_BURST_NSKY, wav,
                                pta_stream(stream));
}

__global__ void k_transient_psr(double *__restrict__ out, int n, int P) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;  // (r, v)
  if (idx >= n) return;
  double *x = out + (int64_t)idx * PTA_NT_NCOL + PTA_NT_COL_PSR;
  *x = pta_nt_psr(*x, P);
}

extern "C" int pta_transient_uniform(uint64_t seed, uint64_t r0, int R, int V, int P, const double *lo, const double *hi, double *out,
                                     void *stream) {
  PTA_REQUIRE(lo && hi && out, PTA_E_ARG, "pta_transient_uniform: NULL argument");
  PTA_REQUIRE(R > 0 && V >= 1 && V <= PTA_BURST_WMAX && P > 0, PTA_E_ARG, "pta_transient_uniform: R=%d V=%d P=%d", R, V, P);
  PTA_REQUIRE((int64_t)R * V * PTA_NT_NCOL < (1LL << 31), PTA_E_ARG, "pta_transient_uniform: problem too large");
  int rc = pta_box_uniform_launch(seed, r0, R, V, PTA_NT_NCOL, PTA_STREAM_NT, 0u, lo, hi, out, pta_stream(stream));
  if (rc != PTA_OK) return rc;
  hipLaunchKernelGGL(k_transient_psr, dim3(pta_cdiv((int64_t)R * V, 256)), dim3(256), 0, pta_stream(stream), out, R * V, P);
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}

// ---------------------------------------------------------------- tables
// wavelets at or past the realisation's count are neither read nor written
__device__ __forceinline__ int burst_count(const int32_t *count, int r, int W) { return count ? min(max(count[r], 0), W) : W; }

__global__ void k_engine_burst_params(pta_burst_engine b, int R) {
  const int per = b.n_wav + b.n_psr;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // (r, wavelet w or W + pulsar a)
  if (idx >= (int64_t)R * per) return;
  const int j = (int)(idx % per);
  const int64_t r = idx / per;
  if (j < b.n_wav) {
    if (j >= burst_count(b.count, (int)r, b.n_wav)) return;
    const int64_t row = r * b.n_wav + j;
    pta_burst_wavelet_row(b.src + row * PTA_BURST_NCOL, b.wav + row * PTA_BURST_NTAB);
  } else {
    const int a = j - b.n_wav;
    double kp, kc;
    pta_burst_antenna(b.sky + r * PTA_BURST_NSKY, b.phat + 3 * a, kp, kc);
    b.kk[(r * b.n_psr + a) * 2] = kp;
    b.kk[(r * b.n_psr + a) * 2 + 1] = kc;
  }
}

extern "C" int pta_engine_burst_params(const pta_burst_engine *burst_host, int R, void *stream) {
  PTA_REQUIRE(burst_host, PTA_E_ARG, "pta_engine_burst_params: NULL argument");
  const pta_burst_engine &b = *burst_host;
  PTA_REQUIRE(b.sky && b.src && b.phat && b.wav && b.kk, PTA_E_ARG, "pta_engine_burst_params: NULL table");
  PTA_REQUIRE(R > 0 && b.n_psr > 0 && b.n_wav >= 1 && b.n_wav <= PTA_BURST_WMAX, PTA_E_ARG, "pta_engine_burst_params: R=%d n_psr=%d n_wav=%d", R,
              b.n_psr, b.n_wav);
  const int64_t total = (int64_t)R * (b.n_wav + b.n_psr);
  PTA_REQUIRE(total < (1LL << 31), PTA_E_ARG, "pta_engine_burst_params: problem too large");
  hipLaunchKernelGGL(k_engine_burst_params, dim3(pta_cdiv(total, 128)), dim3(128), 0, pta_stream(stream), b, R);
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}

__global__ void k_engine_transient_params(pta_transient_engine t, int R) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // (r, v)
  if (idx >= (int64_t)R * t.n_wav) return;
  if ((int)(idx % t.n_wav) >= burst_count(t.count, (int)(idx / t.n_wav), t.n_wav)) return;
  pta_nt_row(t.src + idx * PTA_NT_NCOL, t.tab + idx * PTA_NT_NTAB);
}

extern "C" int pta_engine_transient_params(const pta_transient_engine *nt_host, int R, void *stream) {
  PTA_REQUIRE(nt_host, PTA_E_ARG, "pta_engine_transient_params: NULL argument");
  const pta_transient_engine &t = *nt_host;
  PTA_REQUIRE(t.src && t.tab, PTA_E_ARG, "pta_engine_transient_params: NULL table");
  PTA_REQUIRE(R > 0 && t.n_wav >= 1 && t.n_wav <= PTA_BURST_WMAX, PTA_E_ARG, "pta_engine_transient_params: R=%d n_wav=%d", R, t.n_wav);
  const int64_t total = (int64_t)R * t.n_wav;
  PTA_REQUIRE(total < (1LL << 31), PTA_E_ARG, "pta_engine_transient_params: problem too large");
  hipLaunchKernelGGL(k_engine_transient_params, dim3(pta_cdiv(total, 128)), dim3(128), 0, pta_stream(stream), t, R);
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}

// ---------------------------------------------------------------- the terms
// sum over wavelets 0 .. nw-1 of realisation r (rows of wav) seen from a pulsar with (kp, kc), at t: the table rows and (kp, kc) are
// uniform over the wave (scalar loads).  A wavelet whose envelope is exactly 0 for every active lane of the wave is passed over by a
// scalar branch; the sum is the same bits with and without it (0.0 + x g, g = +0).
__device__ __forceinline__ double burst_term(const double *__restrict__ wav, int nw, double kp, double kc, double t) {
  double acc = 0.0;
  for (int w = 0; w < nw; ++w) {
    const double *row = wav + (int64_t)w * PTA_BURST_NTAB;
    const double arg = pta_wavelet_arg(row[0], row[1], t);
    if (__all(arg < PTA_BURST_ARG_ZERO)) continue;
    double C, S;
    pta_burst_fold(kp, kc, row, C, S);
    acc += pta_wavelet_value(row[0], row[2], C, S, arg, t);
  }
  return acc;
}

// sum over the transients of realisation r that live in pulsar a, at t: the test on the pulsar is uniform over the workgroup
__device__ __forceinline__ double transient_term(const double *__restrict__ tab, int nv, int a, double t) {
  double acc = 0.0;
  for (int v = 0; v < nv; ++v) {
    const double *row = tab + (int64_t)v * PTA_NT_NTAB;
    if ((int)row[0] != a) continue;
    const double arg = pta_wavelet_arg(row[1], row[2], t);
    if (__all(arg < PTA_BURST_ARG_ZERO)) continue;
    acc += pta_wavelet_value(row[1], row[3], row[4], row[5], arg, t);
  }
  return acc;
}

// workgroup = (pulsar a, realisation r): c[r, a, :] = sum_i Q[i, :] term_i over the pulsar's TOAs.  Order: a lane sums its TOAs
// (i = lane, lane + 256, ...) in ascending order, then a binary tree over the 256 lanes through LDS.  Pulsars of <= 3 TOAs and
// realisations without a wavelet get c = 0.
__global__ __launch_bounds__(256) void k_engine_burst_quad(const double *__restrict__ toa_s, const int32_t *__restrict__ psr_off,
                                                           const double *__restrict__ quad_q, const double *__restrict__ wav,
                                                           const double *__restrict__ kk, const int32_t *__restrict__ count, int W, int P,
                                                           double *__restrict__ quad_c) {
  __shared__ double red[3][256];
  const int a = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
  const int n0 = psr_off[a], n1 = psr_off[a + 1];
  const int nw = burst_count(count, r, W);
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  if (n1 - n0 > 3 && nw > 0) {
    const double kp = kk[((int64_t)r * P + a) * 2], kc = kk[((int64_t)r * P + a) * 2 + 1];
    for (int col = n0 + tid; col < n1; col += 256) {
      const double v = burst_term(wav + (int64_t)r * W * PTA_BURST_NTAB, nw, kp, kc, toa_s[col]);
      const double *q = quad_q + 3 * (int64_t)col;
      s0 += q[0] * v;
      s1 += q[1] * v;
      s2 += q[2] * v;
    }
  }
  red[0][tid] = s0;
  red[1][tid] = s1;
  red[2][tid] = s2;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) {
      red[0][tid] += red[0][tid + s];
      red[1][tid] += red[1][tid + s];
      red[2][tid] += red[2][tid + s];
    }
    __syncthreads();
  }
  if (tid < 3) quad_c[((int64_t)r * P + a) * 3 + tid] = red[tid][0];
}

static int burst_quad_refusal(const pta_burst_engine &b) { return !(b.psr_off && b.quad_q && b.quad_c); }

extern "C" int pta_engine_burst_quad(const pta_burst_engine *burst_host, int R, void *stream) {
  PTA_REQUIRE(burst_host, PTA_E_ARG, "pta_engine_burst_quad: NULL argument");
  const pta_burst_engine &b = *burst_host;
  PTA_REQUIRE(b.toa_s && b.wav && b.kk && !burst_quad_refusal(b), PTA_E_ARG, "pta_engine_burst_quad: TOAs / table missing");
  PTA_REQUIRE(R > 0 && R <= 65535 && b.n_psr > 0 && b.n_wav >= 1 && b.n_wav <= PTA_BURST_WMAX, PTA_E_ARG,
              "pta_engine_burst_quad: R=%d n_psr=%d n_wav=%d", R, b.n_psr, b.n_wav);
  hipLaunchKernelGGL(k_engine_burst_quad, dim3(b.n_psr, R), dim3(256), 0, pta_stream(stream), b.toa_s, b.psr_off, b.quad_q, b.wav, b.kk, b.count,
                     b.n_wav, b.n_psr, b.quad_c);
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}

// workgroup = one engine tile (<= PTA_ENGINE_TILE consecutive TOAs of one pulsar) x BURST_ADD_RG realisations, a lane per TOA.  QUAD: the
// term minus Q_i . c[r, a] (c from pta_engine_burst_quad, which evaluated the same term), 0 for a pulsar of <= 3 TOAs.  A realisation
// without a wavelet leaves out untouched when accumulating.
template <bool QUAD>
__global__ __launch_bounds__(PTA_ENGINE_TILE) void k_engine_burst_add(const int32_t *__restrict__ tile_psr, const int32_t *__restrict__ tile_start,
                                                                      const int32_t *__restrict__ tile_count, const double *__restrict__ toa_s,
                                                                      const double *__restrict__ wav, const double *__restrict__ kk,
                                                                      const int32_t *__restrict__ count, int W, int P,
                                                                      const int32_t *__restrict__ psr_off, const double *__restrict__ quad_q,
                                                                      const double *__restrict__ quad_c, int R, double *__restrict__ out,
                                                                      int64_t ld_out, int accumulate) {
  const int tile = blockIdx.x;
  const int i = threadIdx.x;
  if (i >= tile_count[tile]) return;  // no barriers below
  const int a = tile_psr[tile];
  const int64_t col = (int64_t)tile_start[tile] + i;
  const double t = toa_s[col];
  double q0 = 0.0, q1 = 0.0, q2 = 0.0;
  bool few = false;
  if (QUAD) {
    few = psr_off[a + 1] - psr_off[a] <= 3;
    q0 = quad_q[3 * col], q1 = quad_q[3 * col + 1], q2 = quad_q[3 * col + 2];
  }
  const int r_lo = blockIdx.y * BURST_ADD_RG, r_hi = min(R, r_lo + BURST_ADD_RG);
  for (int r = r_lo; r < r_hi; ++r) {
    const int nw = burst_count(count, r, W);
    if (nw == 0 && accumulate) continue;
    const int64_t ra = (int64_t)r * P + a;
    double v = burst_term(wav + (int64_t)r * W * PTA_BURST_NTAB, nw, kk[2 * ra], kk[2 * ra + 1], t);
    if (QUAD) {
      const double *c = quad_c + 3 * ra;
      v = few ? 0.0 : v - ((q0 * c[0] + q1 * c[1]) + q2 * c[2]);
    }
    double *o = out + (int64_t)r * ld_out + col;
    *o = accumulate ? *o + v : v;
  }
}

extern "C" int pta_engine_burst_add(const pta_engine_plan *plan_host, const pta_burst_engine *burst_host, int R, double *out, int64_t ld_out,
                                    int accumulate, void *stream) {
  PTA_REQUIRE(plan_host && burst_host && out, PTA_E_ARG, "pta_engine_burst_add: NULL argument");
  const pta_engine_plan &p = *plan_host;
  const pta_burst_engine &b = *burst_host;
  PTA_REQUIRE(p.tile_psr && p.tile_start && p.tile_count && b.toa_s && b.wav && b.kk, PTA_E_ARG, "pta_engine_burst_add: tiles / TOAs / table missing");
  PTA_REQUIRE(R > 0 && p.n_tiles > 0 && b.n_psr == p.n_psr && ld_out >= p.n_toa && b.n_wav >= 1 && b.n_wav <= PTA_BURST_WMAX, PTA_E_ARG,
              "pta_engine_burst_add: R=%d n_tiles=%d n_psr=%d/%d ld_out=%lld n_wav=%d", R, p.n_tiles, b.n_psr, p.n_psr, (long long)ld_out, b.n_wav);
  PTA_REQUIRE(((uintptr_t)out & 7) == 0, PTA_E_ARG, "pta_engine_burst_add: out must be 8-byte aligned");
  const unsigned groups = pta_cdiv(R, BURST_ADD_RG);
  PTA_REQUIRE(groups <= 65535, PTA_E_ARG, "pta_engine_burst_add: R=%d too large for one launch", R);
  const bool quad = b.quad_q != NULL;
  if (quad) {
    PTA_REQUIRE(!burst_quad_refusal(b), PTA_E_ARG, "pta_engine_burst_add: remove_quad needs psr_off, quad_q and quad_c");
    int rc = pta_engine_burst_quad(burst_host, R, stream);
    if (rc != PTA_OK) return rc;
  }
  const dim3 grid(p.n_tiles, groups), block(PTA_ENGINE_TILE);
  hipStream_t s = pta_stream(stream);
  const int acc = accumulate ? 1 : 0;
  if (quad)
    hipLaunchKernelGGL((k_engine_burst_add<true>), grid, block, 0, s, p.tile_psr, p.tile_start, p.tile_count, b.toa_s, b.wav, b.kk, b.count, b.n_wav,
                       p.n_psr, b.psr_off, b.quad_q, b.quad_c, R, out, ld_out, acc);
  else
    hipLaunchKernelGGL((k_engine_burst_add<false>), grid, block, 0, s, p.tile_psr, p.tile_start, p.tile_count, b.toa_s, b.wav, b.kk, b.count, b.n_wav,
                       p.n_psr, b.psr_off, b.quad_q, b.quad_c, R, out, ld_out, acc);
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}

__global__ __launch_bounds__(PTA_ENGINE_TILE) void k_engine_transient_add(const int32_t *__restrict__ tile_psr, const int32_t *__restrict__ tile_start,
                                                                          const int32_t *__restrict__ tile_count, const double *__restrict__ toa_s,
                                                                          const double *__restrict__ tab, const int32_t *__restrict__ count, int V,
                                                                          int R, double *__restrict__ out, int64_t ld_out, int accumulate) {
  const int tile = blockIdx.x;
  const int i = threadIdx.x;
  if (i >= tile_count[tile]) return;  // no barriers below
  const int a = tile_psr[tile];
  const int64_t col = (int64_t)tile_start[tile] + i;
  const double t = toa_s[col];
  const int r_lo = blockIdx.y * BURST_ADD_RG, r_hi = min(R, r_lo + BURST_ADD_RG);
  for (int r = r_lo; r < r_hi; ++r) {
    const int nv = burst_count(count, r, V);
    if (nv == 0 && accumulate) continue;
    const double v = transient_term(tab + (int64_t)r * V * PTA_NT_NTAB, nv, a, t);
    double *o = out + (int64_t)r * ld_out + col;
    *o = accumulate ? *o + v : v;
  }
}

extern "C" int pta_engine_transient_add(const pta_engine_plan *plan_host, const pta_transient_engine *nt_host, int R, double *out, int64_t ld_out,
                                        int accumulate, void *stream) {
  PTA_REQUIRE(plan_host && nt_host && out, PTA_E_ARG, "pta_engine_transient_add: NULL argument");
  const pta_engine_plan &p = *plan_host;
  const pta_transient_engine &t = *nt_host;
  PTA_REQUIRE(p.tile_psr && p.tile_start && p.tile_count && t.toa_s && t.tab, PTA_E_ARG, "pta_engine_transient_add: tiles / TOAs / table missing");
  PTA_REQUIRE(R > 0 && p.n_tiles > 0 && t.n_psr == p.n_psr && ld_out >= p.n_toa && t.n_wav >= 1 && t.n_wav <= PTA_BURST_WMAX, PTA_E_ARG,
              "pta_engine_transient_add: R=%d n_tiles=%d n_psr=%d/%d ld_out=%lld n_wav=%d", R, p.n_tiles, t.n_psr, p.n_psr, (long long)ld_out,
              t.n_wav);
  PTA_REQUIRE(((uintptr_t)out & 7) == 0, PTA_E_ARG, "pta_engine_transient_add: out must be 8-byte aligned");
  const unsigned groups = pta_cdiv(R, BURST_ADD_RG);
  PTA_REQUIRE(groups <= 65535, PTA_E_ARG, "pta_engine_transient_add: R=%d too large for one launch", R);
  hipLaunchKernelGGL(k_engine_transient_add, dim3(p.n_tiles, groups), dim3(PTA_ENGINE_TILE), 0, pta_stream(stream), p.tile_psr, p.tile_start,
                     p.tile_count, t.toa_s, t.tab, t.count, t.n_wav, R, out, ld_out, accumulate ? 1 : 0);
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}
