// A binned binary population per realisation (ReplicaEngine.set_population): theta of the catalogue and free-spectrum paths, made on chip.
//   pta_pop_draw_select  one workgroup per (realisation, frequency bin): Poisson counts of the bin's cells (pta_pop.h; or counts read
//                        from the caller), w = ((N hs2) fo) t_obs, the k loudest cells kept in LDS, the rest summed
//   pta_pop_theta        one workgroup per realisation: the selection concatenated bin-major, the labels gathered, 0.5 log10(free_spec)
// Selection: an LDS candidate buffer of POP_CAP >= PTA_POP_KMAX + PTA_POP_CHUNK entries and a threshold (tau, tau_idx) in LDS that
// changes only between barriers.  A lane pushes (w, N, original index) when its cell beats the threshold in the order "larger w first,
// then the lower original index" (an LDS counter hands out the slot: the buffer's content as a SET does not depend on the arrival
// order), else adds w to its own accumulator.  When the next chunk might not fit, the workgroup sorts the buffer by that order
// (bitonic, a total order: the sorted buffer is deterministic), keeps the first k, adds the evicted entry at position p to the
// accumulator of thread (p - k) mod 256 and sets the threshold to the k-th entry.  After the last chunk one more sort; then the thread
// accumulators are summed by a fixed tree (xor butterfly per wave, (w0 + w1) + (w2 + w3) over the waves).  No global atomics, no split
// over workgroups, every loop bounded by the chunk count, log2^2 of POP_CAP or the sampler's 255 / 64: a (realisation, bin) result is the
// same bits whatever R, r0 or the other rows of the launch are.
#include "pta_common.h"
#include "pta_rng.h"
#include "pta_pop.h"

#define POP_THREADS 256
#define POP_UNROLL (PTA_POP_CHUNK / POP_THREADS)
#define POP_CAP 2048  // a power of two (bitonic network) >= PTA_POP_KMAX + PTA_POP_CHUNK

static_assert(POP_CAP >= PTA_POP_KMAX + PTA_POP_CHUNK && (POP_CAP & (POP_CAP - 1)) == 0, "candidate buffer: k + one chunk, a power of two");
static_assert(PTA_POP_CHUNK % POP_THREADS == 0, "a chunk is a whole number of cells per thread");

struct pop_lds {
  double w[POP_CAP];
  double n[POP_CAP];
  int32_t idx[POP_CAP];
  double part[POP_THREADS / 64];
  double tau;
  int32_t tau_idx;
  int32_t count;
};

// (wa, ia) comes before (wb, ib): larger w first, ties to the lower original index.  The pad entries (-1, INT32_MAX) come last.
__device__ __forceinline__ bool pop_before(double wa, int32_t ia, double wb, int32_t ib) { return wa > wb || (wa == wb && ia < ib); }

// sort the first cnt entries of the buffer (cnt the same in every thread), keep min(cnt, k), hand the evicted ones to the thread
// accumulators, move the threshold.  Entered and left with the buffer quiescent (a barrier behind the last push; ends with a barrier).
__device__ __forceinline__ void pop_prune(pop_lds &s, int cnt, int k, double &acc) {
  const int tid = threadIdx.x;
  int n = 2;
  while (n < cnt) n <<= 1;  // <= POP_CAP
  for (int p = cnt + tid; p < n; p += POP_THREADS) {
    s.w[p] = -1.0;
    s.n[p] = 0.0;
    s.idx[p] = INT32_MAX;
  }
  for (int size = 2; size <= n; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int t = tid; t < (n >> 1); t += POP_THREADS) {
        const int i = 2 * t - (t & (stride - 1)), j = i + stride;
        const double wi = s.w[i], wj = s.w[j];
        const int32_t ii = s.idx[i], ij = s.idx[j];
        const bool first_half = (i & size) == 0;  // this pair is ordered "before" first; the other half the other way round
        if (first_half ? pop_before(wj, ij, wi, ii) : pop_before(wi, ii, wj, ij)) {
          const double ni = s.n[i], nj = s.n[j];
          s.w[i] = wj, s.w[j] = wi;
          s.idx[i] = ij, s.idx[j] = ii;
          s.n[i] = nj, s.n[j] = ni;
        }
      }
    }
  __syncthreads();
  const int keep = min(cnt, k);
  for (int p = keep + tid; p < cnt; p += POP_THREADS) acc += s.w[p];
  __syncthreads();
  if (tid == 0) {
    s.count = keep;
    if (cnt >= k) {
      s.tau = s.w[k - 1];
      s.tau_idx = s.idx[k - 1];
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(POP_THREADS) void k_pop_draw_select(pta_pop_plan pl, uint64_t seed, uint64_t r0, const double *__restrict__ counts,
                                                                 int64_t ld_counts, double *__restrict__ counts_out, int64_t ld_counts_out,
                                                                 int32_t *__restrict__ sel_cell, double *__restrict__ sel_number,
                                                                 double *__restrict__ sel_w, int32_t *__restrict__ sel_count,
                                                                 double *__restrict__ free_spec) {
  __shared__ pop_lds s;
  const int tid = threadIdx.x;
  const int F = pl.n_bins, k = pl.k;
  const int64_t r = blockIdx.x / F;
  const int bin = (int)(blockIdx.x % F);
  const uint64_t rho = r0 + (uint64_t)r;
  pta_rng_stage_tables();  // Box-Muller tables -> LDS for the rates of the normal regime (pta_rng.h)
  if (tid == 0) {
    s.count = 0;
    s.tau = 0.0;  // only w > 0 is ever selected
    s.tau_idx = -1;
  }
  __syncthreads();
  const int lo = pl.cell_ptr[bin], hi = pl.cell_ptr[bin + 1];
  double acc = 0.0;
  for (int base = lo; base < hi; base += PTA_POP_CHUNK) {  // at most ceil(n_sorted / PTA_POP_CHUNK) steps
    const int cnt = s.count;
    if (cnt + PTA_POP_CHUNK > POP_CAP) pop_prune(s, cnt, k, acc);  // cnt is the same in every thread
    const double tau = s.tau;
    const int32_t tau_idx = s.tau_idx;
    __syncthreads();  // every thread has read the counter and the threshold before the first push of this chunk
#pragma unroll
    for (int u = 0; u < POP_UNROLL; ++u) {
      const int i = base + u * POP_THREADS + tid;
      if (i < hi) {
        const int32_t cell = pl.orig[i];
        const double N = counts ? counts[r * ld_counts + cell] : pta_pop_poisson(seed, rho, (uint32_t)cell, pl.number[i]);
        if (counts_out) counts_out[r * ld_counts_out + cell] = N;
        const double w = pta_pop_weight(N, pl.hs2[i], pl.fo[i], pl.t_obs);
        if (pop_before(w, cell, tau, tau_idx)) {
          const int slot = atomicAdd(&s.count, 1);  // LDS counter; < POP_CAP by the prune rule above
          if (slot < POP_CAP) {
            s.w[slot] = w;
            s.n[slot] = N;
            s.idx[slot] = cell;
          }
        } else {
          acc += w;
        }
      }
    }
    __syncthreads();
  }
  pop_prune(s, min(s.count, POP_CAP), k, acc);
  const int keep = s.count;
  const int64_t o = ((int64_t)r * F + bin) * k;
  for (int p = tid; p < keep; p += POP_THREADS) {
    sel_cell[o + p] = s.idx[p];
    sel_number[o + p] = s.n[p];
    sel_w[o + p] = s.w[p];
  }
  for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m);
  if ((tid & 63) == 0) s.part[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    sel_count[(int64_t)r * F + bin] = keep;
    free_spec[(int64_t)r * F + bin] = 1e-100 + ((s.part[0] + s.part[1]) + (s.part[2] + s.part[3]));
  }
}

static int pop_check(const pta_pop_plan &pl, int R, const char *who) {
  PTA_REQUIRE(R > 0 && pl.n_cells > 0 && pl.n_sorted >= 0 && pl.n_sorted <= pl.n_cells, PTA_E_ARG, "%s: R=%d n_cells=%d n_sorted=%d", who, R,
              pl.n_cells, pl.n_sorted);
  PTA_REQUIRE(pl.n_bins >= 1 && pl.n_bins <= PTA_POP_FMAX, PTA_E_ARG, "%s: n_bins=%d (1..%d)", who, pl.n_bins, PTA_POP_FMAX);
  PTA_REQUIRE(pl.k >= 1 && pl.k <= PTA_POP_KMAX, PTA_E_ARG, "%s: k=%d (1..%d)", who, pl.k, PTA_POP_KMAX);
  PTA_REQUIRE((int64_t)R * pl.n_bins * pl.k < (1LL << 31), PTA_E_ARG, "%s: problem too large", who);
  return PTA_OK;
}

extern "C" int pta_pop_draw_select(const pta_pop_plan *plan, uint64_t seed, uint64_t r0, int R, const double *counts, int64_t ld_counts,
                                   double *counts_out, int64_t ld_counts_out, int32_t *sel_cell, double *sel_number, double *sel_w,
                                   int32_t *sel_count, double *free_spec, void *stream) {
  PTA_REQUIRE(plan && sel_cell && sel_number && sel_w && sel_count && free_spec, PTA_E_ARG, "pta_pop_draw_select: NULL argument");
  const pta_pop_plan &pl = *plan;
  PTA_REQUIRE(pl.cell_ptr && pl.number && pl.hs2 && pl.fo && pl.orig, PTA_E_ARG, "pta_pop_draw_select: NULL table");
  const int rc = pop_check(pl, R, "pta_pop_draw_select");
  if (rc != PTA_OK) return rc;
  PTA_REQUIRE(pl.t_obs > 0.0 && pl.t_obs < INFINITY, PTA_E_ARG, "pta_pop_draw_select: t_obs=%g", pl.t_obs);
  PTA_REQUIRE(!counts || ld_counts >= pl.n_cells, PTA_E_ARG, "pta_pop_draw_select: ld_counts=%lld too small", (long long)ld_counts);
  PTA_REQUIRE(!counts_out || ld_counts_out >= pl.n_cells, PTA_E_ARG, "pta_pop_draw_select: ld_counts_out=%lld too small", (long long)ld_counts_out);
  hipLaunchKernelGGL(k_pop_draw_select, dim3((unsigned)((int64_t)R * pl.n_bins)), dim3(POP_THREADS), 0, pta_stream(stream), pl, seed, r0, counts,
                     ld_counts, counts_out, ld_counts_out, sel_cell, sel_number, sel_w, sel_count, free_spec);
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}

__global__ __launch_bounds__(64) void k_pop_theta(pta_pop_plan pl, const int32_t *__restrict__ sel_cell, const double *__restrict__ sel_number,
                                                  const int32_t *__restrict__ sel_count, const double *__restrict__ free_spec,
                                                  double *__restrict__ log10_mc, double *__restrict__ log10_fgw, double *__restrict__ log10_dist,
                                                  double *__restrict__ pop_number, int32_t *__restrict__ pop_cell, int32_t *__restrict__ cw_count,
                                                  double *__restrict__ hc, int64_t ld_hc) {
  __shared__ int32_t pre[PTA_POP_FMAX + 1];
  const int tid = threadIdx.x;
  const int F = pl.n_bins, k = pl.k, S = F * k;
  const int64_t r = blockIdx.x;
  if (tid == 0) {
    int32_t sum = 0;
    for (int b = 0; b < F; ++b) {  // F <= 64
      pre[b] = sum;
      sum += min(max(sel_count[r * F + b], 0), k);  // the clamp keeps every walk inside the row whatever the array holds
    }
    pre[F] = sum;
  }
  __syncthreads();
  const int total = pre[F];
  const double nan = __builtin_nan("");
  for (int e = tid; e < S; e += 64) {
    const int b = e / k, j = e - b * k;
    if (j >= pre[b + 1] - pre[b]) continue;
    const int64_t d = r * S + pre[b] + j;
    const int32_t c = sel_cell[r * S + e];
    const bool ok = c >= 0 && c < pl.n_cells;
    log10_mc[d] = ok ? pl.log10_mc[c] : nan;
    log10_fgw[d] = ok ? pl.log10_fo[c] : nan;
    log10_dist[d] = ok ? pl.log10_dl[c] : nan;
    pop_number[d] = sel_number[r * S + e];
    pop_cell[d] = c;
  }
  for (int e = total + tid; e < S; e += 64) {
    const int64_t d = r * S + e;
    log10_mc[d] = log10_fgw[d] = log10_dist[d] = pop_number[d] = nan;
    pop_cell[d] = -1;
  }
  for (int b = tid; b < F; b += 64) hc[r * ld_hc + b] = 0.5 * log10(free_spec[r * F + b]);
  if (tid == 0) cw_count[r] = total;
}

extern "C" int pta_pop_theta(const pta_pop_plan *plan, int R, const int32_t *sel_cell, const double *sel_number, const int32_t *sel_count,
                             const double *free_spec, double *log10_mc, double *log10_fgw, double *log10_dist, double *pop_number,
                             int32_t *pop_cell, int32_t *cw_count, double *gwb_log10_hc, int64_t ld_hc, void *stream) {
  PTA_REQUIRE(plan && sel_cell && sel_number && sel_count && free_spec && log10_mc && log10_fgw && log10_dist && pop_number && pop_cell && cw_count &&
                  gwb_log10_hc,
              PTA_E_ARG, "pta_pop_theta: NULL argument");
  const pta_pop_plan &pl = *plan;
  PTA_REQUIRE(pl.log10_mc && pl.log10_fo && pl.log10_dl, PTA_E_ARG, "pta_pop_theta: NULL table");
  const int rc = pop_check(pl, R, "pta_pop_theta");
  if (rc != PTA_OK) return rc;
  PTA_REQUIRE(ld_hc >= pl.n_bins, PTA_E_ARG, "pta_pop_theta: ld_hc=%lld too small", (long long)ld_hc);
  hipLaunchKernelGGL(k_pop_theta, dim3((unsigned)R), dim3(64), 0, pta_stream(stream), pl, sel_cell, sel_number, sel_count, free_spec, log10_mc,
                     log10_fgw, log10_dist, pop_number, pop_cell, cw_count, gwb_log10_hc, ld_hc);
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}
