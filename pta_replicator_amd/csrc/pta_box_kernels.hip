// The uniform box draw behind every per-realisation prior (pta_hyper_uniform, pta_hyper_uniform_field, pta_cw_uniform,
// pta_cw_catalog_uniform, pta_bwm_uniform: the entries keep their own argument checks and call the launcher):
//   pta_box_uniform_launch  out[R, S, n_par]: column j of source s of realisation r0 + r = pta_box_draw (pta_rng.h) of pair j of stream
//                           (kind, field0 + s) in the box (lo[j], hi[j]); S = 1 is the plain [R, n_par] table
#include "pta_common.h"
#include "pta_rng.h"

__global__ void k_box_uniform(uint64_t seed, uint64_t r0, int R, int S, int n_par, uint32_t kind, uint32_t field0,
                              const double *__restrict__ lo, const double *__restrict__ hi, double *__restrict__ out) {
  const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;  // (r, s, j): R S n_par < 2^31, so 32-bit index arithmetic
  if (idx >= (uint32_t)R * S * n_par) return;
  const uint32_t j = idx % n_par, rs = idx / n_par;
  const uint32_t s = rs % S, r = rs / S;
  out[idx] = pta_box_draw(seed, r0 + r, pta_stream_id(kind, field0 + s), j, lo[j], hi[j]);
}

// the caller has checked the pointers, R, S, n_par > 0, R S n_par < 2^31 and field0 + S - 1 <= 0xFFFFFF
int pta_box_uniform_launch(uint64_t seed, uint64_t r0, int R, int S, int n_par, uint32_t kind, uint32_t field0, const double *lo,
                           const double *hi, double *out, hipStream_t stream) {
  hipLaunchKernelGGL(k_box_uniform, dim3(pta_cdiv((int64_t)R * S * n_par, 256)), dim3(256), 0, stream, seed, r0, R, S, n_par, kind, field0, lo,
                     hi, out);
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}
