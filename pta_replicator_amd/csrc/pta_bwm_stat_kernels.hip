// Earth-term burst-with-memory matched filter of whole ensembles (pta_replicator_amd/bwm_statistic.py holds the definitions and the
// realisation-independent preparation).  The projection Q[r, a, j] = W_a[j] . r_a is pta_fstat_project (csrc/pta_fstat_kernels.hip),
// unchanged; this file holds what follows it:
//
//   pta_bwm_stat   N_rjs = sum_a phi_as q_raj (a 2-vector) on the matrix cores, Fb = 1/2 N^T M_js^-1 N and A = M_js^-1 N in registers; the
//                  full map (and the amplitudes), or the per-tile maxima folded over the sky tiles in ascending order
//
// The kernel and the launcher are pta_sky_stat.h's, shared with pta_fstat_fe; what is the burst's own is the policy below.
#include "pta_sky_stat.h"

// 16 epochs per workgroup, the rows of a wave's A tile in their order: accumulator register e of a lane is its cell e (epoch j0 + g +
// 4 e) in both chains, the two components of N_rjs.  M_js^-1 is 2 x 2, packed (00, 01, 11).
struct bwm_stat {
  static constexpr int JB = 16, NC = 4, NM = 3, QPJ = 1;
  static constexpr bool AMP = true;
  static __device__ __forceinline__ int64_t qoff(int a, int C, int) { return (int64_t)a * C; }
  static __device__ __forceinline__ int acol(int m) { return m; }
  static __device__ __forceinline__ double value(const double (&mi)[3], const pta_f64x4 &np_, const pta_f64x4 &nc_, int cell, double &a0, double &a1) {
    a0 = fma(mi[1], nc_[cell], mi[0] * np_[cell]);  // A = M^-1 N
    a1 = fma(mi[2], nc_[cell], mi[1] * np_[cell]);
    return 0.5 * fma(nc_[cell], a1, np_[cell] * a0);  // 1/2 N^T A
  }
};

extern "C" int pta_bwm_stat_plan(int P, int J, int R, int S, int32_t *plan) { return pta_sky_stat_plan<bwm_stat>("pta_bwm_stat_plan", P, J, R, S, plan); }

extern "C" int pta_bwm_stat(const double *Q, int64_t ld_q, int P, int C, int J, int R, const double *phi, int S, const double *Minv, double *fb,
                            int64_t ld_fb, double *amp, int64_t ld_amp, double *fb_max, int64_t ld_max, int32_t *fb_arg, int64_t ld_arg,
                            double *part_val, int32_t *part_arg, void *stream) {
  PTA_REQUIRE(Q && phi && Minv, PTA_E_ARG, "pta_bwm_stat: NULL argument");
  PTA_REQUIRE(P >= 2 && P <= PTA_FSTAT_PMAX && J >= 1 && C >= J && C <= PTA_FSTAT_CMAX && R > 0 && S >= 1, PTA_E_ARG,
              "pta_bwm_stat: P=%d (2..%d) J=%d C=%d (J <= C <= %d) R=%d S=%d", P, PTA_FSTAT_PMAX, J, C, PTA_FSTAT_CMAX, R, S);
  PTA_REQUIRE(ld_q >= (int64_t)P * C, PTA_E_ARG, "pta_bwm_stat: ld_q=%lld < P*C=%lld", (long long)ld_q, (long long)P * C);
  return pta_sky_stat_launch<bwm_stat>("pta_bwm_stat", "fb", Q, ld_q, P, C, J, R, phi, S, Minv, fb, ld_fb, amp, ld_amp, fb_max, ld_max, fb_arg, ld_arg,
                                       part_val, part_arg, stream);
}
