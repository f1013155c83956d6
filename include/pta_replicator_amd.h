/*
 * pta_replicator_amd — C ABI of the MI355X (gfx950) stochastic-injection hot path.
 *
 * The reference (bencebecsy/pta_replicator) is pure Python with no FFI layer of its own
 * (SURVEY.md §8b); this header therefore defines the boundary a maintainer would bind with
 * ctypes (INTEGRATION.md shows the stub).  Each entry point cites the reference code it
 * replaces as file:line under /root/reference/pta_replicator/.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes; no torch / C++ types.
 *  - Every `double*` / `int32_t*` is a DEVICE pointer to contiguous memory owned by the
 *    caller (e.g. torch.Tensor.data_ptr()) unless the parameter name ends in `_host`.
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream). Calls are
 *    asynchronous on that stream; no allocation, no synchronisation inside.
 *  - Return 0 on success, a negative PTA_E_* code otherwise; pta_last_error() gives the
 *    thread-local message. No exceptions cross the boundary.
 *  - Batches: R realisations are the leading axis; `ld_*` are row strides in elements.
 *    `accumulate` = 0 overwrites `out`, 1 adds into it.
 *  - Everything is IEEE binary64, like the reference (it casts PINT's longdouble columns to
 *    float64 before any arithmetic: red_noise.py:123, :287).
 *  - No process-wide state: every option that changes what a call computes or how (Gaussian-transform mode, kernel
 *    variants) is an argument or a field of the plan struct passed to that call, so concurrent callers on different
 *    streams / threads cannot influence each other (ABI 2; ABI 1 had pta_set_* switches).
 */
#ifndef PTA_REPLICATOR_AMD_H
#define PTA_REPLICATOR_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PTA_ABI_VERSION 8

#define PTA_OK 0
#define PTA_E_ARG (-1)     /* bad argument (sizes, NULL pointers, unsupported lmax ...) */
#define PTA_E_HIP (-2)     /* HIP runtime error; message carries hipGetErrorString */
#define PTA_E_NOTPD (-3)   /* reserved: matrix not positive definite (see `info` of pta_potrf_batched) */

/* ---------------------------------------------------------------- library ---------- */
int pta_abi_version(void);
const char *pta_last_error(void);
/* number of CUs / wavefront size / gcnArchName of the current HIP device */
int pta_device_info(int *cu_count, int *wavefront, char *arch, int arch_len);

/* ---------------------------------------------------------------- RNG -------------- */
/* Throughput-mode draws. The reference consumes NumPy's global legacy stream
 * (red_noise.py:119,127,176,238-240; white_noise.py:80,105-109,155,182); on the device every
 * deviate is Philox-4x32-10(key = seed, counter = (pair, stream, realisation)) + Box-Muller.
 * stream ids: (kind << 24) | pulsar, kind = 1 GWB, 2 RN, 3 WN, 4 ECORR, 5 TD (N_a x N_a factor), 6 TDGW (GWB grid factor),
 * 7 HYPER (pulsar field 0: per-realisation hyperparameters, pair j = parameter column, uniform u2; pta_hyper_uniform.  Field 1: the
 * nodes of a per-realisation GWB spectrum, pair j = node j; pta_hyper_uniform_field.  Fields 3, 4, 5: per-realisation EFAC, log10
 * EQUAD and log10 ECORR, pair j = white-noise / ECORR group j; pta_hyper_uniform_field),
 * 8 CW (pulsar field 0: per-realisation CW source labels, pair j = label column, uniform u2; pta_cw_uniform.  In a catalogue the
 * field is the source index s, pta_cw_catalog_uniform),
 * 9 BWM (pulsar field 0: per-realisation burst-with-memory labels, pair j = label column, uniform u2; pta_bwm_uniform),
 * 13 BURST (field 0: the sky labels of a per-realisation wavelet burst, field 1 + w: wavelet w; pair j = label column; pta_burst_uniform),
 * 14 NT (field v: noise transient v of the realisation, pair j = label column; pta_transient_uniform),
 * 15 CE (field e: chromatic event slot e of the realisation, pair j = label column; pta_chrom_event_uniform). */

/* `rng_fast` (argument or plan field of every call that draws on chip) selects the Gaussian transform: 0 (default) = fp64
 * Box-Muller with < 1 ulp log / sincos, 1 = "fast RNG math": the same uniforms through the hardware fp32 log / sqrt / sin /
 * cos (deviates accurate to ~1e-6).  It is part of what defines realisation r: all ranks of a job must use the same value
 * (pta_replicator_amd.distributed checks).                                                                              */

/* Known-answer access to the raw generator: out[i] = 4 x u32 of
 * Philox4x32-10(counter = ctr[i][0..3], key = key[0..1]).  ctr/key/out are device u32.   */
int pta_rng_philox_raw(const uint32_t *ctr, const uint32_t *key, int n, uint32_t *out, void *stream);

/* Dump the normals the fused kernels would use, in the layout the replay kernels read:
 *   interleave = 1: z0[r*ld + 2p] = first, z0[r*ld + 2p + 1] = second deviate of pair p (z1 unused)
 *   interleave = 0: z0[r*ld + p] = first, z1[r*ld + p] = second deviate of pair p
 * for pairs p in [0, npairs), realisations r0 .. r0+R-1.                                   */
int pta_rng_fill_normal(uint64_t seed, uint64_t r0, int R, uint32_t stream_id, int npairs, int interleave,
                        double *z0, double *z1, int64_t ld, int rng_fast, void *stream);
/* The same fill for all blocks of a pta_td_plan in ONE launch: z[r * ld + blk_zoff[b] + j] = deviate j of stream (stream_kind, b),
 * j < blk_n[b] rounded up to even (pairs are written whole), r < R.  blk_n / blk_zoff: device arrays (blk_zoff even), max_n = the
 * largest blk_n; ld even, z 16-byte aligned.                                                                                    */
int pta_rng_fill_normal_blocks(uint64_t seed, uint64_t r0, int R, uint32_t stream_kind, int n_blocks, const int32_t *blk_n,
                               const int32_t *blk_zoff, int max_n, double *z, int64_t ld, int rng_fast, void *stream);

/* ---------------------------------------------------------------- red noise -------- */
/* Fourier design matrix, transposed: Ft[c*N + i] = column c of F for TOA i.
 * Replaces create_fourier_design_matrix_red (red_noise.py:36-103).
 *   arg = ((2 pi) * (t[i] - t_ref)) * f[k] + phase[k]        (phase may be NULL = 0)
 *   cos_first = 0 (default convention, t_ref = 0): c = 2k sin, c = 2k+1 cos   (:98-101)
 *   cos_first = 1 (libstempo convention, t_ref = t[0]): c = 2k cos, c = 2k+1 sin (:92-96) */
int pta_rn_basis(const double *t, int N, double t_ref, const double *f, const double *phase, int nmodes,
                 int cos_first, double *Ft, int64_t ldf, void *stream);

/* out[r*ld_out + i] (+)= sum_c Ft[c*ldf + i] * coef[r*ld_coef + c],  c < K.
 * Replaces dt = F @ (sqrt(prior) * randn) (red_noise.py:127-128); coef = sqrt(prior)*z.    */
int pta_rn_synth(const double *Ft, int64_t ldf, int N, int K, const double *coef, int64_t ld_coef, int R, double *out,
                 int64_t ld_out, int accumulate, void *stream);

/* ---------------------------------------------------------------- white noise ------ */
/* out[r,i] (+)= (efac[i]*sigma[i])*z1[r,i] + (tnequad ? equad[i] : efac[i]*equad[i])*z2[r,i]
 * Replaces add_measurement_noise's arithmetic (white_noise.py:105-109).                    */
int pta_wn(const double *sigma, const double *efac, const double *equad, int N, int tnequad, const double *z1,
           const double *z2, int64_t ld_z, int R, double *out, int64_t ld_out, int accumulate, void *stream);

/* Greedy epoch bucketing on the HOST (realisation independent). Replaces quantize_fast
 * (white_noise.py:7-44) without the dense U: epoch_of_host[i] = column of U holding TOA i;
 * first_index_host[e] = first (earliest) TOA of epoch e, whose flag labels the epoch (:35).
 * order_host = np.argsort(times) to reproduce the reference's tie order exactly, or NULL for a
 * stable sort.  first_index_host must have room for N entries.                             */
int pta_quantize_epochs(const double *times_host, int N, double dt, const int64_t *order_host,
                        int32_t *epoch_of_host, int32_t *first_index_host, int *n_epochs);

/* HOST helper of the CW-catalogue path: out_host[i] = x_host[3i .. 3i+2] . y_host[0..2], summed as fma(x2, y2, fma(x1, y1, x0 * y0)) -
 * the association np.dot (OpenBLAS ddot) uses for the antenna-pattern dot products of deterministic.py:364-372, so that the
 * per-source scalars of a whole catalogue are bit-identical to the reference's per-source loop without a Python-level loop.   */
int pta_dot3_host(const double *x_host, int64_t n, const double *y_host, double *out_host);
/* out_host[i] = pow(x_host[i], y) through libm's scalar pow (what the reference's per-source scalar expressions evaluate to;
 * NumPy's array power differs from it by an ulp on a few per cent of arguments).                                        */
int pta_pow_host(const double *x_host, double y, int64_t n, double *out_host);
/* HOST helper of replay mode: NumPy's LEGACY normal stream, stream i = np.random.RandomState(seeds_host[i]).randn(counts_host[i])
 * value for value (MT19937 by init_genrand, 53-bit doubles, polar method with the cached second deviate: what np.random.seed(seed);
 * np.random.randn(n) of white_noise.py:79-80,105-109,154-155,182 and red_noise.py:112-113,127 yields), written to out_host +
 * offsets_host[i]; the streams are drawn on n_threads host threads (0 = one per core, at most 16).  The state the LAST stream is left in comes back
 * in last_key_host [624], last_pos_has_host [2] = (pos, has_gauss), last_gauss_host [1] (any NULL: not wanted) - the caller installs it
 * with np.random.set_state so that the global stream continues as after the reference's sequential calls.                       */
int pta_legacy_randn(const uint32_t *seeds_host, const int64_t *counts_host, const int64_t *offsets_host, int n_streams,
                     double *out_host, uint32_t *last_key_host, int32_t *last_pos_has_host, double *last_gauss_host, int n_threads);

/* out[r,i] (+)= ecorr_epoch[epoch_of[i]] * z[r*ld_z + epoch_of[i]]
 * Replaces dt = (U*ecorrvec) @ randn(E) (white_noise.py:182): a gather, not an N x E matvec. */
int pta_ecorr(const int32_t *epoch_of, const double *ecorr_epoch, int N, int E, const double *z, int64_t ld_z, int R,
              double *out, int64_t ld_out, int accumulate, void *stream);

/* ---------------------------------------------------------------- ORF -------------- */
/* locs[a*2+0] = phi (RA, rad), locs[a*2+1] = theta (colatitude, rad) (red_noise.py:205-223). */

/* HOST helper (ABI 8) of the ORF set-up: arg_host[a*P+b] = sin(theta_a) sin(theta_b) cos(phi_a - phi_b) + cos(theta_a) cos(theta_b), the
 * argument of calczeta's arccos (spharmORFbasis.py:24), evaluated left to right through libm's scalar sin / cos like the reference's
 * per-pair loop (spharmORFbasis.py:400-408) - in C++ instead of 20 100 Python-level iterations at 200 pulsars (61 ms -> < 1 ms).
 * same_host[a*P+b] = 1 where both coordinates are identical (the exact-equality branch :23).  Symmetric [P, P] host arrays.
 * arccos / cos of the result stay with NumPy (its float64 arccos is not libm's on AVX512 hosts): spharmORFbasis.pair_zeta_cos. */
int pta_orf_pair_arguments(const double *locs_host, int P, double *arg_host, uint8_t *same_host);

/* lmax = 0, clm = [sqrt(4 pi)] fast path: orf[a*P+b] = 2*HD(zeta_ab), 2 on zeta == 0.
 * Equals red_noise.py:224-226 with the defaults.                                           */
int pta_orf_hd(const double *locs, int P, double *orf, void *stream);

/* basis[(k*P + a)*P + b], k = l*l + (m + l): spharmORFbasis.correlated_basis
 * (spharmORFbasis.py:385-434 and callees :14-382). lmax <= 8.
 * zeta_cos (device, may be NULL): zeta_cos[2*(a*P+b) + 0/1] = the pair's angular separation zeta and cos(zeta) exactly as the
 * reference computes them (calczeta :14-35, np.cos at :166; host libm).  The l >= 3 sums are ill-conditioned in cos(zeta)
 * (~1e5-1e6), so 1-2 ulp between device and libm acos/cos were a 7e-10 parity error; with the host's values it is the sums'
 * own rounding only.  NULL = both are derived on the device.                                   */
int pta_orf_basis(const double *locs, const double *zeta_cos, int P, int lmax, double *basis, void *stream);

/* orf = 2 * sum_k clm[k] * basis[k]  (red_noise.py:225-226). clm is a device array.        */
int pta_orf_combine(const double *basis, const double *clm, int nbasis, int P, double *orf, void *stream);

/* In-place lower Cholesky of B row-major n x n matrices (reads the lower triangle, zeroes the
 * strict upper one - np.linalg.cholesky's result, red_noise.py:235).  info[b] = 0, or j+1 if the
 * leading minor of order j+1 is not positive definite (LAPACK convention).  Blocked right-looking:
 * LDS panel factorisation + fp64 MFMA (v_mfma_f64_16x16x4_f64) trailing update.             */
int pta_potrf_batched(double *A, int n, int B, int32_t *info, void *stream);

/* The same factorisation for matrices with a leading dimension and a batch stride: matrix b is row-major at A + b * strideA
 * with row pitch lda >= n.  Schedule: right-looking over panels of NB = 1024 columns whose trailing update runs with K = NB
 * (the 128 x 128-tile fp64 MFMA GEMM reaches 56 TFLOP/s at K = 1024 against 36-40 at K = 256); each panel is factored
 * RECURSIVELY - left half, update of the right half with K = half the width, right half - down to 64 columns, where the
 * diagonal block is factored and inverted in registers and the rows below are solved by an MFMA product with that inverse.
 * A batch is split into two independent chains of matrices on internal streams (created on first use, joined back into
 * `stream` before returning), so that one chain's serial, memory-bound panel steps overlap the other's MFMA-bound updates.
 * flags: PTA_POTRF_ZERO_UPPER zeroes the strict upper triangle (np.linalg.cholesky's result); without it the upper triangle
 * is left holding scratch (the parked inverses of the diagonal blocks) - all TD mode needs, since pta_td_trmm_rng reads the
 * lower triangle only.  PTA_POTRF_NO_LOOKAHEAD keeps every launch on `stream` (one chain).  PTA_POTRF_NB(k) overrides the
 * panel width with k * 256 columns, PTA_POTRF_CHAINS(c) the number of chains (1..4) - both for A/B timing.             */
#define PTA_POTRF_ZERO_UPPER 1
#define PTA_POTRF_NO_LOOKAHEAD 2
#define PTA_POTRF_NB(k) (((k) & 0xFF) << 8) /* panel width override, in units of 256 columns */
#define PTA_POTRF_CHAINS(c) (((c) & 0xF) << 16) /* number of concurrent chains of matrices (default 2) */
#define PTA_POTRF_VALU 8          /* cross-check: VALU reference GEMM and substitution panel solve instead of the MFMA kernels */
#define PTA_POTRF_SUBSTITUTION 4  /* panel solves by forward substitution instead of the MFMA product with the inverted diagonal
                                     block: LAPACK-grade backward error also when the diagonal blocks are very ill-conditioned
                                     (cond(L11) * eps enters the product form) - used for the GWB grid covariance, cond ~ 3e14 */
#define PTA_POTRF_REG_STAGING 32  /* A/B: the 128 x 128-tile updates stage their operand slabs through registers (pta_dgemm algo 1)
                                     instead of by LDS DMA (global_load_lds_dwordx4, pta_dgemm algo 2 - the default) */
#define PTA_POTRF_DIAG_AHEAD 128   /* workspace scheme: the next panel's diagonal phase runs on an internal side stream as soon as its
                                     block of the trailing update is done, beside the rest of that update */
#define PTA_POTRF_DIAG64 16         /* A/B (workspace scheme): the panel's diagonal block by the 64-column recursion (k_potf2 / k_trsm_mfma /
                                     k_syrk64) + one inversion pass instead of the 128-column base case k_diag128 */
#define PTA_POTRF_LOCKSTEP 64       /* A/B (workspace scheme): all chains start together instead of one diagonal phase apart */
#define PTA_POTRF_EPI1 0x100000     /* A/B: the 128 x 128-tile products prefetch their C tile behind the last slab and store interior tiles
                                       unpredicated (pta_dgemm algo 3; also honoured by pta_potrf_ragged_plan) */
#define PTA_POTRF_LEFT 0x200000     /* workspace scheme (ABI 8), LEFT-LOOKING panel order: a finished panel is not applied to the trailing matrix;
                                     * before a panel is factored its block column is updated once with everything to its left (one tile
                                     * product of K = the panel's first column: a C tile is read and written once, not once per panel) */
#define PTA_POTRF_LEFT_SPLIT 0x400000 /* with PTA_POTRF_LEFT: the part of that update that only needs panels <= q - 2 runs ahead on an internal
                                       * side stream beside panel q - 1's diagonal phase and substitution */
#define PTA_POTRF_SOLVE_ROWS 0x800000 /* workspace scheme (ABI 8): the substitution on the rows below a panel as ONE launch - a workgroup keeps a
                                       * 128-row tile and walks the panel's 128-column blocks (reading back its own stores through L2: sc1 loads)
                                       * instead of one launch per block */
int pta_potrf_batched_ex(double *A, int n, int64_t lda, int64_t strideA, int B, int32_t *info, int flags, void *stream);

/* The same factorisation with a caller-owned workspace (device memory, `work_doubles` doubles, at least
 * pta_potrf_workspace_doubles(n, B, flags) - B * 1152^2 doubles = 10.6 MB per matrix at the default panel width; 0 = the workspace
 * scheme does not apply: n <= panel width, or the VALU / SUBSTITUTION paths).  With it a panel is factored on its nbo x nbo DIAGONAL
 * block only - a recursion whose base case is a whole 128-column group, factored AND inverted (W_jj) by one workgroup per matrix -,
 * the strips S_j = [-W_jj L11[j, <j] | W_jj] go to the workspace, and the rows below are solved by blocked substitution - ONE tile product X_j = [X_{<j} | B_j] S_j^T per 128 columns,
 * K = 128 (j + 1), in place - instead of by the recursion over the panel's full height: no 64-column solves or K = 64 updates over
 * all rows, a quarter of the launches, and what is left of the latency-bound kernels works on the diagonal block's few rows.
 * PTA_POTRF_DIAG_AHEAD additionally runs the next panel's diagonal phase on an internal side stream beside the trailing update.
 * cond(diagonal blocks) * eps enters X, as it does through the 64 x 64 inverses of pta_potrf_batched_ex; ill-conditioned matrices
 * take PTA_POTRF_SUBSTITUTION (workspace ignored).  Measured on the MI355X (tests/test_gpu_td_reference.py): on a
 * quiet TD covariance (cond 2.5e5) the normwise backward error ||A - L L^T||_F / (eps/2 ||A||_F) is 4 to 11, LAPACK's 3 to 5; on a
 * loud red-noise covariance (cond 2.7e9, 256-column panels) 30 to 9e3 where LAPACK has 3 to 5 - 1e2 to 1e3 times LAPACK's, largest
 * when one 128-column block holds all of the red noise (n = 384, 385) - and 6 at n = 1026 with the default 1024-column panels;
 * every entry stays inside the componentwise bound derived for the product form (tests/td_reference.py), filled to 0.09 at the most.
 * work == NULL or too small: identical to pta_potrf_batched_ex.                                                                  */
int64_t pta_potrf_workspace_doubles(int n, int B, int flags);
int pta_potrf_batched_ws(double *A, int n, int64_t lda, int64_t strideA, int B, int32_t *info, int flags, double *work,
                         int64_t work_doubles, void *stream);

/* Creates the internal streams / events the chained schedules of pta_potrf_batched_ws / pta_potrf_ragged use (per calling thread and
 * device; nchain <= 0: the default two chains + their look-ahead streams) NOW instead of inside the first factorisation - a HIP stream
 * is a hardware queue, ~10 ms each to create (ABI 7; profiles/r05_prepare_td_first_call.txt).  Optional: the schedules create on demand. */
int pta_potrf_warmup(int nchain);

/* RAGGED batch (ABI 6): B matrices of DIFFERENT orders factored as ONE schedule - the shape of a real pulsar timing array (the
 * reference's noise_dicts/ng15_dict.json: 68 pulsars, 68 TOA counts; test_partim: 7758 / 23023 / 35037 TOAs), which the reference
 * handles by looping over pulsars (red_noise.py:286-298) and a batch-by-equal-order scheme would run as B batches of one.
 * Matrix b: order n[b], row-major lower triangle at A + off[b], leading dimension ld[b]; n, off, ld are HOST arrays, all entries
 * EVEN (16-byte operand rows: pad an odd order with an identity row / column at its end) and ld[b] >= n[b].
 * The matrices are end-aligned: embedded in a virtual matrix whose bottom-right corner they share, so that at every time step
 * (one panel of NB columns counted from the END; NB = 1024, or 2048 when the flop-weighted mean order is >= 16384, or PTA_POTRF_NB) all matrices that have been reached have the same panel boundaries,
 * trailing size and tile grids - every kernel of the step is one launch over them; a matrix enters at the step that contains its
 * first column, with the panel cut at its front (masked inside the kernels).  The diagonal phases (latency chains) are paid once
 * per time step instead of once per matrix and panel.  Chains / look-ahead / workspace scheme as pta_potrf_batched_ws.
 *   1. pta_potrf_ragged_plan(n, off, ld, B, flags, plan_host, &work_doubles) fills plan_host[pta_potrf_ragged_plan_words(B)]
 *      (int64 words; flags: PTA_POTRF_CHAINS / PTA_POTRF_NB / PTA_POTRF_NO_LOOKAHEAD) and returns the workspace size;
 *   2. the caller copies the plan to device memory (plan_dev) - it is reusable for any number of factorisations of this layout;
 *   3. pta_potrf_ragged(A, plan_host, plan_dev, info, work, work_doubles, stream): asynchronous; info[b] (device, caller's order)
 *      = 0 or the 1-based index of the first non-positive pivot of matrix b.  The upper triangles are left holding scratch.   */
int64_t pta_potrf_ragged_plan_words(int B);
int pta_potrf_ragged_plan(const int32_t *n, const int64_t *off, const int64_t *ld, int B, int flags, int64_t *plan_host,
                          int64_t *work_doubles);
int pta_potrf_ragged(double *A, const int64_t *plan_host, const int64_t *plan_dev, int32_t *info, double *work,
                     int64_t work_doubles, void *stream);


/* ---------------------------------------------------------------- GWB -------------- */
/* The reference's chain (red_noise.py:238-287): w -> M@w -> *sqrt(C), zero DC/Nyquist -> Hermitian
 * pack to n = 2Nf-2 -> real(ifft)/dt -> crop [i0, i0+npts) -> linear interpolation onto TOAs.
 * Only npts of the n time samples are ever used, and mixing with M commutes with the DFT, so the
 * device evaluates   G0 = W . T   (pruned inverse DFT as a dense fp64 GEMM on MFMA, T the twiddle
 * matrix with sqrt(C)/(n dt) folded in), then G = M . G0 on the npts grid, then interpolates.  */

/* T[(c*(Nf-2) + k-1)*ldt + jj], c = 0 (cos) / 1 (sin), k = 1..Nf-2, jj < npts:
 *   T0 =  (2/(n dt)) sqrtC[k] cos(2 pi (i0+jj) k / n),   T1 = -(2/(n dt)) sqrtC[k] sin(...)
 * (red_noise.py:265-279, :285 with i0 = 10).                                              */
int pta_gwb_twiddle(const double *sqrtC, int Nf, int npts, int i0, double inv_dt, double *T, int64_t ldt, void *stream);

/* G0[m*ldg + jj] = sum_k wre[m,k] T0[k-1,jj] + wim[m,k] T1[k-1,jj];  w interleaved (re,im),
 * row stride ldw doubles, w[m*ldw + 2k] = Re w[m,k].  algo: 0 = VALU reference kernel,
 * 1 = MFMA kernel.                                                                          */
int pta_gwb_idft(const double *w, int64_t ldw, int M, int Nf, const double *T, int64_t ldt, int npts, double *G0,
                 int64_t ldg, int algo, void *stream);

/* Throughput mode: same transform with w generated on chip - row m = r*P + a uses stream (GWB, a) of
 * realisation r0 + r, pair k -> (Re, Im) of w[a,k] (red_noise.py:238-240) - and with the output window's
 * mirror symmetry exploited:  x[c + j'] = E - O, x[c - j'] = E + O  around the window centre c, which
 * halves the flops.  pta_gwb_twiddle_sym lays the half-window twiddles out slab by slab exactly as the
 * kernel stages them through LDS (Tsym) plus the per-bin rotation e^{2 pi i c k / n} (rot); sizes in doubles
 * come from pta_gwb_twiddle_sym_size.  `variant` selects the column tiling of a workgroup - 0 = 19 tiles of 16 (the
 * whole half window of npts = 600, one wave per SIMD), 1 (recommended) = 10 tiles (two chunks, two waves per SIMD),
 * 2 = 7 tiles (three chunks) - and, since the Tsym layout depends on it, must be the same in all three calls.   */
int64_t pta_gwb_twiddle_sym_size(int Nf, int npts, int variant, int64_t *rot_doubles);
int pta_gwb_twiddle_sym(const double *sqrtC, int Nf, int npts, int i0, double inv_dt, double *Tsym, double *rot,
                        int variant, void *stream);
int pta_gwb_idft_rng(uint64_t seed, uint64_t r0, int R, int P, int Nf, const double *Tsym, const double *rot, int npts,
                     double *G0, int64_t ldg, int variant, int rng_fast, void *stream);

/* The same stage as a chirp-z (Bluestein) transform, the default of the batched engine whenever
 * (Nf-2) + npts - 2 < 4096 (pta_gwb_czt_fits): x_j = (2/(n dt)) Re(W^{j^2/2} sum_k (sqrtC_k w_k W^{k^2/2}) W^{-(j-k)^2/2}),
 * one circular convolution of length 4096 per (realisation, pulsar) row = two in-LDS radix-8 fp64 FFTs,
 * ~0.5 MFLOP per row instead of 3.6 MFLOP of dense DFT.  pta_gwb_czt_setup fills pre[2*4096] (pre-chirp with
 * sqrtC), FB[2*4096] (chirp spectrum / 4096, digit-reversed order, stored [q][b] per 8-point butterfly b), tw[2*4096] (FFT twiddles), post[2*npts].
 * (FB: the chirp W^{-u^2/2} on the lags u = min(i0 - (Nf-2), 0) .. i0 + npts - 2, lag u in slot u mod 4096; logical position 8 b + q of
 * its radix-8 decimation-in-frequency spectrum, the frequency with the position's four octal digits reversed, sits at FB[2 (512 q + b)].)
 * pta_gwb_czt: w == NULL draws on chip (stream (GWB, a), pair k, like pta_gwb_idft_rng), else w[R*P x ldw]
 * interleaved (re, im) rows as in pta_gwb_idft (ldw = 0: one row of draws shared by all rows - timing probe).
 * pta_gwb_czt_fits: 1 when Nf >= 3, npts >= 1, i0 >= 1, the lags fit the convolution, (Nf-2) + npts - 2 < 4096, and so does the
 * window itself, i0 + npts - 2 < 4096; else 0, and pta_gwb_czt_setup, pta_gwb_czt and pta_gwb_czt_scaled refuse with PTA_E_ARG.  */
int pta_gwb_czt_fits(int Nf, int npts, int i0);
/* pta_gwb_czt `variant`: 0 (default): six LDS exchanges, draws / product / output in registers, computed twiddles;
 *                        1: every stage through LDS with table twiddles (cross-check); 10+f: ladder step f (25 = the default
 *                        without its twiddle reuse and pruned last butterfly; 137 = all steps, with the LDS twiddle table; all steps from 25 up are
 *                        bit-identical to each other)                                                                    */
int pta_gwb_czt_setup(const double *sqrtC, int Nf, int npts, int i0, double inv_dt, double *pre, double *FB, double *tw,
                      double *post, void *stream);
int pta_gwb_czt(uint64_t seed, uint64_t r0, const double *w, int64_t ldw, int R, int P, int Nf, int npts, int i0,
                const double *pre, const double *FB, const double *tw, const double *post, double *G0, int64_t ldg,
                int variant, int rng_fast, void *stream);

/* Per-realisation GWB spectrum (ABI 8, additive): the two on-chip-draw transforms above with every drawn pair of bin k of row
 * (r, a) multiplied by scale[r * ld_scale + k] (k = 1 .. Nf-2) before the pre-chirp / twiddle product.  With scale =
 * hcf(theta_r) / hcf0 (pta_gwb_spectrum_scale) the row is the one a table built for theta_r gives: the ORF mix is linear and the
 * spectrum common to all pulsars, M (s o w) = s o (M w) per bin (red_noise.py:267-270).  pta_gwb_czt_scaled: w must be NULL,
 * variant 0 or 1.                                                                                                       */
int pta_gwb_czt_scaled(uint64_t seed, uint64_t r0, const double *w, int64_t ldw, int R, int P, int Nf, int npts, int i0,
                       const double *pre, const double *FB, const double *tw, const double *post, double *G0, int64_t ldg,
                       int variant, int rng_fast, const double *scale, int64_t ld_scale, void *stream);
int pta_gwb_idft_rng_scaled(uint64_t seed, uint64_t r0, int R, int P, int Nf, const double *Tsym, const double *rot, int npts,
                            double *G0, int64_t ldg, int variant, int rng_fast, const double *scale, int64_t ld_scale, void *stream);
/* scale[r * ld_scale + k] = hcf(f[k]; 10^log10_A[r], gamma[r]) / hcf0[k], k < Nf, r < R (ld_scale >= Nf): hcf = A (f / f1yr)^((3 - gamma)/2),
 * f1yr = 1 / 3.16e7, with turnover != 0 divided by (1 + (f / f0)^(power (alpha - beta)))^(1 / power) (red_noise.py:245-251).
 * hcf0 = the configured spectrum's hcf on the grid f (red_noise.gwb_spectrum_hcf).                                      */
int pta_gwb_spectrum_scale(const double *f, const double *hcf0, int Nf, int R, const double *log10_A, const double *gamma, int turnover,
                           double f0, double beta, double power, double *scale, int64_t ld_scale, void *stream);
/* The same factor for a spectrum given per realisation (ABI 8, additive): log10_hc[r * ld_hc + j], j < M, the log10 characteristic
 * strain of realisation r at the M >= 2 (<= 4096) nodes of a userSpec, sorted by frequency.  hc_r(f) is the userSpec branch of
 * red_noise.gwb_spectrum_hcf (red_noise.py:255-263): log10 hc linear in log10 f between the nodes, constant outside them.  The
 * host tabulates per bin k what does not depend on the values: seg[k] = j with xp[j] <= log10 f[k] < xp[j + 1], dx[k] = log10 f[k] -
 * xp[j], dxp[k] = xp[j + 1] - xp[j]; dxp[k] = 0 marks a bin that takes node seg[k] itself (outside the nodes, or on one).
 *   scale[r * ld_scale + k] = 10^(((fp[j + 1] - fp[j]) / dxp[k]) dx[k] + fp[j]) / hcf0[k],   fp = log10_hc + r * ld_hc
 * (numpy.interp's operations in its order).  The caller points pta_engine_hyper.gw_scale at the result.  ld_hc >= M, ld_scale >= Nf. */
int pta_gwb_spectrum_scale_user(const int32_t *seg, const double *dx, const double *dxp, const double *hcf0, int Nf, int M, int R,
                                const double *log10_hc, int64_t ld_hc, double *scale, int64_t ld_scale, void *stream);

/* G[r,a,:] = sum_b Mchol[a,b] G0[r,b,:]  (the M@w of red_noise.py:268, applied after the DFT). */
/* variant 0 (default): LDS-resident Mchol kernel when P <= 80 (a resident grid that streams the realisations through it and reads
 * only the lower triangle of Mchol: what lies above the diagonal is taken as zero), generic batched MFMA GEMM otherwise; 1: always
 * the generic MFMA GEMM; 2: the generic VALU reference GEMM (cross-check); 3: the LDS kernel as it was before it streamed (one
 * workgroup per 64 samples x 4 realisations, the full square of Mchol read; bit-identical to 0 for a lower-triangular Mchol and
 * finite G0) - the A/B partner of variant 0, GEMM as 1 when P > 80                                                              */
int pta_gwb_mix(const double *Mchol, int P, const double *G0, int R, int npts, int64_t ldg, double *G, int variant, void *stream);

/* An ORF factor per realisation (ABI 8, additive): Mchol[r] = chol(2 sum_k clm[r * ld_clm + k] basis[k]), k < n_lm = (lmax + 1)^2 <= 81,
 * the reference's add_gwb(clm=, lmax=) with a clm per realisation (red_noise.py:225-226, 235).  basis [n_lm, P, P] from pta_orf_basis;
 * Mchol [R, P, P] row-major lower factors, upper triangles zero; info [R] int32.  The sum over k is pta_orf_combine's, so a row equal
 * to a configured clm gives that configuration's ORF bit for bit.  A pivot that is not positive or not finite sets info[r] to its
 * 1-based index (LAPACK's convention) and fills ALL of Mchol[r] with NaN; other realisations are unaffected (nothing is shared
 * between realisations: no atomics, no reduction across them).  P <= 80: one launch, four realisations per workgroup (the basis is
 * read once per workgroup), factored in LDS; P > 80: clm . basis by the batched GEMM, pta_potrf_batched_ex with
 * PTA_POTRF_SUBSTITUTION | PTA_POTRF_ZERO_UPPER, and the same NaN fill.  P <= 4096, ld_clm >= n_lm.                              */
int pta_gwb_orf_factor(const double *basis, int n_lm, int P, const double *clm, int64_t ld_clm, int R, double *Mchol, int32_t *info,
                       void *stream);
/* pta_gwb_mix with a factor per realisation: G[r,a,:] = sum_b Mchol[r * ld_m + a * P + b] G0[r,b,:], ld_m >= P * P doubles per
 * realisation (the full square is read: upper triangles must hold zeros).  variant as pta_gwb_mix: 0 = the LDS kernel when P <= 80
 * (the factor staged once per workgroup and reused over at least four 64-sample tiles of its realisation), else the batched MFMA
 * GEMM; 1: always that GEMM; 2: the VALU reference GEMM.  R <= 65535 per call with variant 0 and P <= 80.                        */
int pta_gwb_mix_batched(const double *Mchol, int64_t ld_m, int P, const double *G0, int R, int npts, int64_t ldg, double *G, int variant,
                        void *stream);

/* jlo[i] = last j with ut[j] <= toa_s[i], clamped to [0, npts-2] (numpy.interp's bracket, which
 * scipy.interpolate.interp1d(kind="linear") delegates to; red_noise.py:286-287).           */
int pta_gwb_bracket(const double *ut, int npts, const double *toa_s, int N, int32_t *jlo, void *stream);

/* w[i] = (toa_s[i] - ut[j]) / (ut[j+1] - ut[j]), j = jlo[i]: the realisation-independent half of the linear
 * interpolation red_noise.py:286-287, so the fused kernel evaluates fp[j] + (fp[j+1] - fp[j]) * w per realisation
 * (no division, no grid lookups in the hot loop; differs from interp1d's slope form by rounding only).   */
int pta_gwb_weights(const double *ut, int npts, const double *toa_s, const int32_t *jlo, int N, double *w, void *stream);

/* out[r*ld_out + i] (+)= slope*(toa_s[i] - ut[j]) + G[j],  j = jlo[i], G row = (r, psr_of_toa[i]).
 * scale multiplies the result (1/86400 gives the day-valued delay of red_noise.py:292).     */
int pta_gwb_interp(const double *G, int64_t ldg, int P, int npts, const double *ut, const double *toa_s,
                   const int32_t *psr_of_toa, const int32_t *jlo, int N, int R, double scale, double *out,
                   int64_t ld_out, int accumulate, void *stream);

/* ---------------------------------------------------------------- CGW -------------- */
/* Continuous-wave residual (deterministic.py:97-163). par_host[PTA_CGW_NPAR] holds the scalar
 * prefactors the Python wrapper computes exactly as deterministic.py:51-109 does:
 *  0 tref  1 w0  2 phase0(orbital)  3 w053  4 fac1  5 fac2  6 fac3  7 incfac1  8 incfac2
 *  9 cos2psi  10 sin2psi  11 fplus  12 fcross  13 pd*(1-cosMu)  14 mode (0 evolve, 1 phase_approx,
 *  2 monochromatic)  15 psrTerm (0/1)  16 omega_p (phase_approx, :126)  17 phase0 + fac2*(w053 -
 *  omega_p^(-5/3)) (phase_approx, :130)                                                      */
#define PTA_CGW_NPAR 18
int pta_cgw(const double *mjd, int N, const double *par_host, double *out, int accumulate, void *stream);

/* Catalogue of N_cw continuous-wave sources for one pulsar (add_catalog_of_cws and its numba kernels,
 * deterministic.py:188-561): out[i] (+)= sum_c waveform_c(mjd[i]), NaN terms dropped (:435,:556).
 * par[c*PTA_CW_NPAR + 0..] (device) = the per-source scalars the reference computes at the top of its loop body (:331-383),
 * evaluated on the HOST (pta_replicator_amd.deterministic.cw_source_params) so that they are bit-identical to the reference's:
 *  0 w0  1 phase0(orbital)  2 w0^(-5/3)  3 fac1  4 fac2  5 fac3  6 incfac1  7 incfac2  8 cos2psi  9 sin2psi  10 fplus  11 fcross
 *  12 pd*(1-cosMu) [s]  13 omega_p (phase_approx, :395)  14 phase0 + fac2*(w053 - omega_p^(-5/3)) (phase_approx, :399)  15 unused
 * mode 0 evolve / 1 phase_approx / 2 monochromatic.  partial_ws sized by pta_cw_catalog_workspace (doubles).             */
#define PTA_CW_NPAR 16
int pta_cw_catalog_workspace(int N, int ncw, int64_t *partial_doubles, int *nchunk);
int pta_cw_catalog(const double *mjd, int N, const double *par, int ncw, int psr_term, int mode, double tref,
                   double *partial_ws, double *out, int accumulate, void *stream);

/* ---------------------------------------------------------------- fused engine ----- */
/* One pass that writes R whole-array realisations: out[r, i] = RN + GWB + WN + ECORR + det,
 * every deviate generated on chip (throughput mode).  All arrays are device pointers; any
 * signal whose pointer is NULL is skipped.                                                  */
#define PTA_ENGINE_TILE 256     /* TOAs per workgroup tile; a tile never straddles two pulsars */
#define PTA_ENGINE_EPMAX 132    /* ECORR pairs (= 264 epochs) a tile can stage through LDS per realisation */
typedef struct {
  int32_t n_toa;              /* sum of N_a */
  int32_t n_psr;              /* P */
  int32_t rn_k;               /* 2*components (0 = no red noise) */
  int32_t gw_npts;            /* 0 = no GWB */
  int32_t tnequad;
  int32_t n_tiles;
  const int32_t *tile_psr;    /* [n_tiles] pulsar of the tile */
  const int32_t *tile_start;  /* [n_tiles] index (in the concatenated TOA axis) of the tile's first TOA */
  const int32_t *tile_count;  /* [n_tiles] TOAs in the tile, <= PTA_ENGINE_TILE */
  const int32_t *tile_ep0;    /* [n_tiles] first ECORR pair index (epoch >> 1) the tile touches */
  const int32_t *tile_epn;    /* [n_tiles] number of pairs it touches; 0 = more than PTA_ENGINE_EPMAX (epochs not
                                 contiguous along the TOA axis): deviates are then evaluated per TOA */
  const int32_t *idx_in_psr;  /* [n_toa] index of the TOA inside its pulsar (WN pair index) */
  const double *Ft;           /* [rn_k x ldf] design matrix rows for the concatenated TOAs */
  int64_t ldf;
  const double *rn_coef;      /* [R x n_psr x rn_k] sqrt(prior)*z, from pta_engine_rn_coef */
  const double *gw_G;         /* [R x n_psr x gw_npts] mixed GWB grid series */
  const int32_t *gw_jlo;      /* [n_toa] bracket of the TOA on the coarse grid, from pta_gwb_bracket */
  const double *gw_w;         /* [n_toa] (t - ut[j]) / (ut[j+1] - ut[j]), from pta_gwb_weights */
  const double *wn_a;         /* [n_toa] efac*sigma */
  const double *wn_b;         /* [n_toa] efac*equad (t2equad) or equad (tnequad) */
  const int32_t *epoch_of;    /* [n_toa] epoch index inside the pulsar */
  const double *ecorr_toa;    /* [n_toa] ecorr of the TOA's epoch (0 = none) */
  const double *det;          /* [n_toa] realisation-independent deterministic delay (e.g. CGW) */
  const double *wn_c;         /* opt-in, INSTEAD of wn_a / wn_b (ABI 3): [n_toa] sqrt(wn_a^2 + wn_b^2) - ONE deviate per TOA with the
                                 combined EFAC/EQUAD amplitude (same distribution as white_noise.py:105-109, half the Box-Muller pairs;
                                 not the reference's draw order: TOA idx takes branch (idx >> 4) & 1 of pair idx & ~16 of stream (WN, a)) */
  int32_t rng_fast;           /* Gaussian transform of the on-chip draws (see "RNG" above); 0 = fp64 (default) */
  int32_t synth_variant;      /* fused-kernel variant: 0 (default) = red-noise F @ y on the matrix cores (16 realisations x 256 TOAs
                                 per workgroup), workgroups dealt to the XCDs in contiguous (tile, realisation-group) ranges; 1 = same
                                 kernel in plain linear workgroup order (A/B); 2 = the red-noise loop's per-lane 64-bit index products
                                 instead of scalar row offsets, a lane's four TOAs 16 apart with 8-byte accesses instead of two adjacent
                                 pairs with 16-byte ones, and never the copy compiled for a plan with GWB, white noise and ECORR
                                 all present (A/B); 6 = all-VALU kernel (kept for cross-checks); 16 + 16 noidx + 32 generic (16, 32, 48,
                                 64) = test hook for the four copies of the kernel: noidx = with the index products of 2, generic =
                                 without the complete-plan copy of 0; all of these bit-identical; 100 + k (k <= 64) =
                                 the default kernel with k KB of unused dynamic LDS per workgroup (occupancy probe of round 3:
                                 profiles/r03_bench_final.json, DESIGN.md §4.1 "measured and not kept"); any other value is refused */
} pta_engine_plan;

/* coef[(r*P + a)*K + c] = amp[a*K + c] * z(seed, r0+r, (RN,a), c)   (red_noise.py:126-127)   */
int pta_engine_rn_coef(uint64_t seed, uint64_t r0, int R, int P, int K, const double *amp, double *coef, int rng_fast, void *stream);

int pta_engine_synth(const pta_engine_plan *plan_host, uint64_t seed, uint64_t r0, int R, double *out, int64_t ld_out,
                     void *stream);

/* One call = R whole-array realisations: pta_engine_rn_coef -> pta_gwb_czt (or pta_gwb_idft_rng) -> pta_gwb_mix ->
 * pta_engine_synth on `stream`, with plan->rn_coef / plan->gw_G taken from the workspace below.  The batched
 * counterpart of one pass of the reference's add_gwb + add_red_noise + add_measurement_noise + add_jitter (+ add_cgw)
 * over the array (red_noise.py:106-298, white_noise.py:47-198).                                            */
typedef struct {
  const double *rn_amp;       /* [n_psr x rn_k] sqrt(prior), red_noise.py:126 (NULL when rn_k == 0) */
  const double *Mchol;        /* [n_psr x n_psr] Cholesky factor of the ORF (NULL when gw_npts == 0) */
  int32_t gw_nf;              /* Nf of the GWB frequency grid */
  int32_t gw_i0;              /* crop offset (10, red_noise.py:285) */
  int32_t use_czt;            /* 1: chirp-z tables below; 0: Tsym / rot of the DFT-GEMM form */
  int32_t czt_variant;        /* `variant` of pta_gwb_czt (0 = default) */
  const double *czt_pre, *czt_FB, *czt_tw, *czt_post; /* from pta_gwb_czt_setup */
  const double *Tsym, *rot;   /* from pta_gwb_twiddle_sym */
  double *ws_coef;            /* [R x n_psr x rn_k] */
  double *ws_G0;              /* [R x n_psr x gw_npts] per-pulsar grid series */
  double *ws_G;               /* [R x n_psr x gw_npts] mixed grid series */
  int32_t idft_variant;       /* `variant` Tsym was built with (pta_gwb_twiddle_sym) */
  int32_t mix_variant;        /* `variant` of pta_gwb_mix (0 = default) */
} pta_engine_tables;

int pta_engine_generate(const pta_engine_plan *plan_host, const pta_engine_tables *tables_host, uint64_t seed, uint64_t r0, int R,
                        double *out, int64_t ld_out, void *stream);

/* ---------------------------------------------------------------- per-realisation hyperparameters (ABI 8, additive) */
/* out[r * n_par + j] = lo[j] + (hi[j] - lo[j]) u (one fma), u = uniform u2 of pair j of stream (HYPER, 0), realisation r0 + r:
 * theta of a realisation is a pure function of (seed, realisation).  lo / hi: device [n_par].                            */
int pta_hyper_uniform(uint64_t seed, uint64_t r0, int R, int n_par, const double *lo, const double *hi, double *out, void *stream);
/* The same from stream (HYPER, field), 0 <= field < 2^24: field 0 is pta_hyper_uniform bit for bit; field 1 holds the nodes of a
 * per-realisation GWB spectrum (pair j = node j), so the columns of field 0 do not move when a spectrum is sampled too.       */
int pta_hyper_uniform_field(uint64_t seed, uint64_t r0, int R, int n_par, int field, const double *lo, const double *hi, double *out,
                            void *stream);

/* pta_engine_rn_coef with sqrt(prior) computed per (r, a, c) (red_noise.py:126):
 *   coef[(r*P + a)*K + c] = sqrt(A^2 (f / fyr)^-gamma / (12 pi^2 Tspan_a) yr^3) * z(seed, r0+r, (RN,a), c),
 * f = rn_f[a * K/2 + c/2] [Hz], Tspan_a = rn_tspan[a] [s], A = 10^log10_A[r*P + a], gamma = gamma[r*P + a], yr = 365.25 d.
 * log10_A = NaN takes amp_fixed[a*K + c] (the configured amplitude).  Same deviates as pta_engine_rn_coef.                */
int pta_engine_rn_coef_hyper(uint64_t seed, uint64_t r0, int R, int P, int K, const double *rn_f, const double *rn_tspan,
                             const double *log10_A, const double *gamma, const double *amp_fixed, double *coef, int rng_fast,
                             void *stream);

/* theta of a batch of pta_engine_generate_hyper; row r of every array belongs to realisation r0 + r.  A NULL member means "as
 * configured", and the stage it feeds is then the kernel pta_engine_generate runs.                                        */
typedef struct {
  const double *gw_scale;     /* [R x ld_gw_scale] precomputed per-realisation spectrum scale; NULL = from gw_log10_A / gw_gamma */
  int64_t ld_gw_scale;        /* >= gw_nf */
  const double *gw_log10_A;   /* [R] (NULL with gw_scale NULL: configured spectrum) */
  const double *gw_gamma;     /* [R] */
  const double *gw_f;         /* [gw_nf] frequency grid of the GWB (red_noise.py:230-232) */
  const double *gw_hcf0;      /* [gw_nf] hcf of the configured spectrum on that grid */
  int32_t gw_turnover;        /* turnover arguments of the configured GWB (f0, beta, power stay fixed) */
  double gw_f0, gw_beta, gw_power;
  double *ws_scale;           /* [R x ld_gw_scale] workspace pta_gwb_spectrum_scale writes */
  const double *rn_f;         /* [n_psr x rn_k/2] red-noise frequencies [Hz] */
  const double *rn_tspan;     /* [n_psr] Tspan [s] */
  const double *rn_log10_A;   /* [R x n_psr] (NULL: configured red noise); NaN = configured amplitude of that pulsar */
  const double *rn_gamma;     /* [R x n_psr] */
  const double *gw_mchol;     /* [R x ld_gw_mchol] ORF factor per realisation (pta_gwb_orf_factor); NULL = pta_engine_tables.Mchol for all */
  int64_t ld_gw_mchol;        /* >= n_psr^2 */
} pta_engine_hyper;

/* pta_engine_generate with per-realisation theta: pta_engine_rn_coef_hyper -> pta_gwb_spectrum_scale -> pta_gwb_czt_scaled (or
 * pta_gwb_idft_rng_scaled) -> pta_gwb_mix (pta_gwb_mix_batched with gw_mchol) -> pta_engine_synth (unchanged).  White noise, ECORR and deterministic signals as
 * configured in the plan.                                                                                                 */
int pta_engine_generate_hyper(const pta_engine_plan *plan_host, const pta_engine_tables *tables_host, const pta_engine_hyper *hyper_host,
                              uint64_t seed, uint64_t r0, int R, double *out, int64_t ld_out, void *stream);

/* ---------------------------------------------------------------- one CW source per realisation (ABI 8, additive) */
/* out[r * n_par + j] = lo[j] + (hi[j] - lo[j]) u (one fma), u = uniform u2 of pair j of stream (CW, 0), realisation r0 + r.  Columns
 * j: 0 cos_gwtheta, 1 gwphi, 2 log10_mc [Msun], 3 log10_fgw [Hz], 4 log10 h or log10 dist [Mpc], 5 phase0, 6 psi, 7 cos_inc,
 * 8 + a pdist of pulsar a [kpc].  lo / hi: device [n_par].                                                               */
int pta_cw_uniform(uint64_t seed, uint64_t r0, int R, int n_par, const double *lo, const double *hi, double *out, void *stream);

/* The source of every realisation of a batch (deterministic.py:13-185 with one source per realisation).  Device pointers.     */
#define PTA_CW_ENGINE_NPAR 16
typedef struct {
  int32_t n_psr;              /* P */
  int32_t mode;               /* 0 evolve, 1 phase_approx, 2 monochromatic (add_cgw's evolve / phase_approx flags) */
  int32_t psr_term;           /* 0 / 1 */
  int32_t amp_is_h;           /* 1: column 4 of src is log10 h (strain); 0: log10 dist [Mpc] */
  int32_t has_pdist;          /* 1: columns 8 .. 8 + P - 1 of src hold pdist [kpc] per realisation; 0: pdist[] below */
  double tref;                /* [s] */
  const double *phat;         /* [n_psr x 3] pulsar unit vectors (ptheta = pi/2 - dec, pphi = ra) */
  const double *pdist;        /* [n_psr] pulsar distances [kpc] (has_pdist = 0) */
  const double *toa_s;        /* [n_toa] MJD * 86400 over the concatenated TOAs */
  const double *src;          /* [R x ld_src] source columns of realisation r0 + r (the layout of pta_cw_uniform) */
  int64_t ld_src;             /* >= 8 (+ n_psr with has_pdist) */
  double *par;                /* [R x n_psr x PTA_CW_ENGINE_NPAR] scalar table written by pta_engine_cw_params */
} pta_cw_engine;

/* par[(r * P + a) * PTA_CW_ENGINE_NPAR + k] from src row r and pulsar a: w0, orbital phase0, Phi = 1 / (32 (mc w0)^(5/3)), fac1,
 * fac3 w0^(-1/3), incfac1, incfac2, cos 2psi, sin 2psi, F+, Fx, pd (1 - cos mu) [s], and for phase_approx omega_p, its phase offset
 * and fac3 omega_p^(-1/3).  One thread per (r, a).                                                                       */
int pta_engine_cw_params(const pta_cw_engine *cw_host, int R, void *stream);

/* out[r * ld_out + i] (+)= CW residual of realisation r at TOA i for r < R (accumulate = 1 adds, 0 writes), over the plan's TOA
 * tiles (tile_psr / tile_start / tile_count, n_tiles, n_psr, n_toa; nothing else of the plan is read).  The evolving phase uses
 * phase0 - Phi d (5 + d (10 + d (10 + d (5 + d)))), d = expm1(log1p(-fac1 t) / 8): the reference's expression without its
 * cancellation.  A TOA whose contribution is not finite (after the merger) gets 0 (deterministic.py:435,556).  No atomics.  */
int pta_engine_cw_add(const pta_engine_plan *plan_host, const pta_cw_engine *cw_host, int R, double *out, int64_t ld_out, int accumulate,
                      void *stream);

/* ---------------------------------------------------------------- a catalogue of CW sources per realisation (ABI 8, additive) */
/* out[(r * S + s) * 8 + j] = lo[j] + (hi[j] - lo[j]) u (one fma), u = uniform u2 of pair j of stream (CW, s), realisation r0 + r: S
 * independent sources from the same 8 boxes (the source columns of pta_cw_uniform).  Source 0 is pta_cw_uniform's draw bit for bit;
 * S - 1 must fit the 24-bit stream field.  lo / hi: device [8].                                                              */
int pta_cw_catalog_uniform(uint64_t seed, uint64_t r0, int R, int S, const double *lo, const double *hi, double *out, void *stream);

/* S sources per realisation, of which realisation r uses the first count[r].  Device pointers.
 * Table: par[((r * n_psr + a) * n_src + s) * NPAR + k], the source index fastest among the table's rows.  NPAR by mode:
 *   mode 0: PTA_CW_CATALOG_NPAR_EVOLVE = 16, the row of pta_engine_cw_params;
 *   mode 1, 2: PTA_CW_CATALOG_NPAR_FOLDED = 8, {Cs0, Cc0, W0, Cs1, Cc1, W1, 0, 0}: the term is Cs0 sin(W0 t) + Cc0 cos(W0 t)
 *   [+ Cs1 sin(W1 t) + Cc1 cos(W1 t): phase_approx with the pulsar term only], the antenna patterns, inclination and polarisation
 *   factors, phase0 and the pulsar term's phase offset folded into the constants (csrc/pta_cw_catalog.h).                  */
#define PTA_CW_CATALOG_NPAR_EVOLVE 16
#define PTA_CW_CATALOG_NPAR_FOLDED 8
typedef struct {
  int32_t n_psr;              /* P */
  int32_t n_src;              /* S >= 1, S - 1 <= 0xFFFFFF */
  int32_t mode;               /* 0 evolve, 1 phase_approx, 2 monochromatic */
  int32_t psr_term;           /* 0 / 1 */
  int32_t amp_is_h;           /* 1: column 4 of a source is log10 h (strain); 0: log10 dist [Mpc] */
  int32_t has_pdist;          /* 1: pdist is [R x ld_pdist], per realisation (shared by its sources); 0: [n_psr] */
  double tref;                /* [s] */
  const double *phat;         /* [n_psr x 3] pulsar unit vectors */
  const double *pdist;        /* pulsar distances [kpc] */
  int64_t ld_pdist;           /* >= n_psr (has_pdist = 1) */
  const double *toa_s;        /* [n_toa] MJD * 86400 over the concatenated TOAs */
  const double *src;          /* [R x ld_src]: source s of realisation r at src[r * ld_src + 8 s .. + 7] (the columns of pta_cw_uniform) */
  int64_t ld_src;             /* >= 8 n_src */
  const int32_t *count;       /* [R] sources in use per realisation, 0 .. n_src (clamped to that range), or NULL = n_src each */
  double *par;                /* [R x n_psr x n_src x NPAR] table written by pta_engine_cw_catalog_params */
} pta_cw_catalog_engine;

/* the table rows of every (r, a, s) with s < count[r]; rows past the count are neither read nor written.  One thread per row.  */
int pta_engine_cw_catalog_params(const pta_cw_catalog_engine *cw_host, int R, void *stream);

/* out[r * ld_out + i] (+)= sum over s < count[r], ascending, of the residual of source s of realisation r at TOA i (accumulate = 1
 * adds, 0 writes), over the plan's TOA tiles.  The sum is formed in a register and added once; a source's term that is not finite (a
 * TOA after its merger) contributes exactly 0, per source.  count[r] = 0 adds 0.  No atomics.                               */
int pta_engine_cw_catalog_add(const pta_engine_plan *plan_host, const pta_cw_catalog_engine *cw_host, int R, double *out, int64_t ld_out,
                              int accumulate, void *stream);

/* ---------------------------------------------------------------- one burst with memory per realisation (ABI 8, additive) */
/* out[r * 5 + j] = lo[j] + (hi[j] - lo[j]) u (one fma), u = uniform u2 of pair j of stream (BWM = 9, 0), realisation r0 + r.  Columns j:
 * 0 cos_gwtheta, 1 gwphi, 2 log10_h, 3 psi, 4 t0_mjd.  lo / hi: device [5].                                                   */
#define PTA_BWM_NSRC 5
int pta_bwm_uniform(uint64_t seed, uint64_t r0, int R, const double *lo, const double *hi, double *out, void *stream);

/* The burst of every realisation of a batch (deterministic.py:822-884 with one burst per realisation).  Device pointers.        */
typedef struct {
  int32_t n_psr;              /* P */
  const double *phat;         /* [n_psr x 3] pulsar unit vectors (ptheta = pi/2 - dec, pphi = ra) */
  const double *toa_s;        /* [n_toa] MJD * 86400 over the concatenated TOAs */
  const double *src;          /* [R x ld_src] burst columns of realisation r0 + r (the layout of pta_bwm_uniform) */
  int64_t ld_src;             /* >= PTA_BWM_NSRC */
  double *coef;               /* [R x n_psr] pol * strain, written by pta_engine_bwm_params */
  double *t0_s;               /* [R] burst epoch [s] = t0_mjd * 86400, written by pta_engine_bwm_params */
} pta_bwm_engine;

/* coef[r * P + a] = 10^log10_h (cos 2psi F+_a + sin 2psi Fx_a) and t0_s[r] = 86400 t0_mjd from src row r; sin(gwtheta) = sqrt((1 - c)
 * (1 + c)) of the cos_gwtheta column.  One thread per (r, a).                                                                   */
int pta_engine_bwm_params(const pta_bwm_engine *bwm_host, int R, void *stream);

/* out[r * ld_out + i] (+)= (toa_s[i] < t0_s[r] ? 0 : coef[r, a] * (toa_s[i] - t0_s[r])) for r < R, a the pulsar of TOA i (accumulate =
 * 1 adds, 0 writes), over the plan's TOA tiles (tile_psr / tile_start / tile_count, n_tiles, n_psr, n_toa; nothing else of the plan is
 * read).  Two adjacent TOAs per lane and 16-byte accesses wherever the row's address allows; out and ld_out need 8-byte alignment
 * only.  Nothing outside the tiles' columns is touched.  No atomics.                                                            */
int pta_engine_bwm_add(const pta_engine_plan *plan_host, const pta_bwm_engine *bwm_host, int R, double *out, int64_t ld_out, int accumulate,
                       void *stream);

/* ---------------------------------------------------------------- white-noise parameters per realisation (ABI 8, additive) */
/* EFAC / EQUAD / ECORR of every (realisation, group) of a batch; a group is a (pulsar, backend flag) pair, groups ordered pulsar-major,
 * so the groups of one pulsar are contiguous.  The fused synthesis runs without the terms given here (plan.wn_a / wn_b, plan.ecorr_toa /
 * epoch_of NULL) and pta_engine_wn_add redraws their deviates - same stream, same counter - with the realisation's own amplitudes
 * (white_noise.py:105-109, :182).  Device pointers.                                                                              */
#define PTA_WN_HYPER_GMAX 16  /* groups of one pulsar (of either kind) pta_engine_wn_add can stage */
typedef struct {
  int32_t n_psr;              /* P */
  int32_t n_wn;               /* G_wn: EFAC / EQUAD groups, the columns of ea / eb */
  int32_t n_ec;               /* G_ec: ECORR groups, the columns of ec */
  int32_t tnequad;            /* 1: eb = equad, 0: eb = efac equad */
  int32_t max_per_psr;        /* the caller's bound on the groups of one pulsar, of either kind: <= PTA_WN_HYPER_GMAX */
  const double *sigma;        /* [n_toa] TOA errors [s] */
  const int32_t *wn_group;    /* [n_toa] EFAC / EQUAD group of the TOA, -1 = none (amplitudes 0) */
  const int32_t *ec_group;    /* [n_toa] ECORR group of the TOA's epoch, -1 = none (amplitude 0) */
  const int32_t *wn_psr0;     /* [n_psr + 1] first EFAC / EQUAD group of every pulsar */
  const int32_t *ec_psr0;     /* [n_psr + 1] first ECORR group of every pulsar */
  const double *efac_conf;    /* [n_wn] configured efac */
  const double *equad_conf;   /* [n_wn] configured equad [s] (0 = none) */
  const double *ecorr_conf;   /* [n_ec] configured ecorr [s] */
  const double *efac;         /* [R x ld_efac] labels of realisation r0 + r, NaN = as configured; NULL = all as configured */
  int64_t ld_efac;
  const double *log10_equad;  /* [R x ld_equad] likewise */
  int64_t ld_equad;
  const double *log10_ecorr;  /* [R x ld_ecorr] likewise */
  int64_t ld_ecorr;
  double *ea;                 /* [R x n_wn] efac, written by pta_engine_wn_params; NULL (with eb) = no EFAC / EQUAD term */
  double *eb;                 /* [R x n_wn] efac 10^log10_equad, or 10^log10_equad with tnequad */
  double *ec;                 /* [R x n_ec] 10^log10_ecorr; NULL = no ECORR term */
} pta_engine_wn_hyper;

/* The amplitude tables of R realisations from the labels and the configured values (ea, eb where ea is given, ec where ec is).  One
 * thread per (r, group); every pow of the path is here.                                                                          */
int pta_engine_wn_params(const pta_engine_wn_hyper *wn_host, int R, void *stream);

/* out[r * ld_out + i] = (out[r * ld_out + i] + (ea[r, g(i)] sigma[i] z1 + eb[r, g(i)] z2)) + ec[r, h(i)] z_e for r < R (accumulate = 1;
 * 0 writes the terms alone), over the plan's TOA tiles (tile_*, n_tiles, n_psr, n_toa, idx_in_psr, epoch_of and rng_fast are read,
 * nothing else of the plan).  (z1, z2) = pair idx_in_psr[i] of stream (WN, a), z_e = deviate epoch_of[i] of stream (ECORR, a) of
 * realisation r0 + r: the deviates of pta_engine_synth.  A term whose table is NULL is left out.  Two adjacent TOAs per lane and
 * 16-byte accesses wherever the row's address allows; out and ld_out need 8-byte alignment only.  Nothing outside the tiles' columns
 * is touched.  No atomics.                                                                                                       */
int pta_engine_wn_add(const pta_engine_plan *plan_host, const pta_engine_wn_hyper *wn_host, uint64_t seed, uint64_t r0, int R, double *out,
                      int64_t ld_out, int accumulate, void *stream);

/* ---------------------------------------------------------------- one chromatic Gaussian process per pulsar (ABI 8, additive) */
/* dt_i = (nu_ref / nu_i)^chi sum_c F_ic sqrt(phi_c) z_c per pulsar (DM variations at chi = 2), F and phi those of the red noise
 * (red_noise.py:106-128), z from stream (CHROM = 10, pulsar) of the realisation.  The row weights are part of the design matrix the
 * caller hands over.  Added after the fused synthesis, like the terms above.  Device pointers.                                   */
typedef struct {
  int32_t n_psr;              /* P */
  int32_t k;                  /* K_c = 2 x components, even */
  int32_t rng_fast;           /* the Gaussian transform of the plan's rng_fast */
  const double *Ft;           /* [k x ldf] weighted design matrix over the concatenated TOAs, row c = column c of w . F */
  int64_t ldf;                /* >= n_toa */
  const double *amp;          /* [n_psr x k] configured sqrt(phi), a row of zeros = no process for that pulsar */
  const double *f;            /* [n_psr x k / 2] frequencies [Hz] of the column pairs (read with log10_A) */
  const double *tspan;        /* [n_psr] Tspan [s] (read with log10_A) */
  const double *log10_A;      /* [R x ld_theta] labels of realisation r0 + r, NaN = as configured; NULL = all as configured */
  const double *gamma;        /* [R x ld_theta] likewise (needed beside log10_A) */
  int64_t ld_theta;           /* >= n_psr */
  double *coef;               /* [R x n_psr x k] sqrt(phi) z, written by pta_engine_chrom_coef, read by pta_engine_chrom_add */
} pta_chrom_engine;

/* coef[(r * P + a) * k + c] = amp(r, a, c) * z, z = deviate c of stream (CHROM, a) of realisation r0 + r: pair c >> 1, branch c & 1 (the
 * mapping pta_engine_rn_coef uses for stream RN).  amp = the configured table, or - log10_A given and not NaN at (r, a) -
 * sqrt(A^2 (f / f_yr)^-gamma / (12 pi^2 Tspan) yr^3) at the column's frequency.  One thread per (r, a, pair).                   */
int pta_engine_chrom_coef(const pta_chrom_engine *chrom_host, uint64_t seed, uint64_t r0, int R, void *stream);

/* out[r * ld_out + i] (+)= sum_c Ft[c * ldf + i] coef[(r * P + a) * k + c] for r < R, a the pulsar of TOA i (accumulate = 1 adds, 0
 * writes), over the plan's TOA tiles (tile_psr / tile_start / tile_count, n_tiles, n_psr, n_toa; nothing else of the plan is read).  The
 * product runs on the fp64 matrix cores in a fixed order of c: a realisation's term is bit-identical in every batch, row slot and view.
 * Two adjacent TOAs per lane and 16-byte accesses wherever the row's address allows; out and ld_out need 8-byte alignment only.
 * Nothing outside the tiles' columns is touched.  No atomics.                                                                    */
int pta_engine_chrom_add(const pta_engine_plan *plan_host, const pta_chrom_engine *chrom_host, int R, double *out, int64_t ld_out,
                         int accumulate, void *stream);

/* ---------------------------------------------------------------- common red processes with an ORF each (ABI 8, additive) */
/* Up to PTA_CPROC_MAX Gaussian processes common to the array (clock error = monopole, ephemeris error = dipole, CURN, HD, any
 * positive semi-definite [P, P] ORF), all on the array-wide Fourier basis f_k = k / T, sin column then cos column:
 *   dt_{a,i} += sum_c F_ic y_ac,  y_ac = sum_p sqrt(phi_pc) sum_j B_p[a, j] z_pcj,  B_p B_p^T = Gamma_p,
 * phi the red-noise prior at tspan = T, z from stream (CPROC = 12, p) of the realisation.  Added after the fused synthesis, like the
 * terms above.  Device pointers.                                                                                                 */
#define PTA_CPROC_MAX 4         /* processes per engine */
#define PTA_CPROC_KMAX 64       /* columns: 2 x 32 frequencies */
typedef struct {
  int32_t n_psr;              /* P */
  int32_t n_proc;             /* 1 .. PTA_CPROC_MAX */
  int32_t k;                  /* K = 2 x the most components of any process, even, <= PTA_CPROC_KMAX */
  int32_t rng_fast;           /* the Gaussian transform of the plan's rng_fast */
  int32_t kp[PTA_CPROC_MAX];  /* columns of process p, even, 2 .. k: it leaves columns >= kp untouched */
  int32_t rho[PTA_CPROC_MAX]; /* rank of its ORF factor, 1 .. P */
  const double *B[PTA_CPROC_MAX]; /* [n_psr x rho] row-major factor of its ORF */
  const double *amp;          /* [n_proc x k] configured sqrt(phi) */
  double tspan;               /* T [s]: f_k = k / T, and the Tspan of the prior */
  const double *log10_A;      /* [R x ld_theta] labels of realisation r0 + r, NaN = as configured; NULL = all as configured */
  const double *gamma;        /* [R x ld_theta] likewise (needed beside log10_A) */
  int64_t ld_theta;           /* >= n_proc */
  const double *sc1;          /* [n_toa x 2] (sin, cos)(2 pi frac(t / T)) of every TOA, 16-byte aligned (read by pta_engine_cproc_add) */
  double *coef;               /* [R x n_psr x k] y, written by pta_engine_cproc_coef, read by pta_engine_cproc_add; 16-byte aligned */
} pta_cproc_engine;

/* coef[(r * P + a) * k + c] = sum over the processes p with c < kp[p], ascending, of amp(r, p, c) * sum_j B_p[a * rho + j] z_j (ascending j,
 * one fma per term), z_j = deviate n = c rho + j of stream (CPROC, p) of realisation r0 + r: pair n >> 1, branch n & 1.  amp = the
 * configured table, or - log10_A given and not NaN at (r, p) - sqrt(A^2 (f / f_yr)^-gamma / (12 pi^2 T) yr^3) at f = (c / 2 + 1) / T.
 * One workgroup per (r, c): the deviates are drawn once into LDS, one thread per pulsar mixes them.  No atomics.                  */
int pta_engine_cproc_coef(const pta_cproc_engine *cproc_host, uint64_t seed, uint64_t r0, int R, void *stream);

/* out[r * ld_out + i] (+)= sum_k coef[(r * P + a) * k + 2 k'] sin(2 pi (k' + 1) x_i) + coef[.. + 2 k' + 1] cos(2 pi (k' + 1) x_i) for r < R, a
 * the pulsar of TOA i, x_i = frac(t_i / T) (accumulate = 1 adds, 0 writes), over the plan's TOA tiles (tile_psr / tile_start /
 * tile_count, n_tiles, n_psr, n_toa; nothing else of the plan is read).  No design matrix: harmonic k' + 1 comes from harmonic k' by a
 * rotation through sc1 in registers, in one fixed order: a realisation's term is bit-identical in every batch, row slot and view.
 * Two adjacent TOAs per lane and 16-byte accesses wherever the row's address allows; out and ld_out need 8-byte alignment only.
 * Nothing outside the tiles' columns is touched.  No atomics.                                                                    */
int pta_engine_cproc_add(const pta_engine_plan *plan_host, const pta_cproc_engine *cproc_host, int R, double *out, int64_t ld_out,
                         int accumulate, void *stream);

/* ---------------------------------------------------------------- TD mode ---------- */
/* Dense time-domain path named by BASELINE.json's north_star (no counterpart in the reference,
 * which never forms an N_toa x N_toa object: SURVEY.md §0.2, App. A.1).
 * C[i,j] = sum_c phi[c] Ft[c,i] Ft[c,j] + (i==j) sigma2[i] + (epoch_of[i]==epoch_of[j]) ecorr2[i]
 * i.e. the covariance of the reference's RN (red_noise.py:98-101,126-128) + WN/ECORR
 * (white_noise.py:105-109,182) synthesis.  Only the lower triangle (col <= row) is written - that is
 * all pta_potrf_batched reads.  HBM traffic: 8 bytes per element of the triangle, written once; at K = 60 the
 * rank-K product costs 16.6 flop per byte, so the fp64 matrix rate, not HBM, bounds it.      */
int pta_td_cov_assemble(const double *Ft, int64_t ldf, int N, int K, const double *phi, const double *sigma2,
                        const int32_t *epoch_of, const double *ecorr2, double *C, int64_t ldc, void *stream);

/* The same assembly for all pulsars (blocks) of an array in ONE launch of 128 x 128 tiles: block b covers TOAs
 * [blk_off[b], blk_off[b] + blk_n[b]) of the concatenated axis (Ft columns, sigma2, epoch_of, ecorr2 are indexed by it),
 * phi[b*K + c] are its prior variances, and its covariance goes to Cbase + blk_pos[b] with row pitch blk_ld[b] (the layout
 * pta_td_plan describes; all index arrays are device pointers).  max_n = the largest blk_n.                              */
int pta_td_cov_assemble_all(const double *Ft, int64_t ldf, int K, const double *phi, const double *sigma2,
                            const int32_t *epoch_of, const double *ecorr2, double *Cbase, const int64_t *blk_pos,
                            const int32_t *blk_ld, const int32_t *blk_n, const int32_t *blk_off, int n_blocks, int max_n,
                            void *stream);

/* The same assembly by the COLUMN-WALKING kernel (ABI 7; 1 <= K <= 64, 64 ldf < 2^29): a wave keeps the phi-scaled operand of 64
 * columns in registers and walks down the rows 16 at a time; a store instruction writes four rows x 256 bytes (whole cache lines: a
 * lane's accumulators hold two neighbouring columns, 16 bytes per lane); work items = (block, 256-column group, segment of 512 rows),
 * exactly as many as the blocks' orders need - a ragged array launches no empty workgroups.
 * PRECONDITION (as for pta_td_plan): blk_pos[b] and blk_ld[b] must be EVEN - the 16-byte stores assume it; the entry point checks the
 * alignment of Cbase only (the arrays live on the device), engine_td builds both even (orders padded to even, pitches to 16).  pta_td_cov_walk_items writes item0[b] = first item of block b (b <= n_blocks: item0[n_blocks] = the total,
 * also returned; -1 on a bad argument) from the HOST copy of the orders; the caller keeps a device copy of item0 for the launch.
 * Every k index is clamped to K - 1 before it forms an address: nothing behind the [K, ldf] design matrix is ever read.
 * epoch_first (optional, device, indexed like epoch_of): the smallest TOA index INSIDE ITS BLOCK that shares the TOA's epoch - lets a step
 * whose rows have no epoch partner among the wave's columns skip the ECORR arithmetic (every step off the diagonal for time-ordered
 * TOAs); NULL keeps it everywhere.  variant (the SAME K and variant for both calls): 0 or 1 are accepted and select the SAME kernel
 * (reserved for further work-item geometries). */
int64_t pta_td_cov_walk_items(const int32_t *blk_n_host, int n_blocks, int K, int variant, int32_t *item0_host);
int pta_td_cov_assemble_walk(const double *Ft, int64_t ldf, int K, const double *phi, const double *sigma2,
                             const int32_t *epoch_of, const double *ecorr2, double *Cbase, const int64_t *blk_pos,
                             const int32_t *blk_ld, const int32_t *blk_n, const int32_t *blk_off, int n_blocks,
                             const int32_t *item0, int64_t n_items, const int32_t *epoch_first, int variant, void *stream);

/* ASSEMBLY + FACTORISATION of a uniform batch in one call (ABI 8; csrc/pta_td_fused.hip): the covariances are never written.  In the
 * left-looking panel order a tile of the lower triangle is touched once before its panel is factored - by its block column's update
 * C - L[:, <k0] L[:, <k0]^T - so that update COMPUTES C = F diag(phi) F^T + diag(sigma2) + ECORR (red_noise.py:98-101,126-128,
 * white_noise.py:105-109,182) in front of the factor product (four more K slabs of the same MFMA stream) and stores without reading:
 * no assembly launch, no 2 x 8 bytes per element of round trip (6.8 GB written + read at 68 x 5000^2).
 *   Fr [B n, 64]  row-major rows of the design matrix over the batch's concatenated TOAs (matrix b's rows = [b n, (b + 1) n)), columns
 *                 >= kf ZERO;   Gr [B n, 64] = -phi_k Fr[i, k];   kf = red-noise columns in use (0 .. 64; 0 skips the phase)
 *   sigma2 [B n], epoch_of [B n] / ecorr2 [B n] (both or neither NULL): as pta_td_cov_assemble_all
 *   A, n, lda, strideA, B, info, flags, work, work_doubles: as pta_potrf_batched_ws (A's contents are ignored; PTA_POTRF_LEFT is implied;
 *   the workspace scheme must apply: n > panel width and a workspace of pta_potrf_workspace_doubles(n, B, flags) doubles; n, lda, strideA
 *   even).  The factors equal pta_td_cov_assemble_walk + pta_potrf_batched_ws(PTA_POTRF_LEFT) to rounding (the K = 60 product is summed
 *   in another order), not bit for bit. */
int pta_td_assemble_potrf(const double *Fr, const double *Gr, int kf, const double *sigma2, const int32_t *epoch_of, const double *ecorr2,
                          double *A, int n, int64_t lda, int64_t strideA, int B, int32_t *info, int flags, double *work,
                          int64_t work_doubles, void *stream);

/* out[r*ld_out + i] (+)= sum_{j<=i} L[i*ldl + j] z[r*ld_z + j]   (L z, the draw of the dense path;
 * Z . L^T on the fp64 MFMA GEMM).  z holds N(0,1) deviates: NumPy's in replay mode, or
 * pta_rng_fill_normal(stream (TD, pulsar)) in throughput mode.                              */
int pta_td_trmm(const double *L, int64_t ldl, int N, const double *z, int64_t ld_z, int R, double *out, int64_t ld_out,
                int accumulate, int algo, void *stream);   /* algo: 1 = MFMA GEMM, 0 = VALU reference GEMM */

/* Throughput form of the same draw: Z is never materialised - every lane GENERATES its MFMA A operand in registers
 * (stream kind PTA_STREAM_TD / PTA_STREAM_TDGW, deviate j of row m = pair j >> 1, branch j & 1), so one launch covers all
 * pulsars:   out[m, blk_off[b] + i] = sum_{j <= i} L_b[i, j] z(m, b, j)  (+ GWB interpolation + deterministic delay).
 *   rows_per_real == 1 : row m = realisation r0 + m, factor block b = pulsar b, stream (stream_kind, b)   (per-pulsar N_a x N_a factors)
 *   rows_per_real == P : ONE factor block shared by all rows; row m = (realisation r0 + m / P, pulsar m % P), stream
 *                        (stream_kind, m % P)   (the npts x npts factor of the GWB grid covariance)
 * Factor b is row-major at Lbase + blk_pos[b] with leading dimension blk_ld[b]; blk_pos and blk_ld must be EVEN (16-byte
 * double2 loads) and only elements on or below the diagonal are read (pta_potrf_batched_ex may leave the upper triangle
 * unzeroed).  Work items = strips of up to PTA_TD_STRIP consecutive rows of one factor (item_n0, item_rows), sorted by the caller by
 * decreasing min(n, n0 + rows) (their K extent) so that the long strips start first.
 * Optional epilogue (rows_per_real == 1 only): gw_G[(m * n_blocks + b) * gw_npts + j] is the mixed GWB grid series of
 * (realisation m, pulsar b), interpolated with gw_jlo / gw_w exactly as pta_engine_synth does (red_noise.py:286-287);
 * det is added to every row.  All three are indexed by OUTPUT column.                                              */
#define PTA_TD_STRIP 256
typedef struct {
  const double *Lbase;
  const int64_t *blk_pos;     /* [n_blocks] element offset of factor b inside Lbase (even) */
  const int32_t *blk_ld;      /* [n_blocks] leading dimension (even, >= blk_n) */
  const int32_t *blk_n;       /* [n_blocks] order of factor b */
  const int32_t *blk_off;     /* [n_blocks] first output column of block b */
  const int32_t *item_blk;    /* [n_items] factor block of the strip */
  const int32_t *item_n0;     /* [n_items] first row of the strip (a multiple of 16; of PTA_TD_STRIP when item_rows is NULL) */
  int32_t n_blocks;
  int32_t n_items;
  int32_t rows_per_real;
  uint32_t stream_kind;       /* 5 = PTA_STREAM_TD, 6 = PTA_STREAM_TDGW */
  int32_t rng_fast;           /* 0 = fp64 Box-Muller (default), 1 = fp32 transcendentals; per call, not process-wide */
  int32_t gw_npts;
  const double *gw_G;         /* NULL = no GWB epilogue */
  const int32_t *gw_jlo;
  const double *gw_w;
  const double *det;          /* NULL = none */
  const double *z;            /* ABI 3 (ABI 7: also with rows_per_real > 1, row m = output row m): NULL = every deviate is generated in registers (default); else the deviates
                                 are READ: z[m * ld_z + blk_zoff[b] + j] = deviate j of row m for factor block b - what pta_rng_fill_normal
                                 (interleave = 1) writes for stream (stream_kind, b).  Same numbers either way, bit-identical output.
                                 A row must be READABLE up to blk_zoff[b] + blk_n[b] rounded up to a multiple of 4 (ld_z at least that);
                                 what lies behind a block's blk_n[b] deviates is never used, finite or not (ABI 6: the "16 finite doubles
                                 behind the last block" of ABI 5 is gone - the kernel clamps whole groups and zeroes k >= blk_n[b]) */
  int64_t ld_z;
  const int32_t *blk_zoff;    /* [n_blocks] first column of block b's deviates inside a row of z (even: pta_rng_fill_normal writes pairs) */
  const int32_t *item_rows;   /* ABI 8: [n_items] rows of the strip (1 .. PTA_TD_STRIP), or NULL = PTA_TD_STRIP for every strip (cut at the factor's
                                 last row).  Lets the caller put a factor's PARTIAL strip FIRST (rows [0, f), K extent f <= 256) instead of last
                                 (K extent = the factor's order): a strip always costs 16 column tiles per K slab, so the dead tiles of a
                                 partial strip are multiplied by its K - 7 of 16 tiles x K = 5000 per 5000-TOA pulsar = 3.9 % of the launch
                                 when the partial strip is the last one, nothing to speak of when it is the first (round 6).  Strips of one
                                 factor must tile its rows without overlap. */
} pta_td_plan;

int pta_td_trmm_rng(const pta_td_plan *plan_host, uint64_t seed, uint64_t r0, int M, double *out, int64_t ld_out, void *stream);

/* ---------------------------------------------------------------- host-sink replacement ---- */
/* Linearised timing-model fit of a whole ensemble, in place:  rows[r, off_a + i]  <-  r - M_a (M_a^T W_a M_a)^-1 M_a^T W_a r  for every
 * realisation r < R and pulsar a < P - what refitting the timing model after an injection removes from the residuals (the reference goes
 * through PINT once per pulsar: simulate.py:40-69).  Mt[k*ld + i] = column k of the design matrices over the concatenated TOAs (k < m <= 12),
 * Qt[k*ld + i] = row k of (M^T W M)^-1 M^T W (host, realisation independent), psr_off[P + 1] the pulsars' TOA offsets (device int32).
 * One workgroup = one pulsar x 8 realisations; the m x 8 column reductions run as wavefront shuffles + one LDS exchange.          */
int pta_tm_project(const double *Qt, const double *Mt, int64_t ld, int m, const int32_t *psr_off, int P, double *rows, int64_t ld_rows, int R,
                   void *stream);

/* ---------------------------------------------------------------- optimal statistic (ABI 8, additive) ---- */
/* Per-realisation half of the Hellings-Downs cross-correlation optimal statistic (the realisation-independent half - W_a, Z_a, den_ab
 * and the ORF weights - is host NumPy: pta_replicator_amd/optimal_statistic.py).  The reference has no counterpart: its realisations
 * leave as par/tim files for a CPU analysis code.
 * Projection:  Y[r * ld_y + a * C + c] = sum_i Wt[c * ldw + psr_off[a] + i] * rows[r * ld_rows + psr_off[a] + i]  for r < R, a < P, c < C,
 * i < psr_off[a + 1] - psr_off[a] (ragged pulsars; psr_off [P + 1] device int32); C = 2 n_f in 1..64, ld_y >= P * C.  fp64 MFMA, one
 * workgroup per pulsar x 64 or 128 realisations; every residual is read once.  A realisation's Y is bit-identical whatever R, its
 * row in the batch or the launch geometry (fixed reduction order over TOAs, no split across workgroups).                          */
int pta_os_project(const double *Wt, int64_t ldw, int C, const int32_t *psr_off, int P, const double *rows, int64_t ld_rows, int R, double *Y,
                   int64_t ld_y, void *stream);
/* Pair reduction:  num_p = Y[r, pair_a[p], :] . Y[r, pair_b[p], :]  (p < n_pairs, pairs a < b), A2[r * ld_a2 + o] = sum_p wt[o * n_pairs + p] num_p
 * for o < n_orf <= 8 (wt = Gamma_o / sum Gamma_o^2 den).  pair_out (optional, NULL = none): pair_out[r * ld_pair + p] = num_p / den[p], or
 * num_p when den is NULL.  One workgroup per realisation with its Y row in LDS (P * C <= 8192 doubles); fixed summation order. */
int pta_os_pairs(const double *Y, int64_t ld_y, int P, int C, int R, const int32_t *pair_a, const int32_t *pair_b, int n_pairs, const double *wt,
                 int n_orf, double *A2, int64_t ld_a2, const double *den, double *pair_out, int64_t ld_pair, void *stream);

/* ---- optimal statistic under per-realisation noise parameters (ABI 8, additive) ----
 * The noise model of the statistic follows theta per realisation (red noise and the GWB auto-term; white noise, ECORR and the timing
 * model stay fixed).  Host NumPy (optimal_statistic.py: matched_operator) builds per pulsar V = U^T P0' [K, N_a] and A = U^T P0' U
 * [K, K], U = [F_rn | F], K = K_rn + C <= 128; pta_os_project gives q = V r_a (in blocks of <= 64 rows of V).  Per (realisation,
 * pulsar), with prior variances b [K] over the pulsar's mean white-noise variance s and D = diag(sqrt b):
 *     Mc = I + D A D = L L^T,   H = L^-1 D [q | A[:, F]],   X = S^1/2 (q_F - H_F^T h_q) / s,   Z = S^1/2 (A_FF - H_F^T H_F) S^1/2 / s
 * (F = the last C columns; S [C] the unit spectrum), then num_ab = X_a . X_b, den_ab = tr(Z_a Z_b) per realisation.
 *
 * pta_os_matched_prior: b[(r * P + a) * K + k], K = K_rn + C.  Columns k < K_rn: pta_rn_amp(rn_f[a * K_rn / 2 + k / 2], rn_tspan[a],
 * rn_log10_A[r * P + a], rn_gamma[r * P + a])^2 / s[a], or rn_phi[a * K_rn + k] / s[a] where rn_log10_A is NaN or the pointer NULL.
 * Columns K_rn + c: 10^(2 gw_log10_A[r]) S(f = (c / 2 + 1) / T; gw_gamma[r]) / s[a] with the unit spectrum
 * S = fyr^(gamma - 3) f^-gamma / (12 pi^2 T), or 0 when gw_log10_A is NULL (no GW auto-term).                                       */
int pta_os_matched_prior(int R, int P, int K_rn, int C, const double *rn_f, const double *rn_tspan, const double *rn_phi, const double *rn_log10_A,
                         const double *rn_gamma, double T, const double *gw_log10_A, const double *gw_gamma, const double *s, double *b,
                         void *stream);
/* pta_os_matched_prior_spec: pta_os_matched_prior with the GW columns from a per-realisation spectrum (log10_hc, ld_hc, M as for
 * pta_gwb_spectrum_scale_user): column K_rn + c is hc_r(f)^2 / (12 pi^2 f^3 T) / s[a], f = (c / 2 + 1) / T, the same quantity as above
 * with hc^2 = A^2 (f yr)^(3 - gamma); seg, dx, dxp [C / 2]: the interpolation tables of the C / 2 frequencies.                        */
int pta_os_matched_prior_spec(int R, int P, int K_rn, int C, const double *rn_f, const double *rn_tspan, const double *rn_phi,
                              const double *rn_log10_A, const double *rn_gamma, double T, const int32_t *seg, const double *dx, const double *dxp,
                              int M, const double *log10_hc, int64_t ld_hc, const double *s, double *b, void *stream);
/* pta_os_matched_solve: X[(r * P + a) * C + c] and the packed lower triangle Z[(r * P + a) * C (C + 1) / 2 + c (c + 1) / 2 + c2] (c2 <= c)
 * from A [P, K, K] (symmetric), b [R, P, K] (>= 0, zeros allowed), S [C], s [P] and q: element (r, a, k) at
 * q[r * ld_q + P * k0 + a * cb + (k - k0)], k0 = (k / q_block) * q_block, cb = min(q_block, K - k0) - what pta_os_project writes when it
 * is called once per block of q_block rows of V with Y = q + P * k0 (q_block >= K: plain [R, P, K]).  1 <= C <= 64, C <= K <= 128
 * (PTA_E_ARG beyond).  One workgroup per (r, a), factor and right-hand sides in LDS (up to 131 KiB); Mc has eigenvalues >= 1 for any
 * finite b, so the factorisation cannot fail.  Bit-identical per (r, a) whatever R.                                                    */
int pta_os_matched_solve(const double *A, int P, int K, int C, int R, const double *b, const double *q, int64_t ld_q, int q_block, const double *S,
                         const double *s, double *X, double *Z, void *stream);
/* pta_os_matched_pairs: num_p = X[r, pair_a[p]] . X[r, pair_b[p]], den_p = tr(Z[r, pair_a[p]] Z[r, pair_b[p]]) (packed triangles),
 * A2[r * ld_a2 + o] = sum_p G[o * n_pairs + p] num_p / sum_p G2[o * n_pairs + p] den_p, sigma[r * ld_sigma + o] = (sum_p G2 den_p)^-1/2 for
 * o < n_orf <= 8 (G2 = G * G); optionally (both or neither) rho[r * ld_pair + p] = num_p / den_p and sigma_pair[r * ld_pair + p] =
 * den_p^-1/2.  One workgroup per realisation, one wave per pair; fixed summation order.                                               */
int pta_os_matched_pairs(const double *X, const double *Z, int P, int C, int R, const int32_t *pair_a, const int32_t *pair_b, int n_pairs,
                         const double *G, const double *G2, int n_orf, double *A2, int64_t ld_a2, double *sigma, int64_t ld_sigma, double *rho,
                         double *sigma_pair, int64_t ld_pair, void *stream);

/* ---- per-frequency optimal statistic (ABI 8, additive) ----
 * The cross-correlated power of every Fourier bin instead of one broadband amplitude.  C = 2 n_f even, column 2 k / 2 k + 1 = sin / cos
 * of bin k.  Per pair p = (a < b):  n_p[k] = X_a[2k] X_b[2k] + X_a[2k+1] X_b[2k+1],
 * D_p[k, j] = sum_{i in {2k, 2k+1}} sum_{l in {2j, 2j+1}} Z_a[i, l] Z_b[i, l];  per ORF o < n_orf <= 8:  b_o = sum_p G[o, p] n_p,
 * F_o = sum_p G[o, p]^2 D_p.  mode 0 ("full"): a2_o = F_o^-1 b_o, sigma_o[k] = sqrt((F_o^-1)_kk); mode 1 ("narrowband"):
 * a2_o[k] = b_o[k] / F_o[k, k], sigma_o[k] = F_o[k, k]^-1/2.
 *
 * pta_os_pairs_pf (fixed noise): Y [R, P C] of pta_os_project; op = F^-1 [n_orf, n_f, n_f] (mode 0) or 1 / diag F [n_orf, n_f] (mode 1),
 * prepared by the host; a2[r * ld_a2 + o * n_f + k].  One workgroup per realisation, Y_r in LDS (P * C * 8 <= 64 KiB).
 *
 * pta_os_matched_pairs_pf (per-realisation noise): X [R, P, C] and the packed Z [R, P, C (C + 1) / 2] of pta_os_matched_solve, G and
 * G2 = G * G [n_orf, n_pairs]; a2[r * ld_a2 + o * n_f + k], sigma[r * ld_sigma + o * n_f + k] and, where fisher is not NULL,
 * fisher[r * ld_fisher + (o * n_f + k) * n_f + j] = F_o[k, j].  One workgroup per realisation; F_o is accumulated in registers, joined
 * and solved in LDS (Jacobi-scaled Cholesky, up to 74 KiB).  A non-positive pivot (mode 1: diagonal entry) gives NaN in a2 and
 * sigma of that (realisation, ORF).  Both: 2 <= C <= 64 (PTA_E_ARG beyond, as for odd C, n_orf > 8 and NULL operands); fixed
 * summation order, bit-identical per realisation whatever R.                                                                        */
int pta_os_pairs_pf(const double *Y, int64_t ld_y, int P, int C, int R, const int32_t *pair_a, const int32_t *pair_b, int n_pairs,
                    const double *G, int n_orf, const double *op, int mode, double *a2, int64_t ld_a2, void *stream);
int pta_os_matched_pairs_pf(const double *X, const double *Z, int P, int C, int R, const int32_t *pair_a, const int32_t *pair_b, int n_pairs,
                            const double *G, const double *G2, int n_orf, int mode, double *a2, int64_t ld_a2, double *sigma,
                            int64_t ld_sigma, double *fisher, int64_t ld_fisher, void *stream);

/* ---- marginalised log-likelihood on a grid of noise parameters (ABI 8, additive) ----
 * The noise model is the one of the statistic above (white noise, ECORR and the timing model fixed and the timing model marginalised
 * with a flat prior; red noise on the K_rn red-noise columns, a common uncorrelated process with the GWB spectrum on the last C).
 * Host NumPy (optimal_statistic.py: lnl_operator) builds per pulsar V, A and s as above, the m <= 16 timing-model rows
 * G = chol(M^T N'^-1 M)^-1 M^T N'^-1, dinv = 1 / d (N' = diag(d) + ECORR epochs), the Sherman-Morrison weights g_e of the epochs and
 * the constant c_a = ln det N_a + ln det(M^T N_a^-1 M) + (N_a - m) ln 2 pi.  pta_os_project over the K + m rows of [V; G] (in blocks of
 * q_block rows, Y = q + P * k0) gives q; element (r, a, k) lies at q[r * ld_q + P * k0 + a * cb + (k - k0)], k0 = (k / q_block) * q_block,
 * cb = min(q_block, K + m - k0).  With b [G, P, K] the prior variances of the G grid points (pta_os_matched_prior with the grid in place
 * of the realisations), D = diag(sqrt b) and Mc = I + D A D = L L^T:
 *     ln L[g, a, r] = -1/2 [ (r^T P0' r - || L^-1 D q ||^2) / s[a] + 2 sum_k ln L_kk + c[a] ]
 * K <= 128 (PTA_E_ARG beyond, as for C > K and NULL operands).  Every value is bit-identical whatever R, G and the chunks it is
 * computed in; no atomics.
 *
 * pta_lnl_quad: r0[r * P + a] = sum_i x_i^2 dinv_i - sum_e g_e (sum_{i in e} x_i dinv_i)^2 over the TOAs psr_off[a] .. psr_off[a + 1] of row r,
 * x_i = r_i - sum_{k < m} Ht[k * ldh + psr_off[a] + i] q[r, a, K + k] the residual of the timing-model fit (Ht [m, sum N_a] the rows of
 * H^T, H = M (M^T N'^-1 M)^-1/2, so that H G r = M beta_hat): the N'^-1 norm of x equals r^T N'^-1 r - || G r ||^2 without its cancellation.  Epochs need not be contiguous in TOA order: pulsar a owns epochs psr_ep[a] .. psr_ep[a + 1]
 * (psr_ep [P + 1]; NULL = no ECORR anywhere), epoch e the entries ep_ptr[e] .. ep_ptr[e + 1] of ep_idx (TOA indices within the pulsar)
 * and the weight ep_g[e].  q and Ht may be NULL when m = 0.  One workgroup per (r, a), fixed summation order.                              */
int pta_lnl_quad(const double *rows, int64_t ld_rows, int R, const int32_t *psr_off, int P, const double *dinv, const int32_t *psr_ep,
                 const int32_t *ep_ptr, const int32_t *ep_idx, const double *ep_g, const double *q, int64_t ld_q, int q_block, int K, int m,
                 const double *Ht, int64_t ldh, double *r0, void *stream);
/* pta_lnl_factor: per (g, a) the Cholesky factor of Mc from A [P, K, K] (symmetric) and b [G, P, K] (>= 0; zeros leave identity rows; Mc
 * has eigenvalues >= 1, so the factorisation cannot fail), logdet[g * P + a] = 2 sum_k ln L_kk, and the operator of the blocked
 * substitution, stored transposed: Lt[((g * P + a) * K + k) * K + i] = L[i, k], inside the 16 x 16 diagonal blocks (i / 16 == k / 16) the
 * inverse of that block of L instead, zeros for i < k.  One workgroup per (g, a), packed factor in LDS (66 KiB at K = 128).  C (the
 * GWB columns) is checked against K only.                                                                                           */
int pta_lnl_factor(const double *A, int P, int K, int C, int G, const double *b, double *Lt, double *logdet, void *stream);
/* pta_lnl_apply: lnl_pulsar[g * ld_g + a * ld_a + r] = ln L[g, a, r] for g < G, a < P, r < R from pta_lnl_factor's Lt and logdet, the same
 * b, q (Kt = K + m operator rows in the layout above; rows >= K are not read), r0 [R, P], s [P], c [P].  y = L^-1 D q is a forward
 * substitution in blocks of 16 rows on the fp64 matrix cores (v_mfma_f64_16x16x4_f64): the blocks left of the diagonal multiply the
 * y already found, the inverted diagonal block finishes the block row.  One workgroup per pulsar x 128 realisations x a run of grid
 * points, the operator staged in LDS (up to 145 KiB); the zero upper triangle is never touched.                                      */
int pta_lnl_apply(const double *Lt, const double *logdet, const double *b, int P, int K, int C, int G, const double *q, int64_t ld_q, int q_block,
                  int Kt, int R, const double *r0, const double *s, const double *c, double *lnl_pulsar, int64_t ld_g, int64_t ld_a, void *stream);
/* pta_lnl_reduce: lnl[g * ld_lnl + r] = sum_a lnl_pulsar[g * ld_g + a * ld_a + r], pulsars in ascending order.                          */
int pta_lnl_reduce(const double *lnl_pulsar, int64_t ld_g, int64_t ld_a, int P, int G, int R, double *lnl, int64_t ld_lnl, void *stream);

/* ---- likelihood ratio of a correlated common process on a (log10_A, gamma) grid (ABI 8, additive) ----
 * ln L(r | common process with ORF Gamma and spectrum g) - ln L(r | noise only) under the configured intrinsic noise (white noise,
 * ECORR, red noise, chromatic columns; timing model marginalised): with Gamma = B B^T, B [P, rho], Y = W r the projections of
 * pta_os_project on the C = 2 n_f columns of the array-wide Fourier basis scaled by the unit spectrum at gamma_ref, and
 * T [n, n], n = rho C, T[(i, k), (j, l)] = sum_a B[a, i] B[a, j] Z_a[k, l] (host: optimal_statistic.clnl_plan),
 *     M_g = I + D_g T D_g = L_g L_g^T,  D_g = I_rho (x) diag(d_g),  d_g,k = 10^log10_A[g] (f_k yr)^((gamma_ref - gamma[g]) / 2),  f_k = (k / 2 + 1) / Tspan
 *     lnl_ratio[g, r] = 1/2 || L_g^-1 D_g Y'_r ||^2 - sum_i ln L_g,ii,   Y'_r[i C + k] = sum_a B[a, i] Y[r, a, k].
 * M_g has eigenvalues >= 1 for every finite grid point.  One ORF per call; the factorisation between pta_clnl_assemble and
 * pta_clnl_solve is pta_potrf_batched_ex (lda = n, strideA = n n, B = G).  1 <= C <= 64, n <= 65535, G <= 65535 per call, NULL
 * operands and short leading dimensions: PTA_E_ARG before any device call.  Every value (g, r) is bit-identical whatever R, G, the
 * leading dimensions and the chunks it is computed in; no atomics.
 *
 * pta_clnl_mix: Yp[r * ld_yp + i * C + k] = sum_a Bt[i * P + a] Y[r * ld_y + a * C + k], Bt = B^T [rho, P], pulsars in ascending order,
 * one workgroup per realisation with its Y in LDS (P C <= 8192).                                                                      */
int pta_clnl_mix(const double *Y, int64_t ld_y, int P, int C, int R, const double *Bt, int rho, double *Yp, int64_t ld_yp, void *stream);
/* pta_clnl_assemble: M[g] [n, n] row-major for g < G: the diagonal and the lower triangle of M_g from T [n, n] (row-major, symmetric; the
 * lower triangle is read), zeros above the diagonal; log10_A, gamma [G].                                                              */
int pta_clnl_assemble(const double *T, int rho, int C, double gamma_ref, double Tspan, const double *log10_A, const double *gamma, int G,
                      double *M, void *stream);
/* pta_clnl_rhs: V[(g * n + i) * ld_v + r] = d_g,(i mod C) Yp[r * ld_yp + i] for g < G, i < n, r < R (ld_v >= R).                         */
int pta_clnl_rhs(const double *Yp, int64_t ld_yp, int rho, int C, int R, double gamma_ref, double Tspan, const double *log10_A,
                 const double *gamma, int G, double *V, int64_t ld_v, void *stream);
/* pta_clnl_solve: V[g] <- L_g^-1 V[g] in place and quad[g * ld_quad + r] = sum_i V[g][i, r]^2 (rows ascending), L [G, n, n] the factors
 * (the lower triangle is read).  Blocked forward substitution over blocks of 64 rows: the blocks left of the diagonal by pta_dgemm
 * (fp64 matrix cores, batch = grid points), the diagonal block from LDS with one column per thread.                                   */
int pta_clnl_solve(const double *L, int n, int G, double *V, int64_t ld_v, int R, double *quad, int64_t ld_quad, void *stream);
/* pta_clnl_finish: lnl_ratio[g * ld_g + r] = quad[g * ld_quad + r] / 2 - sum_i ln L[g][i, i], the logarithms summed in a fixed order.    */
int pta_clnl_finish(const double *L, int n, int G, const double *quad, int64_t ld_quad, int R, double *lnl_ratio, int64_t ld_g, void *stream);

/* ---- continuous-wave F-statistics per realisation (ABI 8, additive) ----
 * Fixed-noise Fp (incoherent, per GW frequency) and earth-term Fe (coherent, per GW frequency and sky point).  Host NumPy
 * (pta_replicator_amd/f_statistic.py) builds per pulsar W_a [2 J, N_a] (rows 2 j, 2 j + 1 = [sin, cos](2 pi f_j t)^T P_a^-1), the
 * inverses of G_aj = E_aj^T P_a^-1 E_aj, the antenna patterns phi [P, S, 2] = (F+, Fx) and the inverses of
 * M_js = sum_a (phi_as phi_as^T) (x) G_aj.  Per realisation q_raj = Q[r, a, 2 j : 2 j + 2]:
 *     Fp[r, j] = 1/2 sum_a q^T G_aj^-1 q,    Fe[r, j, s] = 1/2 N^T M_js^-1 N,  N = sum_a phi_as (x) q_raj  (+ sin, + cos, x sin, x cos).
 * Every value is bit-identical whatever R, the chunk or the output mode it is computed in; no atomics.
 *
 * pta_fstat_project: Q[r * ld_q + a * C + c] = sum_i Wt[c * ldw + psr_off[a] + i] * rows[r * ld_rows + psr_off[a] + i] for r < R, a < P,
 * c < C = 2 J (even, 2 .. PTA_FSTAT_CMAX), i < psr_off[a + 1] - psr_off[a]: pta_os_project's contract without its 64-column limit.  A
 * ragged grouped GEMM on v_mfma_f64_16x16x4_f64: all pulsars in one launch, one workgroup per pulsar x 128 (64 in a small launch)
 * realisations x up to 128 columns, K over the pulsar's own TOAs in ascending slabs of 16 (zeros past its end in both operands), no split-K.               */
#define PTA_FSTAT_CMAX 4096
#define PTA_FSTAT_PMAX 128
#define PTA_FSTAT_SKY_TILE 64
int pta_fstat_project(const double *Wt, int64_t ldw, int C, const int32_t *psr_off, int P, const double *rows, int64_t ld_rows, int R, double *Q,
                      int64_t ld_q, void *stream);
/* pta_fstat_fp: fp[r * ld_fp + j] = 1/2 sum_a (g0 x^2 + 2 g1 x y + g2 y^2), (x, y) = Q[r * ld_q + a * 2 J + 2 j + (0, 1)], (g0, g1, g2) =
 * Ginv[(a * J + j) * 3 + (0, 1, 2)] the packed symmetric G_aj^-1; pulsars in ascending order.  Q 16-byte aligned, ld_q even.       */
int pta_fstat_fp(const double *Q, int64_t ld_q, int P, int J, int R, const double *Ginv, double *fp, int64_t ld_fp, void *stream);
/* pta_fstat_fe: phi[(a * S + s) * 2 + (0, 1)] = (F+, Fx); Minv[(j * S + s) * 10 + i] the upper triangle of M_js^-1, row-major.  2 <= P <=
 * PTA_FSTAT_PMAX.  Two output modes, one per call: fe != NULL writes the full map fe[r * ld_fe + j * S + s] (fe_max, fe_arg NULL);
 * fe == NULL writes fe_max[r * ld_max + j] = max_s Fe and fe_arg[r * ld_arg + j] = the lowest sky index attaining it, reduced in the
 * kernel over 16 sky points at a time into the workspaces part_val, part_arg [R * J * pta_fstat_fe_tiles(S)] and folded over those
 * in ascending order - the map is never written.  N is formed on the fp64 matrix cores (K = P in groups of four pulsars, ascending) and
 * goes into the quadratic form in registers.                                                                                        */
int64_t pta_fstat_fe_tiles(int S);
int pta_fstat_fe(const double *Q, int64_t ld_q, int P, int J, int R, const double *phi, int S, const double *Minv, double *fe, int64_t ld_fe,
                 double *fe_max, int64_t ld_max, int32_t *fe_arg, int64_t ld_arg, double *part_val, int32_t *part_arg, void *stream);

/* ---- Earth-term burst-with-memory matched filter per realisation (ABI 8, additive) ----
 * Definitions and the host preparation: pta_replicator_amd/bwm_statistic.py.  The projection is pta_fstat_project with the J ramp
 * templates as operator rows, C = J rounded up to even (a zero row for the pad): Q[r * ld_q + a * C + j] = W_a[j] . r_a.
 * pta_bwm_stat: phi[(a * S + s) * 2 + (0, 1)] = (F+, Fx); Minv[(j * S + s) * 3 + (0, 1, 2)] = the packed symmetric 2 x 2 M_js^-1
 * (00, 01, 11).  2 <= P <= PTA_FSTAT_PMAX, J <= C <= PTA_FSTAT_CMAX.  N_rjs = sum_a phi_as q_raj is formed on the fp64 matrix cores (K =
 * P in groups of four pulsars, ascending, one chain per output) and goes into A = M^-1 N and Fb = 1/2 N^T A in registers.  Two output
 * modes, one per call: fb != NULL writes the full map fb[r * ld_fb + j * S + s] and, with amp != NULL (16-byte aligned, ld_amp even),
 * the amplitude estimates amp[r * ld_amp + (j * S + s) * 2 + (0, 1)] = (h cos 2psi, h sin 2psi) (fb_max, fb_arg NULL); fb == NULL
 * writes fb_max[r * ld_max + j] = max_s Fb and fb_arg[r * ld_arg + j] = the lowest sky index attaining it (amp NULL), reduced over 16
 * sky points at a time into the workspaces part_val, part_arg [R * J * pta_fstat_fe_tiles(S)] and folded over those in ascending
 * order - the map is never written.  No atomics: a value is the same bits in every mode, chunk and row slot.                        */
int pta_bwm_stat(const double *Q, int64_t ld_q, int P, int C, int J, int R, const double *phi, int S, const double *Minv, double *fb,
                 int64_t ld_fb, double *amp, int64_t ld_amp, double *fb_max, int64_t ld_max, int32_t *fb_arg, int64_t ld_arg, double *part_val,
                 int32_t *part_arg, void *stream);

/* ---- a binned binary population per realisation: Poisson counts, loudest-k, residual spectrum (ABI 8, additive) ----
 * The model, the sampler and the validation: pta_replicator_amd/_pop.py, csrc/pta_pop.h.  B cells, of which n_sorted lie inside the F
 * frequency bins; the sorted tables list those bin by bin (cell_ptr), inside a bin by (regime of the rate, rate).                  */
#define PTA_POP_KMAX 128 /* loudest cells kept per (realisation, bin)          */
#define PTA_POP_FMAX 64  /* frequency bins                                      */
#define PTA_POP_CHUNK 1024 /* cells a workgroup of pta_pop_draw_select takes per step (256 threads x 4) */
typedef struct {
  int32_t n_cells;         /* B: original cells = the length of a counts row and of the label tables                  */
  int32_t n_sorted;        /* cells inside the bin edges                                                              */
  int32_t n_bins;          /* F <= PTA_POP_FMAX                                                                       */
  int32_t k;               /* outlier_per_bin, 1 .. PTA_POP_KMAX                                                      */
  double t_obs;            /* [s]                                                                                     */
  const int32_t *cell_ptr; /* [F + 1] bin k owns sorted cells cell_ptr[k] .. cell_ptr[k + 1] - 1                      */
  const double *number;    /* [n_sorted] expected count of the cell                                                   */
  const double *hs2;       /* [n_sorted] squared source strain                                                        */
  const double *fo;        /* [n_sorted] observed frequency [Hz]                                                      */
  const int32_t *orig;     /* [n_sorted] original cell index                                                          */
  const double *log10_mc;  /* [B] log10 observer-frame chirp mass [Msun], by original index                           */
  const double *log10_fo;  /* [B] log10 observed frequency [Hz]                                                       */
  const double *log10_dl;  /* [B] log10 luminosity distance [Mpc]                                                     */
} pta_pop_plan;
/* pta_pop_draw_select: one workgroup per (realisation r0 + r, bin).  N of every cell of the bin is drawn (pta_pop_poisson: stream (11,
 * attempt), pair = original cell index) or, with counts != NULL, read from counts[r * ld_counts + original index]; w = ((N hs2) fo)
 * t_obs; the k cells with the largest w > 0 are kept (ties: the lower original index first) and the rest summed.  Outputs:
 * sel_cell, sel_number, sel_w [R, F, k] (entries below sel_count[r, bin] are written, loudest first), sel_count [R, F], free_spec
 * [R, F] = 1e-100 + the sum of the rest; counts_out != NULL also receives N at [r * ld_counts_out + original index] (cells outside the
 * edges are not touched).  No global atomics and no split over workgroups: a (realisation, bin) result does not depend on R, r0 or
 * the other rows of the launch.  Allocates nothing, synchronises nothing.                                                        */
int pta_pop_draw_select(const pta_pop_plan *plan, uint64_t seed, uint64_t r0, int R, const double *counts, int64_t ld_counts,
                        double *counts_out, int64_t ld_counts_out, int32_t *sel_cell, double *sel_number, double *sel_w, int32_t *sel_count,
                        double *free_spec, void *stream);
/* pta_pop_theta: one workgroup per realisation: the selection concatenated bin-major into rows of S = F k entries, log10_mc, log10_fgw,
 * log10_dist, pop_number [R, S] (NaN past the count) and pop_cell [R, S] (-1 past it) gathered from the label tables, cw_count [R], and
 * gwb_log10_hc[r * ld_hc + bin] = 0.5 log10(free_spec).                                                                          */
int pta_pop_theta(const pta_pop_plan *plan, int R, const int32_t *sel_cell, const double *sel_number, const int32_t *sel_count,
                  const double *free_spec, double *log10_mc, double *log10_fgw, double *log10_dist, double *pop_number, int32_t *pop_cell,
                  int32_t *cw_count, double *gwb_log10_hc, int64_t ld_hc, void *stream);

/* ---------------------------------------------------------------- multi-GPU -------- */
/* The path's one collective (BASELINE.json north_star: "RCCL over xGMI only to all-gather the final residual arrays
 * back to rank 0"): realisations are sharded by contiguous row ranges - rank r owns rows [a_r, b_r) of the [total_rows x n_cols]
 * ensemble, sizes differing by at most one (a_r = r * (total / world) + min(r, total % world)) - and rank `dst` receives every
 * shard directly into its rows of `out` (point-to-point ncclRecv into row slices inside one group: no staging buffers, no
 * concatenation).  `comm` is the caller's ncclComm_t (RCCL); `local` this rank's shard [b_r - a_r, n_cols], `out` (on `dst` only)
 * the [total_rows, n_cols] result.  Asynchronous on `stream`.  world == 1: a device-to-device copy, no communicator needed.  RCCL is
 * bound at run time from the copy already loaded into the process (PyTorch's), so the library has no link-time dependency on it.
 * The reference has no counterpart (single process).
 * Restriction (world > 1): rows must be contiguous on both sides - ld_local == n_cols and, on `dst`, ld_out == n_cols (a send is
 * matched by ONE receive of the same count, so a wider destination would need row-wise sends too); to fill a window of a wider ensemble
 * tensor, gather into a [total_rows, n_cols] tensor and copy.  world == 1 accepts any leading dimensions.  Thread-safe (the RCCL
 * binding is resolved once).                                                                                                    */
int pta_gather_rank0(void *comm, int rank, int world, int dst, const double *local, int64_t total_rows, int64_t n_cols,
                     int64_t ld_local, double *out, int64_t ld_out, void *stream);

/* ---------------------------------------------------------------- fp64 GEMM -------- */
/* C[b] = alpha * A[b] * op(B[b]) + beta * C[b], row-major, batch `batch` with element strides.
 * A element (m,k) = A[m*lda + k*ska] (ska = 2 reads the real or imaginary plane of interleaved
 * complex rows); transB = 0: B is [K x N]; 1: B is [N x K].  lower_only = 1 touches only col <= row
 * (SYRK).  algo 0 = VALU reference kernel, 1 = v_mfma_f64_16x16x4_f64 kernel, 2 (3: with the C-tile prefetch epilogue, A/B) = the MFMA kernel whose 128 x 128-tile form stages
 * its operand slabs by LDS DMA (transB = 1, ska = 1, even K / lda / ldb / strides, 16-byte aligned A and B; else as algo 1). */
int pta_dgemm(int transB, int M, int N, int K, double alpha, const double *A, int64_t lda, int64_t ska,
              const double *B, int64_t ldb, double beta, double *C, int64_t ldc, int lower_only, int batch,
              int64_t strideA, int64_t strideB, int64_t strideC, int algo, void *stream);

/* ---------------------------------------------------------------- microbenchmarks -- */
/* Measure the roofline denominators on the device the library runs on (bench.py):
 * kind 0: fp64 MFMA (v_mfma_f64_16x16x4_f64) TFLOP/s, 1: fp64 FMA TFLOP/s,
 * 2: HBM write GB/s over `bytes`, 3: HBM copy GB/s, 4: Philox+Box-Muller G normals/s, 5: fp64 MFMA in the GEMM kernels'
 * register-tile pattern (4 A x 4 B fragments -> 16 accumulators), 6: that MFMA loop
 * and the FMA loop on alternating waves of the same SIMDs (sum of both rates: do they share the fp64 ALUs?).  kinds 0 / 1 / 4 / 5: `bytes` in 1..32 = 256-thread blocks per CU.       */
int pta_microbench(int kind, int64_t bytes, int iters, int option, double *result_host);   /* option of kind 4: 0 = default fp64 transform, 1 = rng_fast, 2 = the polynomial fp64 transform (A/B); kind 9: issue rate of one VALU instruction in 16 independent chains per lane, option 0 = v_fma_f64, 1 = v_mad_u64_u32, 2 = v_bitop3_b32, `bytes` = workgroups per CU (= waves per SIMD), result in tera lane-instructions / s */

/* Engine-clock probe (ABI 6): one wave on `stream` samples (s_memrealtime [100 MHz ticks], s_memtime [shader cycles]) into
 * samples[2 i], samples[2 i + 1] every `period_us` for `us` microseconds (at most max_samples pairs; unused slots zeroed).  Launch it
 * on a side stream, run the kernels of interest on another, and the slope cycles / (10 ns) between samples is the engine clock in GHz
 * while they ran (bench.py: roofline.engine_clock_GHz; scripts/gpu_r4_clocks.py).  Asynchronous.                                   */
int pta_clock_probe(uint64_t *samples, int max_samples, int us, int period_us, void *stream);

/* self-test of the fp64 MFMA lane layout used by the GEMM kernels: returns 0 when a 16x16x4
 * product with asymmetric operands matches the scalar result on the device.                */
int pta_selftest_mfma_f64(double *max_err_host);

/* ---------------------------------------------------------------- launch plans ----- */
/* What a launcher chooses from the sizes of a launch (additive to ABI 8): each entry runs the very function its launcher calls and
 * writes the choice to `plan`.  No device call, so they work without a GPU; bad sizes are refused with PTA_E_ARG as the launcher
 * refuses them.  The choice only regroups realisations, grid points or tiles: an output value does not depend on it (the tests hold
 * every instance to that, tests/launch_cases.py).
 *   pta_os_project_plan        plan[0..2] = rw (16-realisation tiles per wave, 1 or 2), ct = ceil(C / 16) (1..4), grid.x
 *   pta_lnl_apply_plan         plan[0..2] = kt = ceil(K / 16) (1..8), g_per (grid points per workgroup, 1..16), gz = ceil(G / g_per)
 *   pta_fstat_project_plan     plan[0..1] = bm, bn (realisations x columns of a workgroup's tile: 128 or 64 x 128, 64 or 32)
 *   pta_gwb_mix_batched_plan   plan[0..2] = nta = ceil(P / 16) (1..5), tpw (64-sample tiles per workgroup), grid.x; all three 0 when the
 *                              launch goes to the batched GEMM (variant != 0 or P > 80)
 *   pta_fstat_fe_plan, pta_bwm_stat_plan   plan[0..2] = ks = ceil(P / 4) (1..32), rchunk (realisations per workgroup), ngz = ceil(R / rchunk)
 *   pta_tm_project_plan        plan[0..1] = m (the instance, 1..12), grid.y
 *   pta_dgemm_plan             takes everything pta_dgemm's choice reads: the shape, the strides of A and B, the byte offsets of the A and
 *                              B pointers modulo 16 (offA, offB: 0..15), lower_only, algo and batch.  plan[0..4] =
 *                                kernel: 0 k_dgemm_valu<false>, 1 k_dgemm_valu<true> (the template argument is transB), 2 k_dgemm_mfma<false>,
 *                                        3 k_dgemm_mfma<true>, 4 k_dgemm_mfma128<false, false>, 5 k_dgemm_mfma128<true, false>,
 *                                        6 k_dgemm_mfma128<true, true> (16-byte operand loads), 7 k_dgemm_glds128<false, 0> (operand slabs
 *                                        by LDS DMA), 8 k_dgemm_glds128<false, 1> (the same with the C-tile prefetch epilogue);
 *                                tile:   columns (= rows) of a workgroup's C tile, 128 or 64; 0 for the VALU kernels (a thread per element);
 *                                lower:  0 lower_only off; 1 a 2-D grid whose workgroups (threads, VALU) above the diagonal leave at once;
 *                                        2 a 1-D grid over the tiles on or below the diagonal of a square C; 3 a 1-D grid over those of a
 *                                        trapezoid (M > N: the triangle of the top square, then the rectangle below it);
 *                                grid.x, grid.y.
 *                              Kernels 6..8 need transB, ska = 1, even K, lda, ldb, strideA and strideB, and offA = offB = 0; a transB
 *                              call that misses one of these gets kernel 5.                                                        */
int pta_os_project_plan(int C, int P, int R, int32_t *plan);
int pta_lnl_apply_plan(int P, int K, int G, int R, int32_t *plan);
int pta_fstat_project_plan(int C, int P, int R, int32_t *plan);
int pta_gwb_mix_batched_plan(int P, int R, int npts, int variant, int32_t *plan);
int pta_fstat_fe_plan(int P, int J, int R, int S, int32_t *plan);
int pta_bwm_stat_plan(int P, int J, int R, int S, int32_t *plan);
int pta_tm_project_plan(int m, int P, int R, int32_t *plan);
int pta_dgemm_plan(int transB, int M, int N, int K, int64_t lda, int64_t ska, int64_t ldb, int64_t strideA, int64_t strideB, int offA,
                   int offB, int lower_only, int algo, int batch, int32_t *plan);

/* ---------------------------------------------------------------- chromatic events per realisation (ABI 8, additive) */
/* Deterministic terms in one pulsar that scale with the radio frequency nu_i [MHz] of the TOA: with t = mjd * 86400, t0 = t0_mjd * 86400,
 * A = 10^log10_a [s at nu_ref], s = -1 if sign < 0 else +1, chi = index, tau = 10^log10_tau [s],
 *     dt_i = s A (nu_ref / nu_i)^chi shape(t_i),
 *     kind 0 decay   t >= t0: exp(-(t - t0) / tau),  t < t0: 0
 *     kind 1 cusp    t >= t0: exp(-(t - t0) / tau),  t < t0: exp(-(t0 - t) / tau_pre)   (tau_pre = 10^log10_tau_pre, tau if that is NaN)
 *     kind 2 bump    exp(-1/2 ((t - t0) / tau)^2)
 *     kind 3 annual  sin(2 pi t / 31557600 + phase)                                     (t0, tau unused)
 * A TOA at exactly t0 takes the t >= t0 side (formulas, the exponent fold and its rounding: csrc/pta_chrom_event.h).  Stream kind 15,
 * field = event slot, pair = label column, uniform u2.
 * Labels: src[(r * E + e) * 9 + j], j = PTA_CE_COL_*: 0 psr (an integer 0 .. P-1 held as a double), 1 kind (0 .. 3 held as a double),
 * 2 t0_mjd, 3 log10_tau [s], 4 log10_tau_pre [s] or NaN, 5 log10_a [s], 6 sign, 7 index, 8 phase [rad].
 * Table: tab[(r * E + e) * 10 + j], j = PTA_CE_TAB_*: 0 psr, 1 kind, 2 t0 [s], 3 1 / tau, 4 1 / tau_pre, 5 -1/2 / tau^2, 6 s = -1 or +1,
 * 7 ln A = log10_a ln 10, 8 chi, 9 phase / (2 pi) [turns].                                                                          */
#define PTA_CE_NCOL 9
#define PTA_CE_NTAB 10
#define PTA_CE_EMAX 128
#define PTA_CE_COL_PSR 0
#define PTA_CE_COL_KIND 1
#define PTA_CE_COL_T0_MJD 2
#define PTA_CE_COL_LOG10_TAU 3
#define PTA_CE_COL_LOG10_TAU_PRE 4
#define PTA_CE_COL_LOG10_A 5
#define PTA_CE_COL_SIGN 6
#define PTA_CE_COL_INDEX 7
#define PTA_CE_COL_PHASE 8
#define PTA_CE_TAB_PSR 0
#define PTA_CE_TAB_KIND 1
#define PTA_CE_TAB_T0 2
#define PTA_CE_TAB_INV_TAU 3
#define PTA_CE_TAB_INV_TAU_PRE 4
#define PTA_CE_TAB_NH 5
#define PTA_CE_TAB_SIGN 6
#define PTA_CE_TAB_LNA 7
#define PTA_CE_TAB_CHI 8
#define PTA_CE_TAB_TURNS 9

/* out[R x E x 9] drawn from per-slot boxes lo / hi: device [E x 9]; column j of slot e of realisation r0 + r is the box draw of pair j
 * of stream (15, e) in (lo[e * 9 + j], hi[e * 9 + j]); lo == hi gives exactly lo, which is how a column is fixed (a slot's kind, a fixed
 * pulsar, a fixed sign).  Column 0 is floored and kept in 0 .. P-1, so the box (0, P) draws the pulsar.  1 <= E <= PTA_CE_EMAX.        */
int pta_chrom_event_uniform(uint64_t seed, uint64_t r0, int R, int E, int P, const double *lo, const double *hi, double *out, void *stream);

/* The chromatic events of every realisation of a batch.  Device pointers.                                                           */
typedef struct {
  int32_t n_psr;              /* P */
  int32_t n_ev;               /* E, 1 .. PTA_CE_EMAX */
  const double *toa_s;        /* [n_toa] MJD * 86400 over the concatenated TOAs */
  const double *lnu;          /* [n_toa] ln(nu_ref / nu_i) over the concatenated TOAs */
  const double *src;          /* [R x E x 9] label rows of realisation r0 + r */
  const int32_t *count;       /* [R] events in use, 0 .. E (clamped), or NULL = E; rows past the count are never read */
  double *tab;                /* [R x E x 10] table rows, written by pta_engine_chrom_event_params */
} pta_chrom_event_engine;

/* tab from src: one thread per (r, e); rows at or past count[r] are neither read nor written.                                        */
int pta_engine_chrom_event_params(const pta_chrom_event_engine *ce_host, int R, void *stream);

/* out[r * ld_out + i] (+)= sum over the events e < count[r] whose psr is the pulsar of TOA i, in ascending e in a register, over the
 * plan's TOA tiles (as pta_engine_bwm_add reads the plan): one exp per (event, TOA) for kinds 0 - 2, exp and a sine in turns for kind
 * 3; needs toa_s, lnu and tab.  accumulate = 1: one read-modify-write per element of a pulsar that holds a live event of the
 * realisation; the elements of every other (realisation, pulsar) are neither read nor written and keep their bits.  accumulate = 0:
 * every element of rows 0 .. R-1 is written, +0.0 where there is no event.  No atomics; a realisation's term is the same bits in every
 * batch and row slot.                                                                                                                */
int pta_engine_chrom_event_add(const pta_engine_plan *plan_host, const pta_chrom_event_engine *ce_host, int R, double *out, int64_t ld_out,
                               int accumulate, void *stream);

/* ---------------------------------------------------------------- sine-Gaussian wavelets per realisation (ABI 8, additive) */
/* The reference's add_burst / add_noise_transient (deterministic.py:718-819) with the callables taken from one family,
 *     wavelet(t) = exp(-1/2 ((t - t0) / tau)^2) cos(2 pi f (t - t0) + phi),   t = mjd * 86400, t0 = t0_mjd * 86400
 * (formulas and the folded form: csrc/pta_burst.h).  Stream kinds 13 (burst: field 0 the sky row, field 1 + w wavelet w) and 14
 * (transients: field v), pair = label column, uniform u2.
 * Burst labels: sky[r * 3 + j], j: 0 cos_gwtheta, 1 gwphi, 2 psi; wavelets src[(r * W + w) * 7 + j], j: 0 t0_mjd, 1 log10_tau [s],
 * 2 log10_f [Hz], 3 log10_a_plus [s], 4 phase_plus, 5 log10_a_cross [s], 6 phase_cross.
 * Transient labels: src[(r * V + v) * 6 + j], j: 0 psr (an integer 0 .. P-1 held as a double), 1 t0_mjd, 2 log10_tau, 3 log10_f,
 * 4 log10_a [s], 5 phase.                                                                                                          */
#define PTA_BURST_NSKY 3
#define PTA_BURST_NCOL 7
#define PTA_NT_NCOL 6
#define PTA_BURST_WMAX 128

/* sky[R x 3] and wav[R x W x 7] drawn from the boxes lo / hi: device [10], the three sky columns first, then the seven wavelet
 * columns (every wavelet of a realisation from the same boxes).  1 <= W <= PTA_BURST_WMAX.                                        */
int pta_burst_uniform(uint64_t seed, uint64_t r0, int R, int W, const double *lo, const double *hi, double *sky, double *wav, void *stream);

/* out[R x V x 6] drawn from the boxes lo / hi: device [6]; the caller gives column 0 the box (0, P) and the entry floors it (and keeps
 * it <= P - 1).  1 <= V <= PTA_BURST_WMAX.                                                                                        */
int pta_transient_uniform(uint64_t seed, uint64_t r0, int R, int V, int P, const double *lo, const double *hi, double *out, void *stream);

/* The burst of every realisation of a batch.  Device pointers.                                                                    */
typedef struct {
  int32_t n_psr;              /* P */
  int32_t n_wav;              /* W, 1 .. PTA_BURST_WMAX */
  const double *phat;         /* [n_psr x 3] pulsar unit vectors (ptheta = pi/2 - dec, pphi = ra) */
  const double *toa_s;        /* [n_toa] MJD * 86400 over the concatenated TOAs */
  const double *sky;          /* [R x 3] sky rows of realisation r0 + r */
  const double *src;          /* [R x W x 7] wavelet rows */
  const int32_t *count;       /* [R] wavelets in use, 0 .. W (clamped), or NULL = W; rows past the count are never read */
  double *wav;                /* [R x W x 7] (t0_s, -1/2 / tau^2, f, A+ cos phi+, A+ sin phi+, Ax cos phix, Ax sin phix), written by
                                 pta_engine_burst_params */
  double *kk;                 /* [R x n_psr x 2] (k+, kx), written by pta_engine_burst_params */
  const int32_t *psr_off;     /* remove_quad: [n_psr + 1] first TOA of every pulsar; else NULL */
  const double *quad_q;       /* remove_quad: [n_toa x 3] orthonormal basis of (1, t, t^2) over every pulsar's TOAs; else NULL */
  double *quad_c;             /* remove_quad: [R x n_psr x 3] = Q_a^T term, written by pta_engine_burst_quad */
} pta_burst_engine;

/* wav and kk from sky / src: one thread per wavelet row and per (r, a).                                                           */
int pta_engine_burst_params(const pta_burst_engine *burst_host, int R, void *stream);

/* quad_c[r, a, :] = sum_i quad_q[i, :] term_r(t_i) over the TOAs of pulsar a (0 for a pulsar of <= 3 TOAs): a workgroup per (a, r),
 * every lane summing its TOAs in ascending order, then a binary tree over the lanes.  No atomics.  R <= 65535.                     */
int pta_engine_burst_quad(const pta_burst_engine *burst_host, int R, void *stream);

/* out[r * ld_out + i] (+)= sum_{w < count[r]} g_w (C_raw cos + S_raw sin)(toa_s[i]) over the plan's TOA tiles (as pta_engine_bwm_add
 * reads the plan), wavelets in ascending order in a register, one read-modify-write.  With quad_q != NULL the entry first runs
 * pta_engine_burst_quad and the element is the term minus quad_q[i, :] . quad_c[r, a, :] (0 for a pulsar of <= 3 TOAs).  accumulate = 1
 * leaves the rows of realisations without a wavelet untouched.  No atomics.                                                       */
int pta_engine_burst_add(const pta_engine_plan *plan_host, const pta_burst_engine *burst_host, int R, double *out, int64_t ld_out,
                         int accumulate, void *stream);

/* The noise transients of every realisation of a batch.  Device pointers.                                                         */
typedef struct {
  int32_t n_psr;              /* P */
  int32_t n_wav;              /* V, 1 .. PTA_BURST_WMAX */
  const double *toa_s;        /* [n_toa] MJD * 86400 over the concatenated TOAs */
  const double *src;          /* [R x V x 6] transient rows of realisation r0 + r */
  const int32_t *count;       /* [R] transients in use, 0 .. V (clamped), or NULL = V; rows past the count are never read */
  double *tab;                /* [R x V x 6] (psr, t0_s, -1/2 / tau^2, f, A cos phi, -A sin phi), written by pta_engine_transient_params */
} pta_transient_engine;

int pta_engine_transient_params(const pta_transient_engine *nt_host, int R, void *stream);

/* out[r * ld_out + i] (+)= sum over the transients v < count[r] whose psr is the pulsar of TOA i, in ascending v; otherwise as
 * pta_engine_burst_add.                                                                                                           */
int pta_engine_transient_add(const pta_engine_plan *plan_host, const pta_transient_engine *nt_host, int R, double *out, int64_t ld_out,
                             int accumulate, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PTA_REPLICATOR_AMD_H */
