// GWB frequency -> time stage as a chirp-z (Bluestein) transform: one workgroup per (realisation, pulsar) row,
// two in-LDS 4096-point fp64 FFTs, draws generated in registers.  See pta_fft.h for the algebra.
// Replaces, per row, the Hermitian pack + np.fft.ifft + crop of red_noise.py:275-285 (the sqrt(C) scaling of :270 is
// folded into the pre-chirp, the 1/dt and ifft normalisation into the post-chirp, the M @ w mix of :268 follows on
// the 600-sample grid in pta_gwb_mix).
#include "pta_common.h"
#include "pta_fft.h"

// setup: twiddles, pre-chirp (with sqrtC), post-chirp (with 2/(n dt)), and the spectrum of the convolution chirp
__global__ __launch_bounds__(PTA_FFT_THREADS) void k_czt_setup(const double *__restrict__ sqrtC, int Nf, int npts, int i0,
                                                               double inv_dt, double *__restrict__ pre,
                                                               double *__restrict__ FB, double *__restrict__ tw,
                                                               double *__restrict__ post) {
  __shared__ double re[PTA_FFT_PLANE], im[PTA_FFT_PLANE];
  const int tid = threadIdx.x;
  const int Kf = Nf - 2;
  const int64_t n = 2 * (int64_t)Nf - 2;
  for (int m = tid; m < PTA_FFT_N; m += PTA_FFT_THREADS) {
    double s, c;
    sincospi((double)(2 * m) / (double)PTA_FFT_N, &s, &c);
    tw[2 * m] = c;
    tw[2 * m + 1] = -s;  // e^{-2 pi i m / 4096}
    // pre-chirp sqrtC_k e^{+ pi i k^2 / n}, k = m + 1
    double pr = 0.0, pi_ = 0.0;
    if (m < Kf) {
      int64_t k = m + 1, q = (k * k) % (2 * n);
      sincospi((double)q / (double)n, &s, &c);
      pr = sqrtC[k] * c;
      pi_ = sqrtC[k] * s;
    }
    pre[2 * m] = pr;
    pre[2 * m + 1] = pi_;
    // convolution chirp b_u = e^{- pi i u^2 / n} on u = j - k in [i0 - Kf, i0 + npts - 2], wrapped mod 4096 (with i0 > Kf from u = 0:
    // lags the window does not need, which only reach outputs outside it)
    int64_t u = m;
    bool used = (m <= i0 + npts - 2);
    if (!used && m >= PTA_FFT_N - (Kf - i0)) {
      u = (int64_t)m - PTA_FFT_N;
      used = true;
    }
    double br = 0.0, bi = 0.0;
    if (used) {
      int64_t q = (u * u) % (2 * n);
      sincospi((double)q / (double)n, &s, &c);
      br = c;
      bi = -s;
    }
    re[PTA_FFT_PHYS(m)] = br;
    im[PTA_FFT_PHYS(m)] = bi;
  }
  for (int jj = tid; jj < npts; jj += PTA_FFT_THREADS) {  // post-chirp (2/(n dt)) e^{+ pi i j^2 / n}
    int64_t j = i0 + jj, q = (j * j) % (2 * n);
    double s, c;
    sincospi((double)q / (double)n, &s, &c);
    double amp = 2.0 * inv_dt / (double)n;
    post[2 * jj] = amp * c;
    post[2 * jj + 1] = amp * s;
  }
  __threadfence_block();
  __syncthreads();
  // (the passes read the twiddles this same block just wrote)
  pta_fft_pass<false, 9>(re, im, tw, tid);
  __syncthreads();
  pta_fft_pass<false, 6>(re, im, tw, tid);
  __syncthreads();
  pta_fft_pass<false, 3>(re, im, tw, tid);
  __syncthreads();
  pta_fft_pass<false, 0>(re, im, tw, tid);
  __syncthreads();
  for (int m = tid; m < PTA_FFT_N; m += PTA_FFT_THREADS) {  // logical (digit-reversed) order, 1/L of the inverse folded in
    // stored butterfly-transposed: element q of the s = 1 butterfly b (logical index 8 b + q) at [q][b], so that the eight
    // loads of the fused kernel are 1 KB-contiguous per wave instead of 64 lanes x 128-byte stride
    const int slot = (m & 7) * (PTA_FFT_N / 8) + (m >> 3);
    FB[2 * slot] = re[PTA_FFT_PHYS(m)] * (1.0 / PTA_FFT_N);
    FB[2 * slot + 1] = im[PTA_FFT_PHYS(m)] * (1.0 / PTA_FFT_N);
  }
}

// the lags u = j - k in [i0 - Kf, i0 + npts - 2] take Kf + npts - 1 <= 4096 slots, and the window's own outputs i0 - 1 .. i0 + npts - 2
// must lie inside the convolution: beyond 4095 the positive lags would claim the slots of the negative ones (k_czt_setup) and the
// last butterfly would index past the plane (k_gwb_czt).  Sums in 64 bits: any int is refused, none wraps.
static bool czt_fits(int Nf, int npts, int i0) {
  return Nf >= 3 && npts >= 1 && i0 >= 1 && (int64_t)(Nf - 2) + npts - 2 < PTA_FFT_N && (int64_t)i0 + npts - 2 < PTA_FFT_N;
}

extern "C" int pta_gwb_czt_setup(const double *sqrtC, int Nf, int npts, int i0, double inv_dt, double *pre, double *FB, double *tw,
                                 double *post, void *stream) {
  PTA_REQUIRE(sqrtC && pre && FB && tw && post, PTA_E_ARG, "pta_gwb_czt_setup: NULL argument");
  PTA_REQUIRE(czt_fits(Nf, npts, i0), PTA_E_ARG, "pta_gwb_czt_setup: Nf=%d npts=%d i0=%d does not fit one 4096-point convolution", Nf, npts, i0);
  hipLaunchKernelGGL(k_czt_setup, dim3(1), dim3(PTA_FFT_THREADS), 0, pta_stream(stream), sqrtC, Nf, npts, i0, inv_dt, pre, FB, tw, post);
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}

extern "C" int pta_gwb_czt_fits(int Nf, int npts, int i0) { return czt_fits(Nf, npts, i0) ? 1 : 0; }

// the production ladder step of k_gwb_czt (variant 0 of both entry points)
// (15 + 16 + 64: the LDS twiddle table of bit 32 measured no faster than the products it replaces - DESIGN.md 4.5 - and stays an A/B step)
#define PTA_CZT_FUSE_DEFAULT (15 + 16 + 64)
// the window [i0 - 1, i0 - 1 + npts) of the transform's output lies inside [0, 1024): the last (s = 512) butterfly, whose outputs are
// o + 512 q, only ever stores q = 0 and q = 1
static int czt_last2(int npts, int i0) { return i0 - 2 + npts < 1024 ? 1 : 0; }

// One workgroup per (realisation, pulsar) row.  FUSE selects how much stays in registers between LDS exchanges:
//   bit 0: forward s=1 butterfly, chirp-spectrum product and inverse s=1 butterfly in one go (two exchanges fewer);
//   bit 1: the last butterfly writes the npts-sample window straight to memory;
//   bit 2: the first butterfly starts from registers (draws generated per thread for its own 512-strided elements);
//   bit 3: one twiddle load per butterfly, the rest by squaring / products (pta_fft_twiddles<.., 1>);
//   bit 4 (16): the s = 512 twiddle set of the first butterfly stays in registers and serves, conjugated, the last one (needs bits 1, 2);
//   bit 5 (32): the twiddle sets the workgroup shares come from an LDS table filled once per workgroup with the product sequence
//           of pta_fft_twiddles<.., 1> - s = 8: o = l & 7, 8 complete sets; s = 64: o < 64, (w1, w2, w4) per o and four products -
//           read by the forward and the inverse pass alike (needs bit 3: the table holds the squared values);
//   bit 6 (64): where the launch says the window lies inside [0, 1024) (`last2`), the last butterfly computes outputs 0 and 1 only
//           (pta_fft_core_inv_out01; needs bit 1).
// Bits 4 to 6 remove work, not roundings: every variant 15 + bits is bit-identical to 15.  The production kernel is 15 + 16 + 64.
// FUSE = 15 is the production kernel: 6 LDS exchanges instead of 10, and - what mattered most on MI355X - 6 instead of 56
// global twiddle loads per thread (the q-strided twiddle gathers, not LDS or the barriers, bounded the first version:
// 3.2 -> 2.0 ms per 65 280 rows; rocprofv3 SQ_INSTS_VALU now accounts for ~95 % of the time).  FUSE = 0 (every stage through
// LDS, table twiddles) is kept as the cross-check.
// SCALED (per-realisation spectrum, pta_gwb_czt_scaled): the drawn pair of bin k of row `row` is multiplied by
// scale[(row / P) * ld_scale + k] = hcf(f_k; theta_r) / hcf0(f_k) before the pre-chirp product, which carries sqrt(C0).  The ORF mix
// that follows is linear and the spectrum is common to all pulsars, so M (s o w) = s o (M w) per bin (red_noise.py:267-270).
// SCALED = false compiles to the kernel without the scale operands.
template <bool RNG, bool FAST, int FUSE, bool SCALED>
__global__ __launch_bounds__(PTA_FFT_THREADS, 4) void k_gwb_czt(uint64_t seed, uint64_t r0, const double *__restrict__ w, int64_t ldw,
                                                                  int M, int P, int Nf, int npts, int i0,
                                                                  const double *__restrict__ pre, const double *__restrict__ FB,
                                                                  const double *__restrict__ tw, const double *__restrict__ post,
                                                                  double *__restrict__ G0, int64_t ldg,
                                                                  const double *__restrict__ scale, int64_t ld_scale, int last2) {
  static_assert(!(FUSE & 16) || (FUSE & 6) == 6, "bit 4 carries the twiddles from the register-fed first butterfly to the storing last one");
  static_assert(!(FUSE & 32) || (FUSE & 8), "bit 5 tabulates the squared twiddles of bit 3");
  static_assert(!(FUSE & 64) || (FUSE & 2), "bit 6 prunes the storing last butterfly");
  __shared__ double re[PTA_FFT_PLANE], im[PTA_FFT_PLANE];
  constexpr bool TAB = (FUSE & 32) != 0;
  // (the two tables are only referenced - and only allocated - when TAB)
  __shared__ pta_cplx tw8[7][8];    // [q - 1][o]: w[q] of the s = 8 butterflies, o = l & 7
  __shared__ pta_cplx tw64[3][64];  // [0, 1, 2][o]: w[1], w[2], w[4] of the s = 64 butterflies
  const int tid = threadIdx.x;
  const int row = blockIdx.x;
  const int Kf = Nf - 2;
  if (TAB) {  // waves 0 and 1; read after the barriers that precede the s = 64 pass
    if (tid < 64) {
      pta_cplx tq[8];
      pta_fft_twiddles<6, 1>(tw, tid, tq);  // only w[1], w[2], w[4] are kept (the products are dead code here)
      tw64[0][tid] = tq[1];
      tw64[1][tid] = tq[2];
      tw64[2][tid] = tq[4];
    } else if (tid < 72) {
      pta_cplx tq[8];
      pta_fft_twiddles<3, 1>(tw, tid - 64, tq);
#pragma unroll
      for (int q = 1; q < 8; ++q) tw8[q - 1][tid - 64] = tq[q];
    }
  }
  if (RNG) {
    pta_rng_stage_tables();  // Box-Muller tables -> LDS (pta_rng.h)
    __syncthreads();
  }
  const uint64_t real = r0 + (uint64_t)(row / P);
  const uint32_t strm = pta_stream_id(PTA_STREAM_GWB, (uint32_t)(row % P));
  const pta_cplx *pre2 = reinterpret_cast<const pta_cplx *>(pre);
  constexpr int TW = (FUSE & 8) ? 1 : 3;
  // the inverse passes use the same twiddles as the forward ones; through an opaque copy of the pointer the compiler reloads
  // them (L1/L2 hits) instead of carrying 28 registers per pass across the whole kernel in scratch
  const double *twi = tw;
  asm volatile("" : "+s"(twi));
  pta_cplx tv[8];  // the s = 512 set: FUSE & 16 keeps it from the first butterfly to the last
  if (FUSE & 4) {
    int b, o;
    pta_cplx v[8];
    pta_fft_map<9>(tid, b, o);
    pta_fft_twiddles<9, TW>(tw, o, tv);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int t = o + 512 * q;
      v[q] = {0.0, 0.0};
      if (t < Kf) {  // uniform per q except in the one 512-block that straddles Kf
        double wr, wi;
        if (RNG) {
          pta_normal_pair(seed, real, strm, (uint32_t)(t + 1), wr, wi, FAST ? 1 : 0);
        } else {
          wr = w[(int64_t)row * ldw + 2 * (t + 1)];
          wi = w[(int64_t)row * ldw + 2 * (t + 1) + 1];
        }
        if (SCALED) {
          const double sc = scale[(int64_t)(row / P) * ld_scale + t + 1];
          wr *= sc;
          wi *= sc;
        }
        const pta_cplx pc = pre2[t];
        v[q] = {wr * pc.re - wi * pc.im, wr * pc.im + wi * pc.re};
      }
    }
    pta_fft_core<false, 9>(v, tv);
    pta_fft_store<9>(re, im, b, o, v);
  } else {
#pragma unroll 1
    for (int i = 0; i < PTA_FFT_N / PTA_FFT_THREADS; ++i) {
      const int t = tid + PTA_FFT_THREADS * i;
      double ar = 0.0, ai = 0.0;
      if (t < Kf) {
        double wr, wi;
        if (RNG) {
          pta_normal_pair(seed, real, strm, (uint32_t)(t + 1), wr, wi, FAST ? 1 : 0);
        } else {
          wr = w[(int64_t)row * ldw + 2 * (t + 1)];
          wi = w[(int64_t)row * ldw + 2 * (t + 1) + 1];
        }
        if (SCALED) {
          const double sc = scale[(int64_t)(row / P) * ld_scale + t + 1];
          wr *= sc;
          wi *= sc;
        }
        const pta_cplx pc = pre2[t];
        ar = wr * pc.re - wi * pc.im;
        ai = wr * pc.im + wi * pc.re;
      }
      re[PTA_FFT_PHYS(t)] = ar;
      im[PTA_FFT_PHYS(t)] = ai;
    }
    __syncthreads();
    pta_fft_pass<false, 9, TW>(re, im, tw, tid);
  }
  __syncthreads();
  // the shared sets of one pass, from the table (same bits as pta_fft_twiddles<.., 1> for this thread's o)
  auto tab64 = [&](pta_cplx *wq) {
    const int o = 8 * (tid >> 6) + (tid & 7);
    wq[1] = tw64[0][o];
    wq[2] = tw64[1][o];
    wq[4] = tw64[2][o];
    pta_fft_twiddle_products(wq);
  };
  auto tab8 = [&](pta_cplx *wq) {
#pragma unroll
    for (int q = 1; q < 8; ++q) wq[q] = tw8[q - 1][tid & 7];
  };
  if (TAB) {
    pta_cplx wq[8];
    tab64(wq);
    pta_fft_pass_w<false, 6>(re, im, tid, wq);
    __syncthreads();
    tab8(wq);
    pta_fft_pass_w<false, 3>(re, im, tid, wq);
  } else {
    pta_fft_pass<false, 6, TW>(re, im, tw, tid);
    __syncthreads();
    pta_fft_pass<false, 3, TW>(re, im, tw, tid);
  }
  __syncthreads();
  if (FUSE & 1) {
    int b, o;
    pta_cplx v[8], fv[8];
    pta_fft_map<0>(tid, b, o);
    const pta_cplx *fb = reinterpret_cast<const pta_cplx *>(FB) + b;
#pragma unroll
    for (int q = 0; q < 8; ++q) fv[q] = fb[q * (PTA_FFT_N / 8)];
    pta_fft_load<0>(re, im, b, o, v);
    pta_dft8<false>(v);
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = pta_cmul(v[q], fv[q]);
    pta_dft8<true>(v);
    pta_fft_store<0>(re, im, b, o, v);
  } else {
    pta_fft_pass<false, 0, TW>(re, im, tw, tid);
    __syncthreads();
#pragma unroll 4
    for (int i = 0; i < PTA_FFT_N / PTA_FFT_THREADS; ++i) {
      const int t = tid + PTA_FFT_THREADS * i;
      const int p = PTA_FFT_PHYS(t);
      const int slot = (t & 7) * (PTA_FFT_N / 8) + (t >> 3);
      const double xr = re[p], xi = im[p], fr = FB[2 * slot], fi = FB[2 * slot + 1];
      re[p] = xr * fr - xi * fi;
      im[p] = xr * fi + xi * fr;
    }
    __syncthreads();
    pta_fft_pass<true, 0, TW>(re, im, twi, tid);
  }
  __syncthreads();
  if (TAB) {
    pta_cplx wq[8];
    tab8(wq);
    pta_fft_pass_w<true, 3>(re, im, tid, wq);
    __syncthreads();
    tab64(wq);
    pta_fft_pass_w<true, 6>(re, im, tid, wq);
  } else {
    pta_fft_pass<true, 3, TW>(re, im, twi, tid);
    __syncthreads();
    pta_fft_pass<true, 6, TW>(re, im, twi, tid);
  }
  __syncthreads();
  const pta_cplx *post2 = reinterpret_cast<const pta_cplx *>(post);
  if (FUSE & 2) {
    int b, o;
    pta_cplx v[8];
    pta_fft_map<9>(tid, b, o);
    if (!(FUSE & 16)) pta_fft_twiddles<9, TW>(twi, o, tv);
    pta_fft_load<9>(re, im, b, o, v);
    auto put = [&](int q) {
      const int jj = o + 512 * q - (i0 - 1);
      if (jj >= 0 && jj < npts) {
        const pta_cplx pp = post2[jj];
        G0[(int64_t)row * ldg + jj] = v[q].re * pp.re - v[q].im * pp.im;
      }
    };
    if ((FUSE & 64) && last2) {  // workgroup-uniform: the window ends below 1024, outputs 2..7 would be dropped
      pta_fft_core_inv_out01<9>(v, tv);
      put(0);
      put(1);
    } else {
      pta_fft_core<true, 9>(v, tv);
#pragma unroll
      for (int q = 0; q < 8; ++q) put(q);
    }
  } else {
    pta_fft_pass<true, 9, TW>(re, im, twi, tid);
    __syncthreads();
    for (int jj = tid; jj < npts; jj += PTA_FFT_THREADS) {
      const int p = PTA_FFT_PHYS(i0 - 1 + jj);
      G0[(int64_t)row * ldg + jj] = re[p] * post2[jj].re - im[p] * post2[jj].im;
    }
  }
}

// w == NULL: draws generated on chip (throughput mode); else w[M x ldw] interleaved (re, im) rows (replay mode)
extern "C" int pta_gwb_czt(uint64_t seed, uint64_t r0, const double *w, int64_t ldw, int R, int P, int Nf, int npts, int i0,
                           const double *pre, const double *FB, const double *tw, const double *post, double *G0, int64_t ldg,
                           int variant, int rng_fast, void *stream) {
  PTA_REQUIRE(pre && FB && tw && post && G0, PTA_E_ARG, "pta_gwb_czt: NULL argument");
  PTA_REQUIRE(R > 0 && P > 0 && P < (1 << 24) && npts > 0 && ldg >= npts, PTA_E_ARG, "pta_gwb_czt: R=%d P=%d npts=%d", R, P, npts);
  PTA_REQUIRE(czt_fits(Nf, npts, i0), PTA_E_ARG, "pta_gwb_czt: Nf=%d npts=%d i0=%d does not fit one 4096-point convolution", Nf, npts, i0);
  PTA_REQUIRE(!w || ldw == 0 || ldw >= 2 * (int64_t)Nf, PTA_E_ARG, "pta_gwb_czt: ldw too small");  // 0 = one row of draws for all rows
  int64_t M64 = (int64_t)R * P;
  PTA_REQUIRE(M64 < (1LL << 31), PTA_E_ARG, "pta_gwb_czt: R*P too large");
  const int M = (int)M64;
  // variant: 0 = fully fused kernel (default, PTA_CZT_FUSE_DEFAULT), 1 = plain cross-check (FUSE = 0), 10 + FUSE = any ladder step
  // (25 = the fused kernel without the twiddle / pruning bits 16, 32, 64; 137 = with all three)
  const int fastm = rng_fast ? 1 : 0;
  const int fuse = variant == 0 ? PTA_CZT_FUSE_DEFAULT : (variant == 1 ? 0 : variant - 10);
  const int last2 = czt_last2(npts, i0);
#define PTA_CZT_X(RNGV, FASTV, FUSEV)                                                                                                  \
  hipLaunchKernelGGL((k_gwb_czt<RNGV, FASTV, FUSEV, false>), dim3(M), dim3(PTA_FFT_THREADS), 0, pta_stream(stream), seed, r0, w, ldw, \
                     M, P, Nf, npts, i0, pre, FB, tw, post, G0, ldg, nullptr, 0, last2)
#define PTA_CZT_XF(FUSEV)              \
  if (w)                               \
    PTA_CZT_X(false, false, FUSEV);    \
  else if (fastm)                      \
    PTA_CZT_X(true, true, FUSEV);      \
  else                                 \
    PTA_CZT_X(true, false, FUSEV)
  switch (fuse) {
    case PTA_CZT_FUSE_DEFAULT: PTA_CZT_XF(PTA_CZT_FUSE_DEFAULT); break;
    case 15 + 16 + 32 + 64: PTA_CZT_XF(15 + 16 + 32 + 64); break;
    case 15: PTA_CZT_XF(15); break;
    case 15 + 16: PTA_CZT_XF(15 + 16); break;
    case 15 + 32: PTA_CZT_XF(15 + 32); break;
    case 15 + 64: PTA_CZT_XF(15 + 64); break;
    case 0: PTA_CZT_XF(0); break;
    case 1: PTA_CZT_XF(1); break;
    case 3: PTA_CZT_XF(3); break;
    case 7: PTA_CZT_XF(7); break;
    case 8: PTA_CZT_XF(8); break;
    default: pta_set_error("pta_gwb_czt: unknown variant %d", variant); return PTA_E_ARG;
  }
#undef PTA_CZT_XF
#undef PTA_CZT_X
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}

// The same transform with a per-realisation spectrum: on-chip draws only, variants 0 (default) and 1 (cross-check).
extern "C" int pta_gwb_czt_scaled(uint64_t seed, uint64_t r0, const double *w, int64_t ldw, int R, int P, int Nf, int npts, int i0,
                                  const double *pre, const double *FB, const double *tw, const double *post, double *G0, int64_t ldg,
                                  int variant, int rng_fast, const double *scale, int64_t ld_scale, void *stream) {
  PTA_REQUIRE(pre && FB && tw && post && G0 && scale, PTA_E_ARG, "pta_gwb_czt_scaled: NULL argument");
  PTA_REQUIRE(!w, PTA_E_ARG, "pta_gwb_czt_scaled: draws are generated on chip (w must be NULL)");
  (void)ldw;
  PTA_REQUIRE(R > 0 && P > 0 && P < (1 << 24) && npts > 0 && ldg >= npts, PTA_E_ARG, "pta_gwb_czt_scaled: R=%d P=%d npts=%d", R, P,
              npts);
  PTA_REQUIRE(czt_fits(Nf, npts, i0), PTA_E_ARG, "pta_gwb_czt_scaled: Nf=%d npts=%d i0=%d does not fit one 4096-point convolution", Nf,
              npts, i0);
  PTA_REQUIRE(ld_scale >= Nf - 1, PTA_E_ARG, "pta_gwb_czt_scaled: ld_scale=%lld < Nf - 1", (long long)ld_scale);
  int64_t M64 = (int64_t)R * P;
  PTA_REQUIRE(M64 < (1LL << 31), PTA_E_ARG, "pta_gwb_czt_scaled: R*P too large");
  const int M = (int)M64;
  PTA_REQUIRE(variant == 0 || variant == 1, PTA_E_ARG, "pta_gwb_czt_scaled: variant %d (0 or 1)", variant);
#define PTA_CZT_S(FASTV, FUSEV)                                                                                                     \
  hipLaunchKernelGGL((k_gwb_czt<true, FASTV, FUSEV, true>), dim3(M), dim3(PTA_FFT_THREADS), 0, pta_stream(stream), seed, r0, nullptr, \
                     0, M, P, Nf, npts, i0, pre, FB, tw, post, G0, ldg, scale, ld_scale, czt_last2(npts, i0))
  if (variant == 0) {
    if (rng_fast)
      PTA_CZT_S(true, PTA_CZT_FUSE_DEFAULT);
    else
      PTA_CZT_S(false, PTA_CZT_FUSE_DEFAULT);
  } else {
    if (rng_fast)
      PTA_CZT_S(true, 0);
    else
      PTA_CZT_S(false, 0);
  }
#undef PTA_CZT_S
  PTA_LAUNCH_CHECK();
  return PTA_OK;
}
