// A catalogue of continuous-wave sources per realisation (theta's cw_* keys of shape [R, S], set_cw_prior(n_sources=S)): the label
// draw of source s, the per-(realisation, pulsar, source) scalars and the per-TOA term that pta_engine_cw_catalog_add sums.
//
// Table layout: par[((r * P + a) * S + s) * NPAR + k], the source index fastest among the table's rows, so that the walk over the
// sources of one (realisation, pulsar) is one contiguous stream.  NPAR depends on the mode (pta_cw_catalog_npar):
//   mode 0 (evolve)        16: the scalars of pta_cw_params (pta_cw_hyper.h), evaluated by pta_cw_wave<0, .> - the conditioned phase
//   mode 1 (phase_approx)   8: FOLDED, two sinusoids  {Cs0, Cc0, W0, Cs1, Cc1, W1, 0, 0}
//   mode 2 (monochromatic)  8: FOLDED, one sinusoid   {Cs0, Cc0, W0, 0, 0, 0, 0, 0}
//
// Folding.  Without evolution the orbital phase of a term is linear in t, phase = q + w t, and its residual is
//     alpha (F+ (A cos 2psi + B sin 2psi) + Fx (-A sin 2psi + B cos 2psi)),  A = incfac1 sin 2 phase,  B = incfac2 cos 2 phase
//   = alpha (U sin 2 phase + V cos 2 phase),      U = incfac1 (F+ cos 2psi - Fx sin 2psi),  V = incfac2 (F+ sin 2psi + Fx cos 2psi)
//   = Cs sin(2 w t) + Cc cos(2 w t),              Cs = alpha (U cos 2q - V sin 2q),  Cc = alpha (U sin 2q + V cos 2q)
// with constants per (realisation, source, pulsar).  The Earth term has q = phase0 / 2, w = w0, alpha = fac3 w0^(-1/3); the pulsar term
// of the monochromatic mode has the same w and q - w0 pd (1 - cos mu), so that pulsar - Earth is ONE sinusoid; the pulsar term of
// phase_approx has (omega_p, phase_p, amp_p) of pta_cw_params, a second sinusoid.  No per-TOA polarisation algebra is left.
// Error budget: 2 w t is the exact double of the reference's w t (same rounding, <= 3e3 rad ulp = 5e-13 rad); 2 q carries the
// rounding of w0 pd (1 - cos mu) <= 2e5 rad, 3e-11 rad, which the unfolded form has in t - pd (1 - cos mu) as well.
//
// Everything is __host__ __device__: tests/cw_catalog compiles this header with g++ (-ffp-contract=off).
#pragma once
#include "pta_cw_hyper.h"

#define PTA_CWC_CS0 0
#define PTA_CWC_CC0 1
#define PTA_CWC_W0 2   // 2 omega of sinusoid 0 [rad/s]
#define PTA_CWC_CS1 3
#define PTA_CWC_CC1 4
#define PTA_CWC_W1 5
#define PTA_CW_CATALOG_NPAR_EVOLVE 16  // = PTA_CW_ENGINE_NPAR
#define PTA_CW_CATALOG_NPAR_FOLDED 8

// doubles per (realisation, pulsar, source) of the table
PTA_HD int pta_cw_catalog_npar(int mode) { return mode == 0 ? PTA_CW_CATALOG_NPAR_EVOLVE : PTA_CW_CATALOG_NPAR_FOLDED; }

// label column j of source s of realisation `realisation`: stream (CW, s), pair j, u2 - source 0 is pta_cw_draw
PTA_HD double pta_cw_catalog_draw(uint64_t seed, uint64_t realisation, uint32_t s, uint32_t j, double lo, double hi) {
  return pta_box_draw(seed, realisation, pta_stream_id(PTA_STREAM_CW, s), j, lo, hi);
}

// Cs, Cc of one term: amplitude alpha, orbital phase offset q
PTA_HD void pta_cw_catalog_fold(double U, double V, double alpha, double q, double &cs, double &cc) {
  double s0, c0;
  sincos(2.0 * q, &s0, &c0);
  cs = alpha * (U * c0 - V * s0);
  cc = alpha * (U * s0 + V * c0);
}

// the table row of one (source, pulsar): src = the 8 label columns of the source
PTA_HD void pta_cw_catalog_params(const double *src, int amp_is_h, const double *phat, double pdist, int mode, int psr_term, double *par) {
  if (mode == 0) {
    pta_cw_params(src, amp_is_h, phat, pdist, 0, par);
    return;
  }
  double p[PTA_CW_CATALOG_NPAR_EVOLVE];
  pta_cw_params(src, amp_is_h, phat, pdist, mode, p);
  const double fp = p[PTA_CW_P_FPLUS], fc = p[PTA_CW_P_FCROSS], c2p = p[PTA_CW_P_COS2PSI], s2p = p[PTA_CW_P_SIN2PSI];
  const double U = p[PTA_CW_P_INCFAC1] * (fp * c2p - fc * s2p);
  const double V = p[PTA_CW_P_INCFAC2] * (fp * s2p + fc * c2p);
  const double w0 = p[PTA_CW_P_W0];
  double es, ec;
  pta_cw_catalog_fold(U, V, p[PTA_CW_P_AMP], p[PTA_CW_P_PHASE0], es, ec);
  double cs0 = -es, cc0 = -ec, W0 = 2.0 * w0, cs1 = 0.0, cc1 = 0.0, W1 = 0.0;
  if (psr_term) {
    double ps, pc;
    if (mode == 1) {  // sinusoid 0 = the pulsar term at omega_p, sinusoid 1 = - the Earth term
      pta_cw_catalog_fold(U, V, p[PTA_CW_P_AMP_P], p[PTA_CW_P_PHASE_P], ps, pc);
      cs1 = cs0, cc1 = cc0, W1 = W0;
      cs0 = ps, cc0 = pc, W0 = 2.0 * p[PTA_CW_P_OMEGA_P];
    } else {  // same frequency: pulsar - Earth in one sinusoid
      pta_cw_catalog_fold(U, V, p[PTA_CW_P_AMP], p[PTA_CW_P_PHASE0] - w0 * p[PTA_CW_P_PDC], ps, pc);
      cs0 = ps - es, cc0 = pc - ec;
    }
  }
  par[PTA_CWC_CS0] = cs0;
  par[PTA_CWC_CC0] = cc0;
  par[PTA_CWC_W0] = W0;
  par[PTA_CWC_CS1] = cs1;
  par[PTA_CWC_CC1] = cc1;
  par[PTA_CWC_W1] = W1;
  par[6] = 0.0;
  par[7] = 0.0;
}

// residual [s] of one source of the catalogue at t = mjd * 86400 - tref; 0 where it is not finite (after its merger), per source
template <int MODE, int PSR_TERM>
PTA_HD double pta_cw_catalog_term(const double *par, double t) {
  if (MODE == 0) return pta_cw_wave<0, PSR_TERM>(par, t);
  double s, c;
  sincos(par[PTA_CWC_W0] * t, &s, &c);
  double r = par[PTA_CWC_CS0] * s + par[PTA_CWC_CC0] * c;
  if (MODE == 1 && PSR_TERM) {
    sincos(par[PTA_CWC_W1] * t, &s, &c);
    r = r + (par[PTA_CWC_CS1] * s + par[PTA_CWC_CC1] * c);
  }
  return isfinite(r) ? r : 0.0;
}

// the sum over the first n sources of one (realisation, pulsar), ascending, as pta_engine_cw_catalog_add forms it
template <int MODE, int PSR_TERM>
PTA_HD double pta_cw_catalog_sum(const double *par, int n, double t) {
  const int npar = MODE == 0 ? PTA_CW_CATALOG_NPAR_EVOLVE : PTA_CW_CATALOG_NPAR_FOLDED;
  double acc = 0.0;
  for (int s = 0; s < n; ++s) acc += pta_cw_catalog_term<MODE, PSR_TERM>(par + (int64_t)s * npar, t);
  return acc;
}

// runtime-mode form of pta_cw_catalog_sum (host checks)
PTA_HD double pta_cw_catalog_sum_rt(const double *par, int n, double t, int mode, int psr_term) {
  if (mode == 0) return psr_term ? pta_cw_catalog_sum<0, 1>(par, n, t) : pta_cw_catalog_sum<0, 0>(par, n, t);
  if (mode == 1) return psr_term ? pta_cw_catalog_sum<1, 1>(par, n, t) : pta_cw_catalog_sum<1, 0>(par, n, t);
  return psr_term ? pta_cw_catalog_sum<2, 1>(par, n, t) : pta_cw_catalog_sum<2, 0>(par, n, t);
}
