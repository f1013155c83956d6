// One burst with memory per realisation in throughput / TD mode (ReplicaEngine.set_bwm): the uniform prior map of the burst labels,
// the per-(realisation, pulsar) antenna coefficient of add_gw_memory (deterministic.py:834-864) and the per-TOA ramp (:867-872).
//
//     dt(t) = 0 for t < t0, else (pol * strain) * (t - t0),   pol = cos 2psi F+ + sin 2psi Fx,   t = mjd * 86400,  t0 = t0_mjd * 86400
//
// with m, n, Omega of the source direction as the reference writes them.  The source's polar angle enters as its cosine (the label
// that is uniform on the sphere); sin = sqrt((1 - c)(1 + c)), so there is no acos / cos round trip.
//
// Everything is __host__ __device__: tests/bwm compiles this header with g++ (-ffp-contract=off) and checks it against the golden
// output of the reference and against a long-double evaluation of its expression.
#pragma once
#include <stdint.h>
#include <math.h>
#include "pta_rng.h"

// columns of the per-realisation burst table (the labels, and the pairs of stream (BWM, 0) that draw them)
#define PTA_BWM_COL_COS_GWTHETA 0
#define PTA_BWM_COL_GWPHI 1
#define PTA_BWM_COL_LOG10_H 2
#define PTA_BWM_COL_PSI 3
#define PTA_BWM_COL_T0_MJD 4
#define PTA_BWM_NSRC 5

// label column j of realisation `realisation` drawn uniformly from [lo, hi): stream (BWM, 0), pair j, u2 (the map of pta_cw_draw)
PTA_HD double pta_bwm_draw(uint64_t seed, uint64_t realisation, uint32_t j, double lo, double hi) {
  return pta_box_draw(seed, realisation, pta_stream_id(PTA_STREAM_BWM, 0u), j, lo, hi);
}

// (F+, Fx) of a pulsar (unit vector phat) for a source at (cos_gwtheta, gwphi): m = (sin phi, -cos phi, 0), n = (-cos theta cos phi,
// -cos theta sin phi, sin theta), Omega = (-sin theta cos phi, -sin theta sin phi, -cos theta) (deterministic.py:838-861)
PTA_HD void pta_bwm_antenna(double cos_gwtheta, double gwphi, const double *phat, double &fplus, double &fcross) {
  const double c = cos_gwtheta;
  const double s = sqrt((1.0 - c) * (1.0 + c));  // sin(gwtheta), accurate at c -> +-1
  double sgp, cgp;
  sincos(gwphi, &sgp, &cgp);
  const double mp = sgp * phat[0] - cgp * phat[1];
  const double np_ = (-c * cgp * phat[0] - c * sgp * phat[1]) + s * phat[2];
  const double op = (-s * cgp * phat[0] - s * sgp * phat[1]) - c * phat[2];
  fplus = 0.5 * (mp * mp - np_ * np_) / (1.0 + op);
  fcross = (mp * np_) / (1.0 + op);
}

// pol * strain of one burst (src: the PTA_BWM_NSRC label columns) seen from one pulsar (deterministic.py:864, :872)
PTA_HD double pta_bwm_coef(const double *src, const double *phat) {
  double fp, fc, s2p, c2p;
  pta_bwm_antenna(src[PTA_BWM_COL_COS_GWTHETA], src[PTA_BWM_COL_GWPHI], phat, fp, fc);
  sincos(2.0 * src[PTA_BWM_COL_PSI], &s2p, &c2p);
  const double pol = c2p * fp + s2p * fc;
  return pol * pow(10.0, src[PTA_BWM_COL_LOG10_H]);
}

// burst epoch in seconds, rounded as deterministic.py:868 rounds it
PTA_HD double pta_bwm_t0(const double *src) { return src[PTA_BWM_COL_T0_MJD] * 86400.0; }

// residual [s] at t = mjd * 86400: one compare, one subtract, one multiply (a TOA exactly at t0 gets coef * 0)
PTA_HD double pta_bwm_ramp(double coef, double t0, double t) { return t < t0 ? 0.0 : coef * (t - t0); }
