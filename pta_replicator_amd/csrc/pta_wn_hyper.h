// White-noise parameters per realisation (theta's wn_efac, wn_log10_equad, wn_log10_ecorr): the amplitudes of a (realisation, group)
// from its labels and the configured values, and the per-element expression of pta_engine_wn_add.
//
// A group is a (pulsar, backend flag) pair of set_white_noise / set_jitter.  Per realisation r, TOA i of group g and epoch e of
// ECORR group h (white_noise.py:105-109, :182):
//
//     dt[i] = (efac[r, g] sigma[i]) z1[i] + (efac[r, g] equad[r, g] | equad[r, g]) z2[i] + ecorr[r, h] z[e(i)]
//
// with the deviates generate() draws (streams (WN, a) and (ECORR, a), pta_rng.h).  A label that is NaN, or a key that is not given,
// takes the configured value of the group: the configured efac, the configured equad and ecorr in seconds (0 = none), the values
// prepare() computed, so that such a group's amplitudes are those of the fixed engine bit for bit.
//
// Everything is __host__ __device__: tests/wn_hyper compiles this header with g++ (-ffp-contract=off) and checks it against NumPy
// and a long-double evaluation of the expression.
#pragma once
#include <stdint.h>
#include <math.h>
#include "pta_rng.h"

#ifndef PTA_WN_HYPER_GMAX
#define PTA_WN_HYPER_GMAX 16  // groups of one pulsar whose amplitude rows a workgroup of pta_engine_wn_add stages
#endif

// a label or, where it is NaN (x != x), the configured value
PTA_HD double pta_wn_pick(double label, double configured) { return label != label ? configured : label; }

// equad / ecorr [s] of a label log10(value [s]); NaN = the configured value in seconds
PTA_HD double pta_wn_pow10(double log10_label, double configured) { return log10_label != log10_label ? configured : pow(10.0, log10_label); }

// (ea, eb) of a group: ea multiplies sigma z1, eb multiplies z2 (tnequad: equad alone, else efac equad; white_noise.py:105-109)
PTA_HD void pta_wn_amplitudes(double efac_label, double log10_equad_label, double efac_conf, double equad_conf, int tnequad, double &ea,
                              double &eb) {
  const double efac = pta_wn_pick(efac_label, efac_conf);
  const double equad = pta_wn_pow10(log10_equad_label, equad_conf);
  ea = efac;
  eb = tnequad ? equad : efac * equad;
}

// the EFAC / EQUAD term of one TOA: three products and one sum, in this order
PTA_HD double pta_wn_white(double ea, double sigma, double z1, double eb, double z2) { return (ea * sigma) * z1 + eb * z2; }

// the element of pta_engine_wn_add: (o + white) + ec z_e, a term that is switched off left out (o = 0 where the kernel writes)
PTA_HD double pta_wn_element(double o, bool has_wn, double ea, double sigma, double z1, double eb, double z2, bool has_ec, double ec,
                             double ze) {
  double v = o;
  if (has_wn) v = v + pta_wn_white(ea, sigma, z1, eb, z2);
  if (has_ec) v = v + ec * ze;
  return v;
}
