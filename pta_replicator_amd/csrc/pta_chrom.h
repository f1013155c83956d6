// One chromatic Gaussian process per pulsar (ReplicaEngine.set_chromatic_noise; DM variations at index 2):
//   dt_i = (nu_ref / nu_i)^chi sum_k F_ik y_k,  y_k = sqrt(phi_k) z_k,
// F and phi those of the red noise (red_noise.py:106-128), z from a stream of its own.  The row weights are applied on the host to the
// design matrix (Ft_chrom = w . Ft): no device pow.  Struct: pta_chrom_engine (include/pta_replicator_amd.h).
#pragma once
#include <stdint.h>
#include <math.h>
#include "pta_rng.h"
#include "pta_hyper.h"

// realisations per workgroup of pta_engine_chrom_add, a multiple of 16 (one MFMA row tile); chosen among 16, 32 and 64 by measurement
// (profiles/r24_chrom_throughput.json; the probe builds of scripts/gpu_chrom_throughput.py define it on the command line)
#ifndef PTA_CHROM_RG
#define PTA_CHROM_RG 16
#endif
#define PTA_CHROM_PITCH (PTA_ENGINE_TILE + 2)  // doubles per realisation row of the staged tile: even (16-byte pairs), two past the tile for
                                               // the never-used second element of a shifted last pair

// sqrt(prior) of coefficient c of pulsar a in one realisation: the configured table where log10_A is NaN ("as configured") or no
// theta is given, else pta_rn_amp at the column's frequency (sin and cos column share it)
PTA_HD double pta_chrom_amp(const double *amp_conf, const double *f, const double *tspan, int a, int K, int c, bool theta, double log10_A,
                            double gamma) {
  if (!theta || isnan(log10_A)) return amp_conf[(int64_t)a * K + c];
  return pta_rn_amp(f[(int64_t)a * (K / 2) + (c >> 1)], tspan[a], log10_A, gamma);
}
