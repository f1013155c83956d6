// TEST HARNESS (not product code): the pruned last inverse butterfly of pta_fft.h (outputs 0 and 1 only) against the full one,
// compiled with g++.  Two uses (tests/test_fft_pruned_host.py): as a shared library driven through ctypes, and - with
// -DFFT_PRUNED_MAIN - as a stand-alone program with its own inputs, which is the build that runs under the sanitizers.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../pta_replicator_amd/csrc/pta_rng.h"
#include "../../pta_replicator_amd/csrc/pta_fft.h"

extern "C" {

// n butterflies: vin[n][8][2] inputs, win[n][8][2] twiddles (w[0] unused); full[n][8][2] <- pta_fft_core<true, 9>,
// pruned[n][2][2] <- outputs 0, 1 of pta_fft_core_inv_out01<9>
void fp_butterflies(const double *vin, const double *win, int n, double *full, double *pruned) {
  for (int i = 0; i < n; ++i) {
    pta_cplx v[8], u[8], w[8];
    for (int q = 0; q < 8; ++q) {
      v[q] = u[q] = pta_cplx{vin[16 * i + 2 * q], vin[16 * i + 2 * q + 1]};
      w[q] = pta_cplx{win[16 * i + 2 * q], win[16 * i + 2 * q + 1]};
    }
    pta_fft_core<true, 9>(v, w);
    pta_fft_core_inv_out01<9>(u, w);
    for (int q = 0; q < 8; ++q) {
      full[16 * i + 2 * q] = v[q].re;
      full[16 * i + 2 * q + 1] = v[q].im;
    }
    for (int q = 0; q < 2; ++q) {
      pruned[4 * i + 2 * q] = u[q].re;
      pruned[4 * i + 2 * q + 1] = u[q].im;
    }
  }
}

// the twiddle set a thread builds for itself (pta_fft_twiddles<.., 1>) against w[1], w[2], w[4] read back from a table plus
// pta_fft_twiddle_products - the two ways the chirp-z kernel obtains a set; returns the number of differing doubles
int fp_twiddle_table_mismatches(const double *tw) {
  int bad = 0;
  for (int o = 0; o < 64; ++o) {
    pta_cplx a[8], b[8], tab[3];
    pta_fft_twiddles<6, 1>(tw, o, a);
    tab[0] = a[1];
    tab[1] = a[2];
    tab[2] = a[4];
    b[1] = tab[0];
    b[2] = tab[1];
    b[4] = tab[2];
    pta_fft_twiddle_products(b);
    for (int q = 1; q < 8; ++q) bad += memcmp(&a[q], &b[q], sizeof(pta_cplx)) != 0;
  }
  return bad;
}
}

#ifdef FFT_PRUNED_MAIN
static uint64_t lcg_state = 0x9E3779B97F4A7C15ull;
static double lcg_uniform() {  // (-1, 1)
  lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(int64_t)(lcg_state >> 11) / 4503599627370496.0 - 1.0;
}

int main() {
  const int n = 10000;
  double *vin = (double *)malloc(sizeof(double) * 16 * n), *win = (double *)malloc(sizeof(double) * 16 * n);
  double *full = (double *)malloc(sizeof(double) * 16 * n), *pruned = (double *)malloc(sizeof(double) * 4 * n);
  if (!vin || !win || !full || !pruned) return 2;
  for (int i = 0; i < 16 * n; ++i) {
    vin[i] = lcg_uniform() * (i % 5 == 0 ? 1e-9 : 1.0);
    win[i] = lcg_uniform();
  }
  for (int i = 0; i < 16; ++i) vin[i] = (i & 1) ? -0.0 : 0.0;  // signed zeros through the sums
  fp_butterflies(vin, win, n, full, pruned);
  int bad = 0;
  for (int i = 0; i < n; ++i) bad += memcmp(full + 16 * i, pruned + 4 * i, 4 * sizeof(double)) != 0;
  double tw[2 * PTA_FFT_N];
  for (int m = 0; m < PTA_FFT_N; ++m) {
    tw[2 * m] = lcg_uniform();
    tw[2 * m + 1] = lcg_uniform();
  }
  bad += fp_twiddle_table_mismatches(tw);
  free(vin);
  free(win);
  free(full);
  free(pruned);
  printf("fft_pruned_check: %d butterflies, %d mismatches\n", n, bad);
  return bad ? 1 : 0;
}
#endif
