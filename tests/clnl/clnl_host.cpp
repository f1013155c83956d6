// TEST HARNESS (not product code): compiles pta_replicator_amd/csrc/pta_clnl.h with g++ so that the grid point's scale d_g,k, the entry of
// M_g and the epilogue of the correlated likelihood kernels can be checked against NumPy on a machine without a GPU.  Loaded by
// tests/test_clnl_host.py via ctypes.
#include <stdint.h>
#include "../../pta_replicator_amd/csrc/pta_clnl.h"

extern "C" void ch_scale(int C, double T, double gamma_ref, const double *log10_A, const double *gamma, int G, double *d) {
  for (int g = 0; g < G; ++g)
    for (int k = 0; k < C; ++k) d[g * C + k] = pta_clnl_scale(k, T, gamma_ref, log10_A[g], gamma[g]);
}

extern "C" double ch_m_entry(double di, double tij, double dj, int diag) { return pta_clnl_m_entry(di, tij, dj, diag); }

extern "C" double ch_value(double quad, double half_logdet) { return pta_clnl_value(quad, half_logdet); }
