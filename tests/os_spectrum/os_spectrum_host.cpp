// TEST HARNESS (not product code): compiles pta_replicator_amd/csrc/pta_os_spectrum.h with g++ so that the map between the frequency
// blocks of the per-frequency Fisher matrix and the packed triangle of Z can be checked against NumPy on a machine without a GPU.
// Loaded by tests/test_os_spectrum_host.py via ctypes.
#include "../../pta_replicator_amd/csrc/pta_os_spectrum.h"

// out[6 e .. 6 e + 5] = k, j, idx[0..3] of block e < n_f (n_f + 1) / 2 as pta_osp_block_kj / pta_osp_block_entries give them; returns
// the number of blocks, or -1 - e if pta_osp_block(k, j) does not give e back
extern "C" int osp_blocks(int C, int32_t *out) {
  const int nf = C / 2, nb = pta_osp_nblocks(nf);
  for (int e = 0; e < nb; ++e) {
    int k, j, idx[4];
    pta_osp_block_kj(e, k, j);
    if (pta_osp_block(k, j) != e) return -1 - e;
    pta_osp_block_entries(k, j, idx);
    out[6 * e] = k;
    out[6 * e + 1] = j;
    for (int q = 0; q < 4; ++q) out[6 * e + 2 + q] = idx[q];
  }
  return nb;
}
