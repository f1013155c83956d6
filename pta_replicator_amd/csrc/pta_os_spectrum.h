// Per-frequency optimal statistic: the map between the n_f (n_f + 1) / 2 frequency blocks (k >= j) of the Fisher matrix and the
// packed lower triangle of Z that pta_os_matched_solve writes (entry (i, l <= i) of the C x C matrix at i (i + 1) / 2 + l, C = 2 n_f,
// column 2 k / 2 k + 1 = sin / cos of frequency k).  __host__ __device__: tests/os_spectrum compiles this header with g++ against
// NumPy.
#pragma once
#include <stdint.h>

#ifndef PTA_HD
#if defined(__HIPCC__)
#define PTA_HD __host__ __device__ __forceinline__
#else
#define PTA_HD inline
#endif
#endif

// number of blocks (k, j <= k) of n_f frequencies, and the linear index of one: rows of the block triangle in ascending k
PTA_HD int pta_osp_nblocks(int nf) { return nf * (nf + 1) / 2; }
PTA_HD int pta_osp_block(int k, int j) { return k * (k + 1) / 2 + j; }

// (k, j) of block e: k = the largest integer with k (k + 1) / 2 <= e (e <= 527: exact in integers)
PTA_HD void pta_osp_block_kj(int e, int &k, int &j) {
  int r = 0;
  while ((r + 1) * (r + 2) / 2 <= e) ++r;
  k = r;
  j = e - r * (r + 1) / 2;
}

// whether block e lies on the diagonal (k == j)
PTA_HD bool pta_osp_is_diagonal(int e) {
  int k, j;
  pta_osp_block_kj(e, k, j);
  return k == j;
}

// packed index of entry (i, l <= i)
PTA_HD int pta_osp_packed(int i, int l) { return i * (i + 1) / 2 + l; }

// The four packed entries whose products Z_a[.] Z_b[.] sum to D_ab[k, j] = sum_{i in {2k, 2k+1}} sum_{l in {2j, 2j+1}} Z_a[i, l] Z_b[i, l],
// j <= k.  Off the diagonal all four (i, l) lie below the diagonal of Z.  In a diagonal block (2k, 2k+1) is the transpose of
// (2k+1, 2k): that packed entry is listed twice.
PTA_HD void pta_osp_block_entries(int k, int j, int idx[4]) {
  const int r0 = pta_osp_packed(2 * k, 0), r1 = pta_osp_packed(2 * k + 1, 0);
  idx[0] = r0 + 2 * j;
  idx[1] = (j < k) ? r0 + 2 * j + 1 : r1 + 2 * j;
  idx[2] = r1 + 2 * j;
  idx[3] = r1 + 2 * j + 1;
}
