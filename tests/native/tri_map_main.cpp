// Coverage of the wave -> block deal of update_tri_kernel (gpk_tri_map.h), checked on the CPU: plain C++17, no HIP
// header.  Prints one line per finding and "ok <blocks> <busiest wave> <busiest SIMD pair>" when there is none;
// the exit status is the number of findings.
#include <stdio.h>

#include "gpk_tri_map.h"

int main() {
  using namespace gpk;
  int bad = 0;
  int owners[kTriEdge + 1][kTriEdge] = {};
  int per_wave[kTriWaves] = {}, max_wave = 0, max_pair = 0;
  for (int w = 0; w < kTriWaves; ++w) {
    const TriWave& d = kTriDeal[w];
    if (d.n < 0 || d.n > kTriPerWave) {
      printf("wave %d: %d blocks\n", w, d.n);
      ++bad;
      continue;
    }
    for (int b = 0; b < d.n; ++b) {
      const int i = d.blk[b].i, j = d.blk[b].j;
      // a tile block on or below the diagonal, or a y block
      if (j < 0 || j >= kTriEdge || i < j || i > kTriY) {
        printf("wave %d block %d: (%d, %d) is not a block of the map\n", w, b, i, j);
        ++bad;
        continue;
      }
      ++owners[i][j];
      ++per_wave[w];
      // the kernel's fragment reads must cover both operands of the block
      if (!tri_wave_reads(w, i, true) || !tri_wave_reads(w, j, true)) {
        printf("wave %d block (%d, %d): operand rows not read\n", w, i, j);
        ++bad;
      }
      if (i != kTriY && (!tri_wave_reads(w, i, false) || !tri_wave_reads(w, j, false))) {
        printf("wave %d block (%d, %d): operand rows not read without the y blocks\n", w, i, j);
        ++bad;
      }
    }
    if (per_wave[w] > max_wave) max_wave = per_wave[w];
  }
  int blocks = 0;
  for (int i = 0; i <= kTriY; ++i)
    for (int j = 0; j < kTriEdge; ++j) {
      const int want = (i == kTriY || i >= j) ? 1 : 0;
      if (owners[i][j] != want) {
        printf("block (%d, %d): %d owners, expected %d\n", i, j, owners[i][j], want);
        ++bad;
      }
      blocks += owners[i][j];
    }
  // waves w and w + 4 share a SIMD
  for (int w = 0; w < kTriWaves / 2; ++w) {
    const int pair = per_wave[w] + per_wave[w + kTriWaves / 2];
    if (pair > max_pair) max_pair = pair;
  }
  if (blocks != kTriBlocks || kTriBlocks != 44) {
    printf("%d blocks dealt, kTriBlocks %d, expected 44\n", blocks, kTriBlocks);
    ++bad;
  }
  if (max_wave > 6) {
    printf("a wave has %d blocks (> 6)\n", max_wave);
    ++bad;
  }
  if (max_pair > 11) {
    printf("a SIMD pair has %d blocks (> 11)\n", max_pair);
    ++bad;
  }
  if (!bad) printf("ok %d %d %d\n", blocks, max_wave, max_pair);
  return bad;
}
