// The deal of a diagonal update tile's blocks over the waves of update_tri_kernel (gpk_update_tri.hip).  Plain C++17,
// no HIP header: the kernel unrolls over this table at compile time and tests/native/tri_map_main.cpp checks its
// coverage on the CPU.
//
// A 128 x 128 diagonal tile (j, j) of the trailing update is 8 x 8 blocks of 16 x 16, of which the 36 with row block
// I >= column block J are ever read; the y row's tile below it, (last, j), has one live 16-row block: 8 more.  Waves
// w and w + 4 of a 512-thread workgroup share a SIMD, and the busiest SIMD sets the pace at every chunk barrier, so
// the 44 blocks are dealt by column strip: strip J has 9 - J blocks (I = J .. 7 and the y block), strips J and
// 7 - J together 11 -- SIMD J takes both, wave J six blocks and wave J + 4 five.
#pragma once

namespace gpk {

constexpr int kTriEdge = 8;     // 16 x 16 blocks per tile edge
constexpr int kTriY = 8;        // the row-block index that stands for the y row's block
constexpr int kTriWaves = 8;
constexpr int kTriPerWave = 6;  // most blocks of one wave
constexpr int kTriBlocks = kTriEdge * (kTriEdge + 1) / 2 + kTriEdge;  // 36 + 8

struct TriBlock {
  int i, j;  // row block (0 .. 7, kTriY) and column block of the tile
};
struct TriWave {
  int n;  // blocks of this wave
  TriBlock blk[kTriPerWave];
};

constexpr TriWave kTriDeal[kTriWaves] = {
    {6, {{0, 0}, {1, 0}, {2, 0}, {3, 0}, {4, 0}, {5, 0}}},
    {6, {{1, 1}, {2, 1}, {3, 1}, {4, 1}, {5, 1}, {6, 1}}},
    {6, {{2, 2}, {3, 2}, {4, 2}, {5, 2}, {6, 2}, {7, 2}}},
    {6, {{3, 3}, {4, 3}, {5, 3}, {6, 3}, {7, 3}, {kTriY, 3}}},
    {5, {{6, 0}, {7, 0}, {kTriY, 0}, {7, 7}, {kTriY, 7}}},
    {5, {{7, 1}, {kTriY, 1}, {6, 6}, {7, 6}, {kTriY, 6}}},
    {5, {{kTriY, 2}, {5, 5}, {6, 5}, {7, 5}, {kTriY, 5}}},
    {5, {{4, 4}, {5, 4}, {6, 4}, {7, 4}, {kTriY, 4}}},
};

// whether wave w reads rows of 16-row block r (0 .. 7, kTriY) as an operand of one of its blocks (with_y: the y blocks
// are part of the launch)
constexpr bool tri_wave_reads(int w, int r, bool with_y) {
  for (int b = 0; b < kTriDeal[w].n; ++b) {
    const TriBlock k = kTriDeal[w].blk[b];
    if (k.i == kTriY && !with_y) continue;
    if (k.i == r || k.j == r) return true;
  }
  return false;
}

}  // namespace gpk
