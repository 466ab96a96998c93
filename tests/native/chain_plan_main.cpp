// The chain planner without the HIP toolchain: built by tests/test_chain_plan_native.py from this file, gpk_tune.cpp
// and gpk_chain_plan.cpp with the system C++ compiler (no HIP include path), it prints one line per shape --
// "<kind> <diagonal blocks> <grid> <ntasks> <crc32 of the task words>" -- which the test compares with the same
// digest of the library's gpk_chain_plan_ex.  Knobs: the defaults (and the environment's, as in the library).
//
//   chain_plan_main           the test's shapes
//   chain_plan_main --sweep   the same shapes under chain_uq 0 / 1 / 2 x chain_u128 0 / 1 x chain_s128 0 / 1, each list
//                             also through chain_split_lists (for a sanitizer build: -fsanitize=address,undefined)
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "gpk_chain_plan.h"
#include "gpk_const.h"

namespace {

uint32_t crc32(const std::vector<int32_t>& words) {  // (zlib's: reflected 0xEDB88320, little-endian bytes)
  uint32_t c = 0xFFFFFFFFu;
  for (int32_t w : words)
    for (int b = 0; b < 4; ++b) {
      c ^= ((uint32_t)w >> (8 * b)) & 0xFFu;
      for (int i = 0; i < 8; ++i) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
    }
  return ~c;
}

int shapes(bool split) {
  const char* kinds[3] = {"plain", "eye", "f32"};
  for (int kind = 0; kind < 3; ++kind)
    for (int nblk : {1, 2, 3, 5, 9, 17, 33})
      for (int grid : {1, 7, 64, 256}) {
        const bool eye = kind == 1, f32 = kind == 2;
        const int64_t n_pad = (int64_t)nblk * gpk::NB, y_row = eye ? 2 * n_pad : n_pad;
        std::vector<int32_t> ord =
            gpk::chain_order(n_pad, y_row, grid, 1, gpk::chain_knobs(gpk::tune_now(), n_pad, eye, f32, grid), eye);
        if (ord.empty()) {
          fprintf(stderr, "chain_order: empty list for %s %d %d\n", kinds[kind], nblk, grid);
          return 1;
        }
        printf("%s %d %d %zu %08x", kinds[kind], nblk, grid, ord.size() / 4, crc32(ord));
        if (split) {
          const size_t n = ord.size();
          const int32_t nb = gpk::chain_split_lists(ord);
          if (ord.size() != n || nb < nblk) return 1;  // (list B holds at least the D tasks)
          printf(" %d %08x", nb, crc32(ord));
        }
        printf("\n");
      }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return shapes(false);
  if (strcmp(argv[1], "--sweep")) return 2;
  for (int uq = 0; uq <= 2; ++uq)
    for (int u128 = 0; u128 <= 1; ++u128)
      for (int s128 = 0; s128 <= 1; ++s128) {
        gpk::tune().chain_uq = uq;
        gpk::tune().chain_u128 = u128;
        gpk::tune().chain_s128 = s128;
        printf("# chain_uq %d chain_u128 %d chain_s128 %d\n", uq, u128, s128);
        if (int rc = shapes(true)) return rc;
      }
  return 0;
}
