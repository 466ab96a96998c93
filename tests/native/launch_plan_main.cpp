// The launch path's schedule without the HIP toolchain: built by tests/test_launch_plan_native.py from this file,
// gpk_tune.cpp and gpk_launch_plan.cpp with the system C++ compiler (no HIP include path), it prints one line per shape
// -- "<kind> <diagonal blocks> <m> <batch> <kbuild> <nsteps> <crc32 of the step records>" -- which the test compares
// with the same digest of the library's gpk_launch_plan.  Knobs: the defaults (and the environment's, as in the library).
//
//   launch_plan_main           the test's shapes
//   launch_plan_main --sweep   the same shapes under ingroup 1 / 2 / 3 x lookahead 0 / 1 x group 2 / 8 x group_first
//                              1 / 8 x fuse_trsm 0 / 1 / 2 x band_skip 0 / 1 (for a sanitizer build:
//                              -fsanitize=address,undefined)
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "gpk_const.h"
#include "gpk_launch_plan.h"

namespace {

uint32_t crc32(const std::vector<gpk::LaunchStep>& steps) {  // (zlib's: reflected 0xEDB88320, the records' bytes)
  uint32_t c = 0xFFFFFFFFu;
  const unsigned char* p = reinterpret_cast<const unsigned char*>(steps.data());
  for (size_t i = 0; i < steps.size() * sizeof(gpk::LaunchStep); ++i) {
    c ^= p[i];
    for (int b = 0; b < 8; ++b) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
  }
  return ~c;
}

int shapes() {
  const char* kinds[3] = {"plain", "eye", "f32"};
  std::vector<gpk::LaunchStep> steps;
  for (int kind = 0; kind < 3; ++kind)
    for (int nblk : {1, 2, 3, 5, 9, 17, 65})
      for (int64_t m : {0, 77})
        for (int batch : {1, 32})
          for (int kbuild = 0; kbuild <= 1; ++kbuild) {
            const bool eye = kind == 1, f32 = kind == 2;
            if (eye && m != 0) continue;                        // identity rows: m = n, listed under m = 0
            if (kbuild && (kind != 0 || m != 0)) continue;      // the fused K build: f64, no extra rows
            const int64_t n_pad = (int64_t)nblk * gpk::NB, y_row = n_pad + (eye ? n_pad : m);
            const gpk::LaunchShape sh{f32, batch, eye ? n_pad : m, n_pad, y_row, (y_row + gpk::NB) / gpk::NB * gpk::NB};
            gpk::launch_plan(sh, eye, true, kbuild != 0, gpk::tune_now(), steps);
            int64_t ndiag = 0, first_kb = -1;
            for (const gpk::LaunchStep& s : steps) {
              if (s.kbuild && first_kb < 0) first_kb = ndiag;
              ndiag += s.kind == gpk::LP_DIAG;
            }
            if (ndiag != nblk || (kbuild && first_kb != gpk::launch_first_group(gpk::tune_now(), eye, n_pad))) {
              fprintf(stderr, "launch_plan: %s %d: %lld diagonal blocks, K build after %lld\n", kinds[kind], nblk,
                      (long long)ndiag, (long long)first_kb);
              return 1;
            }
            printf("%s %d %lld %d %d %zu %08x\n", kinds[kind], nblk, (long long)m, batch, kbuild, steps.size(),
                   crc32(steps));
          }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return shapes();
  if (strcmp(argv[1], "--sweep")) return 2;
  gpk::Tune& t = gpk::tune();
  for (int ingroup = 1; ingroup <= 3; ++ingroup)
    for (int la = 0; la <= 1; ++la)
      for (int group : {2, 8})
        for (int first : {1, 8})
          for (int fuse = 0; fuse <= 2; ++fuse)
            for (int band = 0; band <= 1; ++band) {
              t.ingroup = ingroup;
              t.lookahead = la;
              t.group = t.group_eye = group;
              t.group_first = first;
              t.fuse_trsm = fuse;
              t.band_skip = band;
              printf("# ingroup %d lookahead %d group %d group_first %d fuse_trsm %d band_skip %d\n", ingroup, la,
                     group, first, fuse, band);
              if (int rc = shapes()) return rc;
            }
  return 0;
}
