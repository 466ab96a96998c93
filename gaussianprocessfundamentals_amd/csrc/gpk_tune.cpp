// The knob table's generated parts (gpk_tune.h): the name lookup, the environment-initialised process-wide instance
// and the per-thread overrides.  Plain C++17, no HIP header.
#include "gpk_tune.h"

#include <ctype.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

namespace gpk {

namespace {

// Knob names of gpk_tune / gpk_tune_thread (env: nullptr for "GPK_" + the key in upper case).
struct Knob {
  const char* key;
  const char* env;
  int64_t Tune::*field;
};
#define GPK_KNOB_ROW(field, dflt) {#field, nullptr, &Tune::field},
#define GPK_KNOB_ROW_N(field, dflt, key, env) {key, env, &Tune::field},
const Knob kKnobs[] = {GPK_KNOBS(GPK_KNOB_ROW, GPK_KNOB_ROW_N)};
#undef GPK_KNOB_ROW
#undef GPK_KNOB_ROW_N

thread_local std::vector<std::pair<int64_t Tune::*, int64_t>> t_tune_over;

}  // namespace

int64_t env_i64(const char* name, int64_t dflt) {
  const char* v = getenv(name);
  return (v && *v) ? (int64_t)atoll(v) : dflt;
}

Tune& tune() {
  static Tune t = [] {
    Tune t0;
    for (const Knob& k : kKnobs) {
      std::string env = "GPK_" + std::string(k.key);
      for (char& c : env) c = (char)toupper((unsigned char)c);
      t0.*(k.field) = env_i64(k.env ? k.env : env.c_str(), t0.*(k.field));
    }
    return t0;
  }();
  return t;
}

int64_t Tune::*knob_field(const char* key) {
  for (const Knob& k : kKnobs)
    if (!strcmp(key, k.key)) return k.field;
  return nullptr;
}

Tune tune_now() {
  Tune t = tune();
  for (const auto& o : t_tune_over) t.*(o.first) = o.second;
  return t;
}

void tune_thread_set(int64_t Tune::*f, int64_t value, bool set, int64_t* old_value, int32_t* old_set) {
  auto it = std::find_if(t_tune_over.begin(), t_tune_over.end(),
                         [&](const std::pair<int64_t Tune::*, int64_t>& o) { return o.first == f; });
  if (old_set) *old_set = it != t_tune_over.end() ? 1 : 0;
  if (old_value) *old_value = it != t_tune_over.end() ? it->second : tune().*f;
  if (it != t_tune_over.end()) t_tune_over.erase(it);
  if (set) t_tune_over.emplace_back(f, value);
}

// (declared for the kernels' units in gpk_internal.h)
bool tune_asm_feat() { return tune_now().asm_feat != 0; }
bool tune_asm_f32_fast() { return tune_now().asm_f32_fast != 0; }
int tune_asm_f32_chunk() { return (int)std::max<int64_t>(1, std::min<int64_t>(64, tune_now().asm_f32_chunk)); }
bool tune_cp_skip() { return tune_now().cp_skip != 0; }

}  // namespace gpk
