// Stand-alone host program for tests/test_im_layout.py: includes the layout
// header alone (so its static_asserts run at this build's HKV_QW / HKV_GTAB_W),
// prints every field of the verify intermediates as "name off len", then
// re-runs the live-set checks at run time and prints "ok <sets>".
#include <cstdio>

#include "../haskoin-node_amd/csrc/hkv_layout.h"

using namespace hkv;

template <int N>
static bool check(const char* name, const Field (&f)[N], int words) {
  const bool ok = live_set_ok(f, words);
  if (!ok) std::printf("live set %s: overlap or out of range\n", name);
  return ok;
}

int main() {
  const struct {
    const char* name;
    Field f;
  } fields[] = {
      {"IM_FLAGS", IM_FLAGS}, {"IM_QX", IM_QX},     {"IM_W", IM_W},       {"IM_S", IM_S},
      {"IM_M", IM_M},         {"IM_R", IM_R},       {"IM_C", IM_C},       {"IM_DIG", IM_DIG},
      {"IM_GDIG", IM_GDIG},   {"IM_BX", IM_BX},     {"IM_BY", IM_BY},     {"IM_BZ", IM_BZ},
      {"IM_NUM", IM_NUM},     {"IM_NUMN", IM_NUMN}, {"IM_DEN", IM_DEN},   {"IM_AX", IM_AX},
      {"IM_AY", IM_AY},       {"IM_AZ", IM_AZ},     {"IM_RARE_LIST", IM_RARE_LIST},
      {"AUX_AX", AUX_AX},     {"AUX_AY", AUX_AY},   {"AUX_AZ", AUX_AZ},   {"AUX_Y0", AUX_Y0},
      {"AUX_FLAGS", AUX_FLAGS}, {"AUX_SQ", AUX_SQ},
  };
  std::printf("QW %d GTAB_W %d NWIN %d GWIN %d IM_WORDS %d AUX_WORDS %d\n", QW, GTAB_W, NWIN, GWIN, IM_WORDS, AUX_WORDS);
  for (const auto& e : fields) std::printf("%s %d %d\n", e.name, e.f.off, e.f.len);
  bool ok = true;
  int sets = 0;
#define LIVE(set, words) ok = check(#set, set, words) && ok, ++sets
  LIVE(LIVE_PROLOGUE_INV, IM_WORDS);
  LIVE(LIVE_INV_GLV, IM_WORDS);
  LIVE(LIVE_GLV_ECMULT, IM_WORDS);
  LIVE(LIVE_CHAIN_FINISH, IM_WORDS);
  LIVE(LIVE_FINISH_RARE, IM_WORDS);
  LIVE(LIVE_FINISH_VERDICT, IM_WORDS);
  LIVE(LIVE_SMALL_IM, IM_WORDS);
  LIVE(LIVE_SMALL_AUX, AUX_WORDS);
  // the predicate itself: touching ranges are disjoint, nested and crossing ones overlap
  ok = ok && !fields_overlap({0, 8}, {8, 8}) && fields_overlap({0, 9}, {8, 8}) && fields_overlap({8, 1}, {0, 16}) &&
       !fields_overlap({33, 1}, {35, 8});
  const Field clash[] = {IM_FLAGS, IM_S, IM_AY}, past[] = {IM_GDIG};
  ok = ok && !live_set_ok(clash, IM_WORDS) && !live_set_ok(past, IM_WORDS - 1);
  // every word the digits need lies inside the buffer the host sizes by IM_WORDS
  ok = ok && IM_DIG.len == NWIN && IM_GDIG.len == 2 * GWIN && IM_WORDS == IM_GDIG.off + 2 * GWIN &&
       IM_DIG.off + IM_DIG.len <= IM_GDIG.off;
  if (!ok) return 1;
  std::printf("ok %d\n", sets);
  return 0;
}
