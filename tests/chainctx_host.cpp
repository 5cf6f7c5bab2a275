// chainctx_host.cpp — haskoin-node_amd/csrc/hkv_chainctx.h compiled as plain
// C++ (tests/test_chainctx_model.py builds it with AddressSanitizer and
// UndefinedBehaviorSanitizer): the rule's functions on the case files that
// tests/chainctx_model.py writes, every field compared with the model's. The
// composition here is the serial one (a running sum, a running real-bits
// value); the device's scans are checked on the GPU against the same model.
//
//   chainctx_host <case file>...   prints "ok <headers>" per file, exit 0
//   chainctx_host                  checks the median network on all 2^11
//                                  zero-one inputs and prints "network ok"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../haskoin-node_amd/csrc/hkv_chainctx.h"

using namespace hkv;

static bool read_limbs(FILE* f, uint32_t v[8]) {
  for (int j = 0; j < 8; ++j)
    if (fscanf(f, "%" SCNx32, &v[j]) != 1) return false;
  return true;
}

static int fail(const char* path, size_t i, const char* what, uint64_t got, uint64_t want) {
  fprintf(stderr, "%s: header %zu %s: got %" PRIx64 ", want %" PRIx64 "\n", path, i, what, got, want);
  return 1;
}

static int run_case(const char* path) {
  FILE* f = fopen(path, "r");
  if (!f) return fprintf(stderr, "cannot open %s\n", path), 2;
  ChainCtx x;
  memset(&x, 0, sizeof x);
  uint32_t n = 0, n_cp = 0;
  bool ok = fscanf(f, "%" SCNx32 " %" SCNx32, &x.height0, &x.n_prev_times) == 2 && x.n_prev_times >= 1 &&
            x.n_prev_times <= CHAIN_MTP_SPAN;
  for (uint32_t j = 0; ok && j < x.n_prev_times; ++j) ok = fscanf(f, "%" SCNx32, &x.prev_times[j]) == 1;
  ok = ok && fscanf(f, "%" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx64, &x.parent_bits, &x.period_first_time,
                    &x.period_real_bits, &x.now) == 4;
  ok = ok && read_limbs(f, x.parent_work) && read_limbs(f, x.pow_limit);
  ok = ok && fscanf(f, "%" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32,
                    &x.interval, &x.target_timespan, &x.min_diff_spacing, &x.bip34_height, &x.bip66_height,
                    &x.bip65_height, &x.flags) == 7;
  ok = ok && fscanf(f, "%" SCNx32 " %" SCNx32, &n, &n_cp) == 2;
  if (!ok) return fclose(f), fprintf(stderr, "%s: bad context\n", path), 2;
  x.limit_bits = cc_encode_compact(x.pow_limit);
  std::vector<uint32_t> cp_h(n_cp), cp_x((size_t)n_cp * 8);
  for (uint32_t k = 0; ok && k < n_cp; ++k) ok = fscanf(f, "%" SCNx32, &cp_h[k]) == 1 && read_limbs(f, &cp_x[(size_t)k * 8]);
  std::vector<uint32_t> ver(n), tim(n), bit(n), hsh((size_t)n * 8), e_mtp(n), e_want(n), e_fl(n), e_work((size_t)n * 8);
  for (uint32_t i = 0; ok && i < n; ++i)
    ok = fscanf(f, "%" SCNx32 " %" SCNx32 " %" SCNx32, &ver[i], &tim[i], &bit[i]) == 3 &&
         read_limbs(f, &hsh[(size_t)i * 8]) &&
         fscanf(f, "%" SCNx32 " %" SCNx32 " %" SCNx32, &e_mtp[i], &e_want[i], &e_fl[i]) == 3 &&
         read_limbs(f, &e_work[(size_t)i * 8]);
  fclose(f);
  if (!ok) return fprintf(stderr, "%s: bad case\n", path), 2;

  // the time of header h of the batch (h < 0: the context's), 0xFFFFFFFF before the oldest
  auto time_at = [&](int64_t h) -> uint32_t {
    if (h >= 0) return tim[(size_t)h];
    if (-h <= (int64_t)x.n_prev_times) return x.prev_times[x.n_prev_times - (uint32_t)(-h)];
    return 0xFFFFFFFFu;
  };
  uint32_t work[8];
  memcpy(work, x.parent_work, sizeof work);
  uint64_t real = (1ull << 32) | x.period_real_bits;
  for (uint32_t i = 0; i < n; ++i) {
    ChainIn in;
    in.H = x.height0 + i;
    in.version = ver[i], in.time = tim[i], in.bits = bit[i];
    in.parent_time = time_at((int64_t)i - 1);
    in.parent_bits = i ? bit[i - 1] : x.parent_bits;
    in.parent_real = (uint32_t)real;
    in.first_time = (in.H % x.interval == 0 && i >= x.interval) ? tim[i - x.interval] : x.period_first_time;
    for (uint32_t j = 0; j < CHAIN_MTP_SPAN; ++j) in.window[j] = time_at((int64_t)i - 1 - j);
    const uint64_t before = (uint64_t)i + x.n_prev_times;
    in.c = before < CHAIN_MTP_SPAN ? (uint32_t)before : CHAIN_MTP_SPAN;
    in.checkpoint_ok = true;
    const uint32_t c = cc_checkpoint_at(cp_h.data(), n_cp, in.H);
    if (c != CHAIN_CP_NONE) in.checkpoint_ok = memcmp(&hsh[(size_t)i * 8], &cp_x[(size_t)c * 8], 32) == 0;
    uint32_t mtp = 0, want = 0;
    const uint32_t fl = chain_verdict(x, in, mtp, want);
    uint32_t hw[8];
    cc_header_work(bit[i], hw);
    cc_add256(work, work, hw);
    real = cc_real_join(real, cc_real_of(x, in.H, bit[i]));
    if (mtp != e_mtp[i]) return fail(path, i, "mtp", mtp, e_mtp[i]);
    if (want != e_want[i]) return fail(path, i, "want", want, e_want[i]);
    if (fl != e_fl[i]) return fail(path, i, "flags", fl, e_fl[i]);
    for (int j = 0; j < 8; ++j)
      if (work[j] != e_work[(size_t)i * 8 + j]) return fail(path, i, "work limb", work[j], e_work[(size_t)i * 8 + j]);
  }
  printf("ok %" PRIu32 "\n", n);
  return 0;
}

// the zero-one principle: a comparator network that sorts every 0/1 input sorts every input
static int check_network() {
  for (uint32_t m = 0; m < (1u << CHAIN_MTP_SPAN); ++m)
    for (uint32_t c = 1; c <= CHAIN_MTP_SPAN; ++c) {
      uint32_t w[CHAIN_MTP_SPAN], ones = 0;
      for (uint32_t j = 0; j < CHAIN_MTP_SPAN; ++j) {
        w[j] = j < c ? ((m >> j) & 1u) : 0xFFFFFFFFu;
        ones += j < c ? ((m >> j) & 1u) : 0u;
      }
      // element c / 2 of c sorted bits is 1 exactly when more than c - 1 - c / 2 of them are
      const uint32_t want = (c / 2 >= c - ones) ? 1u : 0u;
      if (cc_median(w, c) != want) return fprintf(stderr, "network: input %x of %u\n", m, c), 1;
      for (uint32_t j = 0; j + 1 < CHAIN_MTP_SPAN; ++j)
        if (w[j] > w[j + 1]) return fprintf(stderr, "network: input %x of %u is not sorted\n", m, c), 1;
    }
  printf("network ok\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return check_network();
  for (int a = 1; a < argc; ++a) {
    const int rc = run_case(argv[a]);
    if (rc) return rc;
  }
  return 0;
}
