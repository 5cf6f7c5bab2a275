// Stand-alone run of oracle/secp_fast.c's record builders (hkvo_fast_chosen_records,
// hkvo_fast_gtable_records), built by tests/test_secp_fast.py with
// -fsanitize=address,undefined: every pin mode, the redraws, the threaded table
// sweeps with ragged blocks (positive, negative and strided), the last byte of
// every output buffer, and each error return that can be provoked. Every record
// built must verify in both modes. Prints "ok <records>" or the first failure
// and exits 1.
#include "../oracle/secp_fast.c"  // first: it sets its feature-test macro before any system header

#include <stdio.h>

#define CHECK(c, ...)              \
  do {                             \
    if (!(c)) {                    \
      printf("FAIL: " __VA_ARGS__); \
      printf("\n");                \
      return 1;                    \
    }                              \
  } while (0)

static int all_verify(const uint8_t* recs, size_t n, const char* what) {
  for (size_t i = 0; i < n; ++i)
    for (int mode = 0; mode < 2; ++mode)
      if (!hkvo_fast_verify_record(recs + 168 * i, mode)) {
        printf("FAIL: %s record %zu rejected in mode %d\n", what, i, mode);
        return 0;
      }
  return 1;
}

static void put_sc(uint8_t* b, const sc* a) { be_from_u256(b, a->d); }

int main(void) {
  size_t total = 0;
  // chosen records: fillers for all three scalars, the three pins in turn
  {
    enum { N = 300 };
    uint8_t *u1 = malloc(32 * N), *u2 = malloc(32 * N), *d = malloc(32 * N), *pin = malloc(N), *out = malloc(168 * N);
    for (size_t i = 0; i < N; ++i) {
      sc a, b, c;
      sc_filler(&a, 11, i, 0);
      sc_filler(&b, 12, i, 0);
      sc_filler(&c, 13, i, 0);
      if (i % 7 == 0) memset(&a, 0, sizeof a);  // u1 = 0 is a valid request (msg32 = 0)
      put_sc(u1 + 32 * i, &a);
      put_sc(u2 + 32 * i, &b);
      put_sc(d + 32 * i, &c);
      pin[i] = (uint8_t)(1 + i % 3);
    }
    CHECK(hkvo_fast_chosen_records(u1, u2, d, pin, N, out) == 0, "chosen records");
    if (!all_verify(out, N, "chosen")) return 1;
    total += N;
    // error returns: u2 = 0, d = 0, a scalar >= n, an unknown pin, u1 + u2 d = 0
    memset(u2 + 32 * 5, 0, 32);
    CHECK(hkvo_fast_chosen_records(u1, u2, d, pin, N, out) == -(8 * 5 + HKVO_E_U2_ZERO), "u2 = 0 not reported");
    memset(d + 32 * 3, 0, 32);
    CHECK(hkvo_fast_chosen_records(u1, u2, d, pin, N, out) == -(8 * 3 + HKVO_E_ARG), "d = 0 not reported");
    memset(u1 + 32 * 2, 0xFF, 32);
    CHECK(hkvo_fast_chosen_records(u1, u2, d, pin, N, out) == -(8 * 2 + HKVO_E_ARG), "u1 >= n not reported");
    pin[1] = 0;
    CHECK(hkvo_fast_chosen_records(u1, u2, d, pin, N, out) == -(8 * 1 + HKVO_E_ARG), "pin 0 not reported");
    {
      sc one = {{1, 0, 0, 0}}, minus1;
      sc_negate(&minus1, &one);
      put_sc(u1, &one);
      put_sc(u2, &one);
      put_sc(d, &minus1);
      CHECK(hkvo_fast_chosen_records(u1, u2, d, pin, N, out) == -(8 * 0 + HKVO_E_INFINITY), "R = infinity not reported");
    }
    CHECK(hkvo_fast_chosen_records(u1, u2, d, pin, 0, out) == 0, "n = 0");
    free(u1), free(u2), free(d), free(pin), free(out);
  }
  // table sweeps: counts that leave ragged blocks and a ragged last thread
  {
    enum { MAXC = 2100 };
    uint8_t* out = malloc(168 * MAXC);
    static const struct { int t; uint64_t j0, step; size_t count; int neg; } runs[] = {
        {0, 1, 1, 2100, 0},  {1, (1 << 19) - 1000, 1, 1001, 0}, {5, 1, 64, 1025, 1}, {11, 7, 1, 257, 1},
        {12, 1, 1, 255, 0},  {13, 1, 1, 255, 0},                {6, 1 << 19, 1, 1, 0}, {3, 1, 1, 1, 1},
        {10, 3, 1 << 18, 2, 0}};
    for (size_t k = 0; k < sizeof runs / sizeof runs[0]; ++k) {
      CHECK(hkvo_fast_gtable_records_strided(runs[k].t, runs[k].j0, runs[k].step, runs[k].count, runs[k].neg, out) == 0,
            "table run %zu", k);
      if (!all_verify(out, runs[k].count, "table")) return 1;
      total += runs[k].count;
    }
    CHECK(hkvo_fast_gtable_records(2, 1, 300, 0, out) == 0, "table 2");
    if (!all_verify(out, 300, "table 2")) return 1;
    total += 300;
    // out of range: table 14, j = 0, j past 2^19, 256 2^248 >= n, the negative form without a next window
    CHECK(hkvo_fast_gtable_records(14, 1, 1, 0, out) == -HKVO_E_ARG, "table 14 accepted");
    CHECK(hkvo_fast_gtable_records(0, 0, 1, 0, out) == -HKVO_E_ARG, "j = 0 accepted");
    CHECK(hkvo_fast_gtable_records(0, (1 << 19), 2, 0, out) == -HKVO_E_ARG, "j = 2^19 + 1 accepted");
    CHECK(hkvo_fast_gtable_records(13, 256, 1, 0, out) == -HKVO_E_ARG, "u1 >= n accepted");
    CHECK(hkvo_fast_gtable_records(12, 1, 1, 1, out) == -HKVO_E_ARG, "negative form in window 6 accepted");
    CHECK(hkvo_fast_gtable_records(4, 1, 0, 0, out) == 0, "count = 0");
    free(out);
  }
  free(g_pre);
  free(g_pre128);
  printf("ok %zu\n", total);
  return 0;
}
