// Host check of csrc/hkv_joint_digits.h (built under ASan and UBSan by
// tests/test_joint_digits.py). Standard input, hex words: line 1 the 64 class
// constants of the Python model; every further line k1 (5 words, two's
// complement), k2 (5 words) and the model's 11 packed digit words. Checks the
// header's table, joint_recode on each row, and jd_signed on each row's
// magnitudes.
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../haskoin-node_amd/csrc/hkv_joint_digits.h"

static bool read_words(const std::string& line, std::vector<uint32_t>& out) {
  std::istringstream in(line);
  std::string tok;
  out.clear();
  while (in >> tok) out.push_back((uint32_t)std::stoul(tok, nullptr, 16));
  return !out.empty();
}

// |k| and its sign of a five-word two's complement value
static bool magnitude(const uint32_t k[5], uint32_t mag[5]) {
  const bool neg = (k[4] >> 31) != 0;
  uint64_t c = neg ? 1 : 0;
  for (int q = 0; q < 5; ++q) {
    const uint64_t v = (uint64_t)(neg ? ~k[q] : k[q]) + c;
    mag[q] = (uint32_t)v;
    c = v >> 32;
  }
  return neg;
}

int main() {
  std::string line;
  std::vector<uint32_t> w;
  if (!std::getline(std::cin, line) || !read_words(line, w) || w.size() != 64) {
    std::printf("bad table line\n");
    return 2;
  }
  for (uint32_t c = 0; c < 64; ++c) {
    if (hkv::jd_class(c) != w[c]) {
      std::printf("class %u: %x, model %x\n", c, hkv::jd_class(c), w[c]);
      return 1;
    }
  }
  size_t rows = 0;
  while (std::getline(std::cin, line)) {
    if (!read_words(line, w)) continue;
    if (w.size() != 10 + hkv::JD_WORDS) {
      std::printf("row %zu: %zu words\n", rows, w.size());
      return 2;
    }
    uint32_t out[hkv::JD_WORDS];
    hkv::joint_recode(&w[0], &w[5], out);
    for (int q = 0; q < hkv::JD_WORDS; ++q) {
      if (out[q] != w[10 + q]) {
        std::printf("row %zu word %d: %x, model %x\n", rows, q, out[q], w[10 + q]);
        return 1;
      }
    }
    for (int h = 0; h < 2; ++h) {
      uint32_t mag[5];
      const bool neg = magnitude(&w[5 * h], mag);
      hkv::jd_signed(mag, neg);
      for (int q = 0; q < 5; ++q) {
        if (mag[q] != w[5 * h + q]) {
          std::printf("row %zu half %d: jd_signed word %d\n", rows, h, q);
          return 1;
        }
      }
    }
    ++rows;
  }
  std::printf("ok %zu rows\n", rows);
  return 0;
}
