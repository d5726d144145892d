// tests/cpp/normal_mirror.cpp -- laser::Rng::randomNormalTensor and laser::randomNormalTensor from a compiled C++ caller
// (include/laser.hpp).  The device's normal fill against normal_core.h compiled into this program, position by position (the
// same bits; built with -ffp-contract=off), the offset bookkeeping, two draws against one, and refused parameters.  Prints
// SUCCESS.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "laser.hpp"
#include "normal_core.h"

static int fails = 0;
static void expect(const char *what, bool ok) {
  if (!ok) {
    std::printf("FAIL %s\n", what);
    fails++;
  }
}

static std::vector<float> host_fill(int64_t n, float mean, float std, uint64_t seed, uint64_t subseq, uint64_t offset) {
  std::vector<float> out((size_t)n);
  for (int64_t i = 0; i < n; i++) {
    const unsigned long long p = offset + (unsigned long long)i;
    unsigned int o[4];
    lh_philox_block(seed, subseq, p >> 2, o);
    const int first = (int)(p & 2);
    out[(size_t)i] = lh_normal_scale_f32(lh_normal_z(o[first], o[first + 1], (int)(p & 1)), mean, std);
  }
  return out;
}

int main() {
  const uint64_t seed = 0x1234567887654321ull, subseq = 5;
  laser::Rng rng(seed, subseq, 3);
  const std::vector<float> a = rng.randomNormalTensor({7, 151}, 0.25f, 1.5f).to_host();
  expect("the offset advances by the element count", rng.offset == 3 + 7 * 151);
  const std::vector<float> want = host_fill(7 * 151, 0.25f, 1.5f, seed, subseq, 3);
  expect("randomNormalTensor = normal_core.h on the host, bit for bit", std::memcmp(a.data(), want.data(), a.size() * sizeof(float)) == 0);

  laser::Rng one(seed, subseq, 3), two(seed, subseq, 3);
  const std::vector<float> whole = laser::randomNormalTensor({1000}, 0.0f, 1.0f, one).to_host();
  std::vector<float> cut = laser::randomNormalTensor({333}, 0.0f, 1.0f, two).to_host();  // ends inside a pair
  const std::vector<float> rest = laser::randomNormalTensor({667}, 0.0f, 1.0f, two).to_host();
  cut.insert(cut.end(), rest.begin(), rest.end());
  expect("two draws are one draw cut in two", one.offset == two.offset && std::memcmp(whole.data(), cut.data(), whole.size() * sizeof(float)) == 0);
  bool bounded = true;
  for (float z : whole) bounded = bounded && std::fabs(z) <= 5.77f;
  expect("|z| <= 5.77", bounded);

  laser::Rng other(seed, subseq + 1, 3);
  const std::vector<float> b = other.randomNormalTensor({1000}).to_host();
  expect("another subseq is another stream", std::memcmp(whole.data(), b.data(), b.size() * sizeof(float)) != 0);

  int refused = 0;
  const float bad[][2] = {{NAN, 1.0f}, {INFINITY, 1.0f}, {0.0f, -1.0f}, {0.0f, NAN}, {0.0f, INFINITY}};
  for (const auto &p : bad) {
    try {
      rng.randomNormalTensor({4}, p[0], p[1]);
    } catch (const laser::Error &) {
      refused++;
    }
  }
  expect("a non-finite mean and a negative or non-finite std are refused", refused == 5 && rng.offset == 3 + 7 * 151);

  if (fails == 0) std::printf("SUCCESS\n");
  return fails ? 1 : 0;
}
