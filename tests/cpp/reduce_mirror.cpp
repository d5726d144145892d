// tests/cpp/reduce_mirror.cpp -- laser::reduce_sum / reduce_min / reduce_max and laser::forEachReduce from a compiled C++
// caller (include/laser.hpp): sums of exactly representable values against a host loop, min / max, a transposed view
// against its contiguous copy (same logical order, same bits), an int64 sum that wraps, and a dot product with a double
// accumulator.  Prints SUCCESS.
#include <cstdio>
#include <cstring>
#include <vector>

#include "laser.hpp"

static int fails = 0;
template <typename T>
static void expect_bits(const char *what, T got, T want) {
  if (std::memcmp(&got, &want, sizeof(T)) != 0) {
    std::printf("FAIL %s: %.17g vs %.17g\n", what, (double)got, (double)want);
    fails++;
  }
}

int main() {
  const int64_t R = 301, Cn = 517, n = R * Cn;
  std::vector<float> x(n), y(n);
  std::vector<int64_t> k(n);
  float lo = 1e30f, hi = -1e30f;
  int64_t sum_exact = 0;
  uint64_t ksum = 0;
  for (int64_t i = 0; i < n; i++) {
    x[i] = (float)((i * 7919) % 2001 - 1000);  // integers: every partial sum is exact in float
    y[i] = (float)(i % 13) - 6.0f;
    k[i] = (int64_t)((uint64_t)i * 0x9E3779B97F4A7C15ull);
    sum_exact += (int64_t)x[i];
    ksum += (uint64_t)k[i];
    lo = x[i] < lo ? x[i] : lo;
    hi = x[i] > hi ? x[i] : hi;
  }
  auto tx = laser::newTensor<float>({R, Cn}), ty = laser::newTensor<float>({R, Cn});
  auto tk = laser::newTensor<int64_t>({n});
  laser::copyFromRaw(tx, x.data(), n);
  laser::copyFromRaw(ty, y.data(), n);
  laser::copyFromRaw(tk, k.data(), n);

  expect_bits("reduce_sum", laser::reduce_sum(tx), (float)sum_exact);
  expect_bits("reduce_min", laser::reduce_min(tx), lo);
  expect_bits("reduce_max", laser::reduce_max(tx), hi);
  expect_bits("reduce_sum int64 (wraps)", laser::reduce_sum(tk), (int64_t)ksum);

  // a transposed view and its contiguous copy hold the same values in the same logical order
  auto tt = laser::newTensor<float>({Cn, R});
  laser::forEach("t = s", {laser::out("t", tt), laser::in("s", tx.transposed())});
  expect_bits("transposed view = contiguous copy", laser::reduce_sum(tx.transposed()), laser::reduce_sum(tt));

  double dot = 0;
  for (int64_t i = 0; i < n; i++) dot += (double)x[i] * (double)y[i];  // exact: small integers
  expect_bits("forEachReduce dot", laser::forEachReduce<double>("acc += (double)x * y", "acc += other", 0.0,
                                                                {laser::in("x", tx), laser::in("y", ty)}), dot);

  if (fails == 0) std::printf("SUCCESS\n");
  return fails ? 1 : 0;
}
