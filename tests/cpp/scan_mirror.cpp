// tests/cpp/scan_mirror.cpp -- laser::cumsum, searchsorted, cdfSample and cdfSampleAndRemove from a compiled C++ caller
// (include/laser.hpp): a float row longer than a tile against the order written out by hand, an int64 row that wraps, the
// reference's searchsorted vectors on both sides, draws at u = 0 and at the largest u below 1, draw-and-remove until a row is
// empty (the caller's weights untouched), the generator forms against the buffer forms, and the refusals.  Prints SUCCESS.
#include <cstdio>
#include <cstring>
#include <vector>

#include "laser.hpp"

static int fails = 0;
static void expect(const char *what, bool ok) {
  if (!ok) {
    std::printf("FAIL %s\n", what);
    fails++;
  }
}

int main() {
  int64_t plan[4];
  laser::check(laser_hip_cumsum_plan(1, 1 << 20, 4, 0, plan));
  const int64_t R = (1 << 20) / (plan[3] * 256);  // tiles of 256 R elements
  expect("a run of 8, 16 or 32", R == 8 || R == 16 || R == 32);

  // two rows of 2 tiles + 3 elements, 60 % zeros in the second
  const int64_t rows = 2, n = 2 * 256 * R + 3;
  std::vector<float> x(rows * n), want(rows * n);
  unsigned s = 2463534242u;
  for (int64_t i = 0; i < rows * n; i++) {
    s ^= s << 13, s ^= s >> 17, s ^= s << 5;
    x[i] = (i >= n && s % 10 < 6) ? 0.0f : (float)(s >> 8) / 16777216.0f;
  }
  for (int64_t r = 0; r < rows; r++) {
    volatile float loc = 0, carry = 0, out = 0;
    for (int64_t i = 0; i < n; i++) {
      loc = i % R == 0 ? x[r * n + i] : loc + x[r * n + i];
      out = i < R ? loc : carry + loc;
      want[r * n + i] = out;
      if (i % R == R - 1) carry = out;
    }
  }
  auto tx = laser::newTensor<float>({rows, n});
  laser::copyFromRaw(tx, x.data(), rows * n);
  auto cdf = laser::cumsum(tx);
  const std::vector<float> got = cdf.to_host();
  expect("cumsum: the bits of the order written out", got.size() == want.size() && std::memcmp(got.data(), want.data(), got.size() * 4) == 0);
  bool mono = true;
  for (int64_t r = 0; r < rows; r++)
    for (int64_t i = 1; i < n; i++) mono = mono && got[r * n + i] >= got[r * n + i - 1] && (x[r * n + i] != 0 || got[r * n + i] == got[r * n + i - 1]);
  expect("cumsum: monotone, and a zero weight does not move it", mono);

  const int64_t big[4] = {INT64_MAX, 1, INT64_MAX, 2};
  auto tb = laser::newTensor<int64_t>({4});
  laser::copyFromRaw(tb, big, 4);
  const std::vector<int64_t> wb = laser::cumsum(tb).to_host();
  expect("cumsum int64 wraps", wb[0] == INT64_MAX && wb[1] == INT64_MIN && wb[2] == -1 && wb[3] == 1);

  // sanityChecks of bench_multinomial_samplers.nim:71-82
  const int32_t a[10] = {0, 3, 9, 9, 10, 1, 2, 3, 4, 5}, v[6] = {2, 4, 9, 0, 2, 6};
  auto ta = laser::newTensor<int32_t>({2, 5});
  auto tv = laser::newTensor<int32_t>({2, 3});
  laser::copyFromRaw(ta, a, 10);
  laser::copyFromRaw(tv, v, 6);
  expect("searchsorted, left side", laser::searchsorted(ta, tv).to_host() == std::vector<int32_t>({1, 2, 2, 0, 1, 5}));
  expect("searchsorted, right side", laser::searchsorted(ta, tv, false).to_host() == std::vector<int32_t>({1, 2, 4, 0, 2, 5}));

  // draws
  const float w[10] = {0.0f, 0.5f, 0.0f, 1.5f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  const float top = 1.0f - 1.0f / 16777216.0f;
  const float u[6] = {0.0f, top, 0.5f, 0.0f, top, 0.5f};
  auto tw = laser::newTensor<float>({2, 5});
  auto tu = laser::newTensor<float>({2, 3});
  laser::copyFromRaw(tw, w, 10);
  laser::copyFromRaw(tu, u, 6);
  const std::vector<int32_t> idx = laser::cdfSample(laser::cumsum(tw), tu).to_host();
  expect("cdfSample: first and last positive element, 0.5 of 2.0 in element 3, -1 on the empty row",
         idx == std::vector<int32_t>({1, 3, 3, -1, -1, -1}));
  const std::vector<int32_t> rem = laser::cdfSampleAndRemove(tw, tu).to_host();
  expect("cdfSampleAndRemove: both positive elements once, then -1", rem == std::vector<int32_t>({1, 3, -1, -1, -1, -1}));
  const std::vector<float> after = tw.to_host();
  expect("cdfSampleAndRemove works on a private copy", std::memcmp(after.data(), w, sizeof w) == 0);

  // the generator forms: the same indices as a fill followed by the buffer forms
  laser::Rng r1(7, 1), r2(7, 1), r3(7, 1);
  auto fill = laser::randomTensor<float>({rows, 4}, 0.0f, 1.0f, r1);
  expect("cdfSample(rng) equals the buffer form", laser::cdfSample(cdf, r2, 4).to_host() == laser::cdfSample(cdf, fill).to_host());
  expect("cdfSampleAndRemove(rng) equals the buffer form", laser::cdfSampleAndRemove(tx, r3, 4).to_host() == laser::cdfSampleAndRemove(tx, fill).to_host());
  expect("the generators advanced by rows * num", r2.offset == (uint64_t)rows * 4 && r3.offset == r2.offset && r1.offset == r2.offset);

  bool threw = false;
  try {
    laser::cumsum(laser::newTensor<float>({2, 3, 4}));
  } catch (const laser::Error &) {
    threw = true;
  }
  expect("rank 3 is refused", threw);
  threw = false;
  try {
    laser::cdfSample(cdf, laser::newTensor<float>({3, 2}));
  } catch (const laser::Error &) {
    threw = true;
  }
  expect("uniform numbers of another row count are refused", threw);
  if (fails == 0) std::printf("SUCCESS\n");
  return fails ? 1 : 0;
}
