// tests/cpp/random_mirror.cpp -- laser::Rng, laser::randomTensor and the Sampler's seeded draws from a compiled C++ caller
// (include/laser.hpp).  Prints one line per result, a name and the elements as hex bit patterns, for the test to compare with
// the numpy model; checks the bookkeeping and the refusals itself.  Prints SUCCESS.
#include <cinttypes>
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
template <typename T>
static void show(const char *name, const std::vector<T> &v) {
  std::printf("%s", name);
  for (const T &x : v) {
    if (sizeof(T) == 8) {
      uint64_t b;
      std::memcpy(&b, &x, 8);
      std::printf(" %016" PRIx64, b);
    } else {
      uint32_t b;
      std::memcpy(&b, &x, 4);
      std::printf(" %08" PRIx32, b);
    }
  }
  std::printf("\n");
}

int main() {
  laser::Rng rng(0x0123456789ABCDEFull, (1ull << 40) + 7);
  auto f = laser::randomTensor<float>({2, 5}, -1.0f, 1.0f, rng);
  expect("ten float32 use ten words", rng.offset == 10 && f.shape[0] == 2 && f.shape[1] == 5);
  show("f32", f.to_host());
  auto d = laser::randomTensor<double>({5}, -1.0, 1.0, rng);
  expect("five float64 use ten words", rng.offset == 20);
  show("f64", d.to_host());
  show("i32", laser::randomTensor<int32_t>({6}, -3, 5, rng).to_host());
  show("i64", laser::randomTensor<int64_t>({3}, (int64_t)1 << 40, rng).to_host());  // the `max` form: [0, max]
  expect("six int32 and three int64 use twelve words", rng.offset == 32);
  show("bits", laser::randomBits(7, rng).to_host());
  expect("seven words", rng.offset == 39);

  const int64_t R = 2, N = 5;
  const float w[R * N] = {0.3f, 1.5f, 0.4f, 0.3f, 0.3f, 0.0f, 2.0f, 0.0f, 1.0f, 0.0f};
  auto tw = laser::newTensor<float>({R, N});
  laser::copyFromRaw(tw, w, R * N);
  laser::Sampler s(tw);
  const std::vector<float> before = s.tree.to_host();
  const std::vector<int32_t> idx = s.sample(rng, 4).to_host();
  expect("a seeded draw of (2, 4) uses eight words and leaves the trees alone",
         rng.offset == 47 && idx.size() == 8 && std::memcmp(before.data(), s.tree.to_host().data(), before.size() * 4) == 0);
  show("sample", idx);

  // the same draw from uniform numbers filled by hand: the two-step form
  laser::Rng again(rng.seed, rng.subseq, 39);
  auto u = laser::randomTensor<float>({R, 4}, 0.0f, 1.0f, again);
  expect("seeded draw == uniform fill, then sample", s.sample(u).to_host() == idx && again.offset == 47);

  show("remove", s.sampleAndRemove(rng, 4).to_host());
  expect("draw and remove advances by rows * num", rng.offset == 55);
  const std::vector<uint64_t> off = {rng.offset};
  show("offset", off);

  bool threw = false;
  try {
    laser::randomTensor<float>({4}, 1.0f, 0.0f, rng);
  } catch (const laser::Error &) {
    threw = true;
  }
  expect("an empty range is refused and uses no words", threw && rng.offset == 55);

  if (fails == 0) std::printf("SUCCESS\n");
  return fails ? 1 : 0;
}
