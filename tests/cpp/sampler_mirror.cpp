// tests/cpp/sampler_mirror.cpp -- laser::Sampler from a compiled C++ caller (include/laser.hpp): the tree of the reference's
// demo row against the sums written out by hand, draws at u = 0 and at the largest u below 1, draw-and-remove until the rows
// are empty, update against a rebuild, a vector as one row, and the refusals.  Prints SUCCESS.
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
static bool same(const std::vector<float> &a, const std::vector<float> &b) {
  return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0;
}

int main() {
  const int64_t R = 2, N = 5;
  const float w[R * N] = {0.3f, 1.5f, 0.4f, 0.3f, 0.3f, 0.0f, 2.0f, 0.0f, 0.0f, 0.0f};
  auto tw = laser::newTensor<float>({R, N});
  laser::copyFromRaw(tw, w, R * N);
  laser::Sampler s(tw);
  expect("two rows of five weights: images of 16 elements", s.rows == 2 && s.n == 5 && s.tree.shape[1] == 16);

  // row 0 by hand: leaves at 8 .. 15, then pairs
  std::vector<float> want(32, 0.0f);
  for (int64_t r = 0; r < R; r++) {
    float *t = want.data() + r * 16;
    for (int64_t i = 0; i < N; i++) t[8 + i] = w[r * N + i];
    for (int j = 7; j >= 1; j--) {
      volatile float sum = t[2 * j] + t[2 * j + 1];
      t[j] = sum;
    }
  }
  expect("the tree images", same(s.tree.to_host(), want));

  const float top = 1.0f - 1.0f / 16777216.0f;
  const float u[R * 3] = {0.0f, top, 0.5f, 0.0f, top, 0.5f};
  auto tu = laser::newTensor<float>({R, 3});
  laser::copyFromRaw(tu, u, R * 3);
  const std::vector<int32_t> idx = s.sample(tu).to_host();
  expect("u = 0 draws the first positive element, the largest u the last", idx[0] == 0 && idx[1] == 4 && idx[3] == 1 && idx[4] == 1 && idx[5] == 1);
  expect("u = 0.5 of 2.8 lands in element 1", idx[2] == 1);
  expect("sample leaves the tree alone", same(s.tree.to_host(), want));

  auto one = laser::newTensor<float>({N});  // a vector: one row
  laser::copyFromRaw(one, w, N);
  laser::Sampler s1(one);
  expect("a vector is one row", s1.rows == 1 && same(s1.tree.to_host(), std::vector<float>(want.begin(), want.begin() + 16)));

  // update row 0's element 1 to 0 and row 1's element 4 to 1; against a rebuild
  const int32_t elem[R] = {1, 4};
  const float nw[R] = {0.0f, 1.0f};
  auto te = laser::newTensor<int32_t>({R});
  auto tn = laser::newTensor<float>({R});
  laser::copyFromRaw(te, elem, R);
  laser::copyFromRaw(tn, nw, R);
  s.update(te, tn);
  float w2[R * N];
  std::memcpy(w2, w, sizeof(w));
  w2[1] = 0.0f;
  w2[N + 4] = 1.0f;
  auto tw2 = laser::newTensor<float>({R, N});
  laser::copyFromRaw(tw2, w2, R * N);
  laser::Sampler rebuilt(tw2);
  expect("update = rebuild, bit for bit", same(s.tree.to_host(), rebuilt.tree.to_host()));

  // draw and remove 7 times: row 0 has 4 positive elements left, row 1 has 2
  std::vector<float> u7(R * 7);
  for (size_t i = 0; i < u7.size(); i++) u7[i] = (float)((i * 37) % 100) / 100.0f;
  auto tu7 = laser::newTensor<float>({R, 7});
  laser::copyFromRaw(tu7, u7.data(), R * 7);
  const std::vector<int32_t> rem = s.sampleAndRemove(tu7).to_host();
  bool ok = true;
  for (int64_t r = 0; r < R; r++) {
    const int live = r == 0 ? 4 : 2;
    int seen = 0;
    for (int k = 0; k < 7; k++) {
      const int32_t i = rem[r * 7 + k];
      if (k < live) {
        ok = ok && i >= 0 && i < N && w2[r * N + i] > 0.0f && !(seen >> i & 1);
        if (i >= 0) seen |= 1 << i;
      } else {
        ok = ok && i == -1;
      }
    }
  }
  expect("every positive element once, then -1", ok);
  std::vector<float> empty = s.tree.to_host();
  bool zero = true;
  for (float v : empty) zero = zero && v == 0.0f;
  expect("the emptied trees are all zero", zero);

  bool threw = false;
  try {
    auto bad = laser::newTensor<float>({R + 1, 3});
    s.sample(bad);
  } catch (const laser::Error &) {
    threw = true;
  }
  expect("uniform numbers of another row count are refused", threw);
  threw = false;
  try {
    auto wt = tw.transposed();  // (N, R) with strides (1, N): the elements of a row are not contiguous
    laser::Sampler bad(wt);
  } catch (const laser::Error &) {
    threw = true;
  }
  expect("weights whose rows are not contiguous are refused", threw);

  if (fails == 0) std::printf("SUCCESS\n");
  return fails ? 1 : 0;
}
