// tests/cpp/softmax_axis_mirror.cpp -- laser::softmax_axis from a compiled C++ caller (include/laser.hpp): along axis 0 of a
// matrix against laser::softmax over the rows of the transposed matrix (the same bits), along the middle axis of a rank-3
// tensor against the same columns gathered into rows, a negative axis, in place, and the refusals.  Prints SUCCESS.
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
  const int64_t O = 3, N = 1300, I = 37;  // past the resident bound, a ragged last strip
  std::vector<float> x(O * N * I), xt(O * I * N);
  for (int64_t i = 0; i < O * N * I; i++) x[i] = (float)((i * 7919) % 4001 - 2000) / 100.0f;
  for (int64_t o = 0; o < O; o++)
    for (int64_t k = 0; k < N; k++)
      for (int64_t i = 0; i < I; i++) xt[(o * I + i) * N + k] = x[(o * N + k) * I + i];
  auto tx = laser::newTensor<float>({O, N, I});
  laser::copyFromRaw(tx, x.data(), O * N * I);
  auto tr = laser::newTensor<float>({O * I, N});
  laser::copyFromRaw(tr, xt.data(), O * I * N);

  const std::vector<float> rows = laser::softmax(tr).to_host();
  const std::vector<float> cols = laser::softmax_axis(tx, 1).to_host();
  bool same = true;
  for (int64_t o = 0; o < O && same; o++)
    for (int64_t k = 0; k < N && same; k++)
      for (int64_t i = 0; i < I; i++)
        if (std::memcmp(&cols[(o * N + k) * I + i], &rows[(o * I + i) * N + k], sizeof(float)) != 0) same = false;
  expect("softmax_axis(axis = 1) = softmax over the gathered rows, bit for bit", same);
  const std::vector<float> neg = laser::softmax_axis(tx, -2).to_host();
  expect("axis -2 = axis 1", std::memcmp(neg.data(), cols.data(), cols.size() * sizeof(float)) == 0);

  auto m = laser::newTensor<float>({N, I});
  laser::copyFromRaw(m, x.data(), N * I);
  const std::vector<float> c0 = laser::softmax_axis(m, 0).to_host();
  expect("axis 0 of a matrix = the first outer index of the rank-3 case", std::memcmp(c0.data(), cols.data(), c0.size() * sizeof(float)) == 0);
  const std::vector<float> last = laser::softmax_axis(tr, 1).to_host();
  expect("the last axis = softmax over the rows", std::memcmp(last.data(), rows.data(), rows.size() * sizeof(float)) == 0);

  laser::softmax_axis(tx, tx, 1);
  const std::vector<float> in = tx.to_host();
  expect("in place = out of place", std::memcmp(in.data(), cols.data(), cols.size() * sizeof(float)) == 0);
  double sum = 0;
  for (int64_t k = 0; k < N; k++) sum += cols[k * I + 5];
  expect("a column sums to 1", sum > 0.9999 && sum < 1.0001);

  bool threw = false;
  try {
    laser::softmax_axis(m, 2);
  } catch (const laser::Error &) {
    threw = true;
  }
  expect("an axis outside the rank is refused", threw);
  threw = false;
  try {
    auto mt = m.transposed();  // (I, N) view with strides (1, I): axis 0 leaves no unit-stride run behind it
    auto dst = laser::newTensor<float>({I, N});
    laser::softmax_axis(dst, mt, 0);
  } catch (const laser::Error &) {
    threw = true;
  }
  expect("a view that does not collapse is refused", threw);

  if (fails == 0) std::printf("SUCCESS\n");
  return fails ? 1 : 0;
}
