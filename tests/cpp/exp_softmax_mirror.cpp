// tests/cpp/exp_softmax_mirror.cpp -- laser::exp and laser::softmax from a compiled C++ caller (include/laser.hpp): exp of
// values whose result is known exactly, exp of a transposed view against the contiguous one, softmax of all-equal rows
// (exactly 1 / n for a power of two n), and softmax in place against softmax into a fresh tensor.  Prints SUCCESS.
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
  const int64_t R = 37, N = 1024;
  std::vector<float> x(R * N);
  for (int64_t i = 0; i < R * N; i++) x[i] = (float)((i * 7919) % 4001 - 2000) / 100.0f;
  auto tx = laser::newTensor<float>({R, N});
  laser::copyFromRaw(tx, x.data(), R * N);

  auto te = laser::exp(tx);
  auto tt = laser::newTensor<float>({N, R});
  auto ttv = tt.transposed();  // an R x N view of N x R storage
  laser::exp(ttv, tx);
  auto back = laser::newTensor<float>({R, N});
  laser::copyFrom(back, ttv);
  const std::vector<float> e = te.to_host(), eb = back.to_host();
  expect("exp: strided destination = contiguous", std::memcmp(e.data(), eb.data(), e.size() * sizeof(float)) == 0);
  auto zero = laser::newTensor<float>({4});
  const std::vector<float> one = laser::exp(zero).to_host();
  expect("exp(0) = 1", one[0] == 1.0f && one[3] == 1.0f);

  auto flat = laser::newTensor<float>({3, N});  // zeros: every row all-equal
  const std::vector<float> u = laser::softmax(flat).to_host();
  bool ok = true;
  for (float v : u) ok = ok && v == 1.0f / (float)N;
  expect("softmax of equal rows = 1 / n", ok);

  const std::vector<float> s = laser::softmax(tx).to_host();
  laser::softmax(tx, tx);
  const std::vector<float> sin = tx.to_host();
  expect("softmax in place = out of place", std::memcmp(s.data(), sin.data(), s.size() * sizeof(float)) == 0);
  double sum = 0;
  for (int64_t j = 0; j < N; j++) sum += s[j];
  expect("softmax row sums to 1", sum > 0.9999 && sum < 1.0001);

  if (fails == 0) std::printf("SUCCESS\n");
  return fails ? 1 : 0;
}
