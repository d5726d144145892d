// tests/cpp/foreach_mirror.cpp -- laser::forEach from a compiled C++ caller (include/laser.hpp): Laser's own example
// `x += y * z` in place on float Tensors, a mixed-type body (double out of float and int32 inputs) with a parameter, and
// a transposed read.  Every result is checked element for element against a host loop; prints SUCCESS.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "laser.hpp"

static int fails = 0;
template <typename T>
static void expect_eq(const char *what, const std::vector<T> &got, const std::vector<T> &want) {
  for (size_t i = 0; i < want.size(); i++)
    if (std::memcmp(&got[i], &want[i], sizeof(T)) != 0) {
      std::printf("FAIL %s at %zu: %.17g vs %.17g\n", what, i, (double)got[i], (double)want[i]);
      fails++;
      return;
    }
}

int main() {
  const int64_t R = 37, Cn = 53, n = R * Cn;
  std::vector<float> x(n), y(n), z(n);
  std::vector<int32_t> k(n);
  for (int64_t i = 0; i < n; i++) {
    x[i] = 0.25f * (float)(i % 17) - 1.5f;
    y[i] = 1.0f / (float)(i + 3);
    z[i] = (float)(i % 29) - 7.0f;
    k[i] = (int32_t)(i * 2654435761u);
  }
  auto tx = laser::newTensor<float>({R, Cn}), ty = laser::newTensor<float>({R, Cn}), tz = laser::newTensor<float>({R, Cn});
  auto tk = laser::newTensor<int32_t>({R, Cn});
  auto tw = laser::newTensor<double>({R, Cn});
  laser::copyFromRaw(tx, x.data(), n);
  laser::copyFromRaw(ty, y.data(), n);
  laser::copyFromRaw(tz, z.data(), n);
  laser::copyFromRaw(tk, k.data(), n);

  laser::forEach("x += y * z", {laser::out("x", tx), laser::in("y", ty), laser::in("z", tz)});
  std::vector<float> want(n);
  for (int64_t i = 0; i < n; i++) {
    volatile float p = y[i] * z[i];
    want[i] = x[i] + p;
  }
  expect_eq("x += y * z", tx.to_host(), want);

  laser::forEach("w = (double)y * alpha + k", {laser::out("w", tw), laser::in("y", ty), laser::in("k", tk)}, {laser::param("alpha", 0.5)});
  std::vector<double> wd(n);
  for (int64_t i = 0; i < n; i++) {
    volatile double p = (double)y[i] * 0.5;
    wd[i] = p + (double)k[i];
  }
  expect_eq("mixed types", tw.to_host(), wd);

  // out[i][j] = in[j][i] through a transposed view (the strided kernel)
  auto tt = laser::newTensor<float>({Cn, R});
  laser::forEach("t = y", {laser::out("t", tt), laser::in("y", ty.transposed())});
  std::vector<float> wt(n);
  for (int64_t i = 0; i < Cn; i++)
    for (int64_t j = 0; j < R; j++) wt[i * R + j] = y[j * Cn + i];
  expect_eq("transposed read", tt.to_host(), wt);

  if (fails == 0) std::printf("SUCCESS\n");
  return fails ? 1 : 0;
}
