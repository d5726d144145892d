// tests/cpp/layer_norm_mirror.cpp -- laser::layer_norm and laser::layer_norm_backward from a compiled C++ caller
// (include/laser.hpp), bit for bit against the contract of include/laser_hip.h "Layer normalization" written out here in
// plain float32 C++ (built with -ffp-contract=off; the host's division and sqrtf are correctly rounded) with the sum tree of
// "Reductions" in terms of the index: one shape for each of the three lane mappings, 16389 rows for the column sums' second
// level; y in place over x; inference without statistics; a refused eps.  Prints SUCCESS.
#include <cmath>
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
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); i++)
    if (!((a[i] != a[i] && b[i] != b[i]) || std::memcmp(&a[i], &b[i], sizeof(float)) == 0)) return false;
  return true;
}

// the order of "Reductions" for a 1-D array of float32, in terms of the index: chunks of 8192, element k of a chunk to leaf
// k mod 1024 in ascending k, the leaves folded over bits 1, 0, 9, 8, .., 2 (higher index into lower), the chunk partials
// the same way as one more array
static float tree_sum(const std::vector<float> &x) {
  if (x.size() > 8192) {
    std::vector<float> parts;
    for (size_t at = 0; at < x.size(); at += 8192)
      parts.push_back(tree_sum(std::vector<float>(x.begin() + at, x.begin() + std::min(x.size(), at + 8192))));
    return tree_sum(parts);
  }
  float leaf[1024];
  for (int a = 0; a < 1024; a++) leaf[a] = 0.0f;
  for (size_t k = 0; k < x.size(); k++) leaf[k % 1024] = leaf[k % 1024] + x[k];
  const int bits[10] = {1, 0, 9, 8, 7, 6, 5, 4, 3, 2};
  for (int b : bits)
    for (int a = 0; a < 1024; a++)
      if (!(a >> b & 1)) leaf[a] = leaf[a] + leaf[a | 1 << b];
  return leaf[0];
}

static void check_shape(const int64_t rows, const int64_t n) {
  const float eps = 1e-5f, nf = (float)n;
  std::vector<float> x((size_t)(rows * n)), dy((size_t)(rows * n)), gamma((size_t)n), beta((size_t)n);
  for (int64_t i = 0; i < rows * n; i++) {
    x[i] = 3.0f + (float)((i * 104729) % 2003 - 1001) / 500.0f;
    dy[i] = (float)((i * 7919) % 4001 - 2000) / 1000.0f;
  }
  for (int64_t j = 0; j < n; j++) gamma[j] = 1.0f + (float)((j * 31) % 17 - 8) / 16.0f, beta[j] = (float)((j * 13) % 11 - 5) / 4.0f;
  std::vector<float> y(x.size()), xhat(x.size()), dx(x.size()), mean((size_t)rows), rstd((size_t)rows), t(x.size());
  for (int64_t r = 0; r < rows; r++) {
    std::vector<float> row(x.begin() + r * n, x.begin() + (r + 1) * n), sq((size_t)n), g((size_t)n), gx((size_t)n);
    mean[r] = tree_sum(row) / nf;
    for (int64_t j = 0; j < n; j++) {
      const float d = row[j] - mean[r];
      sq[j] = d * d;
    }
    const float var = tree_sum(sq) / nf;
    rstd[r] = 1.0f / std::sqrt(var + eps);
    for (int64_t j = 0; j < n; j++) {
      const float d = row[j] - mean[r];
      const float h = d * rstd[r];
      const float s = h * gamma[j];
      xhat[r * n + j] = h;
      y[r * n + j] = s + beta[j];
      g[j] = dy[r * n + j] * gamma[j];
      gx[j] = g[j] * h;
      t[r * n + j] = dy[r * n + j] * h;
    }
    const float a = tree_sum(g) / nf, b = tree_sum(gx) / nf;
    for (int64_t j = 0; j < n; j++) {
      const float u = g[j] - a;
      const float v = xhat[r * n + j] * b;
      const float w = u - v;
      dx[r * n + j] = w * rstd[r];
    }
  }
  std::vector<float> dgamma((size_t)n), dbeta((size_t)n);
  for (int64_t j = 0; j < n; j++) {
    std::vector<float> c0((size_t)rows), c1((size_t)rows);
    for (int64_t r = 0; r < rows; r++) c0[r] = t[r * n + j], c1[r] = dy[r * n + j];
    dgamma[j] = tree_sum(c0);
    dbeta[j] = tree_sum(c1);
  }
  auto tx = laser::newTensor<float>({rows, n}), tdy = laser::newTensor<float>({rows, n}), tg = laser::newTensor<float>({n}),
       tb = laser::newTensor<float>({n});
  laser::copyFromRaw(tx, x.data(), rows * n);
  laser::copyFromRaw(tdy, dy.data(), rows * n);
  laser::copyFromRaw(tg, gamma.data(), n);
  laser::copyFromRaw(tb, beta.data(), n);
  const laser::LayerNormResult f = laser::layer_norm(tx, &tg, &tb, eps);
  expect("y is the stated operation order, bit for bit", same(f.y.to_host(), y));
  expect("mean and rstd are the stated ones", same(f.mean.to_host(), mean) && same(f.rstd.to_host(), rstd));
  const laser::LayerNormGrads g = laser::layer_norm_backward(tdy, tx, f.mean, f.rstd, &tg);
  expect("dx is the stated operation order, bit for bit", same(g.dx.to_host(), dx));
  expect("dgamma and dbeta are the stated sum trees of their columns", same(g.dgamma.to_host(), dgamma) && same(g.dbeta.to_host(), dbeta));
  const laser::LayerNormGrads g1 = laser::layer_norm_backward(tdy, tx, f.mean, f.rstd, &tg, true, false);
  expect("dx alone is the same and the parameter gradients stay empty", same(g1.dx.to_host(), dx) && g1.dgamma.storage == nullptr);
  const laser::LayerNormResult f1 = laser::layer_norm(tx, &tg, &tb, eps, false);
  expect("inference: the same y, no statistics", same(f1.y.to_host(), y) && f1.mean.storage == nullptr);
  laser::layer_norm(tx, nullptr, nullptr, tx, &tg, &tb, eps);
  expect("y in place over x is the same", same(tx.to_host(), y));
}

int main() {
  check_shape(9, 37);
  check_shape(5, 1025);
  check_shape(2, 8193);
  check_shape(16389, 5);
  bool threw = false;
  try {
    auto x = laser::newTensor<float>({4, 3});
    laser::layer_norm(x, nullptr, nullptr, -1.0f);
  } catch (const laser::Error &) {
    threw = true;
  }
  expect("a negative eps is refused", threw);
  if (fails == 0) std::printf("SUCCESS\n");
  return fails ? 1 : 0;
}
