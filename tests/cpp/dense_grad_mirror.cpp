// tests/cpp/dense_grad_mirror.cpp -- laser::bias_grad and laser::linear_backward from a compiled C++ caller
// (include/laser.hpp).  dz against the stated float32 operation order (built with -ffp-contract=off), db against the sum
// tree of include/laser_hip.h "Dense-layer backward" written out here in terms of the row index, over one and over three
// chunks of rows; dz in place over dy; only db; linear_backward's db and dz-dependent products against float64 sums within
// (K + 2) * 2^-23 * |A| * |B|; a refused shape.  Prints SUCCESS.
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
static bool same(float a, float b) { return (a != a && b != b) || std::memcmp(&a, &b, sizeof(float)) == 0; }

static float grad_of(laser::Activation act, float dy, float y) {
  if (act == laser::Activation::none) return dy;
  if (act == laser::Activation::relu) return y > 0.0f ? dy : 0.0f;
  if (act == laser::Activation::tanh) {
    const float t = y * y;
    const float u = 1.0f - t;
    return dy * u;
  }
  const float u = 1.0f - y;
  const float v = y * u;
  return dy * v;
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
      if (!(a >> b & 1)) leaf[a] = leaf[a] + leaf[a | 1 << b];  // (an index with an earlier bit set is never read again)
  return leaf[0];
}

int main() {
  const laser::Activation acts[] = {laser::Activation::none, laser::Activation::relu, laser::Activation::tanh, laser::Activation::sigmoid};
  for (const int64_t rows : {int64_t(777), int64_t(16389)}) {
    const int64_t n = 21;
    std::vector<float> dy((size_t)(rows * n)), y((size_t)(rows * n));
    for (int64_t i = 0; i < rows * n; i++) {
      dy[i] = (float)((i * 104729) % 2003 - 1001) / 97.0f;
      y[i] = (float)((i * 7919) % 4001 - 2000) / 2000.0f;
    }
    y[5] = 0.0f, y[6] = -0.0f, y[7] = 1.0f, y[8] = -1.0f;
    auto tdy = laser::newTensor<float>({rows, n}), ty = laser::newTensor<float>({rows, n});
    laser::copyFromRaw(tdy, dy.data(), rows * n);
    laser::copyFromRaw(ty, y.data(), rows * n);
    for (const laser::Activation act : acts) {
      auto db = laser::newTensor<float>({n}), dz = laser::newTensor<float>({rows, n});
      laser::bias_grad(db, &dz, tdy, act == laser::Activation::none ? nullptr : &ty, act);
      const std::vector<float> hz = dz.to_host(), hb = db.to_host();
      bool okz = true, okb = true;
      for (int64_t i = 0; i < rows * n; i++) okz = okz && same(hz[i], grad_of(act, dy[i], y[i]));
      for (int64_t j = 0; j < n; j++) {
        std::vector<float> col((size_t)rows);
        for (int64_t r = 0; r < rows; r++) col[r] = hz[r * n + j];
        okb = okb && same(hb[j], tree_sum(col));
      }
      expect("dz is the stated operation order, bit for bit", okz);
      expect("db is the stated sum tree of each column, bit for bit", okb);
      auto db2 = laser::newTensor<float>({n});
      laser::bias_grad(db2, nullptr, tdy, &ty, act);
      expect("db alone is the same", db2.to_host() == hb || std::memcmp(db2.to_host().data(), hb.data(), n * sizeof(float)) == 0);
      auto in = laser::newTensor<float>({rows, n});
      laser::copyFromRaw(in, dy.data(), rows * n);
      laser::bias_grad(db2, &in, in, &ty, act);
      expect("dz in place over dy is the same", std::memcmp(in.to_host().data(), hz.data(), hz.size() * sizeof(float)) == 0 &&
                                                     std::memcmp(db2.to_host().data(), hb.data(), n * sizeof(float)) == 0);
    }
  }

  {  // linear_backward: Y = tanh(X W + b), X (M, K), W (K, N)
    const int64_t M = 50, K = 12, N = 9;
    std::vector<float> x((size_t)(M * K)), w((size_t)(K * N)), dy((size_t)(M * N)), y((size_t)(M * N));
    for (size_t i = 0; i < x.size(); i++) x[i] = (float)((i * 31) % 17) / 8.0f - 1.0f;
    for (size_t i = 0; i < w.size(); i++) w[i] = (float)((i * 13) % 11) / 5.0f - 1.0f;
    for (size_t i = 0; i < dy.size(); i++) dy[i] = (float)((i * 7) % 23) / 11.0f - 1.0f, y[i] = (float)((i * 5) % 19) / 10.0f - 0.9f;
    auto tx = laser::newTensor<float>({M, K}), tw = laser::newTensor<float>({K, N}), tdy = laser::newTensor<float>({M, N}),
         ty = laser::newTensor<float>({M, N});
    laser::copyFromRaw(tx, x.data(), M * K);
    laser::copyFromRaw(tw, w.data(), K * N);
    laser::copyFromRaw(tdy, dy.data(), M * N);
    laser::copyFromRaw(ty, y.data(), M * N);
    const laser::LinearGrads g = laser::linear_backward(tx, tw, tdy, &ty, laser::Activation::tanh);
    const std::vector<float> dx = g.dx.to_host(), dw = g.dw.to_host(), db = g.db.to_host();
    std::vector<float> dz((size_t)(M * N));
    for (size_t i = 0; i < dz.size(); i++) dz[i] = grad_of(laser::Activation::tanh, dy[i], y[i]);
    bool okb = true, okw = true, okx = true;
    const double eps = std::ldexp(1.0, -23);
    for (int64_t j = 0; j < N; j++) {
      std::vector<float> col((size_t)M);
      for (int64_t r = 0; r < M; r++) col[r] = dz[r * N + j];
      okb = okb && same(db[j], tree_sum(col));
    }
    for (int64_t k = 0; k < K; k++)
      for (int64_t j = 0; j < N; j++) {
        double s = 0, a = 0;
        for (int64_t r = 0; r < M; r++) s += (double)x[r * K + k] * dz[r * N + j], a += std::fabs((double)x[r * K + k] * dz[r * N + j]);
        okw = okw && std::fabs(dw[k * N + j] - s) <= (M + 2) * eps * a;
      }
    for (int64_t r = 0; r < M; r++)
      for (int64_t k = 0; k < K; k++) {
        double s = 0, a = 0;
        for (int64_t j = 0; j < N; j++) s += (double)dz[r * N + j] * w[k * N + j], a += std::fabs((double)dz[r * N + j] * w[k * N + j]);
        okx = okx && std::fabs(dx[r * K + k] - s) <= (N + 2) * eps * a;
      }
    expect("linear_backward: db is the sum tree of dz's columns", okb);
    expect("linear_backward: dw = x^T dz within (M + 2) 2^-23 |x|^T |dz|", okw);
    expect("linear_backward: dx = dz w^T within (N + 2) 2^-23 |dz| |w|^T", okx);
    const laser::LinearGrads g1 = laser::linear_backward(tx, tw, tdy, &ty, laser::Activation::tanh, false);
    expect("need_dx = false leaves dx empty", g1.dx.storage == nullptr && g1.dw.to_host() == dw);
  }

  bool threw = false;
  try {
    auto db = laser::newTensor<float>({3});
    auto d = laser::newTensor<float>({4, 3});
    laser::bias_grad(db, nullptr, d, nullptr, laser::Activation::relu);  // an activation without y
  } catch (const laser::Error &) {
    threw = true;
  }
  expect("an activation without y is refused", threw);

  if (fails == 0) std::printf("SUCCESS\n");
  return fails ? 1 : 0;
}
