// tests/cpp/optim_mirror.cpp -- laser::sgd_step, laser::adam_step, laser::grad_norm and laser::adam_bias_correction from a
// compiled C++ caller (include/laser.hpp), bit for bit against the contract of include/laser_hip.h "Optimizer steps" written
// out here in plain float32 C++ (built with -ffp-contract=off; the host's division and sqrtf are correctly rounded) with the
// sum tree of "Reductions" in terms of the index: a list with an empty tensor, a tail of len % 4 and a tensor past one
// reduction chunk; Nesterov SGD with weight decay, two Adam steps with the clip factor taken from the device; a refused
// momentum.  Prints SUCCESS.
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

// the order of "Reductions" for a 1-D array of float32 (tests/cpp/layer_norm_mirror.cpp has the same function)
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

static float bias_correction(float beta, int64_t step) {
  double r = 1.0, b = (double)beta;
  while (step) {
    if (step & 1) r = r * b;
    b = b * b;
    step >>= 1;
  }
  const double d = 1.0 - r;
  return (float)d;
}

int main() {
  const int64_t sizes[4] = {5, 0, 4099, 8192 + 37};
  std::vector<std::vector<float>> w(4), g(4), m(4), v(4);
  std::vector<laser::Tensor<float>> tw, tg, tm, tv;
  for (int k = 0; k < 4; k++) {
    const int64_t n = sizes[k];
    w[k].resize((size_t)n), g[k].resize((size_t)n), m[k].assign((size_t)n, 0.0f), v[k].assign((size_t)n, 0.0f);
    for (int64_t i = 0; i < n; i++) {
      w[k][i] = (float)((i * 104729 + k) % 2003 - 1001) / 500.0f;
      g[k][i] = (float)((i * 7919 + 3 * k) % 4001 - 2000) / 1000.0f;
    }
    tw.push_back(laser::newTensor<float>({n})), tg.push_back(laser::newTensor<float>({n}));
    tm.push_back(laser::newTensor<float>({n})), tv.push_back(laser::newTensor<float>({n}));
    if (n) laser::copyFromRaw(tw[k], w[k].data(), n), laser::copyFromRaw(tg[k], g[k].data(), n);
  }
  laser::TensorList lw, lg, lm, lv;
  for (int k = 0; k < 4; k++) lw.push_back(&tw[k]), lg.push_back(&tg[k]), lm.push_back(&tm[k]), lv.push_back(&tv[k]);

  // Nesterov SGD with weight decay and a gradient scale
  const float lr = 0.05f, mu = 0.9f, wd = 0.01f, gscale = 0.5f;
  laser::sgd_step(lw, lg, &lm, lr, mu, wd, true, gscale);
  for (int k = 0; k < 4; k++)
    for (size_t i = 0; i < w[k].size(); i++) {
      const float g1 = g[k][i] * gscale;
      const float t0 = wd * w[k][i];
      const float g3 = g1 + t0;
      const float t1 = mu * m[k][i];
      m[k][i] = t1 + g3;
      const float t2 = mu * m[k][i];
      const float d = g3 + t2;
      const float t3 = lr * d;
      w[k][i] = w[k][i] - t3;
    }
  bool ok = true;
  for (int k = 0; k < 4; k++) ok = ok && (sizes[k] == 0 || (same(tw[k].to_host(), w[k]) && same(tm[k].to_host(), m[k])));
  expect("Nesterov SGD with weight decay is the stated operation order, bit for bit", ok);

  // the gradient norm: per-tensor sum trees, the list sum left to right
  float total = 0.0f;
  for (int k = 0; k < 4; k++) {
    std::vector<float> sq(g[k].size());
    for (size_t i = 0; i < sq.size(); i++) sq[i] = g[k][i] * g[k][i];
    total = total + tree_sum(sq);
  }
  const float norm = std::sqrt(total), max_norm = 10.0f, clip = norm > max_norm ? max_norm / norm : 1.0f;
  const laser::GradNorm gn = laser::grad_norm(lg, max_norm);
  expect("the norm and the clip factor are the stated ones", same(gn.norm.to_host(), {norm}) && same(gn.clip.to_host(), {clip}) && clip < 1.0f);

  // two Adam steps (decoupled decay), the clip factor read on the device; m reused from the SGD step as it stands
  const float b1 = 0.9f, b2 = 0.999f, eps = 1e-8f, alr = 1e-2f, omb1 = 1.0f - b1, omb2 = 1.0f - b2, lrwd = alr * wd;
  for (int64_t step = 1; step <= 2; step++) {
    laser::adam_step(lw, lg, lm, lv, step, alr, b1, b2, eps, wd, true, 1.0f, &gn.clip);
    const float bc1 = bias_correction(b1, step), bc2 = bias_correction(b2, step);
    expect("the bias correction is the stated one", laser::adam_bias_correction(b1, step) == bc1 && laser::adam_bias_correction(b2, step) == bc2);
    for (int k = 0; k < 4; k++)
      for (size_t i = 0; i < w[k].size(); i++) {
        const float g1 = g[k][i] * 1.0f;
        const float g3 = g1 * clip;
        const float m0 = b1 * m[k][i];
        const float m1 = omb1 * g3;
        m[k][i] = m0 + m1;
        const float v0 = b2 * v[k][i];
        const float v1 = omb2 * g3;
        const float v2 = v1 * g3;
        v[k][i] = v0 + v2;
        const float mh = m[k][i] / bc1;
        const float vh = v[k][i] / bc2;
        const float den = std::sqrt(vh) + eps;
        const float u = mh / den;
        const float t0 = lrwd * w[k][i];
        const float w1 = w[k][i] - t0;
        const float t1 = alr * u;
        w[k][i] = w1 - t1;
      }
  }
  ok = true;
  for (int k = 0; k < 4; k++)
    ok = ok && (sizes[k] == 0 || (same(tw[k].to_host(), w[k]) && same(tm[k].to_host(), m[k]) && same(tv[k].to_host(), v[k])));
  expect("two Adam steps with decoupled decay and the device's clip factor, bit for bit", ok);

  bool threw = false;
  try {
    laser::sgd_step(lw, lg, nullptr, lr, mu);
  } catch (const laser::Error &) {
    threw = true;
  }
  expect("momentum without its list is refused", threw);
  threw = false;
  try {
    laser::adam_bias_correction(0.9f, 0);
  } catch (const laser::Error &) {
    threw = true;
  }
  expect("step 0 is refused", threw);
  if (fails == 0) std::printf("SUCCESS\n");
  return fails ? 1 : 0;
}
