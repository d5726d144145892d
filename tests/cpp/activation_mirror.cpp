// tests/cpp/activation_mirror.cpp -- laser::tanh, laser::sigmoid, laser::activation and laser::activation_grad from a compiled
// C++ caller (include/laser.hpp).  The device's ltanh and lsigmoid against act_core.h compiled into this program (the same
// bits), relu and the three gradients against the stated float32 operation order (built with -ffp-contract=off), a broadcast
// row, in place, and a refused activation code.  Prints SUCCESS.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "act_core.h"
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

int main() {
  const int64_t L = 4099;
  std::vector<float> x(L), dy(L);
  for (int64_t i = 0; i < L; i++) {
    x[i] = std::ldexp(1.0f + (float)((i * 7919) % 4001) / 4001.0f, (int)(i % 40) - 30) * (i % 3 ? 1.0f : -1.0f);
    dy[i] = (float)((i * 104729) % 2003 - 1001) / 97.0f;
  }
  const float edge[] = {0.0f, -0.0f, 1.0f, -1.0f, INFINITY, -INFINITY, NAN, 1e-45f, -1e-45f, 0.015625f, 9.010914f, 17.32868f, -103.972084f, -87.3365f, -104.0f};
  for (size_t i = 0; i < sizeof(edge) / sizeof(edge[0]); i++) x[i] = edge[i];
  dy[20] = NAN, dy[21] = INFINITY;
  auto tx = laser::newTensor<float>({L});
  laser::copyFromRaw(tx, x.data(), L);
  auto tdy = laser::newTensor<float>({L});
  laser::copyFromRaw(tdy, dy.data(), L);

  const std::vector<float> th = laser::tanh(tx).to_host(), sg = laser::sigmoid(tx).to_host();
  const std::vector<float> re = laser::activation(tx, laser::Activation::relu).to_host();
  bool ok_t = true, ok_s = true, ok_r = true;
  for (int64_t i = 0; i < L; i++) {
    ok_t = ok_t && same(th[i], lh_act_tanh(x[i]));
    ok_s = ok_s && same(sg[i], lh_act_sigmoid(x[i]));
    ok_r = ok_r && same(re[i], x[i] > 0.0f ? x[i] : 0.0f);
  }
  expect("laser::tanh = act_core.h on the host, bit for bit", ok_t);
  expect("laser::sigmoid = act_core.h on the host, bit for bit", ok_s);
  expect("relu is x > 0 ? x : +0 (NaN and -0 give +0)", ok_r && same(re[1], 0.0f) && same(re[6], 0.0f));
  expect("tanh(-0) = -0, tanh(+-Inf) = +-1, sigmoid(+-0) = 0.5, sigmoid(-104) = 0",
         same(th[1], -0.0f) && same(th[4], 1.0f) && same(th[5], -1.0f) && same(sg[0], 0.5f) && same(sg[1], 0.5f) && same(sg[14], 0.0f));

  const laser::Activation acts[] = {laser::Activation::relu, laser::Activation::tanh, laser::Activation::sigmoid};
  const std::vector<float> *ys[] = {&re, &th, &sg};
  for (int k = 0; k < 3; k++) {
    auto ty = laser::newTensor<float>({L});
    laser::copyFromRaw(ty, ys[k]->data(), L);
    const std::vector<float> g = laser::activation_grad(tdy, ty, acts[k]).to_host();
    bool ok = true;
    for (int64_t i = 0; i < L; i++) ok = ok && same(g[i], grad_of(acts[k], dy[i], (*ys[k])[i]));
    expect("activation_grad is the stated operation order, bit for bit", ok);
    laser::activation_grad(ty, tdy, ty, acts[k]);  // dx over y
    const std::vector<float> in = ty.to_host();
    expect("activation_grad with dx = y is the same", std::memcmp(in.data(), g.data(), g.size() * sizeof(float)) == 0);
  }

  auto wide = laser::newTensor<float>({3, L});
  laser::tanh(wide, tx);
  const std::vector<float> w = wide.to_host();
  bool ok = true;
  for (int64_t i = 0; i < 3 * L; i++) ok = ok && same(w[i], th[i % L]);
  expect("tanh broadcasts a row", ok);
  laser::sigmoid(tx, tx);
  const std::vector<float> in = tx.to_host();
  expect("sigmoid in place = out of place", std::memcmp(in.data(), sg.data(), sg.size() * sizeof(float)) == 0);

  bool threw = false;
  try {
    laser::activation(tx, laser::Activation::none);
  } catch (const laser::Error &) {
    threw = true;
  }
  expect("Activation::none is refused", threw);

  if (fails == 0) std::printf("SUCCESS\n");
  return fails ? 1 : 0;
}
