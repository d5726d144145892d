// tests/cpp/log_softmax_mirror.cpp -- laser::log, laser::logsumexp, laser::log_softmax and laser::softmax_cross_entropy from a
// compiled C++ caller (include/laser.hpp).  The device's llog against log_core.h compiled into this program (the same bits),
// the row results against each other by the identities of include/laser_hip.h: log_softmax stays finite where the
// softmax goes subnormal, loss = 0 - log_softmax[label], the gradient off the label has the softmax's bits, label -1 and labels
// outside the row.  Prints SUCCESS.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "laser.hpp"
#include "log_core.h"

static int fails = 0;
static void expect(const char *what, bool ok) {
  if (!ok) {
    std::printf("FAIL %s\n", what);
    fails++;
  }
}
static bool same(float a, float b) { return (a != a && b != b) || std::memcmp(&a, &b, sizeof(float)) == 0; }

int main() {
  // log: positive values over many binades, the edges, and a broadcast row
  const int64_t L = 4099;
  std::vector<float> x(L);
  for (int64_t i = 0; i < L; i++) x[i] = std::ldexp(1.0f + (float)((i * 7919) % 4001) / 4001.0f, (int)(i % 250) - 140);
  x[0] = 0.0f, x[1] = -0.0f, x[2] = 1.0f, x[3] = -1.0f, x[4] = INFINITY, x[5] = -INFINITY, x[6] = NAN, x[7] = 1e-45f, x[8] = 1e-39f;
  auto tx = laser::newTensor<float>({L});
  laser::copyFromRaw(tx, x.data(), L);
  const std::vector<float> lg = laser::log(tx).to_host();
  bool ok = true;
  for (int64_t i = 0; i < L; i++) ok = ok && same(lg[i], lh_log(x[i]));
  expect("laser::log = log_core.h on the host, bit for bit", ok);
  expect("log(1) = +0, log(+-0) = -Inf, log(-1) = NaN", same(lg[2], 0.0f) && lg[0] == -INFINITY && lg[1] == -INFINITY && lg[3] != lg[3]);
  auto wide = laser::newTensor<float>({3, L});
  laser::log(wide, tx);
  const std::vector<float> w = wide.to_host();
  ok = true;
  for (int64_t i = 0; i < 3 * L; i++) ok = ok && same(w[i], lg[i % L]);
  expect("log broadcasts a row", ok);

  // rows: one length per kernel, values that push the softmax into the subnormals
  for (const int64_t N : {5, 1300, 9000}) {
    const int64_t R = 6;
    std::vector<float> v(R * N);
    for (int64_t i = 0; i < R * N; i++) v[i] = (float)((i * 7919) % 4001 - 2000) / 12.0f;  // +-166
    std::vector<int32_t> lab = {0, (int32_t)(N - 1), 3, -1, -2, (int32_t)N};
    auto t = laser::newTensor<float>({R, N});
    laser::copyFromRaw(t, v.data(), R * N);
    auto tl = laser::newTensor<int32_t>({R});
    laser::copyFromRaw(tl, lab.data(), R);
    const std::vector<float> sm = laser::softmax(t).to_host();
    const std::vector<float> lsm = laser::log_softmax(t).to_host();
    const std::vector<float> lse = laser::logsumexp(t).to_host();
    laser::Tensor<float> tg;
    const std::vector<float> loss = laser::softmax_cross_entropy(t, tl, &tg).to_host();
    const std::vector<float> only = laser::softmax_cross_entropy(t, tl).to_host();
    const std::vector<float> g = tg.to_host();
    bool neg = true, finite = true, under = false, grad_ok = true, loss_ok = true, lse_ok = true;
    for (int64_t r = 0; r < R; r++) {
      for (int64_t j = 0; j < N; j++) {
        const float y = lsm[r * N + j];
        neg = neg && y <= 0.0f;
        finite = finite && std::isfinite(y);
        under = under || sm[r * N + j] < 1.17549435e-38f;  // lexp clamps at -88: the softmax is subnormal there
        if (lab[r] >= 0 && lab[r] < N && j != lab[r]) grad_ok = grad_ok && same(g[r * N + j], sm[r * N + j]);
        if (lab[r] == -1) grad_ok = grad_ok && same(g[r * N + j], 0.0f);
        if (lab[r] < -1 || lab[r] >= N) grad_ok = grad_ok && g[r * N + j] != g[r * N + j];
      }
      if (lab[r] >= 0 && lab[r] < N) {
        loss_ok = loss_ok && same(loss[r], 0.0f - lsm[r * N + lab[r]]);
        grad_ok = grad_ok && same(g[r * N + lab[r]], sm[r * N + lab[r]] - 1.0f);
      } else {
        loss_ok = loss_ok && (lab[r] == -1 ? same(loss[r], 0.0f) : loss[r] != loss[r]);
      }
      loss_ok = loss_ok && same(loss[r], only[r]);
      // x - lse is log_softmax to an ulp or two of x (not the same bits: that is why the kernel subtracts twice)
      lse_ok = lse_ok && std::fabs((v[r * N] - lse[r]) - lsm[r * N]) <= 4e-5f * std::fabs(lse[r]) + 1e-5f;
    }
    expect("log_softmax is finite and <= 0 where the softmax has gone subnormal", neg && finite && under);
    expect("loss = 0 - log_softmax[label]; -1 gives +0, other labels outside the row NaN; loss-only form the same", loss_ok);
    expect("grad = softmax - onehot with the softmax's bits; +0 row for -1, NaN row outside", grad_ok);
    expect("logsumexp agrees with log_softmax", lse_ok);
    laser::log_softmax(t, t);
    const std::vector<float> in = t.to_host();
    expect("log_softmax in place = out of place", std::memcmp(in.data(), lsm.data(), lsm.size() * sizeof(float)) == 0);
  }

  bool threw = false;
  try {
    auto m = laser::newTensor<float>({4, 8});
    auto mt = m.transposed();
    laser::log_softmax(mt);
  } catch (const laser::Error &) {
    threw = true;
  }
  expect("rows that are not contiguous are refused", threw);
  threw = false;
  try {
    auto m = laser::newTensor<float>({4, 8});
    auto l3 = laser::newTensor<int32_t>({3});
    laser::softmax_cross_entropy(m, l3);
  } catch (const laser::Error &) {
    threw = true;
  }
  expect("a label count that is not the row count is refused", threw);

  if (fails == 0) std::printf("SUCCESS\n");
  return fails ? 1 : 0;
}
