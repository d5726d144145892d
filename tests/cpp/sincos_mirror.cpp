// tests/cpp/sincos_mirror.cpp -- laser::sin, laser::cos and laser::sincos from a compiled C++ caller (include/laser.hpp).  The
// device's lsin and lcos against sincos_core.h compiled into this program (the same bits; built with -ffp-contract=off), sincos
// against the two, a broadcast row, in place, and a refused pair of destinations.  Prints SUCCESS.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "laser.hpp"
#include "sincos_core.h"

static int fails = 0;
static void expect(const char *what, bool ok) {
  if (!ok) {
    std::printf("FAIL %s\n", what);
    fails++;
  }
}
static bool same(float a, float b) { return (a != a && b != b) || std::memcmp(&a, &b, sizeof(float)) == 0; }

int main() {
  const int64_t L = 4099;
  std::vector<float> x(L);
  for (int64_t i = 0; i < L; i++)  // magnitudes from 2^-40 to 2^100, both signs: both reductions
    x[i] = std::ldexp(1.0f + (float)((i * 7919) % 4001) / 4001.0f, (int)(i % 141) - 40) * (i % 3 ? 1.0f : -1.0f);
  const float edge[] = {0.0f, -0.0f, 1.0f, -1.0f, INFINITY, -INFINITY, NAN, 1e-45f, -1e-45f, 1.5707964f, 3.1415927f, 1048576.0f, 1048575.9f, 3.4028235e38f};
  for (size_t i = 0; i < sizeof(edge) / sizeof(edge[0]); i++) x[i] = edge[i];
  auto tx = laser::newTensor<float>({L});
  laser::copyFromRaw(tx, x.data(), L);

  const std::vector<float> sn = laser::sin(tx).to_host(), cs = laser::cos(tx).to_host();
  bool ok_s = true, ok_c = true;
  for (int64_t i = 0; i < L; i++) {
    ok_s = ok_s && same(sn[i], lh_sin(x[i]));
    ok_c = ok_c && same(cs[i], lh_cos(x[i]));
  }
  expect("laser::sin = sincos_core.h on the host, bit for bit", ok_s);
  expect("laser::cos = sincos_core.h on the host, bit for bit", ok_c);
  expect("sin(+-0) = +-0, cos(+-0) = 1, a subnormal gives itself and 1, Inf gives NaN",
         same(sn[0], 0.0f) && same(sn[1], -0.0f) && same(cs[0], 1.0f) && same(cs[1], 1.0f) && same(sn[7], 1e-45f) && same(cs[8], 1.0f) &&
             sn[4] != sn[4] && cs[5] != cs[5]);

  auto both = laser::sincos(tx);
  const std::vector<float> bs = both.first.to_host(), bc = both.second.to_host();
  expect("sincos = sin and cos", std::memcmp(bs.data(), sn.data(), L * sizeof(float)) == 0 && std::memcmp(bc.data(), cs.data(), L * sizeof(float)) == 0);

  auto wide = laser::newTensor<float>({3, L});
  laser::cos(wide, tx);
  const std::vector<float> w = wide.to_host();
  bool ok = true;
  for (int64_t i = 0; i < 3 * L; i++) ok = ok && same(w[i], cs[i % L]);
  expect("cos broadcasts a row", ok);

  auto tc = laser::newTensor<float>({L});
  laser::sincos(tx, tc, tx);  // the sine over the source
  const std::vector<float> in = tx.to_host(), in2 = tc.to_host();
  expect("sincos with the sine in place = out of place",
         std::memcmp(in.data(), sn.data(), L * sizeof(float)) == 0 && std::memcmp(in2.data(), cs.data(), L * sizeof(float)) == 0);

  bool threw = false;
  try {
    laser::sincos(tc, tc, tx);
  } catch (const laser::Error &) {
    threw = true;
  }
  expect("one buffer for both destinations is refused", threw);

  if (fails == 0) std::printf("SUCCESS\n");
  return fails ? 1 : 0;
}
