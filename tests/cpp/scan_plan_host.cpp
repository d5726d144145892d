// tests/cpp/scan_plan_host.cpp -- laser_amd/csrc/scan_plan.h and scan_core.h as a stand-alone host program (no HIP): reads
// lines "rows n elem_size cus" from standard input and prints "rc variant rows_per_workgroup workgroups tiles" for each; with
// no input it checks a sweep of shapes against the header's own rules, the scan order on rows with zeros (monotone, zero
// steps, in place), the search's known answers and the draw at a denormal total, and prints SUCCESS.  Built with the
// sanitizers by tests/test_scan_cpu.py.
#include <cstdio>
#include <cstring>
#include <vector>

#include "scan_plan.h"

static int fails = 0;
static void expect(bool ok, const char *what) {
  if (!ok) {
    std::printf("FAIL %s\n", what);
    fails++;
  }
}

int main(int argc, char **argv) {
  long long rows, n, out4[4];
  int elem, cus;
  if (argc > 1) {  // "-": answer the lines of standard input
    while (std::scanf("%lld %lld %d %d", &rows, &n, &elem, &cus) == 4) {
      out4[0] = out4[1] = out4[2] = out4[3] = -1;
      const int rc = lh_scan_plan(rows, n, elem, cus, out4);
      std::printf("%d %lld %lld %lld %lld\n", rc, out4[0], out4[1], out4[2], out4[3]);
    }
    return 0;
  }
  const long long R = LH_SCAN_RUN;
  const long long rowss[] = {0, 1, 2, 3, 4, 5, 67, 2047, 2048, 2049, 8191, 8192, 8193, 1ll << 31, 1ll << 50, 0x7fffffffffffffffll};
  const long long ns[] = {1, 2, R - 1, R, R + 1, 64 * R - 1, 64 * R, 64 * R + 1, 256 * R - 1, 256 * R, 256 * R + 1, 512 * R + 1, 50000, 65537,
                          (1ll << 24) - 1, 1ll << 24};
  const int cuss[] = {-1, 0, 1, 7, 256, 304};
  for (long long r : rowss)
    for (long long k : ns)
      for (int c : cuss)
        for (int e : {4, 8}) {
          if (lh_scan_plan(r, k, e, c, out4) != 0) {
            std::printf("FAIL refused %lld %lld\n", r, k);
            fails++;
            continue;
          }
          const long long cap = (long long)(c > 0 ? c : 256) * 8, per = out4[1], tile = 256 / per * R;
          bool ok = out4[0] == (k <= 64 * R ? 0 : 1) && per == (out4[0] == 0 ? 4 : 1);
          ok = ok && out4[3] == (k + tile - 1) / tile && (out4[0] == 1 || out4[3] == 1);
          ok = ok && out4[2] <= cap && (r == 0) == (out4[2] == 0);
          ok = ok && (out4[2] == cap || ((out4[2] - 1) * per < r && out4[2] >= (r + per - 1) / per));
          if (!ok) {
            std::printf("FAIL %lld %lld %d %d -> %lld %lld %lld %lld\n", r, k, e, c, out4[0], out4[1], out4[2], out4[3]);
            fails++;
          }
        }
  expect(lh_scan_plan(1, 0, 4, 0, out4) != 0 && lh_scan_plan(1, (1ll << 24) + 1, 4, 0, out4) != 0 && lh_scan_plan(-1, 4, 4, 0, out4) != 0 &&
             lh_scan_plan(1, 4, 2, 0, out4) != 0 && lh_scan_plan(1, 4, 16, 0, out4) != 0,
         "a refused shape was planned");

  // the order on a row with zeros: run by run against lh_scan_row, monotone, zero steps, in place
  for (long long len : {1ll, 2ll, R - 1, R, R + 1, 5 * R + 3, 1000ll}) {
    std::vector<float> x(len), want(len), got(len);
    unsigned s = 12345u + (unsigned)len;
    for (long long i = 0; i < len; i++) {
      s = s * 1664525u + 1013904223u;
      x[i] = (s >> 28) < 9 ? 0.0f : (float)(s >> 8) * 5.9604644775390625e-8f;
    }
    lh_scan_row<float>(want.data(), x.data(), len);
    float carry = 0;
    for (long long r0 = 0; r0 < len; r0 += R) {  // the same thing the way a lane forms it: loc of a whole run, then the carry
      float run[LH_SCAN_RUN];
      for (long long j = 0; j < R; j++) run[j] = r0 + j < len ? x[r0 + j] : 0.0f;
      lh_scan_local<float, LH_SCAN_RUN>(run);
      if (r0 > 0) lh_scan_add_carry<float, LH_SCAN_RUN>(run, carry);
      carry = run[R - 1];
      for (long long j = 0; j < R && r0 + j < len; j++) got[r0 + j] = run[j];
    }
    expect(std::memcmp(got.data(), want.data(), len * sizeof(float)) == 0, "runs and row differ");
    for (long long i = 1; i < len; i++) {
      expect(want[i] >= want[i - 1], "not monotone");
      if (x[i] == 0) expect(want[i] == want[i - 1], "a zero step moved");
    }
    lh_scan_row<float>(x.data(), x.data(), len);
    expect(std::memcmp(x.data(), want.data(), len * sizeof(float)) == 0, "in place differs");
  }
  {
    unsigned int big[3] = {0xffffffffu, 2u, 5u}, o[3];
    lh_scan_row<unsigned int>(o, big, 3);
    expect(o[0] == 0xffffffffu && o[1] == 1u && o[2] == 6u, "the unsigned sums wrap");
  }
  {
    const int p[5] = {1, 2, 3, 4, 5};
    expect(lh_search<int>(p, 5, 3, false) == 2 && lh_search<int>(p, 5, 3, true) == 3, "search of 3");
    expect(lh_search<int>(p, 5, -10, false) == 0 && lh_search<int>(p, 5, 10, false) == 5 && lh_search<int>(p, 5, 10, true) == 5, "search ends");
    const float nanv = __builtin_nanf("");
    const float q[3] = {1.0f, 2.0f, 3.0f};
    expect(lh_search<float>(q, 3, nanv, false) == 0 && lh_search<float>(q, 3, nanv, true) == 0, "NaN goes left");
  }
  {
    const float tiny = 1.401298464324817e-45f, top = 1.0f - 5.9604644775390625e-8f;
    const float cdf[4] = {0.0f, tiny, tiny, tiny};  // weights 0, tiny, 0, 0
    expect(lh_cdf_draw(cdf, 4, top) == 1 && lh_cdf_draw(cdf, 4, 0.0f) == 1, "the draw at a denormal total");
    const float dead[2] = {0.0f, 0.0f}, inf[2] = {1.0f, __builtin_inff()}, bad[2] = {1.0f, __builtin_nanf("")};
    expect(lh_cdf_draw(dead, 2, 0.5f) == -1 && lh_cdf_draw(inf, 2, 0.5f) == -1 && lh_cdf_draw(bad, 2, 0.5f) == -1, "rows without a total");
  }
  if (fails == 0) std::printf("SUCCESS\n");
  return fails ? 1 : 0;
}
