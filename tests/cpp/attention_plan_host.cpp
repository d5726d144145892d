// tests/cpp/attention_plan_host.cpp -- laser_amd/csrc/attention_plan.h and the softmax gradient's plan of softmax_rows_plan.h
// as a stand-alone host program (no HIP): reads lines "bh tq tk d dv causal vec" from standard input and prints
// "rc BM code workgroups lds units" for each; with no input it checks a sweep of shapes against the headers' own rules (BM = 32,
// the code by `vec` alone, min(1024, bh * ceil(tq / 32)) workgroups, the LDS formula, the limits with nothing written; the
// gradient's plan equal to the softmax rows' but for the table) and prints SUCCESS.  Built with the sanitizers by
// tests/test_attention_cpu.py.
#include <cstdio>

#include "attention_plan.h"
#include "softmax_rows_plan.h"

int main(int argc, char **argv) {
  long long bh, tq, tk, d, dv, out5[5];
  int causal, vec;
  if (argc > 1) {  // "-": answer the lines of standard input
    while (std::scanf("%lld %lld %lld %lld %lld %d %d", &bh, &tq, &tk, &d, &dv, &causal, &vec) == 7) {
      for (long long &o : out5) o = -1;
      const int rc = lh_attention_plan(bh, tq, tk, d, dv, causal, vec, out5);
      std::printf("%d %lld %lld %lld %lld %lld\n", rc, out5[0], out5[1], out5[2], out5[3], out5[4]);
    }
    return 0;
  }
  int fails = 0;
  const long long bhs[] = {0, 1, 6, 1024, 1025, 1ll << 20, 1ll << 35};
  const long long tqs[] = {0, 1, 31, 32, 33, 67, 8225, 65536};
  const long long tks[] = {1, 2, 127, 128, 129, 8192, 8193, 65536};
  const long long ds[] = {1, 2, 3, 64, 65, 127, 128};
  for (long long b : bhs)
    for (long long q : tqs)
      for (long long k : tks)
        for (long long f : ds)
          for (int c = 0; c < 2; c++)
            for (int v = 0; v < 2; v++) {
              const int rc = lh_attention_plan(b, q, k, f, 129 - f, c, v, out5);
              if ((c && q > k) || (b != 0 && (q + 31) / 32 > (1ll << 40) / b)) {  // causal past the keys; more than 2^40 units
                if (rc == 0) {
                  std::printf("FAIL %lld x %lld queries on %lld keys, causal %d, planned\n", b, q, k, c);
                  fails++;
                }
                continue;
              }
              const long long units = b * ((q + 31) / 32), ld = (f + (f & 1)) | 1;
              const long long lds = 4096 + 4 * (160 * ld + 32 * 129 + 128 + 1024 + 256 + 64);
              if (rc != 0 || out5[0] != 32 || out5[1] != (v ? 0 : 1) || out5[2] != (units < 1024 ? units : 1024) || out5[3] != lds ||
                  out5[4] != units || lds > 160 * 1024) {
                std::printf("FAIL %lld %lld %lld %lld %d %d -> %d %lld %lld %lld %lld %lld\n", b, q, k, f, c, v, rc, out5[0], out5[1], out5[2],
                            out5[3], out5[4]);
                fails++;
              }
            }
  for (long long &o : out5) o = -7;
  if (lh_attention_plan(-1, 4, 4, 4, 4, 0, 1, out5) == 0 || lh_attention_plan(1, -1, 4, 4, 4, 0, 1, out5) == 0 ||
      lh_attention_plan(1, 4, 0, 4, 4, 0, 1, out5) == 0 || lh_attention_plan(1, 4, LH_ATTENTION_MAX_KEYS + 1, 4, 4, 0, 1, out5) == 0 ||
      lh_attention_plan(1, 4, 4, 0, 4, 0, 1, out5) == 0 || lh_attention_plan(1, 4, 4, LH_ATTENTION_MAX_D + 1, 4, 0, 1, out5) == 0 ||
      lh_attention_plan(1, 4, 4, 4, 0, 0, 1, out5) == 0 || lh_attention_plan(1, 4, 4, 4, LH_ATTENTION_MAX_D + 1, 0, 1, out5) == 0 ||
      lh_attention_plan(1, 5, 4, 4, 4, 1, 1, out5) == 0 || lh_attention_plan(1ll << 40, 33, 4, 4, 4, 0, 1, out5) == 0 ||
      lh_attention_plan(0x7fffffffffffffffll, 0x7fffffffffffffffll, 4, 4, 4, 0, 1, out5) == 0) {
    std::printf("FAIL a refused shape was planned\n");
    fails++;
  }
  for (long long o : out5)
    if (o != -7) {
      std::printf("FAIL a refused shape was written\n");
      fails++;
      break;
    }
  if (lh_attention_plan(1ll << 40, 32, 4, 4, 4, 0, 1, out5) != 0 || out5[4] != (1ll << 40) || out5[2] != 1024 ||
      lh_attention_plan(1, 1ll << 45, 4, 4, 4, 0, 1, out5) != 0 || out5[4] != (1ll << 40) || out5[2] != 1024) {
    std::printf("FAIL the largest unit counts\n");
    fails++;
  }
  // the softmax gradient: the softmax rows' plan without the table
  const long long rowss[] = {0, 1, 3, 4, 5, 8191, 8192, 8193, 1ll << 40}, ns[] = {1, 1024, 1025, 8192, 8193, 1ll << 26};
  for (long long r : rowss)
    for (long long n : ns)
      for (int v = 0; v < 2; v++) {
        long long a[3], g[3];
        if (lh_softmax_rows_plan(r, n, v, a) != 0 || lh_softmax_grad_rows_plan(r, n, v, g) != 0 || a[0] != g[0] || a[1] != g[1] ||
            g[2] != a[2] - LH_SOFTMAX_ROWS_LDS_LUT) {
          std::printf("FAIL softmax_grad plan %lld %lld %d\n", r, n, v);
          fails++;
        }
      }
  long long g[3] = {-7, -7, -7};
  if (lh_softmax_grad_rows_plan(-1, 4, 1, g) == 0 || lh_softmax_grad_rows_plan(4, 0, 1, g) == 0 ||
      lh_softmax_grad_rows_plan(4, (1ll << 26) + 1, 1, g) == 0 || g[0] != -7 || g[1] != -7 || g[2] != -7) {
    std::printf("FAIL softmax_grad plan: a refused shape was planned or written\n");
    fails++;
  }
  if (fails == 0) std::printf("SUCCESS\n");
  return fails ? 1 : 0;
}
