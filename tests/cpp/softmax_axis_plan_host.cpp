// tests/cpp/softmax_axis_plan_host.cpp -- laser_amd/csrc/softmax_axis_plan.h as a stand-alone host program (no HIP): reads
// lines "outer n inner vec cus" from standard input and prints "rc code cw workgroups lds" for each; with no input it checks
// a sweep of shapes against the header's own rules (workgroups within the cap and the strips, codes by the bounds) and prints
// SUCCESS.  Built with the sanitizers by tests/test_softmax_axis_cpu.py.
#include <cstdio>
#include <initializer_list>

#include "softmax_axis_plan.h"

int main(int argc, char **argv) {
  long long outer, n, inner, out4[4];
  int vec, cus;
  if (argc > 1) {  // "-": answer the lines of standard input
    while (std::scanf("%lld %lld %lld %d %d", &outer, &n, &inner, &vec, &cus) == 5) {
      out4[0] = out4[1] = out4[2] = out4[3] = -1;
      const int rc = lh_softmax_axis_plan(outer, n, inner, vec, cus, out4);
      std::printf("%d %lld %lld %lld %lld\n", rc, out4[0], out4[1], out4[2], out4[3]);
    }
    return 0;
  }
  int fails = 0;
  const long long outers[] = {0, 1, 3, 2047, 2048, 2049, 1ll << 31, 1ll << 40, 0x7fffffffffffffffll};
  const long long ns[] = {1, 1024, 1025, 8192, 8193, 1ll << 20};
  const long long inners[] = {2, 3, 15, 16, 17, 33, 1ll << 20, 1ll << 40, 0x7fffffffffffffffll};
  for (long long o : outers)
    for (long long k : ns)
      for (long long i : inners)
        for (int v = 0; v < 2; v++)
          for (int c : {0, 1, 64, 256, 1000}) {
            if (lh_softmax_axis_plan(o, k, i, v, c, out4) != 0) {
              std::printf("FAIL refused %lld %lld %lld\n", o, k, i);
              fails++;
              continue;
            }
            const long long cap = 2048;  // whatever the compute-unit count
            const bool ok = out4[0] == (k <= LH_SOFTMAX_AXIS_RESIDENT_N ? 8 : 9) + (v ? 0 : 4) && out4[1] == LH_SOFTMAX_AXIS_CW &&
                            out4[2] >= (o ? 1 : 0) && out4[2] <= cap && (o == 0) == (out4[2] == 0) && out4[3] > 4096 && out4[3] <= 65536;
            if (!ok) {
              std::printf("FAIL %lld %lld %lld %d %d -> %lld %lld %lld %lld\n", o, k, i, v, c, out4[0], out4[1], out4[2], out4[3]);
              fails++;
            }
          }
  if (lh_softmax_axis_plan(1, (1ll << 20) + 1, 2, 1, 0, out4) == 0 || lh_softmax_axis_plan(1, 0, 2, 1, 0, out4) == 0 ||
      lh_softmax_axis_plan(1, 4, 0, 1, 0, out4) == 0 || lh_softmax_axis_plan(-1, 4, 4, 1, 0, out4) == 0 ||
      lh_softmax_axis_plan(1, (1ll << 26) + 1, 1, 1, 0, out4) == 0) {
    std::printf("FAIL a refused shape was planned\n");
    fails++;
  }
  if (fails == 0) std::printf("SUCCESS\n");
  return fails ? 1 : 0;
}
