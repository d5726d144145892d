// tests/cpp/sampler_plan_host.cpp -- laser_amd/csrc/sampler_plan.h as a stand-alone host program (no HIP): reads lines
// "rows n" from standard input and prints "rc elems code leaves first second" for each; with no input it checks a sweep of
// shapes against the header's own rules (2 P elements, the kernel by P, both grids within the cap) and prints SUCCESS.  Built
// with the sanitizers by tests/test_sampler_cpu.py.
#include <cstdio>

#include "sampler_plan.h"

int main(int argc, char **argv) {
  long long rows, n, out4[4], elems;
  if (argc > 1) {  // "-": answer the lines of standard input
    while (std::scanf("%lld %lld", &rows, &n) == 2) {
      out4[0] = out4[1] = out4[2] = out4[3] = elems = -1;
      const int rc = lh_sampler_plan(rows, n, out4) | lh_sampler_tree_elems(n, &elems);
      std::printf("%d %lld %lld %lld %lld %lld\n", rc, elems, out4[0], out4[1], out4[2], out4[3]);
    }
    return 0;
  }
  int fails = 0;
  const long long rowss[] = {0, 1, 2, 3, 67, 1023, 1024, 1025, 16383, 16384, 16385, 1ll << 31, 1ll << 50, 0x7fffffffffffffffll};
  const long long ns[] = {1, 2, 3, 4, 5, 511, 512, 513, 1023, 1024, 1025, 2048, 2049, 50000, 65536, 65537, (1ll << 24) - 1, 1ll << 24};
  const long long cap = LH_SAMPLER_MAX_WORKGROUPS;
  for (long long r : rowss)
    for (long long k : ns) {
      if (lh_sampler_plan(r, k, out4) != 0 || lh_sampler_tree_elems(k, &elems) != 0) {
        std::printf("FAIL refused %lld %lld\n", r, k);
        fails++;
        continue;
      }
      const long long p = elems / 2;
      bool ok = (p & (p - 1)) == 0 && p >= k && (p == 1 || p / 2 < k);
      ok = ok && out4[0] == (p <= 512 ? 0 : 1) && out4[1] == 1024;
      ok = ok && out4[2] >= (r ? 1 : 0) && out4[2] <= cap && (r == 0) == (out4[2] == 0);
      if (out4[0] == 0) {
        const long long per = 1024 / p;
        ok = ok && out4[3] == 0 && (out4[2] == cap || (out4[2] - 1) * per < r) && (out4[2] == cap || out4[2] * per >= r);
      } else {
        ok = ok && out4[3] == (r < cap ? r : cap) && (out4[2] == cap || out4[2] / (p / 1024) == r);
      }
      if (!ok) {
        std::printf("FAIL %lld %lld -> %lld | %lld %lld %lld %lld\n", r, k, elems, out4[0], out4[1], out4[2], out4[3]);
        fails++;
      }
    }
  if (lh_sampler_plan(1, 0, out4) == 0 || lh_sampler_plan(1, (1ll << 24) + 1, out4) == 0 || lh_sampler_plan(-1, 4, out4) == 0 ||
      lh_sampler_tree_elems(0, &elems) == 0 || lh_sampler_tree_elems((1ll << 24) + 1, &elems) == 0 || lh_sampler_tree_elems(-5, &elems) == 0) {
    std::printf("FAIL a refused shape was planned\n");
    fails++;
  }
  if (fails == 0) std::printf("SUCCESS\n");
  return fails ? 1 : 0;
}
