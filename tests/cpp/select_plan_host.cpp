// tests/cpp/select_plan_host.cpp -- laser_amd/csrc/select_plan.h as a stand-alone host program (no HIP): reads lines
// "rows n k vec" from standard input and prints "rc code workgroups lds" for each.  Built with the sanitizers by
// tests/test_select_cpu.py, which holds the answers against the library's laser_hip_topk_plan.
#include <cstdio>

#include "select_plan.h"

int main() {
  long long rows, n, k, out3[3];
  int vec;
  while (std::scanf("%lld %lld %lld %d", &rows, &n, &k, &vec) == 4) {
    out3[0] = out3[1] = out3[2] = -1;
    const int rc = lh_topk_plan(rows, n, k, vec, out3);
    std::printf("%d %lld %lld %lld\n", rc, out3[0], out3[1], out3[2]);
  }
  return 0;
}
