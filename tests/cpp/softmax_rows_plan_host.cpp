// tests/cpp/softmax_rows_plan_host.cpp -- laser_amd/csrc/softmax_rows_plan.h as a host program (g++ alone, no HIP): reads
// "rows n vec" triples from standard input and prints "rc code workgroups lds" for each.  tests/test_log_softmax_cpu.py builds
// it with -fsanitize=address,undefined and compares the lines with what it works out itself.
#include <cstdio>

#include "softmax_rows_plan.h"

int main() {
  long long rows, n;
  int vec;
  while (std::scanf("%lld %lld %d", &rows, &n, &vec) == 3) {
    long long p[3] = {-1, -1, -1};
    const int rc = lh_softmax_rows_plan(rows, n, vec, p);
    std::printf("%d %lld %lld %lld\n", rc, p[0], p[1], p[2]);
  }
  return 0;
}
