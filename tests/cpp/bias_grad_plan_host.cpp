// tests/cpp/bias_grad_plan_host.cpp -- laser_amd/csrc/bias_grad_plan.h as a stand-alone host program (no HIP): reads lines
// "rows n vec cus" from standard input and prints "rc code workgroups launches scratch" for each; with no input it checks a
// sweep of shapes against the header's own rules (one launch up to 8192 rows and two past them, workgroups = min(2048, units),
// scratch = chunks * n with two launches) and prints SUCCESS.  Built with the sanitizers by tests/test_dense_grad_cpu.py.
#include <cstdio>
#include <initializer_list>

#include "bias_grad_plan.h"

int main(int argc, char **argv) {
  long long rows, n, out4[4];
  int vec, cus;
  if (argc > 1) {  // "-": answer the lines of standard input
    while (std::scanf("%lld %lld %d %d", &rows, &n, &vec, &cus) == 4) {
      out4[0] = out4[1] = out4[2] = out4[3] = -1;
      const int rc = lh_bias_grad_plan(rows, n, vec, cus, out4);
      std::printf("%d %lld %lld %lld %lld\n", rc, out4[0], out4[1], out4[2], out4[3]);
    }
    return 0;
  }
  int fails = 0;
  const long long rowss[] = {0, 1, 4, 1024, 8191, 8192, 8193, 16384, 16385, 40961, 1ll << 20, 1ll << 26};
  const long long ns[] = {1, 3, 15, 16, 17, 37, 1024, 4096, 32768, 32769, 1ll << 31, 1ll << 46};
  for (long long r : rowss)
    for (long long k : ns)
      for (int v = 0; v < 2; v++)
        for (int c : {0, 1, 64, 256, 1000}) {
          if (lh_bias_grad_plan(r, k, v, c, out4) != 0) {
            std::printf("FAIL refused %lld %lld\n", r, k);
            fails++;
            continue;
          }
          const long long chunks = r == 0 ? 1 : (r + 8191) / 8192, strips = (k + 15) / 16;
          const bool small = strips < 2048 && chunks * strips < 2048;  // (chunks <= 8192: the product cannot overflow here)
          const bool ok = out4[0] == (v ? 0 : 1) && out4[1] == (small ? chunks * strips : 2048) && out4[2] == (r <= 8192 ? 1 : 2) &&
                          out4[3] == (r <= 8192 ? 0 : chunks * k);
          if (!ok) {
            std::printf("FAIL %lld %lld %d %d -> %lld %lld %lld %lld\n", r, k, v, c, out4[0], out4[1], out4[2], out4[3]);
            fails++;
          }
        }
  // n = 0: nothing is launched; the widest n with one chunk still plans, whatever its strip count
  if (lh_bias_grad_plan(5, 0, 1, 0, out4) != 0 || out4[1] != 0 || out4[2] != 0 || out4[3] != 0 ||
      lh_bias_grad_plan(100000, 0, 1, 0, out4) != 0 || out4[1] != 0 || out4[2] != 0 || out4[3] != 0 ||
      lh_bias_grad_plan(8192, 0x7fffffffffffffffll, 1, 0, out4) != 0 || out4[1] != 2048 || out4[2] != 1) {
    std::printf("FAIL n = 0 or the widest n\n");
    fails++;
  }
  if (lh_bias_grad_plan((1ll << 26) + 1, 4, 1, 0, out4) == 0 || lh_bias_grad_plan(-1, 4, 1, 0, out4) == 0 ||
      lh_bias_grad_plan(4, -1, 1, 0, out4) == 0 || lh_bias_grad_plan(1ll << 26, 1ll << 48, 1, 0, out4) == 0) {
    std::printf("FAIL a refused shape was planned\n");
    fails++;
  }
  if (fails == 0) std::printf("SUCCESS\n");
  return fails ? 1 : 0;
}
