// tests/cpp/layer_norm_plan_host.cpp -- laser_amd/csrc/layer_norm_plan.h as a stand-alone host program (no HIP): reads lines
// "rows n vec what" from standard input and prints "rc code workgroups launches scratch" for each; with no input it checks a
// sweep of shapes against the header's own rules (the mapping by n alone, four rows per workgroup below 1025, the cap of 2048,
// one launch of the column kernel up to 8192 rows and three past them) and prints SUCCESS.  Built with the sanitizers by
// tests/test_layer_norm_cpu.py.
#include <cstdio>

#include "layer_norm_plan.h"

int main(int argc, char **argv) {
  long long rows, n, out4[4];
  int vec, what;
  if (argc > 1) {  // "-": answer the lines of standard input
    while (std::scanf("%lld %lld %d %d", &rows, &n, &vec, &what) == 4) {
      out4[0] = out4[1] = out4[2] = out4[3] = -1;
      const int rc = lh_layer_norm_plan(rows, n, vec, what, out4);
      std::printf("%d %lld %lld %lld %lld\n", rc, out4[0], out4[1], out4[2], out4[3]);
    }
    return 0;
  }
  int fails = 0;
  const long long rowss[] = {0, 1, 3, 4, 5, 8191, 8192, 8193, 16385, 40961, 1ll << 20, 1ll << 26};
  const long long ns[] = {1, 3, 7, 8, 9, 37, 1024, 1025, 8192, 8193, 1ll << 20, 1ll << 26};
  for (long long r : rowss)
    for (long long k : ns)
      for (int v = 0; v < 2; v++) {
        for (int w = 0; w < 2; w++) {
          if (lh_layer_norm_plan(r, k, v, w, out4) != 0) {
            std::printf("FAIL refused %lld %lld %d\n", r, k, w);
            fails++;
            continue;
          }
          const int code = k <= 1024 ? 0 : k <= 8192 ? 1 : 2;
          const long long want = code == 0 ? (r + 3) / 4 : r;
          const bool ok = out4[0] == code + (v ? 0 : 4) && out4[1] == (want < 2048 ? want : 2048) && out4[2] == (r ? 1 : 0) && out4[3] == 0;
          if (!ok) {
            std::printf("FAIL %lld %lld %d %d -> %lld %lld %lld %lld\n", r, k, v, w, out4[0], out4[1], out4[2], out4[3]);
            fails++;
          }
        }
        if (lh_layer_norm_plan(r, k, v, 2, out4) != 0) {
          std::printf("FAIL refused %lld %lld 2\n", r, k);
          fails++;
          continue;
        }
        const long long chunks = r == 0 ? 1 : (r + 8191) / 8192, strips = (k + LH_LAYER_NORM_CW - 1) / LH_LAYER_NORM_CW;
        const bool ok = out4[0] == (v ? 0 : 1) && out4[1] == (chunks * strips < 2048 ? chunks * strips : 2048) &&
                        out4[2] == (r <= 8192 ? 1 : 3) && out4[3] == (r <= 8192 ? 0 : 8 * chunks * k);
        if (!ok) {
          std::printf("FAIL %lld %lld %d 2 -> %lld %lld %lld %lld\n", r, k, v, out4[0], out4[1], out4[2], out4[3]);
          fails++;
        }
      }
  out4[0] = out4[1] = out4[2] = out4[3] = -7;
  if (lh_layer_norm_plan(-1, 4, 1, 0, out4) == 0 || lh_layer_norm_plan(4, 0, 1, 0, out4) == 0 || lh_layer_norm_plan(4, -1, 1, 1, out4) == 0 ||
      lh_layer_norm_plan(4, (1ll << 26) + 1, 1, 0, out4) == 0 || lh_layer_norm_plan(4, (1ll << 26) + 1, 1, 2, out4) == 0 ||
      lh_layer_norm_plan((1ll << 26) + 1, 4, 1, 2, out4) == 0 || lh_layer_norm_plan(4, 4, 1, 3, out4) == 0 ||
      lh_layer_norm_plan(4, 4, 1, -1, out4) == 0 || out4[0] != -7 || out4[1] != -7 || out4[2] != -7 || out4[3] != -7) {
    std::printf("FAIL a refused shape was planned or written\n");
    fails++;
  }
  // rows past 2^26 are taken by the row kernels: only the column sums have that bound
  if (lh_layer_norm_plan((1ll << 26) + 1, 4, 1, 0, out4) != 0 || out4[1] != 2048 || lh_layer_norm_plan(0x7fffffffffffffffll, 8193, 1, 1, out4) != 0 ||
      out4[1] != 2048) {
    std::printf("FAIL many rows\n");
    fails++;
  }
  if (fails == 0) std::printf("SUCCESS\n");
  return fails ? 1 : 0;
}
