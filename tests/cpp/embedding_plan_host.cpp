// tests/cpp/embedding_plan_host.cpp -- laser_amd/csrc/embedding_plan.h as a stand-alone host program (no HIP): reads lines
// "tokens vocab dim vec cus" from standard input and prints "rc" and the eight plan values for each; with no input it checks a
// sweep of shapes against the header's own rules (a pass per 8 bits of vocab's bit length, the smallest power-of-two tile from
// 512 that keeps the tiles at or below 2^14, four tiles a workgroup, 3 launches a pass and one for starts, two for the sums)
// and prints SUCCESS.  Built with the sanitizers by tests/test_embedding_cpu.py.
#include <cstdio>
#include <initializer_list>

#include "embedding_plan.h"

int main(int argc, char **argv) {
  long long tokens, vocab, dim, out[8];
  int vec, cus;
  if (argc > 1) {  // "-": answer the lines of standard input
    while (std::scanf("%lld %lld %lld %d %d", &tokens, &vocab, &dim, &vec, &cus) == 5) {
      for (long long &o : out) o = -1;
      const int rc = lh_embedding_plan(tokens, vocab, dim, vec, cus, out);
      std::printf("%d %lld %lld %lld %lld %lld %lld %lld %lld\n", rc, out[0], out[1], out[2], out[3], out[4], out[5], out[6], out[7]);
    }
    return 0;
  }
  int fails = 0;
  const long long ts[] = {0, 1, 511, 512, 513, 2048, 2049, 131072, (1ll << 23), (1ll << 23) + 1, (1ll << 24) + 1, 1ll << 26};
  const long long vs[] = {0, 1, 2, 200, 255, 256, 257, 65535, 65536, 65537, (1ll << 24) - 1, 1ll << 24, 1ll << 30};
  const long long ds[] = {0, 1, 4, 17, 4096, 1ll << 40};
  for (long long t : ts)
    for (long long v : vs)
      for (long long d : ds)
        for (int k = 0; k < 2; k++)
          for (int c : {0, 256}) {
            if (lh_embedding_plan(t, v, d, k, c, out) != 0) {
              std::printf("FAIL refused %lld %lld %lld\n", t, v, d);
              fails++;
              continue;
            }
            const long long passes = v <= 255 ? 1 : v <= 65535 ? 2 : v < (1ll << 24) ? 3 : 4;
            long long tile = 512;
            while ((t + tile - 1) / tile > (1ll << 14)) tile *= 2;
            const long long tiles = (t + tile - 1) / tile;
            const long long gs = t == 0 ? 0 : 2 * 256 * tiles * 4 + (passes > 1 ? t * 4 : 0);
            const bool sums = v > 0 && d > 0;
            const bool ok = out[0] == passes && out[1] == tile && out[2] == (tiles + 3) / 4 && out[3] == (k ? 0 : 1) &&
                            out[4] == (t == 0 ? 1 : 3 * passes + 1) && out[5] == (sums ? 2 : 0) && out[6] == gs &&
                            out[7] == (sums ? gs + t * 4 + (v + 1) * 4 : 0) && tile <= 4096;
            if (!ok) {
              std::printf("FAIL %lld %lld %lld %d %d -> %lld %lld %lld %lld %lld %lld %lld %lld\n", t, v, d, k, c, out[0], out[1], out[2],
                          out[3], out[4], out[5], out[6], out[7]);
              fails++;
            }
          }
  if (lh_embedding_plan((1ll << 26) + 1, 4, 4, 1, 0, out) == 0 || lh_embedding_plan(-1, 4, 4, 1, 0, out) == 0 ||
      lh_embedding_plan(4, -1, 4, 1, 0, out) == 0 || lh_embedding_plan(4, (1ll << 30) + 1, 4, 1, 0, out) == 0 ||
      lh_embedding_plan(4, 4, -1, 1, 0, out) == 0) {
    std::printf("FAIL a refused shape was planned\n");
    fails++;
  }
  if (fails == 0) std::printf("SUCCESS\n");
  return fails ? 1 : 0;
}
