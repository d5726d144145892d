// tests/cpp/optim_plan_host.cpp -- laser_amd/csrc/optim_plan.h as a stand-alone host program (no HIP): with "-" it reads
// lines "what count len_0 .. len_{count-1}" from standard input and prints "rc launches workgroups chunks scratch" for each;
// with no argument it checks lists around every boundary against the header's own rules (ceil(count / 64) step launches,
// min(2048, chunks) workgroups, 2 * ceil(count / 192) + 1 launches of the gradient norm) and prints SUCCESS.  Built with the
// sanitizers by tests/test_optim_cpu.py.
#include <cstdio>
#include <vector>

#include "optim_plan.h"

static int fails = 0;
static void expect(const char *what, bool ok) {
  if (!ok) {
    std::printf("FAIL %s\n", what);
    fails++;
  }
}

int main(int argc, char **argv) {
  long long out4[4];
  if (argc > 1) {
    int what;
    long long count;
    while (std::scanf("%d %lld", &what, &count) == 2) {
      std::vector<long long> lens;
      for (long long k = 0; k < count; k++) {
        long long v = 0;
        if (std::scanf("%lld", &v) != 1) return 2;
        lens.push_back(v);
      }
      out4[0] = out4[1] = out4[2] = out4[3] = -1;
      const int rc = lh_optim_plan(what, lens.data(), count, out4);
      std::printf("%d %lld %lld %lld %lld\n", rc, out4[0], out4[1], out4[2], out4[3]);
    }
    return 0;
  }
  const long long lengths[] = {0, 1, 4095, 4096, 4097, 8191, 8192, 8193, 1ll << 26};
  const int counts[] = {0, 1, 64, 65, 129, 192, 193, 65536};
  for (long long len : lengths)
    for (int count : counts) {
      if (len == (1ll << 26) && count > 129) continue;
      const std::vector<long long> lens((size_t)count, len);
      const long long c = (len + 4095) / 4096, rc = len ? (len + 8191) / 8192 : 1;
      for (int what = 0; what < 2; what++) {
        expect("a step list is planned", lh_optim_plan(what, lens.data(), count, out4) == 0);
        const long long groups = c ? (count + 63) / 64 : 0, first = c * (count < 64 ? count : 64);
        expect("step launches, workgroups, chunks, scratch",
               out4[0] == groups && out4[1] == (first < 2048 ? first : 2048) && out4[2] == c * count && out4[3] == 0);
      }
      expect("a norm list is planned", lh_optim_plan(2, lens.data(), count, out4) == 0);
      const long long groups = (count + 191) / 192, total = rc * count;
      expect("norm launches", out4[0] == 2 * groups + 1 && (count > 192 || out4[0] <= 3));
      expect("norm workgroups, chunks, scratch", out4[1] == (count ? rc * (count < 192 ? count : 192) : 1) && out4[2] == total &&
                                                     out4[3] == (count ? (total * 4 + 15) / 16 * 16 + (count * 4ll + 15) / 16 * 16 : 0));
    }
  {  // chunk totals of 2048 and 2049: the cap of the grid
    std::vector<long long> lens(2, 1024ll * 4096);
    expect("2048 chunks", lh_optim_plan(1, lens.data(), 2, out4) == 0 && out4[1] == 2048 && out4[2] == 2048);
    lens[1] += 1;
    expect("2049 chunks", lh_optim_plan(1, lens.data(), 2, out4) == 0 && out4[1] == 2048 && out4[2] == 2049 && out4[0] == 1);
    lens[0] = 2047ll * 4096;
    lens[1] = 0;
    expect("2047 chunks", lh_optim_plan(0, lens.data(), 2, out4) == 0 && out4[1] == 2047);
  }
  {  // a group of empty tensors launches nothing; the first launch is the first group with work
    std::vector<long long> lens(130, 0);
    expect("all empty", lh_optim_plan(0, lens.data(), 130, out4) == 0 && out4[0] == 0 && out4[1] == 0 && out4[2] == 0);
    lens[129] = 5;
    expect("work in the third group only", lh_optim_plan(1, lens.data(), 130, out4) == 0 && out4[0] == 1 && out4[1] == 1 && out4[2] == 1);
    expect("the norm still has one chunk per empty tensor", lh_optim_plan(2, lens.data(), 130, out4) == 0 && out4[0] == 3 && out4[1] == 130);
  }
  out4[0] = out4[1] = out4[2] = out4[3] = -7;
  {
    std::vector<long long> lens(3, 5);
    bool refused = lh_optim_plan(3, lens.data(), 3, out4) != 0 && lh_optim_plan(-1, lens.data(), 3, out4) != 0 &&
                   lh_optim_plan(0, lens.data(), -1, out4) != 0 && lh_optim_plan(0, lens.data(), 65537, out4) != 0 &&
                   lh_optim_plan(0, (const long long *)nullptr, 3, out4) != 0;
    lens[1] = -1;
    refused = refused && lh_optim_plan(0, lens.data(), 3, out4) != 0 && lh_optim_plan(2, lens.data(), 3, out4) != 0;
    lens[1] = (1ll << 26) + 1;
    refused = refused && lh_optim_plan(1, lens.data(), 3, out4) != 0 && lh_optim_plan(2, lens.data(), 3, out4) != 0;
    expect("refused lists are not planned and nothing is written",
           refused && out4[0] == -7 && out4[1] == -7 && out4[2] == -7 && out4[3] == -7);
    expect("an empty list needs no lens", lh_optim_plan(0, (const long long *)nullptr, 0, out4) == 0 && out4[0] == 0);
  }
  if (fails == 0) std::printf("SUCCESS\n");
  return fails ? 1 : 0;
}
