// tests/cpp/philox_host.cpp -- philox_core.h and random_plan.h from a host program built with g++ alone (no HIP): the generator,
// the stream layout, the five outputs of the fills and the launch plan, for tests/test_random_cpu.py to compare with the numpy
// model and with the library.  Reads requests from stdin, one per line, and answers each with one line:
//   kat c0 c1 c2 c3 k0 k1                          (hex)  -> the four words of one block
//   fill KIND seed subseq offset n lo hi           KIND = bits_u32 | uniform_f32 | uniform_f64 | uniform_i32 | uniform_i64;
//                                                  seed, subseq, offset in hex; lo, hi as strtod / strtoll read them
//                                                  -> the n elements as hex bit patterns
//   plan n words_per_elem offset(hex) dst_misaligned cus     -> rc and the four numbers
//   range32 lo hi / range64 lo hi                  -> 1 when the bounds are valid for a float fill, else 0
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "philox_core.h"
#include "random_plan.h"

typedef unsigned long long u64;

static unsigned int word(u64 seed, u64 subseq, u64 w) { return lh_philox_word(seed, subseq, w); }
static u64 pair(u64 seed, u64 subseq, u64 w) { return (u64)word(seed, subseq, w) | (u64)word(seed, subseq, w + 1) << 32; }

int main() {
  char line[512], kind[32], a[64], b[64];
  while (std::fgets(line, sizeof line, stdin)) {
    u64 c[6], seed, subseq, offset;
    long long n;
    int wpe, mis, cus;
    if (std::sscanf(line, "kat %llx %llx %llx %llx %llx %llx", &c[0], &c[1], &c[2], &c[3], &c[4], &c[5]) == 6) {
      unsigned int ctr[4] = {(unsigned)c[0], (unsigned)c[1], (unsigned)c[2], (unsigned)c[3]};
      lh_philox4x32_10(ctr, (unsigned)c[4], (unsigned)c[5]);
      std::printf("%08x %08x %08x %08x\n", ctr[0], ctr[1], ctr[2], ctr[3]);
    } else if (std::sscanf(line, "fill %31s %llx %llx %llx %lld %63s %63s", kind, &seed, &subseq, &offset, &n, a, b) == 7) {
      for (long long i = 0; i < n; i++) {
        if (!std::strcmp(kind, "bits_u32")) {
          std::printf("%08x ", word(seed, subseq, offset + (u64)i));
        } else if (!std::strcmp(kind, "uniform_f32")) {
          const float v = lh_uniform_f32(word(seed, subseq, offset + (u64)i), std::strtof(a, 0), std::strtof(b, 0));
          unsigned int bits;
          std::memcpy(&bits, &v, 4);
          std::printf("%08x ", bits);
        } else if (!std::strcmp(kind, "uniform_i32")) {
          std::printf("%08x ", (unsigned)lh_uniform_i32(word(seed, subseq, offset + (u64)i), (int)std::strtol(a, 0, 10), (int)std::strtol(b, 0, 10)));
        } else if (!std::strcmp(kind, "uniform_f64")) {
          const double v = lh_uniform_f64(pair(seed, subseq, offset + 2 * (u64)i), std::strtod(a, 0), std::strtod(b, 0));
          u64 bits;
          std::memcpy(&bits, &v, 8);
          std::printf("%016llx ", bits);
        } else if (!std::strcmp(kind, "uniform_i64")) {
          std::printf("%016llx ", (u64)lh_uniform_i64(pair(seed, subseq, offset + 2 * (u64)i), std::strtoll(a, 0, 10), std::strtoll(b, 0, 10)));
        } else {
          return 2;
        }
      }
      std::printf("\n");
    } else if (std::sscanf(line, "plan %lld %d %llx %d %d", &n, &wpe, &offset, &mis, &cus) == 5) {
      long long p[4] = {-1, -1, -1, -1};
      const int rc = lh_random_plan(n, wpe, offset, mis, cus, p);
      std::printf("%d %lld %lld %lld %lld\n", rc, p[0], p[1], p[2], p[3]);
    } else if (std::sscanf(line, "range32 %63s %63s", a, b) == 2) {
      std::printf("%d\n", lh_uniform_range_ok_f32(std::strtof(a, 0), std::strtof(b, 0)));
    } else if (std::sscanf(line, "range64 %63s %63s", a, b) == 2) {
      std::printf("%d\n", lh_uniform_range_ok_f64(std::strtod(a, 0), std::strtod(b, 0)));
    } else {
      return 2;
    }
  }
  return 0;
}
