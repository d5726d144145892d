// tests/cpp/normal_core_host.cpp -- laser_amd/csrc/normal_core.h as a host program, in two modes.
//   normal_core_host fill SEED SUBSEQ OFFSET N MEAN STD   writes the N float32 of a normal fill of the stream (SEED, SUBSEQ) from
//                                                        OFFSET (all unsigned 64-bit, any base), position by position as the
//                                                        header states it; MEAN and STD are float32 bit patterns.
//   normal_core_host pairs                               reads pairs of uint32 words (w0, w1) from standard input and writes
//                                                        four float32 for each: the cosine and sine branch from lh_normal_pair,
//                                                        then the two from lh_normal_z (they must agree).
// tests/test_normal_cpu.py builds it with g++ -ffp-contract=off -fsanitize=address,undefined and compares with the numpy model.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "normal_core.h"

static float from_bits(uint32_t b) {
  float f;
  memcpy(&f, &b, 4);
  return f;
}

int main(int argc, char **argv) {
  if (argc == 8 && !strcmp(argv[1], "fill")) {
    const unsigned long long seed = strtoull(argv[2], nullptr, 0), subseq = strtoull(argv[3], nullptr, 0), offset = strtoull(argv[4], nullptr, 0);
    const long long n = strtoll(argv[5], nullptr, 0);
    const float mean = from_bits((uint32_t)strtoul(argv[6], nullptr, 0)), std = from_bits((uint32_t)strtoul(argv[7], nullptr, 0));
    if (n < 0 || !lh_normal_params_ok_f32(mean, std)) return 3;
    std::vector<float> out((size_t)n);
    for (long long i = 0; i < n; i++) {
      const unsigned long long p = offset + (unsigned long long)i;  // wraps mod 2^64
      unsigned int o[4];
      lh_philox_block(seed, subseq, p >> 2, o);
      const int first = (int)(p & 2);  // the pair's first word inside the block: 0 or 2
      out[(size_t)i] = lh_normal_scale_f32(lh_normal_z(o[first], o[first + 1], (int)(p & 1)), mean, std);
    }
    return fwrite(out.data(), sizeof(float), out.size(), stdout) == out.size() ? 0 : 1;
  }
  if (argc == 2 && !strcmp(argv[1], "pairs")) {
    std::vector<uint32_t> in;
    uint32_t buf[4096];
    size_t got;
    while ((got = fread(buf, sizeof(uint32_t), 4096, stdin)) > 0) in.insert(in.end(), buf, buf + got);
    std::vector<float> out(in.size() * 2);
    for (size_t i = 0; i + 1 < in.size(); i += 2) {
      lh_normal_pair(in[i], in[i + 1], &out[2 * i], &out[2 * i + 1]);
      out[2 * i + 2] = lh_normal_z(in[i], in[i + 1], 0);
      out[2 * i + 3] = lh_normal_z(in[i], in[i + 1], 1);
    }
    return fwrite(out.data(), sizeof(float), out.size(), stdout) == out.size() ? 0 : 1;
  }
  fprintf(stderr, "usage: %s fill SEED SUBSEQ OFFSET N MEAN_BITS STD_BITS | pairs\n", argv[0]);
  return 2;
}
