// tests/cpp/log_core_host.cpp -- laser_amd/csrc/log_core.h as a host program, in two modes.
//   log_core_host                      reads float32 values from standard input and writes the bits of llog of each to
//                                      standard output.  tests/test_log_softmax_cpu.py builds it with g++ -ffp-contract=off
//                                      -fsanitize=address,undefined and compares the output with the numpy model bit for bit.
//   log_core_host sweep LO HI STRIDE   walks the positive float32 bit patterns LO, LO + STRIDE, .. <= HI (hexadecimal or
//                                      decimal; all within 1 .. 0x7f7fffff) in increasing order and checks the two
//                                      properties of llog: faithful against (float)log((double)x) -- the result is one of the
//                                      two float32 that bracket the float64 logarithm -- and non-decreasing.  Prints one line
//                                      of JSON with the counts, the maximum and mean error in float32 ulps and the input of the
//                                      maximum; exit status 1 if either property fails.  Built -O2 without sanitizers; the
//                                      full sweep (1 0x7f7fffff 1) takes about a minute.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "log_core.h"

static float from_bits(uint32_t b) {
  float f;
  memcpy(&f, &b, 4);
  return f;
}
static uint32_t bits_of(float f) {
  uint32_t b;
  memcpy(&b, &f, 4);
  return b;
}

static int sweep(uint32_t lo, uint32_t hi, uint32_t stride) {
  if (lo < 1 || hi > 0x7f7fffffu || lo > hi || stride < 1) {
    fprintf(stderr, "sweep: 1 <= LO <= HI <= 0x7f7fffff, STRIDE >= 1\n");
    return 2;
  }
  unsigned long long count = 0, unfaithful = 0, drops = 0, inexact = 0;
  double max_err = 0, sum_err = 0;
  uint32_t max_at = lo, first_bad = 0;
  float prev = -INFINITY;
  for (uint64_t b = lo; b <= hi; b += stride) {
    const float x = from_bits((uint32_t)b);
    const float got = lh_log(x);
    const double want = log((double)x);
    // the two float32 that bracket `want`
    float near = (float)want, down = near, up = near;
    if ((double)near > want) down = nextafterf(near, -INFINITY);
    if ((double)near < want) up = nextafterf(near, INFINITY);
    const bool ok = got == down || got == up;
    if (!ok) {
      if (!unfaithful) first_bad = (uint32_t)b;
      unfaithful++;
    }
    // the error in ulps of the float32 grid at `want`: the spacing of the bracket, or of the binade for an exact result
    double ulp = (double)up - (double)down;
    if (ulp == 0) ulp = want == 0 ? ldexp(1.0, -149) : ldexp(1.0, ilogb(want) - 23);
    const double err = fabs((double)got - want) / ulp;
    if (err > max_err) {
      max_err = err;
      max_at = (uint32_t)b;
    }
    sum_err += err;
    if (bits_of(got) != bits_of(near)) inexact++;
    if (!(got >= prev)) drops++;
    prev = got;
    count++;
  }
  printf("{\"lo\": \"0x%08x\", \"hi\": \"0x%08x\", \"stride\": %u, \"count\": %llu, \"unfaithful\": %llu, \"first_unfaithful\": \"0x%08x\", "
         "\"not_monotone\": %llu, \"not_nearest\": %llu, \"max_ulp\": %.6f, \"max_at\": \"0x%08x\", \"mean_ulp\": %.6f}\n",
         lo, hi, stride, count, unfaithful, first_bad, drops, inexact, max_err, max_at, sum_err / (double)count);
  return unfaithful || drops ? 1 : 0;
}

int main(int argc, char **argv) {
  if (argc == 5 && !strcmp(argv[1], "sweep"))
    return sweep((uint32_t)strtoul(argv[2], nullptr, 0), (uint32_t)strtoul(argv[3], nullptr, 0), (uint32_t)strtoul(argv[4], nullptr, 0));
  if (argc != 1) {
    fprintf(stderr, "usage: %s [sweep LO HI STRIDE]\n", argv[0]);
    return 2;
  }
  std::vector<float> in;
  float buf[4096];
  size_t got;
  while ((got = fread(buf, sizeof(float), 4096, stdin)) > 0) in.insert(in.end(), buf, buf + got);
  std::vector<float> out(in.size());
  for (size_t i = 0; i < in.size(); i++) out[i] = lh_log(in[i]);
  if (fwrite(out.data(), sizeof(float), out.size(), stdout) != out.size()) return 1;
  return 0;
}
