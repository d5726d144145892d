// tests/cpp/sincos_core_host.cpp -- laser_amd/csrc/sincos_core.h as a host program, in two modes.
//   sincos_core_host                        reads float32 values from standard input and writes one 32-byte record for each:
//                                           uint32 bits of lsin(x), of lcos(x), of the two results of lh_sincos(x), then the
//                                           quadrant (uint32) and a pad word, then the uint64 bits of the reduced argument
//                                           (quadrant 0 and argument 0 for NaN and +-Inf).  tests/test_sincos_cpu.py builds it
//                                           with g++ -ffp-contract=off -fsanitize=address,undefined and compares with the
//                                           numpy model.
//   sincos_core_host sweep FN LO HI STRIDE  FN = sin or cos.  Walks the magnitudes with bit patterns LO, LO + STRIDE, .. <= HI
//                                           (all within 0 .. 0x7f7fffff) in increasing order and evaluates FN at +x and -x.
//                                           Checks: faithful against sinl / cosl in long double (the result is one of the two
//                                           float32 that bracket the true value), symmetric (lsin(-x) has the bits of
//                                           -lsin(x), lcos(-x) those of lcos(x)), bounded (|y| <= 1), and monotone over the
//                                           float32 in [0, pi/2] (bits <= 0x3fc90fda): lsin non-decreasing, lcos
//                                           non-increasing; the first step is taken from the float below LO, so adjacent
//                                           ranges leave no gap.  Prints one line of JSON with the counts, the maximum and mean
//                                           error in float32 ulps, the input of the maximum, the results that are not the
//                                           correctly rounded float32, the largest magnitude at which the result still is x
//                                           (sin) or 1 (cos) counted from LO without a gap, and the smallest |reduced
//                                           argument| met with its input; exit status 1 if a property fails.  Built -O2
//                                           without sanitizers.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sincos_core.h"

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
static uint64_t bits_of64(double f) {
  uint64_t b;
  memcpy(&b, &f, 8);
  return b;
}

struct Tally {
  unsigned long long count = 0, unfaithful = 0, inexact = 0;
  long double max_err = 0, sum_err = 0;
  uint32_t max_at = 0, first_bad = 0;
  void add(uint32_t xb, float got, long double want) {
    float near = (float)want, down = near, up = near;  // the two float32 that bracket `want`
    if ((long double)near > want) down = nextafterf(near, -INFINITY);
    if ((long double)near < want) up = nextafterf(near, INFINITY);
    if (!(got == down || got == up)) {
      if (!unfaithful) first_bad = xb;
      unfaithful++;
    }
    long double ulp = (long double)up - (long double)down;
    if (ulp == 0) ulp = (want == 0 || fabsl(want) < 0x1p-126L) ? 0x1p-149L : ldexpl(1.0L, ilogbl(want) - 23);
    const long double err = fabsl((long double)got - want) / ulp;
    if (err > max_err) {
      max_err = err;
      max_at = xb;
    }
    sum_err += err;
    if (got != near) inexact++;
    count++;
  }
};

static const uint32_t kHalfPiBelow = 0x3fc90fdau;  // the largest float32 <= pi/2

static int sweep(const char *fn, uint32_t lo, uint32_t hi, uint32_t stride) {
  const bool is_sin = !strcmp(fn, "sin");
  if ((!is_sin && strcmp(fn, "cos")) || hi > 0x7f7fffffu || lo > hi || stride < 1) {
    fprintf(stderr, "sweep: FN sin or cos, 0 <= LO <= HI <= 0x7f7fffff, STRIDE >= 1\n");
    return 2;
  }
  Tally t;
  unsigned long long drops = 0, not_symmetric = 0, out_of_bounds = 0;
  uint32_t trivial_to = 0, min_r_at = 0;
  bool trivial_run = true, have_trivial = false;
  double min_r = INFINITY;
  float prev = is_sin ? -INFINITY : INFINITY;
  if (lo > 0) prev = is_sin ? lh_sin(from_bits(lo - 1)) : lh_cos(from_bits(lo - 1));
  for (uint64_t b = lo; b <= hi; b += stride) {
    const float xp = from_bits((uint32_t)b), xn = from_bits((uint32_t)b | 0x80000000u);
    const float gp = is_sin ? lh_sin(xp) : lh_cos(xp), gn = is_sin ? lh_sin(xn) : lh_cos(xn);
    const long double wp = is_sin ? sinl((long double)xp) : cosl((long double)xp), wn = is_sin ? -wp : wp;
    if (bits_of(gn) != (is_sin ? bits_of(gp) ^ 0x80000000u : bits_of(gp))) not_symmetric++;
    if (!(fabsf(gp) <= 1.0f) || !(fabsf(gn) <= 1.0f)) out_of_bounds++;
    t.add((uint32_t)b, gp, wp);
    t.add((uint32_t)b | 0x80000000u, gn, wn);
    if (b <= kHalfPiBelow) {
      if (is_sin ? !(gp >= prev) : !(gp <= prev)) drops++;
      prev = gp;
    }
    if (trivial_run && (is_sin ? bits_of(gp) == (uint32_t)b : gp == 1.0f)) {
      trivial_to = (uint32_t)b;
      have_trivial = true;
    } else {
      trivial_run = false;
    }
    double r;
    lh_sc_reduce((uint32_t)b, &r);
    if (b >= 0x3f490fdbu && fabs(r) < min_r) {  // from pi/4 on: below it the argument is x itself
      min_r = fabs(r);
      min_r_at = (uint32_t)b;
    }
  }
  printf("{\"fn\": \"%s\", \"lo\": \"0x%08x\", \"hi\": \"0x%08x\", \"stride\": %u, \"count\": %llu, \"unfaithful\": %llu, "
         "\"first_unfaithful\": \"0x%08x\", \"not_monotone\": %llu, \"not_symmetric\": %llu, \"out_of_bounds\": %llu, "
         "\"not_nearest\": %llu, \"max_ulp\": %.6Lf, \"max_at\": \"0x%08x\", \"mean_ulp\": %.6Lf, \"trivial_to\": \"%s0x%08x\", "
         "\"min_reduced\": %.6e, \"min_reduced_at\": \"0x%08x\"}\n",
         fn, lo, hi, stride, t.count, t.unfaithful, t.first_bad, drops, not_symmetric, out_of_bounds, t.inexact, t.max_err, t.max_at,
         t.sum_err / (long double)t.count, have_trivial ? "" : "none ", trivial_to, min_r == INFINITY ? 0.0 : min_r, min_r_at);
  return t.unfaithful || drops || not_symmetric || out_of_bounds ? 1 : 0;
}

int main(int argc, char **argv) {
  if (argc == 6 && !strcmp(argv[1], "sweep"))
    return sweep(argv[2], (uint32_t)strtoul(argv[3], nullptr, 0), (uint32_t)strtoul(argv[4], nullptr, 0),
                 (uint32_t)strtoul(argv[5], nullptr, 0));
  if (argc != 1) {
    fprintf(stderr, "usage: %s [sweep sin|cos LO HI STRIDE]\n", argv[0]);
    return 2;
  }
  std::vector<float> in;
  float buf[4096];
  size_t got;
  while ((got = fread(buf, sizeof(float), 4096, stdin)) > 0) in.insert(in.end(), buf, buf + got);
  struct Rec {
    uint32_t s, c, ss, sc, q, pad;
    uint64_t r;
  };
  static_assert(sizeof(Rec) == 32, "record layout");
  std::vector<Rec> out(in.size());
  for (size_t i = 0; i < in.size(); i++) {
    const float x = in[i];
    float s, c;
    lh_sincos(x, &s, &c);
    out[i].s = bits_of(lh_sin(x));
    out[i].c = bits_of(lh_cos(x));
    out[i].ss = bits_of(s);
    out[i].sc = bits_of(c);
    out[i].pad = 0;
    const uint32_t babs = bits_of(x) & 0x7fffffffu;
    double r = 0.0;
    out[i].q = babs >= 0x7f800000u ? 0u : (uint32_t)lh_sc_reduce(babs, &r);
    out[i].r = bits_of64(r);
  }
  if (fwrite(out.data(), sizeof(Rec), out.size(), stdout) != out.size()) return 1;
  return 0;
}
