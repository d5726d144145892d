// tests/cpp/act_core_host.cpp -- laser_amd/csrc/act_core.h as a host program, in two modes.
//   act_core_host                         reads float32 values from standard input and writes one 24-byte record for each:
//                                         uint32 bits of ltanh(x), uint32 bits of lsigmoid(x), uint64 bits of E(-min(|x|, 208))
//                                         and uint64 bits of the small-argument polynomial at min(|x|, 2^-6) (a NaN x counts
//                                         as 0 in the last two).  tests/test_activation_cpu.py builds it with g++
//                                         -ffp-contract=off -fsanitize=address,undefined and compares with the numpy model.
//   act_core_host sweep FN LO HI STRIDE   FN = tanh or sigmoid.  Walks the magnitudes with bit patterns LO, LO + STRIDE, ..
//                                         <= HI (all within 0 .. 0x7f7fffff) in increasing order and evaluates FN at +x and
//                                         at -x.  Checks: faithful against tanhl / expl in long double (the result is one of
//                                         the two float32 that bracket the true value), monotone (non-decreasing on the
//                                         positive side, non-increasing in the magnitude on the negative side, f(-0) <= f(+0);
//                                         the first step is taken from the float below LO, so adjacent ranges leave no gap),
//                                         bounded (|tanh| <= 1, 0 <= sigmoid <= 1) and, for tanh, odd bit for bit.  Prints one
//                                         line of JSON with the counts, the maximum and mean error in float32 ulps, the input
//                                         of the maximum, the results that are not the correctly rounded float32, and the
//                                         smallest magnitudes in the range at which the result is 1 (at +x) and, for sigmoid,
//                                         0 (at -x); exit status 1 if a property fails.  Built -O2 without sanitizers.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "act_core.h"

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
    // the error in ulps of the float32 grid at `want`: the spacing of the bracket, or of the binade for an exact result
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

static int sweep(const char *fn, uint32_t lo, uint32_t hi, uint32_t stride) {
  const bool is_tanh = !strcmp(fn, "tanh");
  if ((!is_tanh && strcmp(fn, "sigmoid")) || hi > 0x7f7fffffu || lo > hi || stride < 1) {
    fprintf(stderr, "sweep: FN tanh or sigmoid, 0 <= LO <= HI <= 0x7f7fffff, STRIDE >= 1\n");
    return 2;
  }
  Tally t;
  unsigned long long drops = 0, not_odd = 0, out_of_bounds = 0;
  uint32_t one_from = 0, zero_from = 0;
  bool have_one = false, have_zero = false;
  float prev_p = -INFINITY, prev_n = INFINITY;
  if (lo > 0) {
    prev_p = is_tanh ? lh_act_tanh(from_bits(lo - 1)) : lh_act_sigmoid(from_bits(lo - 1));
    prev_n = is_tanh ? lh_act_tanh(from_bits((lo - 1) | 0x80000000u)) : lh_act_sigmoid(from_bits((lo - 1) | 0x80000000u));
  }
  for (uint64_t b = lo; b <= hi; b += stride) {
    const float xp = from_bits((uint32_t)b), xn = from_bits((uint32_t)b | 0x80000000u);
    float gp, gn;
    long double wp, wn;
    if (is_tanh) {
      gp = lh_act_tanh(xp);
      gn = lh_act_tanh(xn);
      wp = tanhl((long double)xp);
      wn = -wp;
      if (bits_of(gn) != (bits_of(gp) ^ 0x80000000u)) not_odd++;
      if (!(fabsf(gp) <= 1.0f) || !(fabsf(gn) <= 1.0f)) out_of_bounds++;
    } else {
      gp = lh_act_sigmoid(xp);
      gn = lh_act_sigmoid(xn);
      const long double e = expl((long double)xn);  // e^-|x|
      wp = 1.0L / (1.0L + e);
      wn = e / (1.0L + e);
      if (!(gp >= 0.0f && gp <= 1.0f) || !(gn >= 0.0f && gn <= 1.0f)) out_of_bounds++;
      if (!have_zero && gn == 0.0f) {
        have_zero = true;
        zero_from = (uint32_t)b | 0x80000000u;
      }
    }
    if (!have_one && gp == 1.0f) {
      have_one = true;
      one_from = (uint32_t)b;
    }
    t.add((uint32_t)b, gp, wp);
    t.add((uint32_t)b | 0x80000000u, gn, wn);
    if (!(gp >= prev_p)) drops++;
    if (!(gn <= prev_n)) drops++;
    if (b == 0 && !(gn <= gp)) drops++;
    prev_p = gp;
    prev_n = gn;
  }
  printf("{\"fn\": \"%s\", \"lo\": \"0x%08x\", \"hi\": \"0x%08x\", \"stride\": %u, \"count\": %llu, \"unfaithful\": %llu, "
         "\"first_unfaithful\": \"0x%08x\", \"not_monotone\": %llu, \"not_odd\": %llu, \"out_of_bounds\": %llu, \"not_nearest\": %llu, "
         "\"max_ulp\": %.6Lf, \"max_at\": \"0x%08x\", \"mean_ulp\": %.6Lf, \"one_from\": \"0x%08x\", \"zero_from\": \"0x%08x\"}\n",
         fn, lo, hi, stride, t.count, t.unfaithful, t.first_bad, drops, not_odd, out_of_bounds, t.inexact, t.max_err, t.max_at,
         t.sum_err / (long double)t.count, one_from, zero_from);
  return t.unfaithful || drops || not_odd || out_of_bounds ? 1 : 0;
}

int main(int argc, char **argv) {
  if (argc == 6 && !strcmp(argv[1], "sweep"))
    return sweep(argv[2], (uint32_t)strtoul(argv[3], nullptr, 0), (uint32_t)strtoul(argv[4], nullptr, 0),
                 (uint32_t)strtoul(argv[5], nullptr, 0));
  if (argc != 1) {
    fprintf(stderr, "usage: %s [sweep tanh|sigmoid LO HI STRIDE]\n", argv[0]);
    return 2;
  }
  std::vector<float> in;
  float buf[4096];
  size_t got;
  while ((got = fread(buf, sizeof(float), 4096, stdin)) > 0) in.insert(in.end(), buf, buf + got);
  struct Rec {
    uint32_t t, s;
    uint64_t e, p;
  };
  static_assert(sizeof(Rec) == 24, "record layout");
  std::vector<Rec> out(in.size());
  for (size_t i = 0; i < in.size(); i++) {
    const float x = in[i];
    const double a = x != x ? 0.0 : fabs((double)x);
    out[i].t = bits_of(lh_act_tanh(x));
    out[i].s = bits_of(lh_act_sigmoid(x));
    out[i].e = bits_of64(lh_act_exp(-(a < 208.0 ? a : 208.0)));
    out[i].p = bits_of64(lh_act_tanh_small(a < 0x1p-6 ? a : 0x1p-6));
  }
  if (fwrite(out.data(), sizeof(Rec), out.size(), stdout) != out.size()) return 1;
  return 0;
}
