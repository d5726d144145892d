// tests/cpp/exp_core_host.cpp -- laser_amd/csrc/exp_core.h as a host program: reads float32 values from standard input and
// writes the bits of lexp of each to standard output.  tests/test_exp_cpu.py builds it with
// g++ -ffp-contract=off -fsanitize=undefined,address and compares the output with the numpy model bit for bit.
#include <cstdio>
#include <vector>

#include "exp_core.h"

int main() {
  std::vector<float> in;
  float buf[4096];
  size_t got;
  while ((got = fread(buf, sizeof(float), 4096, stdin)) > 0) in.insert(in.end(), buf, buf + got);
  std::vector<float> out(in.size());
  for (size_t i = 0; i < in.size(); i++) out[i] = lh_exp(in[i]);
  if (fwrite(out.data(), sizeof(float), out.size(), stdout) != out.size()) return 1;
  return 0;
}
