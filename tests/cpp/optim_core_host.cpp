// tests/cpp/optim_core_host.cpp -- laser_amd/csrc/optim_core.h compiled for the host (no HIP; -ffp-contract=off, since g++
// does not know the header's pragma): "optim_core_host in.bin out.bin" applies one rule to n elements.
//   in.bin:  int32 kind (0 SGD, 1 Adam, 2 norm and clip, 3 bias correction), int32 n, int32 flags (bit 0 nesterov / decoupled,
//            bit 1 a momentum value, bit 2 a clip factor), int32 pad, int64 step, float p[12], then w[n], g[n], m[n], v[n]
//            SGD p = lr, mu, wd, gscale, c;  Adam p = lr, b1, b2, eps, wd, bc1, bc2, gscale, c;  kind 2: p = total, max_norm;
//            kind 3: p = beta (and step)
//   out.bin: w[n], m[n], v[n]  (kind 2: norm, clip; kind 3: the correction)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "optim_core.h"

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  std::FILE *in = std::fopen(argv[1], "rb");
  if (!in) return 2;
  int32_t head[4];
  int64_t step;
  float p[12];
  if (std::fread(head, 4, 4, in) != 4 || std::fread(&step, 8, 1, in) != 1 || std::fread(p, 4, 12, in) != 12) return 2;
  const int kind = head[0], n = head[1], flags = head[2];
  std::vector<float> w((size_t)n), g((size_t)n), m((size_t)n), v((size_t)n);
  if (kind < 2)
    for (std::vector<float> *a : {&w, &g, &m, &v})
      if (n && std::fread(a->data(), 4, (size_t)n, in) != (size_t)n) return 2;
  std::fclose(in);
  std::FILE *out = std::fopen(argv[2], "wb");
  if (!out) return 2;
  if (kind == 0) {
    const lh_sgd_rule r = lh_sgd_rule_make(p[0], p[1], p[2], flags & 1, p[3], flags >> 1 & 1, flags >> 2 & 1);
    for (int i = 0; i < n; i++) lh_sgd_elem(r, p[4], w[i], g[i], m[i]);
  } else if (kind == 1) {
    const lh_adam_rule r = lh_adam_rule_make(p[0], p[1], p[2], p[3], p[4], flags & 1, p[5], p[6], p[7], flags >> 2 & 1);
    for (int i = 0; i < n; i++) lh_adam_elem(r, p[8], w[i], g[i], m[i], v[i]);
  } else if (kind == 2) {
    float r[2];
    lh_optim_clip(p[0], p[1], r[0], r[1]);
    std::fwrite(r, 4, 2, out);
  } else {
    const float r = lh_adam_bias_correction(p[0], step);
    std::fwrite(&r, 4, 1, out);
  }
  if (kind < 2)
    for (std::vector<float> *a : {&w, &m, &v})
      if (n) std::fwrite(a->data(), 4, (size_t)n, out);
  std::fclose(out);
  return 0;
}
