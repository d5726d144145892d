// tests/cpp/select_mirror.cpp -- a translation unit that calls the row-selection additions of include/laser.hpp
// (tests/test_select_cpu.py compiles it; with a device it runs and checks the results against plain loops).
#include <cstdio>
#include <cstring>
#include <vector>

#include "laser.hpp"

static uint32_t key_of(float x) {
  uint32_t b;
  std::memcpy(&b, &x, 4);
  return (b & 0x80000000u) ? b ^ 0xFFFFFFFFu : b ^ 0x80000000u;
}

int main() {
  const int64_t rows = 3, n = 300, k = 7;
  std::vector<float> h((size_t)(rows * n));
  for (size_t i = 0; i < h.size(); i++) h[i] = (float)((i * 37 + 11) % 101) - 50.0f;      // many ties
  try {
    laser::Tensor<float> x = laser::newTensor<float>({rows, n});
    laser::copyFromRaw(x, h.data(), rows * n);
    laser::TopkResult r = laser::topk(x, k);
    laser::Tensor<int32_t> am = laser::argmax(x), an = laser::argmin(x);
    laser::Tensor<int32_t> back = laser::take_rows(r.indices, laser::newTensor<int32_t>({rows, 2}));
    laser::Rng rng(3);
    laser::Tensor<int32_t> ids = laser::sample_top_k(x, k, rng, 4);
    const std::vector<int32_t> idx = r.indices.to_host(), a = am.to_host(), b = an.to_host(), t = back.to_host(), s = ids.to_host();
    for (int64_t row = 0; row < rows; row++) {
      int64_t best = 0, worst = 0;
      for (int64_t j = 1; j < n; j++) {
        if (key_of(h[row * n + j]) > key_of(h[row * n + best])) best = j;
        if (key_of(h[row * n + j]) < key_of(h[row * n + worst])) worst = j;
      }
      if (a[row] != best || b[row] != worst || idx[row * k] != best || t[row * 2] != best || t[row * 2 + 1] != best) {
        std::printf("FAILED row %lld\n", (long long)row);
        return 1;
      }
      for (int c = 0; c < 4; c++) {
        bool among = false;
        for (int64_t i = 0; i < k; i++) among = among || s[row * 4 + c] == idx[row * k + i];
        if (!among) {
          std::printf("FAILED draw row %lld\n", (long long)row);
          return 1;
        }
      }
    }
  } catch (const laser::Error &e) {
    std::printf("laser::Error %d: %s\n", e.code, e.what());
    return e.code == LASER_HIP_E_NODEVICE ? 3 : 1;
  }
  std::printf("SUCCESS\n");
  return 0;
}
