// tests/cpp/embedding_mirror.cpp -- laser::embedding, laser::embedding_group and laser::embedding_backward from a compiled
// C++ caller (include/laser.hpp).  The gather against a bit copy on the host (-1: +0, any other id outside [0, vocab): quiet
// NaN), the grouping against std::stable_sort of the positions by key, and the gradient against the sum tree of
// include/laser_hip.h "Dense-layer backward" written out here in terms of the occurrence index (built with
// -ffp-contract=off), over ids of none, one, a few, a few hundred and more than 8192 occurrences; the pre-grouped form; a
// refused shape.  Prints SUCCESS.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "laser.hpp"

static int fails = 0;
static void expect(const char *what, bool ok) {
  if (!ok) {
    std::printf("FAIL %s\n", what);
    fails++;
  }
}
static bool same(float a, float b) { return (a != a && b != b) || std::memcmp(&a, &b, sizeof(float)) == 0; }

// the order of "Reductions" for a 1-D array of float32 (tests/cpp/dense_grad_mirror.cpp has the same function)
static float tree_sum(const std::vector<float> &x) {
  if (x.size() > 8192) {
    std::vector<float> parts;
    for (size_t at = 0; at < x.size(); at += 8192)
      parts.push_back(tree_sum(std::vector<float>(x.begin() + at, x.begin() + std::min(x.size(), at + 8192))));
    return tree_sum(parts);
  }
  float leaf[1024];
  for (int a = 0; a < 1024; a++) leaf[a] = 0.0f;
  for (size_t k = 0; k < x.size(); k++) leaf[k % 1024] = leaf[k % 1024] + x[k];
  const int bits[10] = {1, 0, 9, 8, 7, 6, 5, 4, 3, 2};
  for (int b : bits)
    for (int a = 0; a < 1024; a++)
      if (!(a >> b & 1)) leaf[a] = leaf[a] + leaf[a | 1 << b];
  return leaf[0];
}

int main() {
  const int64_t tokens = 10500, vocab = 300, dim = 10;
  std::vector<int32_t> idx((size_t)tokens);
  std::vector<float> w((size_t)(vocab * dim)), dy((size_t)(tokens * dim));
  for (int64_t t = 0; t < tokens; t++) {
    // id 0 more than 8192 times, id 1 a few hundred times, the others a few times or never; some invalid ids
    idx[t] = t % 11 == 3 ? 1 : t % 13 == 5 ? (int32_t)(2 + (t * 7919) % 250) : 0;
    if (t % 101 == 7) idx[t] = -1;
    if (t % 211 == 9) idx[t] = (int32_t)vocab;
    if (t % 307 == 11) idx[t] = -2;
  }
  for (size_t i = 0; i < w.size(); i++) w[i] = (float)((i * 104729) % 2003) / 97.0f - 10.0f;
  w[3] = -0.0f;
  for (size_t i = 0; i < dy.size(); i++) dy[i] = ((float)((i * 7919) % 4001) - 2000.0f) * (float)(1 << (i % 13)) / 4096.0f;
  auto tw = laser::newTensor<float>({vocab, dim}), tdy = laser::newTensor<float>({tokens, dim});
  auto tidx = laser::newTensor<int32_t>({tokens});
  laser::copyFromRaw(tw, w.data(), vocab * dim);
  laser::copyFromRaw(tdy, dy.data(), tokens * dim);
  laser::copyFromRaw(tidx, idx.data(), tokens);

  {  // the gather
    const std::vector<float> y = laser::embedding(tw, tidx).to_host();
    bool ok = y.size() == (size_t)(tokens * dim);
    for (int64_t t = 0; ok && t < tokens; t++)
      for (int64_t j = 0; j < dim; j++) {
        uint32_t want = idx[t] == -1 ? 0u : 0x7fc00000u, got;
        if (idx[t] >= 0 && idx[t] < vocab) std::memcpy(&want, &w[(size_t)(idx[t] * dim + j)], 4);
        std::memcpy(&got, &y[(size_t)(t * dim + j)], 4);
        ok = ok && got == want;
      }
    expect("embedding is a bit copy, +0 for -1 and quiet NaN for a wrong id", ok);
  }

  // the grouping: positions sorted by (key, position)
  auto key = [&](int32_t t) { return idx[t] >= 0 && idx[t] < vocab ? (int64_t)idx[t] : vocab; };
  std::vector<int32_t> order((size_t)tokens), starts((size_t)(vocab + 1), 0);
  for (int64_t t = 0; t < tokens; t++) order[t] = (int32_t)t;
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return key(a) < key(b); });
  for (int64_t t = 0; t < tokens; t++)
    for (int64_t v = key((int32_t)t) + 1; v <= vocab; v++) starts[v]++;
  const laser::EmbeddingGroup g = laser::embedding_group(tidx, vocab);
  expect("order is the stable sort of the positions by key", g.order.to_host() == order);
  expect("starts counts the valid tokens below every id", g.starts.to_host() == starts);

  // the gradient
  std::vector<float> want((size_t)(vocab * dim));
  for (int64_t v = 0; v < vocab; v++)
    for (int64_t j = 0; j < dim; j++) {
      std::vector<float> a;
      for (int32_t k = starts[v]; k < starts[v + 1]; k++) a.push_back(dy[(size_t)(order[k] * dim + j)]);
      want[(size_t)(v * dim + j)] = tree_sum(a);
    }
  expect("the ids cover none, a few, a few hundred and more than 8192 occurrences",
         starts[1] - starts[0] > 8192 && starts[2] - starts[1] > 300 && starts[2] - starts[1] <= 8192 && starts[vocab] < tokens);
  const std::vector<float> dw = laser::embedding_backward(tdy, tidx, vocab).to_host();
  bool ok = dw.size() == want.size();
  for (size_t i = 0; ok && i < dw.size(); i++) ok = same(dw[i], want[i]);
  expect("dw is the stated sum tree of every id's occurrences in token order, bit for bit", ok);
  const std::vector<float> dw2 = laser::embedding_backward(tdy, tidx, vocab, &g).to_host();
  expect("a group given has the same bits", dw2.size() == dw.size() && std::memcmp(dw2.data(), dw.data(), dw.size() * sizeof(float)) == 0);

  bool threw = false;
  try {
    auto y = laser::newTensor<float>({tokens, dim + 1});
    laser::embedding(y, tw, tidx);  // y of another width
  } catch (const laser::Error &) {
    threw = true;
  }
  expect("a destination of another shape is refused", threw);

  if (fails == 0) std::printf("SUCCESS\n");
  return fails ? 1 : 0;
}
