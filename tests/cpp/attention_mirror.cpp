// tests/cpp/attention_mirror.cpp -- laser::attention, laser::softmax_backward and laser::attention_backward from a compiled
// C++ caller (include/laser.hpp), against the contract of include/laser_hip.h "Attention" and "Softmax gradient":
//   the fused forward equals the composition gemm_strided (alpha = scale) + laser::softmax + gemm_strided on the device, +0 and
//     -0 taken as equal, at Tk = 1025 (two P V slices) and d = 65; its row sums are the sums of e = P * s in the tree order;
//   softmax_backward is the stated float32 operations written out here (built with -ffp-contract=off) with the sum tree of
//     "Reductions" in terms of the index, at n = 1025 and n = 8197;
//   attention_backward's dV is the fmaf chain of P^T dO, dQ and dK are the chains of dS with K and Q times scale, dS from the
//     rule above; causal with Tq > Tk is refused.
// Prints SUCCESS.
#include <cmath>
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
static bool same(const std::vector<float> &a, const std::vector<float> &b, bool zeros_equal = false) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); i++) {
    if (a[i] != a[i] && b[i] != b[i]) continue;
    if (zeros_equal && a[i] == 0.0f && b[i] == 0.0f) continue;
    if (std::memcmp(&a[i], &b[i], sizeof(float)) != 0) return false;
  }
  return true;
}

// the order of "Reductions" for a 1-D array of float32 (tests/cpp/optim_mirror.cpp has the same function)
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

static std::vector<float> fill(size_t n, int seed) {
  std::vector<float> x(n);
  for (size_t i = 0; i < n; i++) x[i] = (float)((long long)((i + 17) * 104729 + seed * 7919) % 2003 - 1001) / 1001.0f;
  return x;
}
static laser::Tensor<float> upload(std::initializer_list<int64_t> shape, const std::vector<float> &x) {
  laser::Tensor<float> t = laser::newTensor<float>(shape);
  if (!x.empty()) laser::copyFromRaw(t, x.data(), (int64_t)x.size());
  return t;
}
// alpha * (the k-ascending fmaf chain of a (M, K <= 512) and b (K, N)), row-major
static std::vector<float> chain(const std::vector<float> &a, const std::vector<float> &b, int M, int N, int K, float alpha, bool ta, bool tb) {
  std::vector<float> c((size_t)M * N);
  for (int i = 0; i < M; i++)
    for (int j = 0; j < N; j++) {
      float acc = 0.0f;
      for (int k = 0; k < K; k++) acc = std::fmaf(ta ? a[(size_t)k * M + i] : a[(size_t)i * K + k], tb ? b[(size_t)j * K + k] : b[(size_t)k * N + j], acc);
      c[(size_t)i * N + j] = alpha == 1.0f ? acc : alpha * acc;
    }
  return c;
}

int main() {
  // ---- the fused forward against the composition on the device ----
  {
    const int64_t tq = 40, tk = 1025, d = 65, dv = 33;
    const float scale = laser::attention_default_scale(d);
    const std::vector<float> q = fill(tq * d, 1), k = fill(tk * d, 2), v = fill(tk * dv, 3);
    laser::Tensor<float> tq_ = upload({1, tq, d}, q), tk_ = upload({1, tk, d}, k), tv_ = upload({1, tk, dv}, v);
    const laser::AttentionResult f = laser::attention(tq_, tk_, tv_, scale, false, true, true);
    laser::Tensor<float> s = laser::newTensor<float>({tq, tk}), o = laser::newTensor<float>({tq, dv});
    laser::gemm_strided_dev<float>(tq, tk, d, scale, tq_.unsafe_raw_data(), d, 1, tk_.unsafe_raw_data(), 1, d, 0.0f, s.unsafe_raw_data(), tk, 1, nullptr);
    laser::Tensor<float> p = laser::softmax(s);
    laser::gemm_strided_dev<float>(tq, dv, tk, 1.0f, p.unsafe_raw_data(), tk, 1, tv_.unsafe_raw_data(), dv, 1, 0.0f, o.unsafe_raw_data(), dv, 1, nullptr);
    expect("P of the fused kernel is the composition's", same(f.probs.to_host(), p.to_host(), true));
    expect("O of the fused kernel is the composition's", same(f.out.to_host(), o.to_host(), true));
    const std::vector<float> ph = f.probs.to_host(), sums = f.row_sum.to_host(), oh = f.out.to_host();
    const laser::AttentionResult only = laser::attention(tq_, tk_, tv_, scale);
    expect("O alone has the same bits", same(only.out.to_host(), oh) && !only.probs.storage);
    bool ok = sums.size() == (size_t)tq;
    for (int64_t i = 0; ok && i < tq; i++) {
      float total = 0.0f;
      for (int64_t j = 0; j < tk; j++) total += ph[i * tk + j];
      ok = sums[i] >= 1.0f && std::fabs(total - 1.0f) < 1e-4f;
    }
    expect("row sums are at least 1 and the rows of P sum to 1", ok);
    // causal: row i of P is +0 past i + (Tk - Tq) + 1
    const laser::AttentionResult c = laser::attention(tq_, tk_, tv_, scale, true, true);
    const std::vector<float> pc = c.probs.to_host();
    ok = true;
    for (int64_t i = 0; i < tq; i++)
      for (int64_t j = 0; j < tk; j++) {
        const bool seen = j < i + (tk - tq) + 1;
        uint32_t bits;
        std::memcpy(&bits, &pc[i * tk + j], 4);
        ok = ok && (seen ? pc[i * tk + j] > 0.0f : bits == 0u);
      }
    expect("causal P is positive on the visible keys and +0 on the masked ones", ok);
  }
  // ---- softmax_backward ----
  for (int64_t n : {1025, 8197}) {
    const int64_t rows = 3;
    std::vector<float> y = fill(rows * n, 4), dy = fill(rows * n, 5), want((size_t)(rows * n));
    for (float &e : y) e = std::fabs(e) / (float)n;
    for (int64_t r = 0; r < rows; r++) {
      std::vector<float> prod((size_t)n);
      for (int64_t j = 0; j < n; j++) prod[j] = dy[r * n + j] * y[r * n + j];
      const float D = tree_sum(prod);
      for (int64_t j = 0; j < n; j++) {
        const float t = dy[r * n + j] - D;
        want[r * n + j] = y[r * n + j] * t;
      }
    }
    laser::Tensor<float> ty = upload({rows, n}, y), tdy = upload({rows, n}, dy);
    expect("softmax_backward is the stated operations in the stated order", same(laser::softmax_backward(tdy, ty).to_host(), want));
    laser::softmax_backward(tdy, tdy, ty);
    expect("softmax_backward in place on dy", same(tdy.to_host(), want));
  }
  // ---- attention_backward ----
  {
    const int64_t b = 2, tq = 33, tk = 65, d = 5, dv = 7;
    const float scale = 0.375f;
    const std::vector<float> q = fill(b * tq * d, 6), k = fill(b * tk * d, 7), v = fill(b * tk * dv, 8), dout = fill(b * tq * dv, 9);
    laser::Tensor<float> tq_ = upload({b, tq, d}, q), tk_ = upload({b, tk, d}, k), tv_ = upload({b, tk, dv}, v), td = upload({b, tq, dv}, dout);
    for (int causal = 0; causal < 2; causal++) {
      const std::vector<float> p = laser::attention(tq_, tk_, tv_, scale, causal != 0, true, false, false).probs.to_host();
      const laser::AttentionGrads g = laser::attention_backward(td, tq_, tk_, tv_, scale, causal != 0);
      std::vector<float> wq, wk, wv;
      for (int64_t s = 0; s < b; s++) {
        const std::vector<float> ps(p.begin() + s * tq * tk, p.begin() + (s + 1) * tq * tk), dos(dout.begin() + s * tq * dv, dout.begin() + (s + 1) * tq * dv);
        const std::vector<float> qs(q.begin() + s * tq * d, q.begin() + (s + 1) * tq * d), ks(k.begin() + s * tk * d, k.begin() + (s + 1) * tk * d);
        const std::vector<float> vs(v.begin() + s * tk * dv, v.begin() + (s + 1) * tk * dv);
        const std::vector<float> dvs = chain(ps, dos, (int)tk, (int)dv, (int)tq, 1.0f, true, false);
        std::vector<float> ds = chain(dos, vs, (int)tq, (int)tk, (int)dv, 1.0f, false, true);
        for (int64_t i = 0; i < tq; i++) {
          std::vector<float> prod((size_t)tk);
          for (int64_t j = 0; j < tk; j++) prod[j] = ds[i * tk + j] * ps[i * tk + j];
          const float D = tree_sum(prod);
          for (int64_t j = 0; j < tk; j++) {
            const float t = ds[i * tk + j] - D;
            ds[i * tk + j] = ps[i * tk + j] * t;
          }
        }
        const std::vector<float> dqs = chain(ds, ks, (int)tq, (int)d, (int)tk, scale, false, false), dks = chain(ds, qs, (int)tk, (int)d, (int)tq, scale, true, false);
        wq.insert(wq.end(), dqs.begin(), dqs.end()), wk.insert(wk.end(), dks.begin(), dks.end()), wv.insert(wv.end(), dvs.begin(), dvs.end());
      }
      expect("dV is the chain of P^T dO", same(g.dv.to_host(), wv, true));
      expect("dQ is scale times the chain of dS K", same(g.dq.to_host(), wq, true));
      expect("dK is scale times the chain of dS^T Q", same(g.dk.to_host(), wk, true));
      const laser::AttentionGrads gk = laser::attention_backward(td, tq_, tk_, tv_, scale, causal != 0, false, true, false);
      expect("dK alone has the same bits", same(gk.dk.to_host(), g.dk.to_host()) && !gk.dq.storage && !gk.dv.storage);
    }
    bool threw = false;
    try {
      laser::attention(tk_, tq_, td, scale, true);  // Tq = 65 > Tk = 33
    } catch (const laser::Error &) {
      threw = true;
    }
    expect("causal with Tq > Tk is refused", threw);
  }
  if (fails == 0) std::printf("SUCCESS\n");
  return fails ? 1 : 0;
}
