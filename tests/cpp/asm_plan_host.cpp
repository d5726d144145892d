// tests/cpp/asm_plan_host.cpp -- the launch planner of the assembly kernels (laser_amd/csrc/asm_plan.h, asm_kernels.h, gemm_args.h) as
// a host program: g++ alone builds it (no HIP header, no library, no global behind the planner), under ASan and UBSan in
// tests/test_asm_plan_cpu.py, which feeds it the problem lines of scripts/plan_fingerprint.py and compares the answers with the
// recording in tests/golden/asm_plans_parent.json.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

#include "asm_plan.h"

using namespace laser_hip;

static bool choose(const GemmArgs<float> &a, bool laser_order, int cus, const AsmOptions &o, AsmChoice &c, int &group_m) {
  if (!choose_gemm_f32_asm(a, laser_order, cus, o, c)) return false;
  group_m = AsmFloat<float>::group_m(o, kKernels[c.pick]);
  return true;
}
static bool choose(const GemmArgs<double> &a, bool laser_order, int cus, const AsmOptions &o, AsmChoice &c, int &group_m) {
  if (!choose_gemm_f64_asm(a, laser_order, cus, o, c)) return false;
  group_m = AsmFloat<double>::group_m(o, kKernels[c.pick]);
  return true;
}
static bool classify(const GemmArgs<float> &a, bool laser_order, int cus, const AsmOptions &o, ConvClass &cc) { return conv_asm_classify(a, laser_order, cus, o, cc); }
static int64_t plan_cut(const GemmArgs<float> &a, bool laser_order, int cus, const AsmOptions &o) { return conv_plan_cut(a, laser_order, cus, o); }
static bool cuts_a_tile(int64_t T, int64_t P, int64_t G) { return plan_cuts_a_tile(T, P, G); }
static bool two_level(bool cuts, int64_t T, int64_t G) { return plan_two_level(cuts, T, G); }
static bool sched(SchedArgs &sc, int64_t tiles_m, int64_t tiles_n, int group_m, int64_t G, int64_t P, int64_t slice_len, bool xcd, bool two, int64_t T_cover,
                  const AsmOptions &o) {
  return fill_sched(sc, tiles_m, tiles_n, group_m, G, P, slice_len, 0, 0, xcd, two, o, T_cover);
}

// One problem per line of stdin, as name=value tokens; one answer line each.  t=f32 / f64: a GEMM (M N K batch nt lda ldb ldc csC beta
// bias rsBias csBias bsBias act preA preB bsA bsB bsC); t=conv / cut: a convolution's main launch / its pixel cut (M = output
// channels, Cin H W kH kW sH sW pH pW batch N coW alpha beta bias act); t=i32 / i64: the integer rows.  cus, laser and the options
// (plan kernel tile wgs slice group_m split_tail f32_asm f64_asm conv_walk noseed giveup) on any line.
struct Line {
  std::map<std::string, long long> v;
  std::string t;
  long long get(const char *k, long long def) const {
    const auto it = v.find(k);
    return it == v.end() ? def : it->second;
  }
};

static bool parse(char *s, Line &ln) {
  for (char *tok = std::strtok(s, " \t\r\n"); tok; tok = std::strtok(nullptr, " \t\r\n")) {
    char *eq = std::strchr(tok, '=');
    if (!eq) return false;
    *eq = 0;
    if (std::strcmp(tok, "t") == 0) ln.t = eq + 1;
    else ln.v[tok] = std::strtoll(eq + 1, nullptr, 0);
  }
  return !ln.t.empty();
}

static AsmOptions options_of(const Line &ln) {
  AsmOptions o;
  o.asm_plan = (int)ln.get("plan", o.asm_plan); o.asm_kernel = (int)ln.get("kernel", o.asm_kernel); o.asm_tile = (int)ln.get("tile", o.asm_tile);
  o.asm_wgs = (int)ln.get("wgs", o.asm_wgs); o.asm_slice = (int)ln.get("slice", o.asm_slice); o.asm_group_m = (int)ln.get("group_m", o.asm_group_m);
  o.split_tail = (int)ln.get("split_tail", o.split_tail); o.f32_asm = (int)ln.get("f32_asm", o.f32_asm); o.f64_asm = (int)ln.get("f64_asm", o.f64_asm);
  o.conv_walk = (int)ln.get("conv_walk", o.conv_walk); o.asm_noseed = (int)ln.get("noseed", o.asm_noseed); o.asm_test_giveup = (int)ln.get("giveup", o.asm_test_giveup);
  return o;
}

// the first 64 bytes of the scheduler block (everything but the workspace and flag addresses, which are 0 here)
static void print_sched(const char *name, bool ok, const SchedArgs &sc) {
  if (!ok) {
    std::printf(" %s=refused", name);
    return;
  }
  unsigned char b[64];
  std::memcpy(b, &sc, 64);
  std::printf(" %s=", name);
  for (int i = 0; i < 64; i++) std::printf("%02x", b[i]);
  if (sc.ws != 0 || sc.flags != 0) std::printf("!addr");
}

// the scheduler blocks launch_planned fills for this plan
static void print_plan_sched(const Plan &plan, int tiles_m, int tiles_n, int group_m, const AsmOptions &o) {
  const int64_t T = (int64_t)tiles_m * tiles_n;
  SchedArgs sc;
  if (plan.strided && plan.rem_tiles > 0) {
    const int64_t R = plan.rem_tiles, T1 = T - R, G2 = plan.rem_G, P2 = plan.rem_P;
    const bool cuts2 = cuts_a_tile(R, P2, G2), two2 = two_level(cuts2, R, G2);
    std::memset(&sc, 0, sizeof sc);
    print_sched("sched2", sched(sc, tiles_m, tiles_n, group_m, G2, P2, plan.rem_slice_len, group_m > 0 && (!cuts2 || two2), two2, R, o), sc);
    std::memset(&sc, 0, sizeof sc);
    print_sched("sched", sched(sc, tiles_m, tiles_n, group_m, plan.G, 1, plan.slice_len, group_m > 0, false, T1, o), sc);
    return;
  }
  const bool cuts = plan.persistent && !plan.strided && cuts_a_tile(T, plan.P, plan.G), two = two_level(cuts, T, plan.G);
  std::memset(&sc, 0, sizeof sc);
  print_sched("sched", sched(sc, tiles_m, tiles_n, group_m, plan.G, plan.P, plan.slice_len, group_m > 0 && (!cuts || two), two, 0, o), sc);
  std::printf(" cuts=%d two=%d", (int)cuts, (int)two);
}

template <typename T>
static void gemm_line(const Line &ln) {
  GemmArgs<T> a;
  std::memset(&a, 0, sizeof a);
  a.M = ln.get("M", 0); a.N = ln.get("N", 0); a.K = ln.get("K", 0);
  a.alpha = (T)ln.get("alpha", 1); a.beta = (T)ln.get("beta", 0);
  a.batch = (int32_t)ln.get("batch", 1);
  const bool nt = ln.get("nt", 0) != 0;
  a.rsA = ln.get("lda", a.K); a.csA = ln.get("csA", 1);
  const long long ldb = ln.get("ldb", nt ? a.K : a.N);
  a.rsB = nt ? 1 : ldb; a.csB = nt ? ldb : 1;
  a.csC = ln.get("csC", 1); a.rsC = ln.get("ldc", (a.N - 1) * a.csC + 1);
  a.Mext = ln.get("Mext", a.M); a.Next = ln.get("Next", a.N); a.Kext = ln.get("Kext", a.K);
  a.bsA = ln.get("bsA", a.M * a.rsA); a.bsB = ln.get("bsB", (nt ? a.N : a.K) * ldb); a.bsC = ln.get("bsC", a.M * a.rsC);
  a.bias = ln.get("bias", 0) ? (const T *)(uintptr_t)64 : nullptr;
  a.rsBias = ln.get("rsBias", 0); a.csBias = ln.get("csBias", 1); a.bsBias = ln.get("bsBias", 0);
  a.act = (int32_t)ln.get("act", 0); a.preA = (int32_t)ln.get("preA", 0); a.preB = (int32_t)ln.get("preB", 0);
  a.col0 = ln.get("col0", 0);
  const AsmOptions o = options_of(ln);
  AsmChoice c;
  int group_m = 0;
  if (!choose(a, ln.get("laser", 1) != 0, (int)ln.get("cus", 256), o, c, group_m)) {
    std::printf("pick=-1\n");
    return;
  }
  const Plan &p = c.plan;
  std::printf("pick=%d %s plan=%s G=%lld P=%lld slice=%lld rem=%lld,%lld,%lld,%lld us=%a exact=%d nt=%d ldb=%lld tiles=%dx%d group_m=%d", c.pick, kKernels[c.pick].symbol,
              p.strided ? (p.rem_tiles > 0 ? "hybrid" : "strided") : p.persistent ? "cut" : "plain", (long long)p.G, (long long)p.P, (long long)p.slice_len,
              (long long)p.rem_tiles, (long long)p.rem_G, (long long)p.rem_P, (long long)p.rem_slice_len, p.time_us, (int)c.exact, (int)c.nt, (long long)c.ldb,
              c.tiles_m, c.tiles_n, group_m);
  print_plan_sched(p, c.tiles_m, c.tiles_n, group_m, o);
  std::printf("\n");
}

static void conv_line(const Line &ln, bool cut) {
  GemmArgs<float> a;
  std::memset(&a, 0, sizeof a);
  const long long Cin = ln.get("Cin", 1), kH = ln.get("kH", 1), kW = ln.get("kW", 1), sH = ln.get("sH", 1), sW = ln.get("sW", 1), pH = ln.get("pH", 0), pW = ln.get("pW", 0);
  const long long H = ln.get("H", 1), W = ln.get("W", 1);
  const long long oH = sH > 0 && H + 2 * pH >= kH ? (H + 2 * pH - kH) / sH + 1 : 0, oW = sW > 0 && W + 2 * pW >= kW ? (W + 2 * pW - kW) / sW + 1 : 0, npix = oH * oW;
  a.M = ln.get("M", 0); a.N = ln.get("N", npix); a.K = Cin * kH * kW;
  a.alpha = (float)ln.get("alpha", 1); a.beta = (float)ln.get("beta", 0);
  a.batch = (int32_t)ln.get("batch", 1);
  a.rsA = a.K; a.csA = 1; a.rsC = npix; a.csC = 1;
  a.bsB = Cin * H * W; a.bsC = a.M * npix;
  a.Mext = a.M; a.Next = a.N; a.Kext = a.K;
  a.cH = (int32_t)H; a.cW = (int32_t)W; a.ckH = (int32_t)kH; a.ckW = (int32_t)kW; a.coW = (int32_t)ln.get("coW", oW);
  a.cpH = (int32_t)pH; a.cpW = (int32_t)pW; a.csH = (int32_t)sH; a.csW = (int32_t)sW;
  a.bias = ln.get("bias", 0) ? (const float *)(uintptr_t)64 : nullptr;
  a.rsBias = ln.get("rsBias", 1); a.csBias = ln.get("csBias", 0); a.bsBias = ln.get("bsBias", 0);
  a.act = (int32_t)ln.get("act", 0);
  const AsmOptions o = options_of(ln);
  const bool laser = ln.get("laser", 1) != 0;
  const int cus = (int)ln.get("cus", 256);
  if (cut) {
    std::printf("cut=%lld\n", (long long)plan_cut(a, laser, cus, o));
    return;
  }
  ConvClass cc;
  if (!classify(a, laser, cus, o, cc)) {
    std::printf("pick=-1\n");
    return;
  }
  std::printf("pick=%d walker=%d %s tiles=%dx%d=%lld k=%lldx%lld s=%lldx%lld taps=%lld o=%lldx%lld npix=%lld Cin=%lld Kp=%lld exact=%d", cc.pick, cc.walker, kKernels[cc.pick].symbol,
              cc.tiles_m, cc.tiles_n, (long long)cc.tiles, (long long)cc.kH, (long long)cc.kW, (long long)cc.sH, (long long)cc.sW, (long long)cc.taps, (long long)cc.oH,
              (long long)cc.oW, (long long)cc.npix, (long long)cc.Cin, (long long)cc.Kp, (int)cc.exact);
  Plan plain;      // (launch_conv_f32_asm: one tile per workgroup, plain order of the tile ids)
  plain.G = cc.tiles;
  print_plan_sched(plain, cc.tiles_m, cc.tiles_n, 0, o);
  std::printf("\n");
}

int main() {
  static char buf[4096];
  while (std::fgets(buf, sizeof buf, stdin)) {
    Line ln;
    if (!parse(buf, ln)) {
      std::fprintf(stderr, "bad line\n");
      return 2;
    }
    if (ln.t == "f32") gemm_line<float>(ln);
    else if (ln.t == "f64") gemm_line<double>(ln);
    else if (ln.t == "conv") conv_line(ln, false);
    else if (ln.t == "cut") conv_line(ln, true);
    else if (ln.t == "i32") std::printf("row=%d %s\n", kI32Row, kKernels[kI32Row].symbol);
    else if (ln.t == "i64") std::printf("row=%d %s\n", kI64Row, kKernels[kI64Row].symbol);
    else {
      std::fprintf(stderr, "bad t=%s\n", ln.t.c_str());
      return 2;
    }
  }
  return 0;
}
