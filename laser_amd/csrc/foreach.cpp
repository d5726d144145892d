// laser_amd/csrc/foreach.cpp -- forEach with an arbitrary body (include/laser_hip.h, "forEach with a body"): the device twin
// of Laser's forEach macro (laser/strided_iteration/foreach.nim:192-264) for any number of operands of mixed element types.
//
// A spec (body, operand names / element types / writability, parameter names / types) becomes HIP source by filling the
// kernel template foreach_kernel.hip.in, which the Makefile embeds as a string.  hiprtc compiles it into a code object in
// the process; libhiprtc is dlopen'ed on first use, so liblaser_hip.so does not link it.  laser_hip_foreach_kernel loads the
// module once per (device, spec) and hands out a handle; laser_hip_foreach_dev merges dimensions, picks one of the
// template's three kernels (contiguous vectorised / contiguous scalar / strided) and launches it.
//
// forEachReduce (laser_hip_foreach_reduce_*) is the same machinery with an accumulator: its spec adds the accumulator's
// name and type and a merge statement, its source is forEach's prelude + exp_core.h + reduce_core.h + the spec + the kernels of
// foreach_reduce_kernel.hip.in, and laser_hip_foreach_reduce_dev runs the levels of reduce_levels (reduce.hip).  Its
// modules are cached under keys of their own and counted in foreach_compiles.
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/laser_hip.h"
#include "capi_internal.h"
#include "common.h"
#include "foreach_template.h"  // generated from foreach_kernel.hip.in, foreach_reduce_kernel.hip.in, reduce_core.h and
                                // exp_core.h, log_core.h, act_core.h, sincos_core.h: lh_foreach_template, lh_foreach_reduce_template, lh_reduce_core, lh_exp_core, lh_log_core, lh_act_core, lh_sincos_core

using namespace laser_hip;

namespace {

constexpr int kMaxOps = 8, kMaxParams = 8;
constexpr const char *kTypeName[] = {"float", "double", "int8_t", "int16_t", "int32_t", "int64_t",
                                     "uint8_t", "uint16_t", "uint32_t", "uint64_t"};
constexpr int kTypeSize[] = {4, 8, 1, 2, 4, 8, 1, 2, 4, 8};
constexpr int kNumTypes = 10;
constexpr const char *kKernelName[3] = {"lh_foreach_vector", "lh_foreach_scalar", "lh_foreach_strided"};
constexpr const char *kReduceKernelName[4] = {"lh_reduce_vector", "lh_reduce_scalar", "lh_reduce_strided", "lh_reduce_partials"};

std::atomic<int64_t> g_compiles{0};
std::atomic<int> g_last_variant{-1};

// ---- the spec ---------------------------------------------------------------------------------------------------------
struct Spec {
  std::string body;
  int nops = 0, nparams = 0;
  std::string names[kMaxOps], pnames[kMaxParams];
  int dtypes[kMaxOps] = {}, writable[kMaxOps] = {}, pdtypes[kMaxParams] = {};
  bool reduce = false;  // forEachReduce: the accumulator and its merge below
  std::string acc_name, merge;
  int acc_dtype = 0;
  std::string key() const {  // identifies the compiled module
    std::string k = reduce ? "reduce|" + acc_name + ':' + std::to_string(acc_dtype) + '\0' + merge + '\0' + body : body;
    k += '\0';
    for (int i = 0; i < nops; i++) k += names[i] + ':' + std::to_string(dtypes[i]) + (writable[i] ? "w," : "r,");
    k += '\0';
    for (int i = 0; i < nparams; i++) k += pnames[i] + ':' + std::to_string(pdtypes[i]) + ',';
    return k;
  }
  int vec() const {  // elements per lane of the vectorised kernel: 16 bytes of the widest operand
    int w = 1;
    for (int i = 0; i < nops; i++) w = std::max(w, kTypeSize[dtypes[i]]);
    return 16 / w;
  }
};

bool is_keyword(const std::string &s) {
  static const char *const kw[] = {
      "alignas", "alignof", "and", "and_eq", "asm", "auto", "bitand", "bitor", "bool", "break", "case", "catch", "char",
      "char8_t", "char16_t", "char32_t", "class", "compl", "concept", "const", "consteval", "constexpr", "constinit",
      "const_cast", "continue", "co_await", "co_return", "co_yield", "decltype", "default", "delete", "do", "double",
      "dynamic_cast", "else", "enum", "explicit", "export", "extern", "false", "float", "for", "friend", "goto", "if",
      "inline", "int", "long", "mutable", "namespace", "new", "noexcept", "not", "not_eq", "nullptr", "operator", "or",
      "or_eq", "private", "protected", "public", "register", "reinterpret_cast", "requires", "restrict", "return", "short",
      "signed", "sizeof", "static", "static_assert", "static_cast", "struct", "switch", "template", "this", "thread_local",
      "throw", "true", "try", "typedef", "typeid", "typename", "union", "unsigned", "using", "virtual", "void", "volatile",
      "wchar_t", "while", "xor", "xor_eq"};
  for (const char *k : kw)
    if (s == k) return true;
  return false;
}

int check_name(const char *what, int i, const char *name) {
  if (!name || !name[0]) return fail(LASER_HIP_E_INVALID, "foreach: %s %d has no name", what, i);
  const std::string s = name;
  bool ok = !(s[0] >= '0' && s[0] <= '9');
  for (char c : s) ok = ok && ((c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || (c >= '0' && c <= '9') || c == '_');
  if (!ok) return fail(LASER_HIP_E_INVALID, "foreach: %s name '%s' is not a C identifier", what, name);
  if (is_keyword(s)) return fail(LASER_HIP_E_INVALID, "foreach: %s name '%s' is a C++ keyword", what, name);
  if (s.rfind("lh_", 0) == 0 || s.rfind("__", 0) == 0)
    return fail(LASER_HIP_E_INVALID, "foreach: %s name '%s' is reserved (lh_ and __ prefixes)", what, name);
  if (s == "laser_exp") return fail(LASER_HIP_E_INVALID, "foreach: %s name 'laser_exp' is reserved (exp_core.h)", what);
  if (s == "laser_log") return fail(LASER_HIP_E_INVALID, "foreach: %s name 'laser_log' is reserved (log_core.h)", what);
  if (s == "laser_tanh" || s == "laser_sigmoid")
    return fail(LASER_HIP_E_INVALID, "foreach: %s name '%s' is reserved (act_core.h)", what, name);
  if (s == "laser_sin" || s == "laser_cos")
    return fail(LASER_HIP_E_INVALID, "foreach: %s name '%s' is reserved (sincos_core.h)", what, name);
  return LASER_HIP_OK;
}

int make_spec(Spec &sp, const char *body, int nops, const char *const *names, const int *dtypes, const int *writable,
              int nparams, const char *const *param_names, const int *param_dtypes) {
  if (!body) return fail(LASER_HIP_E_INVALID, "foreach: null body");
  if (nops < 1 || nops > kMaxOps) return fail(LASER_HIP_E_INVALID, "foreach: %d operands (1..%d)", nops, kMaxOps);
  if (nparams < 0 || nparams > kMaxParams)
    return fail(LASER_HIP_E_INVALID, "foreach: %d parameters (0..%d)", nparams, kMaxParams);
  if (!names || !dtypes || !writable || (nparams > 0 && (!param_names || !param_dtypes)))
    return fail(LASER_HIP_E_INVALID, "foreach: null spec array");
  sp.body = body;
  sp.nops = nops;
  sp.nparams = nparams;
  for (int i = 0; i < nops + nparams; i++) {
    const bool op = i < nops;
    const int j = op ? i : i - nops;
    const char *name = op ? names[j] : param_names[j];
    const int dt = op ? dtypes[j] : param_dtypes[j];
    if (int rc = check_name(op ? "operand" : "parameter", j, name)) return rc;
    if (dt < 0 || dt >= kNumTypes) return fail(LASER_HIP_E_INVALID, "foreach: '%s' has unknown element type %d", name, dt);
    for (int k = 0; k < i; k++)
      if ((k < nops ? sp.names[k] : sp.pnames[k - nops]) == name)
        return fail(LASER_HIP_E_INVALID, "foreach: name '%s' used twice", name);
    if (op) {
      sp.names[j] = name;
      sp.dtypes[j] = dt;
      sp.writable[j] = writable[j] != 0;
    } else {
      sp.pnames[j] = name;
      sp.pdtypes[j] = dt;
    }
  }
  return LASER_HIP_OK;
}

bool blank(const char *s) {
  for (; *s; s++)
    if (*s != ' ' && *s != '\t' && *s != '\n' && *s != '\r' && *s != ';') return false;
  return true;
}

// forEachReduce: forEach's spec plus the accumulator (name, type) and the merge statement over it and `other`
int make_reduce_spec(Spec &sp, const char *body, int nops, const char *const *names, const int *dtypes, const int *writable,
                     int nparams, const char *const *param_names, const int *param_dtypes, const char *acc_name, int acc_dtype,
                     const char *merge) {
  if (int rc = make_spec(sp, body, nops, names, dtypes, writable, nparams, param_names, param_dtypes)) return rc;
  if (int rc = check_name("accumulator", 0, acc_name)) return rc;
  if (acc_dtype < 0 || acc_dtype >= kNumTypes)
    return fail(LASER_HIP_E_INVALID, "foreach_reduce: accumulator '%s' has unknown element type %d", acc_name, acc_dtype);
  if (!merge || blank(merge)) return fail(LASER_HIP_E_INVALID, "foreach_reduce: empty merge");
  const std::string acc = acc_name;
  if (acc == "other") return fail(LASER_HIP_E_INVALID, "foreach_reduce: 'other' is the merge's reserved name");
  for (int i = 0; i < nops + nparams; i++) {
    const std::string &n = i < nops ? sp.names[i] : sp.pnames[i - nops];
    if (n == "other") return fail(LASER_HIP_E_INVALID, "foreach_reduce: 'other' is the merge's reserved name");
    if (n == acc) return fail(LASER_HIP_E_INVALID, "foreach_reduce: name '%s' used twice", acc_name);
  }
  sp.reduce = true;
  sp.acc_name = acc;
  sp.acc_dtype = acc_dtype;
  sp.merge = merge;
  return LASER_HIP_OK;
}

// ---- source generation ------------------------------------------------------------------------------------------------
std::string generate(const Spec &sp) {
  std::string s;
  auto t = [&](int k) { return "lh_t" + std::to_string(k); };
  auto v = [&](int k) { return "lh_v" + std::to_string(k); };
  auto vt = [&](int k) { return "lh_vec<" + t(k) + ", LH_E>"; };
  const std::string acc = sp.reduce ? "lh_acc" : "";  // forEachReduce: the accumulator, lh_body's first argument
  s += "#define LH_NOPS " + std::to_string(sp.nops) + "\n#define LH_E " + std::to_string(sp.vec()) + "\n";
  for (int k = 0; k < sp.nops; k++) s += "typedef " + std::string(kTypeName[sp.dtypes[k]]) + " " + t(k) + ";\n";
  if (sp.reduce)
    s += "typedef " + std::string(kTypeName[sp.acc_dtype]) + " lh_acc_t;\n#define LH_EA " +
         std::to_string(16 / kTypeSize[sp.acc_dtype]) + "\n";
  // the body: writable operands by reference, read-only operands and parameters as const copies
  s += "__device__ __forceinline__ void lh_body(";
  if (sp.reduce) s += "lh_acc_t &" + sp.acc_name + (sp.nops + sp.nparams ? ", " : "");
  for (int k = 0; k < sp.nops + sp.nparams; k++) {
    if (k) s += ", ";
    if (k < sp.nops)
      s += std::string(sp.writable[k] ? "" : "const ") + kTypeName[sp.dtypes[k]] + (sp.writable[k] ? " &" : " ") + sp.names[k];
    else
      s += std::string("const ") + kTypeName[sp.pdtypes[k - sp.nops]] + " " + sp.pnames[k - sp.nops];
  }
  s += ") {\n#line 1 \"body\"\n" + sp.body + "\n;\n}\n";
  if (sp.reduce)
    s += "__device__ __forceinline__ void lh_merge(lh_acc_t &" + sp.acc_name + ", const lh_acc_t other) {\n#line 1 \"merge\"\n" +
         sp.merge + "\n;\n}\n";
  const std::string tpl = lh_foreach_template, mark = "\n@LH_SPEC@\n";
  const size_t at = tpl.find(mark) + 1;
  // forEach's prelude, then lexp and llog (exp_core.h, log_core.h: laser_exp and laser_log for the bodies); forEachReduce:
  // then the order (reduce_core.h); then the spec and the kernels.  lsin and lcos (sincos_core.h: laser_sin, laser_cos) follow
  // act_core.h only when the body or the merge names one of them: no other kernel pays for compiling them
  const std::string text = sp.body + "\n" + sp.merge;
  const bool trig = text.find("laser_sin") != std::string::npos || text.find("laser_cos") != std::string::npos ||
                    text.find("lh_sin") != std::string::npos || text.find("lh_cos") != std::string::npos ||
                    text.find("lh_sc_") != std::string::npos;
  const std::string head = tpl.substr(0, at) + lh_exp_core + lh_log_core + lh_act_core + (trig ? std::string(lh_sincos_core) : std::string()) +
                           (sp.reduce ? std::string(lh_reduce_core) : std::string());
  // the lines after the body report their line in the generated source again
  const size_t line = std::count(head.begin(), head.end(), '\n') + std::count(s.begin(), s.end(), '\n') + 2;
  s += "#line " + std::to_string(line) + (sp.reduce ? " \"foreach_reduce.hip\"\n" : " \"foreach.hip\"\n");
  auto call = [&](bool vec) {  // lh_body's arguments: element lh_e of the vectors, or the scalars
    std::string c = "lh_body(";
    if (sp.reduce) c += acc + (vec ? "[lh_e]" : "") + (sp.nops ? ", " : "");
    for (int k = 0; k < sp.nops; k++) c += (k ? ", " : "") + v(k) + (vec ? ".v[lh_e]" : "");
    for (int k = 0; k < sp.nparams; k++)
      c += ", lh_param<" + std::string(kTypeName[sp.pdtypes[k]]) + ">(a, " + std::to_string(k) + ")";
    return c + ");\n";
  };
  s += "__device__ __forceinline__ void lh_element(const lh_args &a, const long long (&o)[LH_NOPS]" +
       (sp.reduce ? std::string(", lh_acc_t &lh_acc") : std::string()) + ") {\n";
  for (int k = 0; k < sp.nops; k++) {
    const std::string ks = std::to_string(k);
    s += std::string("  ") + (sp.writable[k] ? "" : "const ") + t(k) + " " + v(k) + " = ((const " + t(k) + " *)a.p[" + ks +
         "])[o[" + ks + "]];\n";
  }
  s += "  " + call(false);
  for (int k = 0; k < sp.nops; k++)
    if (sp.writable[k]) s += "  ((" + t(k) + " *)a.p[" + std::to_string(k) + "])[o[" + std::to_string(k) + "]] = " + v(k) + ";\n";
  s += "}\n__device__ __forceinline__ void lh_vector(const lh_args &a, long long lh_i" +
       (sp.reduce ? std::string(", lh_acc_t (&lh_acc)[LH_E]") : std::string()) + ") {\n";
  for (int k = 0; k < sp.nops; k++)
    s += std::string("  ") + (sp.writable[k] ? "" : "const ") + vt(k) + " " + v(k) + " = ((const " + vt(k) + " *)a.p[" +
         std::to_string(k) + "])[lh_i];\n";
  s += "#pragma unroll\n  for (int lh_e = 0; lh_e < LH_E; lh_e++) " + call(true);
  for (int k = 0; k < sp.nops; k++)
    if (sp.writable[k]) s += "  ((" + vt(k) + " *)a.p[" + std::to_string(k) + "])[lh_i] = " + v(k) + ";\n";
  s += "}\n";
  if (sp.reduce) return head + s + lh_foreach_reduce_template;
  return head + s + tpl.substr(at + mark.size() - 1);
}

// ---- hiprtc, loaded on first use --------------------------------------------------------------------------------------
struct Rtc {
  std::once_flag once;
  void *h = nullptr;
  std::string why;
  int (*Create)(void **, const char *, const char *, int, const char **, const char **) = nullptr;
  int (*Compile)(void *, int, const char **) = nullptr;
  int (*LogSize)(void *, size_t *) = nullptr;
  int (*Log)(void *, char *) = nullptr;
  int (*CodeSize)(void *, size_t *) = nullptr;
  int (*Code)(void *, char *) = nullptr;
  int (*Destroy)(void **) = nullptr;
  const char *(*ErrorString)(int) = nullptr;
};
Rtc g_rtc;
std::mutex g_compile_mu;  // one compile at a time

bool rtc_load() {
  std::call_once(g_rtc.once, [] {
    void *h = dlopen("libhiprtc.so", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("libhiprtc.so.7", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("/opt/rocm/lib/libhiprtc.so", RTLD_NOW | RTLD_LOCAL);
    if (!h) {
      const char *e = dlerror();
      g_rtc.why = std::string("cannot load libhiprtc.so: ") + (e ? e : "?");
      return;
    }
    bool ok = true;
    auto sym = [&](auto &field, const char *name) {
      *(void **)(&field) = dlsym(h, name);
      if (!field && ok) {
        ok = false;
        g_rtc.why = std::string("libhiprtc.so has no symbol ") + name;
      }
    };
    sym(g_rtc.Create, "hiprtcCreateProgram");
    sym(g_rtc.Compile, "hiprtcCompileProgram");
    sym(g_rtc.LogSize, "hiprtcGetProgramLogSize");
    sym(g_rtc.Log, "hiprtcGetProgramLog");
    sym(g_rtc.CodeSize, "hiprtcGetCodeSize");
    sym(g_rtc.Code, "hiprtcGetCode");
    sym(g_rtc.Destroy, "hiprtcDestroyProgram");
    sym(g_rtc.ErrorString, "hiprtcGetErrorString");
    if (ok) g_rtc.h = h;
  });
  return g_rtc.h != nullptr;
}

// compile `sp` for `arch` into `code`; LASER_HIP_E_COMPILE with the compiler's log in laser_hip_last_error()
int compile(const Spec &sp, const std::string &arch, std::vector<char> &code) {
  if (arch.empty() || arch.find("xnack+") != std::string::npos)
    return fail(LASER_HIP_E_INVALID, "foreach: architecture '%s' is not accepted (xnack+ code objects are not built)",
                    arch.c_str());
  if (!rtc_load()) return fail(LASER_HIP_E_COMPILE, "foreach: %s", g_rtc.why.c_str());
  const std::string src = generate(sp);
  const std::string target = "--offload-arch=" + arch;
  const char *opts[] = {target.c_str(), "-O3", "-std=c++17", "-ffp-contract=off", "-fwrapv"};
  std::lock_guard<std::mutex> lk(g_compile_mu);
  void *prog = nullptr;
  int e = g_rtc.Create(&prog, src.c_str(), "foreach.hip", 0, nullptr, nullptr);
  if (e != 0) return fail(LASER_HIP_E_COMPILE, "foreach: hiprtcCreateProgram: %s", g_rtc.ErrorString(e));
  g_compiles++;
  e = g_rtc.Compile(prog, (int)(sizeof opts / sizeof opts[0]), opts);
  int rc = LASER_HIP_OK;
  if (e != 0) {
    size_t n = 0;
    std::string log;
    if (g_rtc.LogSize(prog, &n) == 0 && n > 0) {
      log.resize(n);
      if (g_rtc.Log(prog, &log[0]) != 0) log.clear();
      log.resize(strlen(log.c_str()));
    }
    rc = fail_text(LASER_HIP_E_COMPILE, "foreach: the body did not compile (" + std::string(g_rtc.ErrorString(e)) + "):\n" + log);
  } else {
    size_t n = 0;
    if (g_rtc.CodeSize(prog, &n) != 0 || n == 0) {
      rc = fail(LASER_HIP_E_COMPILE, "foreach: hiprtc returned no code object");
    } else {
      code.resize(n);
      if (g_rtc.Code(prog, code.data()) != 0) rc = fail(LASER_HIP_E_COMPILE, "foreach: hiprtcGetCode failed");
    }
  }
  g_rtc.Destroy(&prog);
  return rc;
}

int copy_out(const void *data, int64_t n, void *buf, int64_t cap, int64_t *len) {
  if (!len) return fail(LASER_HIP_E_INVALID, "foreach: null length pointer");
  *len = n;
  if (!buf) return LASER_HIP_OK;  // a size query
  if (cap < n) return fail(LASER_HIP_E_INVALID, "foreach: buffer of %lld bytes, %lld needed", (long long)cap, (long long)n);
  memcpy(buf, data, (size_t)n);
  return LASER_HIP_OK;
}

// ---- loaded kernels: one module per (device, spec) --------------------------------------------------------------------
struct Kernel {
  std::mutex mu;        // held while the first caller compiles and loads
  bool ready = false;
  int64_t handle = 0;   // 1 + index in g_handles
  int device = -1, nops = 0, nparams = 0, vec = 1;
  int size[kMaxOps] = {}, writable[kMaxOps] = {};
  bool reduce = false;  // a forEachReduce module: fn[] are kReduceKernelName's four
  int acc_size = 0;
  hipModule_t mod = nullptr;
  hipFunction_t fn[4] = {};
};
std::mutex g_cache_mu;  // guards the two containers below (never held across a compile)
std::unordered_map<std::string, Kernel *> g_cache;
std::vector<Kernel *> g_handles;  // handle h = index h - 1; entries live for the whole process

// launch arguments: the layout of lh_args in foreach_kernel.hip.in
struct ForeachArgs {
  const void *p[8];
  int64_t st[8][6];
  int64_t shape[6];
  int64_t rank, n, inner, chunks, rows, log2p;
  uint64_t prm[8];
};
static_assert(sizeof(ForeachArgs) == 8 * (8 + 48 + 6 + 6 + 8), "ForeachArgs must match lh_args");
// forEachReduce's launch arguments: the layout of lh_rargs in foreach_reduce_kernel.hip.in
struct ReduceArgs {
  ForeachArgs a;
  void *out;
  uint64_t init;
};
static_assert(sizeof(ReduceArgs) == sizeof(ForeachArgs) + 16, "ReduceArgs must match lh_rargs");

// the module of `sp` for the current device, compiled and loaded on first use
int kernel_for(const Spec &sp, int64_t *handle) {
  const char *what = sp.reduce ? "foreach_reduce" : "foreach";
  if (!handle) return fail(LASER_HIP_E_INVALID, "%s: null handle pointer", what);
  if (int rc = ensure_init()) return rc;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return fail(LASER_HIP_E_NODEVICE, "%s: no current HIP device", what);
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return fail(LASER_HIP_E_NODEVICE, "%s: device %d unreadable", what, dev);
  const std::string arch = prop.gcnArchName;  // e.g. "gfx950:sramecc+:xnack-", used as the device reports it
  if (arch.rfind("gfx950", 0) != 0)
    return fail(LASER_HIP_E_NODEVICE, "%s: device %d is %s; liblaser_hip is built for gfx950 (MI355X) only", what, dev,
                    arch.c_str());
  Kernel *k;
  {
    std::lock_guard<std::mutex> lk(g_cache_mu);
    Kernel *&slot = g_cache[std::to_string(dev) + '|' + sp.key()];
    if (!slot) {
      slot = new Kernel();
      g_handles.push_back(slot);
      slot->handle = (int64_t)g_handles.size();
    }
    k = slot;
  }
  std::lock_guard<std::mutex> lk(k->mu);  // concurrent first calls on one spec: the first compiles, the others wait
  if (!k->ready) {
    std::vector<char> code;
    if (int rc = compile(sp, arch, code)) return rc;
    hipModule_t mod = nullptr;
    hipError_t e = hipModuleLoadData(&mod, code.data());
    const int nfn = sp.reduce ? 4 : 3;
    for (int i = 0; i < nfn && e == hipSuccess; i++)
      e = hipModuleGetFunction(&k->fn[i], mod, sp.reduce ? kReduceKernelName[i] : kKernelName[i]);
    if (e != hipSuccess) {
      if (mod) (void)hipModuleUnload(mod);
      return fail(LASER_HIP_E_HIP, "%s: loading the compiled module failed: %s", what, hipGetErrorString(e));
    }
    k->mod = mod;
    k->device = dev;
    k->nops = sp.nops;
    k->nparams = sp.nparams;
    k->vec = sp.vec();
    k->reduce = sp.reduce;
    k->acc_size = sp.reduce ? kTypeSize[sp.acc_dtype] : 0;
    for (int i = 0; i < sp.nops; i++) {
      k->size[i] = kTypeSize[sp.dtypes[i]];
      k->writable[i] = sp.writable[i];
    }
    k->ready = true;
  }
  *handle = k->handle;
  return LASER_HIP_OK;
}

// the loaded kernel of `handle`, checked to be of the kind (forEach / forEachReduce) the caller launches
int kernel_of(int64_t handle, bool reduce, Kernel **out) {
  const char *what = reduce ? "foreach_reduce" : "foreach";
  Kernel *k = nullptr;
  {
    std::lock_guard<std::mutex> lk(g_cache_mu);
    if (handle >= 1 && handle <= (int64_t)g_handles.size()) k = g_handles[handle - 1];
  }
  if (!k) return fail(LASER_HIP_E_HANDLE, "%s: unknown kernel handle %lld", what, (long long)handle);
  {
    std::lock_guard<std::mutex> lk(k->mu);
    if (!k->ready) return fail(LASER_HIP_E_HANDLE, "%s: kernel handle %lld was never loaded", what, (long long)handle);
  }
  if (k->reduce != reduce)
    return fail(LASER_HIP_E_HANDLE, "%s: handle %lld is a %s kernel", what, (long long)handle,
                    k->reduce ? "forEachReduce" : "forEach");
  *out = k;
  return LASER_HIP_OK;
}

// operand checks, dimension merging and the choice of traversal shared by foreach_dev and foreach_reduce_dev; fills `a`
// and returns the variant (0 vectorised, 1 scalar, 2 strided) in *variant.  *total = element count.
int prepare(const Kernel *k, void *const *ptrs, const int64_t *strides, const int64_t *shape, int rank, const void *params,
            ForeachArgs &a, int *variant, int64_t *total) {
  const char *what = k->reduce ? "foreach_reduce" : "foreach";
  if (rank < 0 || rank > kMaxRank) return fail(LASER_HIP_E_INVALID, "%s: rank %d outside 0..%d (LASER_MAXRANK)", what, rank, kMaxRank);
  if (!ptrs || (rank > 0 && (!strides || !shape)) || (k->nparams > 0 && !params))
    return fail(LASER_HIP_E_INVALID, "%s: null pointers / strides / shape / parameters", what);
  const int nops = k->nops;
  int64_t n = 1;
  for (int d = 0; d < rank; d++) {
    if (shape[d] < 0) return fail(LASER_HIP_E_INVALID, "%s: negative extent", what);
    n *= shape[d];
  }
  for (int d = 0; d < rank; d++)
    for (int i = 0; i < nops; i++)
      if (k->writable[i] && shape[d] > 1 && strides[i * rank + d] == 0)
        return fail(LASER_HIP_E_INVALID, "%s: writable operand %d has stride 0 (broadcast) in dimension %d", what, i, d);
  *total = n;
  if (n == 0) return LASER_HIP_OK;
  for (int i = 0; i < nops; i++)
    if (!ptrs[i]) return fail(LASER_HIP_E_INVALID, "%s: operand %d is a null buffer", what, i);
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev != k->device)
    return fail(LASER_HIP_E_INVALID, "%s: handle %lld was made for device %d, the current device is %d", what,
                    (long long)k->handle, k->device, dev);
  const int r = merge_dims(nops, strides, shape, rank, a.st, a.shape);
  for (int i = 0; i < nops; i++) a.p[i] = ptrs[i];
  if (k->nparams) memcpy(a.prm, params, 8 * (size_t)k->nparams);
  a.n = n;
  a.rank = r;
  bool contiguous = r == 1, aligned = true;
  for (int i = 0; i < nops; i++) {
    contiguous = contiguous && a.st[i][0] == 1;
    aligned = aligned && (uintptr_t)ptrs[i] % ((uintptr_t)k->vec * k->size[i]) == 0;
  }
  *variant = contiguous ? (aligned ? 0 : 1) : 2;
  return LASER_HIP_OK;
}

}  // namespace

namespace laser_hip {
int64_t api_foreach_compiles() { return g_compiles.load(); }
int api_last_foreach_variant() { return g_last_variant.load(); }
}  // namespace laser_hip

extern "C" {

int laser_hip_foreach_source(const char *body, int nops, const char *const *names, const int *dtypes, const int *writable,
                             int nparams, const char *const *param_names, const int *param_dtypes, char *buf, int64_t cap,
                             int64_t *len) {
  Spec sp;
  if (int rc = make_spec(sp, body, nops, names, dtypes, writable, nparams, param_names, param_dtypes)) return rc;
  const std::string src = generate(sp);
  return copy_out(src.c_str(), (int64_t)src.size() + 1, buf, cap, len);
}

int laser_hip_foreach_code(const char *body, int nops, const char *const *names, const int *dtypes, const int *writable,
                           int nparams, const char *const *param_names, const int *param_dtypes, const char *arch, void *buf,
                           int64_t cap, int64_t *len) {
  Spec sp;
  if (int rc = make_spec(sp, body, nops, names, dtypes, writable, nparams, param_names, param_dtypes)) return rc;
  if (!arch) return fail(LASER_HIP_E_INVALID, "foreach: null architecture");
  std::vector<char> code;
  if (int rc = compile(sp, arch, code)) return rc;
  return copy_out(code.data(), (int64_t)code.size(), buf, cap, len);
}

int laser_hip_foreach_kernel(const char *body, int nops, const char *const *names, const int *dtypes, const int *writable,
                             int nparams, const char *const *param_names, const int *param_dtypes, int64_t *handle) {
  Spec sp;
  if (int rc = make_spec(sp, body, nops, names, dtypes, writable, nparams, param_names, param_dtypes)) return rc;
  return kernel_for(sp, handle);
}

int laser_hip_foreach_dev(int64_t handle, void *const *ptrs, const int64_t *strides, const int64_t *shape, int rank,
                          const void *params, void *stream) {
  Kernel *k = nullptr;
  if (int rc = kernel_of(handle, false, &k)) return rc;
  ForeachArgs a = {};
  int variant = 0;
  int64_t total = 0;
  if (int rc = prepare(k, ptrs, strides, shape, rank, params, a, &variant, &total)) return rc;
  if (total == 0) return LASER_HIP_OK;
  const int r = (int)a.rank;
  int64_t blocks;
  if (variant < 2) {
    const bool aligned = variant == 0;
    const int64_t work = aligned ? std::max<int64_t>(total / k->vec, total % k->vec) : total;
    blocks = std::min<int64_t>((work + 255) / 256, 2048);  // a capped grid that grid-strides (Guideline 11)
  } else {
    a.inner = a.shape[r - 1];
    a.rows = 1;
    for (int d = 0; d < r - 1; d++) a.rows *= a.shape[d];
    if (a.inner < 1024 && r > 1) {
      a.log2p = 0;
      while ((int64_t(1) << a.log2p) < a.inner) a.log2p++;
      a.chunks = 1;
      blocks = (a.rows + (1024 >> a.log2p) - 1) / (1024 >> a.log2p);
    } else {
      a.log2p = -1;
      a.chunks = (a.inner + 1023) / 1024;
      blocks = a.rows * a.chunks;
    }
    if (blocks > 0x7fffffffLL) return fail(LASER_HIP_E_INVALID, "foreach: %lld workgroups (too many)", (long long)blocks);
  }
  size_t sz = sizeof a;
  void *extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &sz, HIP_LAUNCH_PARAM_END};
  const hipError_t e = hipModuleLaunchKernel(k->fn[variant], (unsigned)blocks, 1, 1, 256, 1, 1, 0, (hipStream_t)stream, nullptr, extra);
  if (e != hipSuccess) return fail(LASER_HIP_E_HIP, "foreach: launch of %s failed: %s", kKernelName[variant], hipGetErrorString(e));
  g_last_variant = variant;
  return LASER_HIP_OK;
}

// ---- forEachReduce ----------------------------------------------------------------------------------------------------
int laser_hip_foreach_reduce_source(const char *body, int nops, const char *const *names, const int *dtypes,
                                    const int *writable, int nparams, const char *const *param_names,
                                    const int *param_dtypes, const char *acc_name, int acc_dtype, const char *merge,
                                    char *buf, int64_t cap, int64_t *len) {
  Spec sp;
  if (int rc = make_reduce_spec(sp, body, nops, names, dtypes, writable, nparams, param_names, param_dtypes, acc_name,
                                acc_dtype, merge))
    return rc;
  const std::string src = generate(sp);
  return copy_out(src.c_str(), (int64_t)src.size() + 1, buf, cap, len);
}

int laser_hip_foreach_reduce_code(const char *body, int nops, const char *const *names, const int *dtypes,
                                  const int *writable, int nparams, const char *const *param_names,
                                  const int *param_dtypes, const char *acc_name, int acc_dtype, const char *merge,
                                  const char *arch, void *buf, int64_t cap, int64_t *len) {
  Spec sp;
  if (int rc = make_reduce_spec(sp, body, nops, names, dtypes, writable, nparams, param_names, param_dtypes, acc_name,
                                acc_dtype, merge))
    return rc;
  if (!arch) return fail(LASER_HIP_E_INVALID, "foreach_reduce: null architecture");
  std::vector<char> code;
  if (int rc = compile(sp, arch, code)) return rc;
  return copy_out(code.data(), (int64_t)code.size(), buf, cap, len);
}

int laser_hip_foreach_reduce_kernel(const char *body, int nops, const char *const *names, const int *dtypes,
                                    const int *writable, int nparams, const char *const *param_names,
                                    const int *param_dtypes, const char *acc_name, int acc_dtype, const char *merge,
                                    int64_t *handle) {
  Spec sp;
  if (int rc = make_reduce_spec(sp, body, nops, names, dtypes, writable, nparams, param_names, param_dtypes, acc_name,
                                acc_dtype, merge))
    return rc;
  return kernel_for(sp, handle);
}

int laser_hip_foreach_reduce_dev(int64_t handle, void *const *ptrs, const int64_t *strides, const int64_t *shape,
                                 int rank, const void *params, const void *init, void *d_out, void *stream) {
  Kernel *k = nullptr;
  if (int rc = kernel_of(handle, true, &k)) return rc;
  if (!init || !d_out) return fail(LASER_HIP_E_INVALID, "foreach_reduce: null init / output");
  ReduceArgs r = {};
  int variant = 0;
  int64_t total = 0;
  if (int rc = prepare(k, ptrs, strides, shape, rank, params, r.a, &variant, &total)) return rc;
  if (total == 0) {  // no operand is read: a launch of the partials kernel over nothing writes init
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev != k->device)
      return fail(LASER_HIP_E_INVALID, "foreach_reduce: handle %lld was made for device %d, the current device is %d",
                      (long long)handle, k->device, dev);
    variant = 3;
  }
  memcpy(&r.init, init, (size_t)k->acc_size);
  const hipStream_t s = (hipStream_t)stream;
  auto launch = [&](int fn, ReduceArgs &args, int64_t blocks) {
    size_t sz = sizeof args;
    void *extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &args, HIP_LAUNCH_PARAM_BUFFER_SIZE, &sz, HIP_LAUNCH_PARAM_END};
    return hipModuleLaunchKernel(k->fn[fn], (unsigned)blocks, 1, 1, 256, 1, 1, 0, s, nullptr, extra);
  };
  auto level0 = [&](int64_t blocks, void *dst) {
    r.out = dst;
    return launch(variant, r, blocks);
  };
  auto partials = [&](const void *in, int64_t count, int64_t blocks, void *dst) {
    ReduceArgs p = {};
    p.a.p[0] = in;
    p.a.n = count;
    p.out = dst;
    p.init = r.init;
    return launch(3, p, blocks);
  };
  const hipError_t e = reduce_levels(total, total ? k->vec : 16 / k->acc_size, k->acc_size, d_out, s, level0, partials);
  if (e != hipSuccess) return fail(LASER_HIP_E_HIP, "foreach_reduce: launch failed: %s", hipGetErrorString(e));
  if (total) g_last_variant = variant;
  return LASER_HIP_OK;
}

}  // extern "C"
