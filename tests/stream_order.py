"""Stream order and host asynchrony of the `_dev` surface: the harness and the case table.

include/laser_hip.h promises that a `_dev` call is "asynchronous on that stream".  The per-family side-stream tests upload,
synchronise, call, synchronise and read back: the inputs are complete before the call and nothing reads the outputs before the
host has waited, so a launch on the wrong stream or a host wait inside the call gives the same bits.  Here the call is issued
while its stream is BLOCKED:

    S:  [spin kernel][gate event] [outputs <- sentinel] [operands <- staged] [the call] [clones of the outputs]

The operand buffers hold a decoy (another valid input of the same shapes) until the copies behind the gate run, and the outputs
are overwritten with a sentinel behind the gate.  A launch that is not ordered on S reads the decoy or is overwritten by the
sentinel; a call that waits on the host returns after the gate has opened.  Every decoy is a valid input of its operation (ids
in range, sorted arrays, positive weights, monotone CDFs, finite floats), so an early read is defined behaviour.

The module imports without a GPU: tests/test_stream_order_cpu.py checks the table against the header, and
tests/test_gpu_stream_order.py runs it.
"""
import contextlib
import ctypes as C
import time

import numpy as np

GUARD = 64                 # elements of sentinel before and after every device buffer
SENT_SETUP = 0xA5          # every byte of a buffer before a run
SENT_GATED = 0x5A          # what the outputs are overwritten with behind the gate
GATE_MIN_MS = 50.0
GATE_FACTOR = 20.0         # gate length = max(GATE_MIN_MS, GATE_FACTOR * t_host): a margin for host jitter, not a measured figure
GATE_MAX_MS = 2000.0
MAX_DRAWS = 8

# entry points include/laser_hip.h itself documents as synchronous: name -> the header's sentence.  They skip only the
# "gate still closed on return" assertion.
SHARDED_SENTENCE = "Both forms are synchronous (return when every device is done); one host thread per GPU drives it."
EXEMPT = {f"laser_hip_gemm_strided_{s}_sharded_dev": SHARDED_SENTENCE for s in ("f32", "f64", "i32", "i64")}
STORAGE_SENTENCE = "Upload and download are complete when the call returns."
EXEMPT["laser_hip_storage_upload_stream"] = STORAGE_SENTENCE
EXEMPT["laser_hip_storage_download_stream"] = STORAGE_SENTENCE


class StreamOrderError(AssertionError):
    """what the harness reports; kind: "bits", "gate-open", "too-slow", "blind", "decoy" """

    def __init__(self, kind, msg):
        super().__init__(f"[{kind}] {msg}")
        self.kind = kind


class Case:
    """One row of the table.  build(seed) -> {name: numpy array}: every buffer and host value of the call.  `outputs` are
    written by the call, `inplace` are read and updated, `temps` are written and not compared (opaque packed panels), `host`
    are passed as numpy values (seeds); the rest are read-only operands.  rules: name -> validity rule of an operand
    ("finite" by default for floats; ("ids", n); "sorted"; "positive"; "cdf"; "unit").  call(la, b): b maps names to torch
    views (host values for `host`).  options: laser_hip options set around every run; path(la): asserts the kernel taken."""

    def __init__(self, name, family, symbols, build, call, outputs, inplace=(), temps=(), host=(), rules=None, scratch=False,
                 options=None, float_mode=0, path=None, sync=False, warm_call=None):
        self.name, self.family, self.symbols = name, family, tuple(symbols)
        self.build, self.call = build, call
        self.outputs, self.inplace, self.temps, self.host = tuple(outputs), tuple(inplace), tuple(temps), tuple(host)
        self.rules = dict(rules or {})
        self.scratch, self.options, self.float_mode, self.path, self.sync = scratch, dict(options or {}), float_mode, path, sync
        self.warm_call = warm_call      # the negative controls only: the correct call, for the synchronised runs

    def operands(self, bufs):
        skip = set(self.outputs) | set(self.temps) | set(self.host)
        return [k for k in bufs if k not in skip]

    def __repr__(self):
        return self.name


# ---- validity of a decoy (numpy only) -----------------------------------------------------------------------------------------
def check_rule(name, arr, rule):
    """None, or what is wrong with operand `name` as an input"""
    a = np.asarray(arr)
    if a.dtype.kind == "f" and not np.isfinite(a).all():
        return f"{name}: not finite"
    if rule in (None, "finite"):
        return None
    if isinstance(rule, tuple) and rule[0] == "ids":
        return None if a.dtype.kind == "i" and a.min() >= 0 and a.max() < rule[1] else f"{name}: ids outside [0, {rule[1]})"
    if rule == "sorted":
        return None if (np.diff(a, axis=-1) >= 0).all() else f"{name}: rows not sorted"
    if rule == "positive":
        return None if (a > 0).all() else f"{name}: not positive"
    if rule == "cdf":
        return None if (np.diff(a, axis=-1) >= 0).all() and (a[..., 0] > 0).all() else f"{name}: not a monotone CDF"
    if rule == "unit":
        return None if (a >= 0).all() and (a < 1).all() else f"{name}: outside [0, 1)"
    return f"{name}: unknown rule {rule!r}"


# ---- device side --------------------------------------------------------------------------------------------------------------
_TORCH = {"float32": "float32", "float64": "float64", "int32": "int32", "int64": "int64", "int8": "int8", "int16": "int16",
          "uint8": "uint8", "uint32": "int32"}


class Arena:
    """a flat device buffer with GUARD sentinel elements on both sides of the body"""

    def __init__(self, arr):
        import torch
        arr = np.asarray(arr)
        self.shape, n = arr.shape, int(arr.size)
        self.flat = torch.empty(n + 2 * GUARD, dtype=getattr(torch, _TORCH[arr.dtype.name]), device="cuda")
        self.body = self.flat[GUARD:GUARD + n].view(self.shape)
        self.fill(SENT_SETUP)

    def fill(self, byte):
        import torch
        self.flat.view(torch.uint8).fill_(byte)

    def guards_hold(self, byte):
        import torch
        b = self.flat.view(torch.uint8)
        e = self.flat.element_size() * GUARD
        return bool((b[:e] == byte).all()) and bool((b[b.numel() - e:] == byte).all())


def same_bytes(a, b):
    import torch
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def to_dev(arr):
    import torch
    a = np.ascontiguousarray(arr)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


_session = {}


def ticks_per_ms():
    """torch.cuda._sleep cycles per millisecond, measured once: one spin between two events, lengthened until it lasts 5 ms"""
    import torch
    if "ticks" not in _session:
        cycles = 1_000_000
        for _ in range(8):
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            torch.cuda._sleep(cycles)
            b.record()
            torch.cuda.synchronize()
            ms = a.elapsed_time(b)
            if ms >= 5.0:
                break
            cycles *= 8
        assert ms > 0, "the spin kernel took no time"
        _session["ticks"] = cycles / ms
    return _session["ticks"]


def close_gate(stream, ms):
    """queue the spin kernel and the gate event on `stream`; the stream does nothing else until the spin ends"""
    import torch
    with torch.cuda.stream(stream):
        torch.cuda._sleep(int(ms * ticks_per_ms()))
        gate = torch.cuda.Event()
        gate.record()
    return gate


def probe(first, second):
    """True when work on `second` completes while `first` is blocked: the two do not share a hardware queue"""
    import torch
    with torch.cuda.stream(second):
        t = torch.zeros(64, device="cuda")
    torch.cuda.synchronize()
    gate = close_gate(first, 40.0)
    with torch.cuda.stream(second):
        t.fill_(1.0)
        ev = torch.cuda.Event()
        ev.record()
    while not ev.query() and not gate.query():
        pass
    done = ev.query()
    closed = not gate.query()
    torch.cuda.synchronize()
    return bool(done and closed)


def streams():
    """(S, S2): S runs independently of the NULL stream, S2 independently of S (probed; at most MAX_DRAWS draws each)"""
    import torch
    if "streams" not in _session:
        null = torch.cuda.default_stream()
        s = s2 = None
        for _ in range(MAX_DRAWS):
            c = torch.cuda.Stream()
            if probe(c, null):
                s = c
                break
        if s is None:
            raise StreamOrderError("blind", f"probe(S, NULL stream): no side stream of {MAX_DRAWS} let the NULL stream run while it was blocked")
        for _ in range(MAX_DRAWS):
            c = torch.cuda.Stream()
            if probe(s, c) and probe(c, s):
                s2 = c
                break
        if s2 is None:
            raise StreamOrderError("blind", f"probe(S1, S2): no second stream of {MAX_DRAWS} ran while the first was blocked")
        _session["streams"] = (s, s2)
    return _session["streams"]


@contextlib.contextmanager
def case_options(la, case):
    """the case's options and float mode, the previous values restored afterwards"""
    old = {k: la.get_option(k) for k in case.options}
    mode = la.get_float_mode()
    try:
        for k, v in case.options.items():
            la.set_option(k, v)
        la.set_float_mode(case.float_mode)
        yield
    finally:
        la.set_float_mode(mode)
        for k, v in old.items():
            la.set_option(k, v)


class Live:
    """the device buffers of one run of a case"""

    def __init__(self, case, shapes):
        self.case = case
        self.arenas = {k: Arena(v) for k, v in shapes.items() if k not in case.host}
        self.ops = case.operands(shapes)

    def views(self, host_values):
        b = {k: a.body for k, a in self.arenas.items()}
        b.update({k: host_values[k] for k in self.case.host})
        return b

    def reset(self, decoy_dev):
        for a in self.arenas.values():
            a.fill(SENT_SETUP)
        for k in self.ops:
            self.arenas[k].body.copy_(decoy_dev[k])

    def results(self):
        return self.case.outputs + self.case.inplace


def enqueue(case, la, live, src_dev, host_values, stream, call=None):
    """on `stream`: outputs <- sentinel, operands <- src, the call, clones of the results.  Returns (clones, host seconds of the
    call); the caller closes the gate before and queries it after."""
    import torch
    with torch.cuda.stream(stream):
        for k in case.outputs + case.temps:
            live.arenas[k].fill(SENT_GATED)
        for k in live.ops:
            live.arenas[k].body.copy_(src_dev[k])
        t0 = time.perf_counter()
        (call or case.call)(la, live.views(host_values))
        dt = time.perf_counter() - t0
    return dt


def clone_results(live, stream):
    import torch
    with torch.cuda.stream(stream):
        return {k: live.arenas[k].flat.clone() for k in live.results()}


def warm(case, la, seed, stream):
    """the synchronised runs of one input set on `stream`, no gate: (host arrays, device copies, want bits, t_host of the
    second call)"""
    import torch
    bufs = case.build(seed)
    dev = {k: to_dev(v) for k, v in bufs.items() if k not in case.host}
    live = Live(case, bufs)
    t_host = 0.0
    for _ in range(2):
        live.reset(dev)
        torch.cuda.synchronize()
        t_host = enqueue(case, la, live, dev, bufs, stream, case.warm_call)
        stream.synchronize()
    if case.path is not None:
        case.path(la)
    want = {k: live.arenas[k].flat.clone() for k in live.results()}
    for k in case.outputs:
        if not live.arenas[k].guards_hold(SENT_GATED):
            raise StreamOrderError("bits", f"{case.name}: the synchronised run wrote outside output {k}")
    for k in case.inplace:
        if not live.arenas[k].guards_hold(SENT_SETUP):
            raise StreamOrderError("bits", f"{case.name}: the synchronised run wrote outside operand {k}")
    torch.cuda.synchronize()
    return bufs, dev, want, t_host


def gate_ms(case, t_host, factor=1.0):
    ms = max(GATE_MIN_MS, GATE_FACTOR * t_host * 1e3) * factor
    if ms > GATE_MAX_MS:
        raise StreamOrderError("too-slow", f"{case.name}: the call takes {t_host * 1e3:.2f} ms on the host; the gate would be {ms:.0f} ms "
                                           f"(> {GATE_MAX_MS:.0f} ms)")
    return ms


def compare(case, what, got, want):
    bad = [k for k in want if not same_bytes(got[k], want[k])]
    if bad:
        raise StreamOrderError("bits", f"{case.name}: {what}: {bad} differ from the synchronised run (results, operands updated in place and "
                                       "their guard elements are compared byte for byte)")


def prepare(case, la, stream):
    """warm runs of the staged and the decoy set; the decoy's result must differ, or the case proves nothing"""
    staged = warm(case, la, 1, stream)
    decoy = warm(case, la, 2, stream)
    if all(same_bytes(staged[2][k], decoy[2][k]) for k in staged[2]):
        raise StreamOrderError("decoy", f"{case.name}: the decoy gives the bits of the staged inputs")
    return staged, decoy


def run_gated(case, la, stats=None):
    """The gated-producer run.  Raises StreamOrderError; `stats` collects t_host per family."""
    import torch
    s, _ = streams()
    with case_options(la, case):
        (bufs, dev, want, t_host), (_, decoy_dev, _, _) = prepare(case, la, s)
        if stats is not None:
            stats[case.family] = max(stats.get(case.family, 0.0), t_host)
        ms = gate_ms(case, t_host)
        live = Live(case, bufs)
        live.reset(decoy_dev)
        torch.cuda.synchronize()
        try:
            gate = close_gate(s, ms)
            enqueue(case, la, live, dev, bufs, s)
            opened = gate.query()
            clones = clone_results(live, s)
        finally:
            s.synchronize()
            torch.cuda.synchronize()
        if opened and not case.sync:
            raise StreamOrderError("gate-open", f"{case.name}: gate open on return: the call waited on the host (t_host = {t_host * 1e3:.3f} ms "
                                                f"in the synchronised run, gate = {ms:.0f} ms)")
        compare(case, "the results", {k: live.arenas[k].flat for k in want}, want)
        compare(case, "the stream-side clones", clones, want)


def run_two_streams(case, la):
    """The same operation queued on a blocked S1 and then run to completion on S2: scratch, workspaces and flags of the two
    calls must not meet."""
    import torch
    s1, s2 = streams()
    with case_options(la, case):
        (bufs1, dev1, want1, t_host), (bufs2, dev2, want2, _) = prepare(case, la, s1)
        warm(case, la, 2, s2)           # (this stream's own workspace, if the plan takes one, is made outside the gate)
        ms = gate_ms(case, t_host, 2.0)
        live1, live2 = Live(case, bufs1), Live(case, bufs2)
        live1.reset(dev2)
        live2.reset(dev1)
        torch.cuda.synchronize()
        try:
            gate = close_gate(s1, ms)
            enqueue(case, la, live1, dev1, bufs1, s1)
            opened = gate.query()
            clones1 = clone_results(live1, s1)
            enqueue(case, la, live2, dev2, bufs2, s2)
            clones2 = clone_results(live2, s2)
            opened2 = gate.query()
            s2.synchronize()
        finally:
            s1.synchronize()
            torch.cuda.synchronize()
        if (opened or opened2) and not case.sync:
            raise StreamOrderError("gate-open", f"{case.name}: S1's gate was open when the call on {'S1' if opened else 'S2'} returned "
                                                f"(t_host = {t_host * 1e3:.3f} ms, gate = {ms:.0f} ms)")
        compare(case, "S2 (run while S1 was blocked)", clones2, want2)
        compare(case, "S1 (blocked)", clones1, want1)
        compare(case, "S1's buffers", {k: live1.arenas[k].flat for k in want1}, want1)


# ---- the case table -----------------------------------------------------------------------------------------------------------
CASES = []


def case(*a, **kw):
    CASES.append(Case(*a, **kw))


def _rng(seed, salt):
    return np.random.default_rng(1000 * salt + seed)


def _f(rng, shape, dtype=np.float32, lo=-1.0, hi=1.0):
    return rng.uniform(lo, hi, shape).astype(dtype)


def _ints(rng, shape, dtype):
    info = np.iinfo(dtype)
    return rng.integers(info.min, info.max, shape, dtype=dtype, endpoint=True)


def _rand(rng, shape, dtype):
    return _f(rng, shape, dtype) if np.dtype(dtype).kind == "f" else _ints(rng, shape, dtype)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _st():
    from laser_amd.tensor import _stream
    return _stream()


def _L():
    from laser_amd import _lib
    return _lib.lib()


def _ok(rc):
    from laser_amd import _lib
    _lib.check(rc)


def _i64s(v):
    return (C.c_int64 * max(len(v), 1))(*v)


def _opt(name, pred, what):
    def path(la):
        v = la.get_option(name)
        assert pred(v), f"{name} = {v}: {what}"
    return path


# -- GEMM ---------------------------------------------------------------------------------------------------------------------
_SFX = {"float32": "f32", "float64": "f64", "int32": "i32", "int64": "i64", "int8": "i8", "int16": "i16"}
_SCALARS = {"f": (0.5, -0.25), "i": (3, -2)}


def _gemm_build(dtype, M, N, K, salt):
    def build(seed):
        r = _rng(seed, salt)
        return {"A": _rand(r, (M, K), dtype), "B": _rand(r, (K, N), dtype), "C": _rand(r, (M, N), dtype)}
    return build


def _gemm_call(dtype):
    alpha, beta = _SCALARS[np.dtype(dtype).kind]

    def call(la, b):
        la.matmul(b["A"], b["B"], alpha, beta, b["C"])      # beta != 0: C0 is a live operand, updated in place
    return call


def gemm_case(name, dtype, shape, salt, **kw):
    s = _SFX[np.dtype(dtype).name]
    case(name, "gemm", [f"laser_hip_gemm_strided_{s}_dev"], _gemm_build(dtype, *shape, salt), _gemm_call(dtype), (), inplace=("C",), **kw)


gemm_case("gemm_f32_mfma", np.float32, (200, 136, 300), 1, options=dict(f32_asm=0, slice_parallel=0),
          path=_opt("last_f32_asm", lambda v: v == 0, "the compiler-scheduled kernel was meant"))
gemm_case("gemm_f32_asm_plain", np.float32, (300, 260, 600), 2, options=dict(f32_asm=2, asm_plan=1, slice_parallel=0),
          path=_opt("last_f32_asm", lambda v: v != 0, "an assembly kernel was meant"))
gemm_case("gemm_f32_asm_cut", np.float32, (3 * 128 + 17, 5 * 128 - 9, 2151), 3, scratch=True,
          options=dict(f32_asm=2, asm_plan=2, asm_kernel=2, slice_parallel=0),
          path=_opt("last_asm_slices", lambda v: v > 1, "a K-cut launch (per-stream workspace and flags) was meant"))
gemm_case("gemm_f32_asm_cut_fast", np.float32, (3 * 128 + 17, 5 * 128 - 9, 2151), 4, scratch=True, float_mode=1,
          options=dict(f32_asm=2, asm_plan=2, slice_parallel=0),
          path=_opt("last_f32_asm", lambda v: v != 0, "an assembly kernel was meant"))
gemm_case("gemm_f32_slice_parallel", np.float32, (67, 131, 3 * 512 + 5), 5, scratch=True)
gemm_case("gemm_f32_skinny", np.float32, (4, 300, 700), 7)
gemm_case("gemm_f64_mfma", np.float64, (150, 130, 300), 8, options=dict(f64_asm=0, slice_parallel=0),
          path=_opt("last_f64_asm", lambda v: v == 0, "the compiler-scheduled kernel was meant"))
gemm_case("gemm_f64_asm", np.float64, (260, 200, 300), 9, options=dict(f64_asm=2, slice_parallel=0),
          path=_opt("last_f64_asm", lambda v: v != 0, "an assembly kernel was meant"))
gemm_case("gemm_f64_slice_parallel", np.float64, (67, 131, 3 * 256 + 5), 10, scratch=True)
gemm_case("gemm_i32_limbs", np.int32, (130, 257, 100), 11, scratch=True, options=dict(i32_asm=0),
          path=_opt("last_i32_asm", lambda v: v == 0, "the compiler-scheduled limb kernel was meant"))
gemm_case("gemm_i32_limbs_asm", np.int32, (130, 257, 100), 12, scratch=True, options=dict(i32_asm=2),
          path=_opt("last_i32_asm", lambda v: v != 0, "the assembly limb kernel was meant"))
gemm_case("gemm_i64_limbs", np.int64, (130, 257, 100), 13, scratch=True, options=dict(i32_asm=0),
          path=_opt("last_i32_asm", lambda v: v == 0, "the compiler-scheduled limb kernel was meant"))
gemm_case("gemm_i64_limbs_asm", np.int64, (130, 257, 100), 14, scratch=True, options=dict(i32_asm=2))
gemm_case("gemm_i8_planes", np.int8, (300, 260, 500), 15, scratch=True,
          path=_opt("last_narrow_mfma", lambda v: v == 1, "the matrix-core digit-plane kernel was meant"))
gemm_case("gemm_i16_planes", np.int16, (300, 260, 500), 16, scratch=True,
          path=_opt("last_narrow_mfma", lambda v: v == 1, "the matrix-core digit-plane kernel was meant"))


def _batched_case(dtype, salt, dims=(3, 70, 50, 90), name=None, **kw):
    s = _SFX[np.dtype(dtype).name]
    batch, M, N, K = dims
    alpha, beta = _SCALARS[np.dtype(dtype).kind]

    def build(seed):
        r = _rng(seed, salt)
        return {"A": _rand(r, (batch, M, K), dtype), "B": _rand(r, (batch, K, N), dtype), "C": _rand(r, (batch, M, N), dtype)}

    def call(la, b):
        la.gemm_strided_batched(batch, M, N, K, alpha, b["A"], K, 1, M * K, b["B"], N, 1, K * N, beta, b["C"], N, 1, M * N)

    case(name or f"gemm_batched_{s}", "gemm", [f"laser_hip_gemm_strided_batched_{s}_dev"], build, call, (), inplace=("C",), scratch=True, **kw)


for _k, _dt in enumerate((np.float32, np.float64, np.int32, np.int64, np.int8, np.int16)):
    _batched_case(_dt, 20 + _k)


def _ex_case(dtype, salt, activation):
    s = _SFX[np.dtype(dtype).name]
    M, N, K = 90, 72, 130

    def build(seed):
        r = _rng(seed, salt)
        return {"A": _f(r, (M, K), dtype), "B": _f(r, (K, N), dtype), "C": _f(r, (M, N), dtype), "bias": _f(r, (N,), dtype)}

    def call(la, b):
        la.matmul(b["A"], b["B"], 0.5, -0.25, b["C"], bias=b["bias"], activation=activation)

    case(f"gemm_ex_{s}", "gemm", [f"laser_hip_gemm_strided_ex_{s}_dev"], build, call, (), inplace=("C",))


# the small-matrix kernel takes device operands only as a batch: batch > 1, M, N <= 64, K <= 128 (gemm_small_takes)
_batched_case(np.float32, 26, (5, 48, 40, 64), "gemm_f32_small_batched",
              path=_opt("last_f32_config", lambda v: v == -2, "the small-matrix kernel was meant"))
_ex_case(np.float32, 30, "tanh")
_ex_case(np.float64, 31, "relu")


def _packed_case(dtype, salt):
    """prepackA and prepackB are the producers of the multiply: three calls chained on the stream, nothing waited for"""
    s = _SFX[np.dtype(dtype).name]
    M, N, K = 150, 140, 200
    alpha, beta = _SCALARS[np.dtype(dtype).kind]

    def build(seed):
        from laser_amd import gemm_prepackA_mem_required, gemm_prepackB_mem_required
        r = _rng(seed, salt)
        return {"A": _rand(r, (M, K), dtype), "B": _rand(r, (K, N), dtype), "C": _rand(r, (M, N), dtype),
                "pa": np.zeros(gemm_prepackA_mem_required(dtype, M, N, K), np.uint8),
                "pb": np.zeros(gemm_prepackB_mem_required(dtype, M, N, K), np.uint8)}

    def call(la, b):
        la.gemm_prepackA(b["pa"], M, N, K, b["A"], K, 1)
        la.gemm_prepackB(b["pb"], M, N, K, b["B"], N, 1)
        la.gemm_packed(M, N, K, alpha, b["pa"], b["pb"], beta, b["C"], N, 1)

    case(f"gemm_packed_{s}", "gemm", [f"laser_hip_gemm_prepackA_{s}_dev", f"laser_hip_gemm_prepackB_{s}_dev", f"laser_hip_gemm_packed_{s}_dev"],
         build, call, (), inplace=("C",), temps=("pa", "pb"), scratch=True)


for _k, _dt in enumerate((np.float32, np.float64, np.int32, np.int64, np.int8, np.int16)):
    _packed_case(_dt, 40 + _k)


# -- convolution and data movement ----------------------------------------------------------------------------------------------
def _conv_case(name, geometry, salt, ex=False, **kw):
    ishape, kshape, padding, strides = geometry

    def oshape():
        from laser_amd import conv2d_out_shape
        return conv2d_out_shape(ishape, kshape, padding, strides)

    def build(seed):
        r = _rng(seed, salt)
        b = {"x": _f(r, ishape), "w": _f(r, kshape), "out": np.zeros(oshape(), np.float32)}
        if ex:
            b["bias"] = _f(r, (kshape[0],))
        return b

    def call(la, b):
        if ex:
            la.conv2d_im2col(b["out"], oshape(), b["x"], ishape, b["w"], kshape, padding, strides, None, bias=b["bias"], activation="relu")
        else:
            la.conv2d_im2col(b["out"], oshape(), b["x"], ishape, b["w"], kshape, padding, strides, None)

    sym = "laser_hip_conv2d_im2col_ex_f32_dev" if ex else "laser_hip_conv2d_im2col_f32_dev"
    case(name, "conv", [sym], build, call, ("out",), **kw)


def conv_geometry(k):
    from tests.poison_views import CONV_GEOMETRIES
    return CONV_GEOMETRIES[k]


# (the options of tests/test_gpu_poison.py CONV_ROUTES for the same geometries)
_conv_case("conv_direct_small", conv_geometry(0), 50, options=dict(conv_direct=1),
           path=_opt("last_f32_config", lambda v: v == -3, "the direct small-channel kernel was meant"))
_conv_case("conv_implicit", conv_geometry(3), 51, ex=True, options=dict(conv_direct=0, conv_patch=1, f32_asm=0))
_conv_case("conv_explicit_scratch", conv_geometry(3), 52, scratch=True, options=dict(conv_direct=0, conv_implicit=0, f32_asm=0))
_conv_case("conv_asm_loader", conv_geometry(5), 53, ex=True, options=dict(f32_asm=2),
           path=_opt("last_f32_asm", lambda v: v != 0, "the assembly loader was meant"))
_conv_case("conv_pixel_tail", conv_geometry(7), 54, scratch=True, options=dict(f32_asm=2, conv_cut_always=1, conv_tail=0, conv_kslice=1),
           path=_opt("last_conv_tail", lambda v: v == 2, "a pixel tail as kc slices + combine was meant"))


def _im2col_case(dtype, salt):
    s = _SFX[np.dtype(dtype).name]
    ishape, kshape, padding, strides = (1, 3, 13, 15), (1, 3, 3, 2), (1, 0), (2, 1)

    def oshape():
        from laser_amd import conv2d_out_shape
        return conv2d_out_shape(ishape, kshape, padding, strides)

    def build(seed):
        o = oshape()
        return {"x": _f(_rng(seed, salt), ishape[1:], dtype), "ws": np.zeros((ishape[1] * kshape[2] * kshape[3], o[2] * o[3]), dtype)}

    def call(la, b):
        la.im2col(b["ws"], oshape(), b["x"], ishape, kshape, padding, strides)

    case(f"im2col_{s}", "movers", [f"laser_hip_im2col_{s}_dev"], build, call, ("ws",))


_im2col_case(np.float32, 55)
_im2col_case(np.float64, 56)


def _transpose_case(dtype, salt):
    b = {1: "b8", 2: "b16", 4: "b32", 8: "b64"}[np.dtype(dtype).itemsize]
    n, nr, nc = 3, 37, 70

    def build(seed):
        return {"src": _rand(_rng(seed, salt), (n, nr, nc), dtype), "dst": np.zeros((n, nc, nr), dtype)}

    def call(la, v):
        la.transpose2D_batched(v["dst"], v["src"], n, nr, nc)

    case(f"transpose_{b}", "movers", [f"laser_hip_transpose2d_batched_{b}_dev"], build, call, ("dst",))


for _k, _dt in enumerate((np.int8, np.int16, np.float32, np.float64)):
    _transpose_case(_dt, 57 + _k)


def _copy_case(dtype, salt):
    b = {4: "b32", 8: "b64"}[np.dtype(dtype).itemsize]

    def build(seed):
        return {"src": _rand(_rng(seed, salt), (5, 33, 17), dtype), "dst": np.zeros((17, 33, 5), dtype)}

    def call(la, v):
        la.copyFrom(la.fromTorch(v["dst"]), la.fromTorch(v["src"]).transpose(2, 1, 0))

    case(f"copy_strided_{b}", "movers", [f"laser_hip_copy_strided_{b}_dev"], build, call, ("dst",))


_copy_case(np.int32, 61)
_copy_case(np.float64, 62)


def _map_case(dtype, salt):
    s = _SFX[np.dtype(dtype).name]
    small = np.dtype(dtype).kind == "i"

    def build(seed):
        r = _rng(seed, salt)
        gen = (lambda sh: r.integers(-1000, 1000, sh).astype(dtype)) if small else (lambda sh: _f(r, sh, dtype))
        return {"a": gen((19, 40)), "b": gen((40, 19)), "u": np.zeros((40, 19), dtype), "d": np.zeros((19, 40), dtype)}

    def call(la, v):
        a, b, u, d = (la.fromTorch(v[k]) for k in ("a", "b", "u", "d"))
        la.forEachMap("scale", u, a.T, alpha=3, beta=1)               # a strided read
        la.forEachMap("axpby", d, a, b.T, alpha=2, beta=-3)

    case(f"map_strided_{s}", "movers", [f"laser_hip_map_strided_unary_{s}_dev", f"laser_hip_map_strided_binary_{s}_dev"], build, call,
         ("u", "d"))


for _k, _dt in enumerate((np.float32, np.float64, np.int32, np.int64)):
    _map_case(_dt, 63 + _k)


def _storage_cases():
    n = 5000

    def build(seed):
        return {"x": _f(_rng(seed, 70), (n,)), "out": np.zeros((n,), np.float32)}

    def call(la, v):
        """a fresh storage (its zero fill ordered on the stream), x added into it, copied out, the second half cleared"""
        t = la.newTensor(np.float32, n)
        la.forEachMap("add", t, t, la.fromTorch(v["x"]))
        la.copyFrom(la.fromTorch(v["out"]), t)
        _ok(_L().laser_hip_storage_set_zero(C.c_void_p(v["out"].data_ptr() + 4 * (n // 2)), 4 * (n - n // 2), _st()))
        del t                                     # back to the storage cache while the stream is still blocked
        t2 = la.newTensor(np.float32, n)          # the same block again: ordered behind the work above, on the device
        la.forEachMap("add", t2, t2, la.fromTorch(v["out"]))
        la.copyFrom(la.fromTorch(v["out"]), t2)

    case("storage_alloc_set_zero", "movers", ["laser_hip_storage_alloc_stream", "laser_hip_storage_set_zero"], build, call, ("out",))

    def call_sync(la, v):
        """download then upload: both complete on return (the header says so), and both ordered behind the producer"""
        h = np.empty(n, np.float32)
        _ok(_L().laser_hip_storage_download_stream(h.ctypes.data_as(C.c_void_p), _ptr(v["x"]), h.nbytes, _st()))
        _ok(_L().laser_hip_storage_upload_stream(_ptr(v["out"]), h.ctypes.data_as(C.c_void_p), h.nbytes, _st()))

    case("storage_download_upload", "movers", ["laser_hip_storage_download_stream", "laser_hip_storage_upload_stream"], build, call_sync,
         ("out",), sync=True)


_storage_cases()


# -- forEach and reductions -------------------------------------------------------------------------------------------------------
def _foreach_cases():
    n = 40_003

    def build(seed):
        r = _rng(seed, 71)
        return {"x": _f(r, (n,)), "y": _f(r, (n,)), "z": _f(r, (n,)), "acc": np.zeros((1,), np.float32)}

    def call(la, v):
        la.forEach("x += y * s + z", params={"s": np.float32(0.75)}, x=v["x"], y=v["y"], z=v["z"])

    case("foreach", "foreach", ["laser_hip_foreach_dev"], build, call, (), inplace=("x",), temps=("acc",))

    def call_reduce(la, v):
        la.forEachReduce("acc += y * z; x = y - z", merge="acc += other", init=np.float32(0), writable=("x",), out=v["acc"],
                         x=v["x"], y=v["y"], z=v["z"])

    case("foreach_reduce", "foreach", ["laser_hip_foreach_reduce_dev"], build, call_reduce, ("acc",), inplace=("x",), scratch=True)


_foreach_cases()


def _reduce_case(dtype, salt):
    s = _SFX[np.dtype(dtype).name]
    n = 100_003                      # more than one level: partials in stream-ordered scratch

    def build(seed):
        r = _rng(seed, salt)
        x = _f(r, (n,), dtype) if np.dtype(dtype).kind == "f" else r.integers(-10_000, 10_000, (n,)).astype(dtype)
        return {"x": x, "sum": np.zeros(1, dtype), "min": np.zeros(1, dtype), "max": np.zeros(1, dtype)}

    def call(la, v):
        la.reduce_sum(v["x"], out=v["sum"])
        la.reduce_min(v["x"], out=v["min"])
        la.reduce_max(v["x"], out=v["max"])

    case(f"reduce_{s}", "reduce", [f"laser_hip_reduce_{op}_{s}_dev" for op in ("sum", "min", "max")], build, call, ("sum", "min", "max"),
         scratch=True)


for _k, _dt in enumerate((np.float32, np.float64, np.int32, np.int64)):
    _reduce_case(_dt, 72 + _k)


# -- pointwise and softmax ---------------------------------------------------------------------------------------------------------
def _pointwise_cases():
    shape = (37, 131)

    def build(seed):
        r = _rng(seed, 80)
        b = {"x": _f(r, shape, lo=-4, hi=4), "p": _f(r, shape, lo=0.01, hi=9.0), "dy": _f(r, shape)}
        b.update({k: np.zeros(shape, np.float32) for k in ("exp", "log", "act", "grad", "sin", "cos", "s2", "c2")})
        return b

    def call(la, v):
        la.exp(v["x"], out=v["exp"])
        la.log(v["p"], out=v["log"])
        la.activation(v["x"], "tanh", out=v["act"])
        la.activation_grad(v["dy"], v["act"], "tanh", out=v["grad"])          # reads the result of the launch before it
        la.sin(v["x"], out=v["sin"])
        la.cos(v["x"], out=v["cos"])
        la.sincos(v["x"], out=(v["s2"], v["c2"]))

    names = ("exp", "log", "act", "act_grad", "sin", "cos", "sincos")
    case("pointwise", "pointwise", [f"laser_hip_{k}_f32_dev" for k in names], build, call,
         ("exp", "log", "act", "grad", "sin", "cos", "s2", "c2"), rules={"p": "positive"})


_pointwise_cases()


def _softmax_rows_case(n, code):
    rows = 5

    def build(seed):
        r = _rng(seed, 81 + code)
        b = {"x": _f(r, (rows, n), lo=-3, hi=3), "dy": _f(r, (rows, n)), "labels": r.integers(0, n, (rows,)).astype(np.int32)}
        b.update({k: np.zeros((rows, n), np.float32) for k in ("y", "dx", "ls", "g")})
        b.update({k: np.zeros((rows,), np.float32) for k in ("lse", "loss")})
        return b

    def call(la, v):
        from laser_amd import _lib
        la.softmax(v["x"], out=v["y"])
        assert la.get_option("last_softmax_kernel") & 3 == code, (n, la.get_option("last_softmax_kernel"))
        la.softmax_backward(v["dy"], v["y"], out=v["dx"])                     # reads the softmax launched just before
        assert _lib.lib().laser_hip_softmax_grad_last_kernel() & 3 == code, (n, _lib.lib().laser_hip_softmax_grad_last_kernel())
        la.logsumexp(v["x"], out=v["lse"])
        la.log_softmax(v["x"], out=v["ls"])
        _ok(_L().laser_hip_softmax_xent_rows_f32_dev(_ptr(v["loss"]), 1, _ptr(v["g"]), n, _ptr(v["x"]), n, _ptr(v["labels"]), rows, n,
                                                     0.25, _st()))

    syms = ["softmax_rows", "softmax_grad_rows", "logsumexp_rows", "log_softmax_rows", "softmax_xent_rows"]
    case(f"softmax_rows_n{n}", "softmax", [f"laser_hip_{k}_f32_dev" for k in syms], build, call, ("y", "dx", "lse", "ls", "loss", "g"),
         rules={"labels": ("ids", n)})


for _n, _code in ((1024, 0), (8192, 1), (8193, 2)):
    _softmax_rows_case(_n, _code)


def _softmax_axis_case(shape, axis, code, salt):
    def build(seed):
        return {"x": _f(_rng(seed, salt), shape, lo=-3, hi=3), "y": np.zeros(shape, np.float32)}

    def call(la, v):
        la.softmax(v["x"], out=v["y"], axis=axis)
        assert la.get_option("last_softmax_kernel") & 11 == code, (shape, axis, la.get_option("last_softmax_kernel"))

    case(f"softmax_axis_code{code}", "softmax", ["laser_hip_softmax_axis_f32_dev"], build, call, ("y",))


_softmax_axis_case((3, 1500, 1), 1, 1, 85)            # inner == 1: the row kernels
_softmax_axis_case((2, 2048, 20), 1, 8, 86)           # a column strip, resident
_softmax_axis_case((2, 2049, 20), 1, 9, 87)           # a column strip, streaming


# -- layers ------------------------------------------------------------------------------------------------------------------------
def _copy_out(la, dst, t):
    la.copyFrom(la.fromTorch(dst.view(t.shape)), t)


def _dense_cases():
    rows, n, k = 8193, 24, 16          # rows > 8192: chunk partials in stream-ordered scratch

    def build(seed):
        r = _rng(seed, 90)
        b = {"dy": _f(r, (rows, n)), "y": _f(r, (rows, n)), "x": _f(r, (rows, k)), "w": _f(r, (k, n))}
        b.update({"db": np.zeros((n,), np.float32), "dz": np.zeros((rows, n), np.float32)})
        b.update({"dx": np.zeros((rows, k), np.float32), "dw": np.zeros((k, n), np.float32), "db2": np.zeros((n,), np.float32)})
        return b

    def call(la, v):
        la.bias_grad(v["dy"], v["y"], "tanh", dz=v["dz"], out=v["db"])
        dx, dw, db = la.linear_backward(v["x"], v["w"], v["dy"], v["y"], "sigmoid")
        _copy_out(la, v["dw"], dw) if hasattr(dw, "unsafe_raw_data") else v["dw"].copy_(dw)
        _copy_out(la, v["dx"], dx) if hasattr(dx, "unsafe_raw_data") else v["dx"].copy_(dx)
        _copy_out(la, v["db2"], db)

    case("dense_backward", "layers", ["laser_hip_bias_grad_f32_dev"], build, call, ("db", "dz", "dx", "dw", "db2"), scratch=True)


_dense_cases()


def _layer_norm_cases():
    rows, n = 8193, 20                 # parameter gradients over 8193 rows: two levels

    def build(seed):
        r = _rng(seed, 91)
        b = {"x": _f(r, (rows, n)), "gamma": _f(r, (n,)), "beta": _f(r, (n,)), "dy": _f(r, (rows, n))}
        b.update({k: np.zeros((rows, n), np.float32) for k in ("y", "dx")})
        b.update({k: np.zeros((rows,), np.float32) for k in ("mean", "rstd")})
        b.update({k: np.zeros((n,), np.float32) for k in ("dgamma", "dbeta")})
        return b

    def call(la, v):
        _, mean, rstd = la.layer_norm(v["x"], v["gamma"], v["beta"], out=v["y"])
        dx, dgamma, dbeta = la.layer_norm_backward(v["dy"], v["x"], mean, rstd, v["gamma"], need_dx=v["dx"])
        for k, t in (("mean", mean), ("rstd", rstd), ("dgamma", dgamma), ("dbeta", dbeta)):
            _copy_out(la, v[k], t)

    case("layer_norm", "layers", ["laser_hip_layer_norm_f32_dev", "laser_hip_layer_norm_grad_f32_dev"], build, call,
         ("y", "dx", "mean", "rstd", "dgamma", "dbeta"), scratch=True)


_layer_norm_cases()


def _embedding_cases():
    vocab, dim, tokens = 301, 24, 9001

    def build(seed):
        r = _rng(seed, 92)
        b = {"w": _f(r, (vocab, dim)), "idx": r.integers(0, vocab, (tokens,)).astype(np.int32), "dy": _f(r, (tokens, dim))}
        b.update({"y": np.zeros((tokens, dim), np.float32), "dw": np.zeros((vocab, dim), np.float32), "dw2": np.zeros((vocab, dim), np.float32),
                  "order": np.zeros((tokens,), np.int32), "starts": np.zeros((vocab + 1,), np.int32)})
        return b

    def call(la, v):
        la.embedding(v["w"], v["idx"], out=v["y"])
        la.embedding_backward(v["dy"], v["idx"], vocab, out=v["dw"])                       # groups by itself, in scratch
        order, starts = la.embedding_group(v["idx"], vocab)
        la.embedding_backward(v["dy"], v["idx"], vocab, out=v["dw2"], group=(order, starts))
        _copy_out(la, v["order"], order)
        _copy_out(la, v["starts"], starts)

    case("embedding", "layers", ["laser_hip_embedding_f32_dev", "laser_hip_embedding_group_i32_dev", "laser_hip_embedding_grad_f32_dev"],
         build, call, ("y", "dw", "dw2", "order", "starts"), rules={"idx": ("ids", vocab)}, scratch=True)


_embedding_cases()


def _optim_cases():
    lens = (5, 40_000, 1, 9001)        # several tensors; grad_norm takes stream-ordered scratch

    def build(seed):
        r = _rng(seed, 93)
        b = {}
        for k, n in enumerate(lens):
            b.update({f"w{k}": _f(r, (n,)), f"g{k}": _f(r, (n,)), f"m{k}": _f(r, (n,), lo=-0.1, hi=0.1), f"v{k}": _f(r, (n,), lo=0.0, hi=0.1),
                      f"p{k}": _f(r, (n,)), f"q{k}": _f(r, (n,), lo=-0.1, hi=0.1)})
        b["norm"] = np.zeros((1,), np.float32)
        return b

    def lists(v, key):
        return [v[f"{key}{k}"] for k in range(len(lens))]

    def call(la, v):
        norm, clip = la.grad_norm(lists(v, "g"), max_norm=0.5)       # clips: the norm of ~49 000 uniform values is far above 0.5
        la.sgd_step(lists(v, "p"), lists(v, "g"), lists(v, "q"), lr=0.1, mu=0.9, wd=0.01, nesterov=True, clip=clip)   # no host wait between
        la.adam_step(lists(v, "w"), lists(v, "g"), lists(v, "m"), lists(v, "v"), 3, lr=0.01, wd=0.01, clip=clip)
        _copy_out(la, v["norm"], norm)

    state = tuple(f"{key}{k}" for key in "wmvpq" for k in range(len(lens)))
    case("optim", "layers", ["laser_hip_grad_norm_f32_dev", "laser_hip_sgd_step_f32_dev", "laser_hip_adam_step_f32_dev"], build, call,
         ("norm",), inplace=state, scratch=True)


_optim_cases()


def _attention_cases():
    def fwd_build(seed):
        r = _rng(seed, 94)
        b, h, tq, tk, d, dv = 1, 2, 5, 8193, 16, 8          # Tk = 8193: chunk partials
        out = {"q": _f(r, (b, h, tq, d)), "k": _f(r, (b, h, tk, d)), "v": _f(r, (b, h, tk, dv))}
        out.update({"o": np.zeros((b, h, tq, dv), np.float32), "probs": np.zeros((b, h, tq, tk), np.float32)})
        return out

    def fwd_call(la, v):
        la.attention(v["q"], v["k"], v["v"], out=v["o"], probs=v["probs"])

    case("attention_tk8193_probs", "attention", ["laser_hip_attention_f32_dev"], fwd_build, fwd_call, ("o", "probs"), scratch=True)

    def bwd(causal):
        b, h, t, d = 2, 2, 70, 16

        def build(seed):
            r = _rng(seed, 95 + causal)
            out = {k: _f(r, (b, h, t, d)) for k in ("q", "k", "v", "do")}
            out.update({k: np.zeros((b, h, t, d), np.float32) for k in ("dq", "dk", "dv")})
            return out

        def call(la, v):
            grads = la.attention_backward(v["do"], v["q"], v["k"], v["v"], causal=bool(causal))
            for k, g in zip(("dq", "dk", "dv"), grads):
                _copy_out(la, v[k], g)

        case(f"attention_backward_{'causal' if causal else 'full'}", "attention", ["laser_hip_attention_f32_dev"], build, call,
             ("dq", "dk", "dv"), scratch=True)

    bwd(0)
    bwd(1)


_attention_cases()


# -- sampling, scans and random ----------------------------------------------------------------------------------------------------
def _tree_elems(n):
    p = 1
    while p < n:
        p *= 2
    return 2 * p


def _sampler_case():
    rows, n, m, k = 6, 1000, 50, 7      # P = 1024 > 512: the two-launch build
    te = _tree_elems(n)

    def build(seed):
        r = _rng(seed, 100)
        b = {"w": _f(r, (rows, n), lo=0.01, hi=1.0), "u": _f(r, (rows, m), lo=0.0, hi=0.999), "u2": _f(r, (rows, k), lo=0.0, hi=0.999),
             "elem": r.integers(0, n, (rows,)).astype(np.int32), "neww": _f(r, (rows,), lo=0.5, hi=5.0),
             "seed": np.int64(1234 + seed)}
        b.update({"tree": np.zeros((rows, te), np.float32), "i1": np.zeros((rows, m), np.int32), "i2": np.zeros((rows, m), np.int32),
                  "i3": np.zeros((rows, k), np.int32), "i4": np.zeros((rows, k), np.int32)})
        return b

    def call(la, v):
        L, s, seed = _L(), _st(), int(v["seed"])
        _ok(L.laser_hip_sampler_build_f32_dev(_ptr(v["tree"]), te, _ptr(v["w"]), n, rows, n, s))        # the tree: made on the stream
        _ok(L.laser_hip_sampler_sample_f32_dev(_ptr(v["i1"]), _ptr(v["tree"]), te, _ptr(v["u"]), rows, n, m, s))
        _ok(L.laser_hip_sampler_sample_rng_f32_dev(_ptr(v["i2"]), _ptr(v["tree"]), te, seed, 1, 5, rows, n, m, s))
        _ok(L.laser_hip_sampler_update_f32_dev(_ptr(v["tree"]), te, _ptr(v["elem"]), _ptr(v["neww"]), rows, n, s))
        _ok(L.laser_hip_sampler_sample_remove_f32_dev(_ptr(v["i3"]), _ptr(v["tree"]), te, _ptr(v["u2"]), rows, n, k, s))
        _ok(L.laser_hip_sampler_sample_remove_rng_f32_dev(_ptr(v["i4"]), _ptr(v["tree"]), te, seed, 2, 0, rows, n, k, s))

    syms = ["build", "sample", "sample_rng", "update", "sample_remove", "sample_remove_rng"]
    case("sampler", "sampling", [f"laser_hip_sampler_{k}_f32_dev" for k in syms], build, call, ("tree", "i1", "i2", "i3", "i4"), host=("seed",),
         rules={"w": "positive", "neww": "positive", "u": "unit", "u2": "unit", "elem": ("ids", n)}, scratch=True)


_sampler_case()


def _scan_case(dtype, salt):
    s = _SFX[np.dtype(dtype).name]
    rows, n, m = 3, 20_001, 77

    def build(seed):
        r = _rng(seed, salt)
        if np.dtype(dtype).kind == "f":
            x, a, v = _f(r, (rows, n), dtype, 0.0, 1.0), np.sort(_f(r, (rows, n), dtype), axis=1), _f(r, (rows, m), dtype)
        else:
            x = r.integers(0, 50, (rows, n)).astype(dtype)
            a, v = np.sort(r.integers(-9000, 9000, (rows, n)).astype(dtype), axis=1), r.integers(-9000, 9000, (rows, m)).astype(dtype)
        return {"x": x, "a": a, "v": v, "cs": np.zeros((rows, n), dtype), "il": np.zeros((rows, m), np.int32), "ir": np.zeros((rows, m), np.int32)}

    def call(la, b):
        L, st = _L(), _st()
        _ok(getattr(L, f"laser_hip_cumsum_{s}_dev")(_ptr(b["cs"]), n, _ptr(b["x"]), n, rows, n, st))
        _ok(getattr(L, f"laser_hip_searchsorted_{s}_dev")(_ptr(b["il"]), _ptr(b["a"]), n, _ptr(b["v"]), rows, n, m, 0, st))
        _ok(getattr(L, f"laser_hip_searchsorted_{s}_dev")(_ptr(b["ir"]), _ptr(b["cs"]), n, _ptr(b["v"]), rows, n, m, 1, st))   # in the scan just made

    case(f"scan_{s}", "sampling", [f"laser_hip_cumsum_{s}_dev", f"laser_hip_searchsorted_{s}_dev"], build, call, ("cs", "il", "ir"),
         rules={"a": "sorted"})


for _k, _dt in enumerate((np.float32, np.float64, np.int32, np.int64)):
    _scan_case(_dt, 101 + _k)


def _cdf_case():
    rows, n, m, k = 4, 3000, 40, 6

    def build(seed):
        r = _rng(seed, 105)
        w = _f(r, (rows, n), lo=0.01, hi=1.0)
        cdf = np.cumsum(w.astype(np.float64), axis=1).astype(np.float32)
        b = {"cdf": cdf, "w": w, "w2": _f(r, (rows, n), lo=0.01, hi=1.0), "u": _f(r, (rows, m), lo=0.0, hi=0.999),
             "u2": _f(r, (rows, k), lo=0.0, hi=0.999), "seed": np.int64(99 + seed)}
        b.update({"i1": np.zeros((rows, m), np.int32), "i2": np.zeros((rows, m), np.int32), "i3": np.zeros((rows, k), np.int32),
                  "i4": np.zeros((rows, k), np.int32), "ws": np.zeros((rows, n), np.float32)})
        return b

    def call(la, v):
        L, s, seed = _L(), _st(), int(v["seed"])
        _ok(L.laser_hip_cdf_sample_f32_dev(_ptr(v["i1"]), _ptr(v["cdf"]), n, _ptr(v["u"]), rows, n, m, s))
        _ok(L.laser_hip_cdf_sample_rng_f32_dev(_ptr(v["i2"]), _ptr(v["cdf"]), n, seed, 0, 3, rows, n, m, s))
        _ok(L.laser_hip_cdf_sample_remove_f32_dev(_ptr(v["i3"]), _ptr(v["w"]), n, _ptr(v["ws"]), n, _ptr(v["u2"]), rows, n, k, s))
        _ok(L.laser_hip_cdf_sample_remove_rng_f32_dev(_ptr(v["i4"]), _ptr(v["w2"]), n, _ptr(v["ws"]), n, seed, 1, 0, rows, n, k, s))

    syms = ["cdf_sample", "cdf_sample_rng", "cdf_sample_remove", "cdf_sample_remove_rng"]
    case("cdf_sample", "sampling", [f"laser_hip_{k}_f32_dev" for k in syms], build, call, ("i1", "i2", "i3", "i4", "ws"), inplace=("w", "w2"),
         host=("seed",), rules={"cdf": "cdf", "w": "positive", "w2": "positive", "u": "unit", "u2": "unit"}, scratch=True)


_cdf_case()


def _random_case():
    n = 100_003

    def build(seed):
        b = {"seed": np.int64(7 + seed)}
        b.update({"bits": np.zeros(n, np.uint32), "f32": np.zeros(n, np.float32), "f64": np.zeros(n, np.float64), "i32": np.zeros(n, np.int32),
                  "i64": np.zeros(n, np.int64), "nrm": np.zeros(n, np.float32)})
        return b

    def call(la, v):
        """no operand: a fill that is not ordered on the stream is overwritten by the sentinel queued behind the gate"""
        L, s, seed = _L(), _st(), int(v["seed"])
        _ok(L.laser_hip_random_bits_u32_dev(_ptr(v["bits"]), n, seed, 0, 0, s))
        _ok(L.laser_hip_random_uniform_f32_dev(_ptr(v["f32"]), n, -1.0, 2.0, seed, 1, 0, s))
        _ok(L.laser_hip_random_uniform_f64_dev(_ptr(v["f64"]), n, -1.0, 2.0, seed, 2, 0, s))
        _ok(L.laser_hip_random_uniform_i32_dev(_ptr(v["i32"]), n, -5, 100, seed, 3, 0, s))
        _ok(L.laser_hip_random_uniform_i64_dev(_ptr(v["i64"]), n, -5, 1 << 40, seed, 4, 0, s))
        _ok(L.laser_hip_random_normal_f32_dev(_ptr(v["nrm"]), n, 0.5, 2.0, seed, 5, 0, s))

    syms = ["bits_u32", "uniform_f32", "uniform_f64", "uniform_i32", "uniform_i64", "normal_f32"]
    case("random_fills", "random", [f"laser_hip_random_{k}_dev" for k in syms], build, call, ("bits", "f32", "f64", "i32", "i64", "nrm"),
         host=("seed",))


_random_case()


# -- one chained case: two training steps of an attention block, issued entirely behind one gate ---------------------------------------
def _chain_case():
    t, d = 48, 16

    def build(seed):
        r = _rng(seed, 110)
        b = {"x": r.normal(0, 1, (t, d)).astype(np.float32), "target": r.normal(0, 1, (1, t, d)).astype(np.float32)}
        b.update({f"w{k}": r.normal(0, 0.3, (d, d)).astype(np.float32) for k in range(3)})
        return b

    def call(la, v):
        import torch
        w = [v[f"w{k}"] for k in range(3)]
        for _ in range(2):
            q, k, vv = (la.matmul(v["x"], wi).reshape(1, t, d) for wi in w)
            o = la.attention(q, k, vv, causal=True, out=torch.empty(1, t, d, device="cuda"))
            do = o - v["target"]
            grads = la.attention_backward(do, q, k, vv, causal=True)
            gw = [la.matmul(v["x"].T, g[0]) for g in grads]
            la.sgd_step(w, gw, lr=0.01)

    case("chain_training_steps", "chain", [], build, call, (), inplace=("w0", "w1", "w2"), scratch=True)


_chain_case()


# ---- the negative controls: fake cases the harness must report ----------------------------------------------------------------------
def _control_build(seed):
    return {"x": _f(_rng(seed, 120), (4099,), lo=-2, hi=2), "y": np.zeros((4099,), np.float32)}


def _control_null_call(la, v):
    """a real entry point on the NULL stream while S is blocked: it reads the (valid) decoy"""
    one = _i64s([1])
    _ok(_L().laser_hip_exp_f32_dev(_ptr(v["y"]), one, _ptr(v["x"]), one, _i64s([4099]), 1, None))


def _control_sync_call(la, v):
    import torch
    torch.cuda.current_stream().synchronize()
    la.exp(v["x"], out=v["y"])


def _control_good_call(la, v):
    la.exp(v["x"], out=v["y"])


CONTROL_NULL_STREAM = Case("control_null_stream", "control", [], _control_build, _control_null_call, ("y",), warm_call=_control_good_call)
CONTROL_HOST_SYNC = Case("control_host_sync", "control", [], _control_build, _control_sync_call, ("y",), warm_call=_control_good_call)
