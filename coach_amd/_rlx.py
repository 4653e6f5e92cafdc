"""ctypes binding of librlx.so — the only way the Python adapters reach the HIP kernels.

``include/rlx.h`` is the single definition of the C ABI, and everything that crosses the boundary is read from it when
this module is imported: the prototypes (``parse_header``), the descriptor structures (``parse_structs`` -> the
``ctypes.Structure`` classes named in ``STRUCT_NAMES``), the ``#define`` / enum constants (``parse_constants``) and the
ABI version.  Nothing here repeats a field list or a number of the header; a new structure, constant or entry point is
added in rlx.h alone (within the grammar its opening comment states) and a structure gets its class name in
``STRUCT_NAMES``.  tests/test_abi_layout.py pins the generated layouts to what a C compiler makes of the same header.
A symbol that is declared but not exported — or the other way round — fails at load time, and so does a library built
from another RLX_ABI_VERSION.
There is deliberately NO fallback: if the library cannot be loaded the product path raises
(``RlxUnavailable``); nothing under ``oracle/`` is ever imported from here.
"""
import ctypes
import os
import re
import subprocess
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
HEADER = os.path.join(_ROOT, "include", "rlx.h")
LIB_PATH = os.path.join(_HERE, "librlx.so")
CSRC = os.path.join(_HERE, "csrc")


class RlxUnavailable(RuntimeError):
    """librlx.so is missing or cannot be loaded; the HIP hot path cannot run."""


class RlxError(RuntimeError):
    """A librlx entry point returned a non-zero rlx_status."""


_CTYPE = {
    "int": ctypes.c_int,
    "unsigned": ctypes.c_uint,
    "unsigned int": ctypes.c_uint,
    "unsigned char": ctypes.c_ubyte,
    "float": ctypes.c_float,
    "double": ctypes.c_double,
    "long long": ctypes.c_longlong,
    "int64_t": ctypes.c_int64,
    "uint64_t": ctypes.c_uint64,
    "uint32_t": ctypes.c_uint32,
    "size_t": ctypes.c_size_t,
}

_DECL = re.compile(r"^\s*(int|const char \*)\s*(rlx_\w+)\s*\(([^;{]*?)\)\s*;", re.M | re.S)
_STRUCT = re.compile(r"typedef\s+struct\s+(rlx_\w+)\s*\{(.*?)\}\s*\1\s*;", re.S)
_MEMBER = re.compile(r"^([\w ]+?) ?((?:\*+ ?)?\w+(?: ?, ?(?:\*+ ?)?\w+)*)$")    # <type> <declarator>, <declarator> ...
_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(RLX_\w+)[ \t]+(-?\d+)[ \t]*$", re.M)
_ENUM = re.compile(r"\benum\b[^{;]*\{([^}]*)\}")


def returns_value(name):
    """rlx.h's naming rule: rlx_abi_version and every rlx_*_supported return a value, not an rlx_status."""
    return name == "rlx_abi_version" or name.endswith("_supported")


def header_text(path=HEADER):
    """rlx.h without its comments."""
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def parse_header(path=HEADER):
    """Return {name: (restype, [(ctype, param_name), ...])} for every declaration in rlx.h."""
    text = header_text(path)
    protos = {}
    for ret, name, args in _DECL.findall(text):
        params = []
        args = " ".join(args.split())
        if args and args != "void":
            for a in args.split(","):
                a = a.strip()
                m = re.match(r"^(.*?)(\w+)$", a)
                ctype_s, pname = m.group(1).strip(), m.group(2)
                if "*" in ctype_s:
                    params.append((ctypes.c_void_p, pname))
                else:
                    key = ctype_s.replace("const ", "").strip()
                    if key not in _CTYPE:
                        raise ValueError("rlx.h: unknown parameter type %r in %s" % (ctype_s, name))
                    params.append((_CTYPE[key], pname))
        protos[name] = (ctypes.c_char_p if "char" in ret else ctypes.c_int, params)
    return protos


def parse_structs(text, names):
    """{rlx_NAME: ctypes.Structure subclass called names[rlx_NAME]} for every `typedef struct rlx_NAME { ... } rlx_NAME;`
    of `text` (a header without comments), in declaration order.  Accepts the grammar rlx.h states and nothing else:
    scalar members of the types in _CTYPE, pointers (all c_void_p), earlier structures by value; anything else — an
    array, a bit-field, a union, a function pointer, an unknown type — is a ValueError naming structure and statement."""
    structs = {}
    found = _STRUCT.findall(text)
    if len(found) != len(re.findall(r"\btypedef\s+struct\b", text)):
        raise ValueError("rlx.h: a structure that is not written `typedef struct rlx_NAME { ... } rlx_NAME;` (after %s)"
                         % ", ".join(n for n, _ in found))
    for name, body in found:
        if name not in names:
            raise ValueError("rlx.h: struct %s has no class name in the table of coach_amd/_rlx.py" % name)
        fields = []
        for stmt in body.split(";"):
            stmt = " ".join(stmt.split())
            if not stmt:
                continue
            m = _MEMBER.match(stmt)
            if not m:
                raise ValueError("rlx.h: struct %s: %r is outside the accepted grammar (scalars, pointers and earlier "
                                 "structures by value; no arrays, bit-fields, unions or function pointers)" % (name, stmt))
            base = re.sub(r"^const ", "", m.group(1))
            for decl in m.group(2).split(","):
                if "*" in decl:         # every pointer is a c_void_p; what it points to must still be a known type
                    known = base == "void" or base in _CTYPE or base in structs or re.fullmatch(r"struct rlx_\w+", base)
                    ctype = ctypes.c_void_p if known else None
                else:
                    ctype = _CTYPE.get(base) or structs.get(base)
                if ctype is None:
                    raise ValueError("rlx.h: struct %s: unknown type %r in %r" % (name, base, stmt))
                fields.append((decl.strip("* "), ctype))
        structs[name] = type(names[name], (ctypes.Structure,),
                             {"_fields_": fields, "__doc__": "%s (include/rlx.h)." % name, "__module__": __name__})
    return structs


def parse_constants(text):
    """{RLX_NAME: int} of every `#define RLX_NAME <integer>` and every enumerator of `text` (a header without comments)."""
    consts = {k: int(v) for k, v in _DEFINE.findall(text)}
    for body in _ENUM.findall(text):
        for item in filter(None, (" ".join(i.split()) for i in body.split(","))):
            m = re.fullmatch(r"(RLX_\w+) ?= ?(-?\d+)", item)
            if not m:
                raise ValueError("rlx.h: enumerator %r needs an explicit integer value" % item)
            consts[m.group(1)] = int(m.group(2))
    return consts


def build_library(verbose=False):
    """Compile every csrc/*.hip for gfx950 into coach_amd/librlx.so (hipcc cross-compiles on CPU)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        raise RlxUnavailable("hipcc not found at %s; cannot build librlx.so" % hipcc)
    jobs = str(max(1, min(16, os.cpu_count() or 1)))
    res = subprocess.run(["make", "-C", CSRC, "-j", jobs, "HIPCC=" + hipcc],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout)
    if res.returncode != 0:
        raise RlxUnavailable("building librlx.so failed (see output above)")
    return LIB_PATH


def _as_arg(a):
    # torch tensors (and anything with data_ptr) are passed as raw device pointers
    if hasattr(a, "data_ptr"):
        if hasattr(a, "is_contiguous") and not a.is_contiguous():
            raise ValueError("librlx expects contiguous tensors")
        return a.data_ptr()
    return a


class _Lib:
    def __init__(self):
        # torch must load ITS libamdhip64.so.7 first so that device pointers, streams and events
        # are shared between torch and librlx (same soname -> the dynamic linker reuses it).
        import torch  # noqa: F401

        if not os.path.exists(LIB_PATH):
            if os.path.exists("/opt/rocm/bin/hipcc"):
                build_library()
            else:
                raise RlxUnavailable(
                    "%s is missing and hipcc is not available to build it. Run "
                    "`python -c 'import __graft_entry__ as g; g.build()'`." % LIB_PATH)
        try:
            self._dll = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
        except OSError as e:  # pragma: no cover - depends on the box
            raise RlxUnavailable("cannot load %s: %s" % (LIB_PATH, e))
        self.protos = parse_header()
        self._fns = {}
        missing = []
        for name, (restype, params) in self.protos.items():
            try:
                fn = getattr(self._dll, name)
            except AttributeError:
                missing.append(name)
                continue
            fn.restype = restype
            fn.argtypes = [t for t, _ in params]
            self._fns[name] = fn
        if missing:
            raise RlxUnavailable("librlx.so does not export: " + ", ".join(missing))
        built = self._fns["rlx_abi_version"]()
        if built != ABI_VERSION:             # struct layouts / buffer contracts of this package and of the binary differ
            raise RlxUnavailable("%s is ABI version %d, this package drives version %d: rebuild it "
                                 "(python -c 'import __graft_entry__ as g; g.build()')" % (LIB_PATH, built, ABI_VERSION))

    def raw(self, name):
        return self._fns[name]

    def last_error(self):
        return self._fns["rlx_last_error"]().decode()

    def __getattr__(self, name):
        fns = self.__dict__.get("_fns", {})
        full = name if name.startswith("rlx_") else "rlx_" + name
        if full not in fns:
            raise AttributeError(name)
        fn = fns[full]
        nparams = len(self.protos[full][1])
        if fn.restype is ctypes.c_char_p:
            def call_str(*args):
                return fn(*args).decode()
            return call_str
        if returns_value(full):
            return fn

        def call(*args):
            global CALL_COUNT
            CALL_COUNT += 1
            if len(args) != nparams:
                raise TypeError("%s expects %d arguments, got %d" % (full, nparams, len(args)))
            rc = fn(*[_as_arg(a) for a in args])
            if rc != 0:
                raise RlxError("%s failed (%d): %s" % (full, rc, self.last_error()))
            return rc
        call.__name__ = full
        setattr(self, name, call)
        return call


_lock = threading.Lock()
_lib = None


def lib():
    """The loaded library (singleton). Raises RlxUnavailable — never falls back."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                _lib = _Lib()
    return _lib


def current_stream():
    """hipStream_t of torch's current stream, as an int usable for the `stream` parameters."""
    import torch
    return torch.cuda.current_stream().cuda_stream


class KernelTimer(object):
    """`with KernelTimer(max_records) as t: <eager librlx calls>` -> t.records = [(kernel name, microseconds), ...] in
    launch order: every kernel the library launched inside the block, timed by its own dispatch timestamps
    (rlx_profile_*, include/rlx.h).  Not usable inside a stream capture."""

    def __init__(self, max_records=4096):
        self.max_records, self.records = int(max_records), []

    def __enter__(self):
        lib().profile_begin(self.max_records)
        return self

    def __exit__(self, *exc):
        n = ctypes.c_int()
        try:
            lib().profile_end(ctypes.byref(n))       # raises when launches overflowed max_records (an undercounting trace)
        except Exception:
            if exc[0] is None:
                raise
        if exc[0] is None:
            name, ms = ctypes.c_char_p(), ctypes.c_float()
            for i in range(n.value):
                lib().profile_read(i, ctypes.byref(name), ctypes.byref(ms))
                self.records.append((name.value.decode().strip("()"), 1e3 * ms.value))
        return False


# ------------------------------------------------- ABI structures and constants, read from rlx.h
STRUCT_NAMES = {          # rlx.h structure -> its class in this module (bound below, so that the names are static)
    "rlx_column": "Column", "rlx_gemm_desc": "GemmDesc", "rlx_splitk_job": "SplitkJob", "rlx_noisy_layer": "NoisyLayer",
    "rlx_per_update_desc": "PerUpdateDesc", "rlx_conv_dw_item": "ConvDwItem",
    "rlx_small_dense_problem": "SmallDenseProblem", "rlx_mlp_dqn_desc": "MlpDqnDesc", "rlx_mlp3": "Mlp3",
    "rlx_fused_net": "FusedNet", "rlx_td3_fused_desc": "Td3FusedDesc", "rlx_sac_fused_desc": "SacFusedDesc",
    "rlx_ppo_fc_heads_desc": "PpoFcHeadsDesc", "rlx_ppo_rows_desc": "PpoRowsDesc", "rlx_observe_desc": "ObserveDesc",
    "rlx_signal_source": "SignalSource", "rlx_adam_split_desc": "AdamSplitDesc",
}
_TEXT = header_text()
STRUCTS = parse_structs(_TEXT, STRUCT_NAMES)
CONSTANTS = parse_constants(_TEXT)

Column, GemmDesc, NoisyLayer = STRUCTS["rlx_column"], STRUCTS["rlx_gemm_desc"], STRUCTS["rlx_noisy_layer"]
PerUpdateDesc, ConvDwItem = STRUCTS["rlx_per_update_desc"], STRUCTS["rlx_conv_dw_item"]
SmallDenseProblem, MlpDqnDesc = STRUCTS["rlx_small_dense_problem"], STRUCTS["rlx_mlp_dqn_desc"]
Mlp3, FusedNet = STRUCTS["rlx_mlp3"], STRUCTS["rlx_fused_net"]
Td3FusedDesc, SacFusedDesc = STRUCTS["rlx_td3_fused_desc"], STRUCTS["rlx_sac_fused_desc"]
PpoFcHeadsDesc, PpoRowsDesc = STRUCTS["rlx_ppo_fc_heads_desc"], STRUCTS["rlx_ppo_rows_desc"]
ObserveDesc, SignalSource = STRUCTS["rlx_observe_desc"], STRUCTS["rlx_signal_source"]
AdamSplitDesc = STRUCTS["rlx_adam_split_desc"]


class SplitkJob(STRUCTS["rlx_splitk_job"]):
    __doc__ = STRUCTS["rlx_splitk_job"].__doc__

    def workspace_floats(self):
        """floats of the workspace the outstanding reduction still reads (0 when nothing is outstanding)."""
        return (self.M * self.N + self.N) * self.batch * self.splits if self.splits > 1 else 0


ABI_VERSION = CONSTANTS["RLX_ABI_VERSION"]      # rlx_abi_version() of a library built from the same header
NOISY_PASSES = CONSTANTS["RLX_NOISY_PASSES"]
NOISY_MAX_LAYERS = CONSTANTS["RLX_NOISY_MAX_LAYERS"]        # layers of one rlx_noisy_sample launch
NOISY_PASS = {"act": 0, "online": 1, "target": 2, "online_next": 3}
assert sorted(NOISY_PASS.values()) == list(range(NOISY_PASSES)), "NOISY_PASS names every pass of RLX_NOISY_PASSES"
ADAM_TICKET_WORDS = CONSTANTS["RLX_ADAM_TICKET_WORDS"]
MAX_SPLITK_JOBS = CONSTANTS["RLX_MAX_SPLITK_JOBS"]
MAX_COLUMNS = CONSTANTS["RLX_MAX_COLUMNS"]
A3C_TARGETS_GIVEN = CONSTANTS["RLX_A3C_TARGETS_GIVEN"]     # rlx_a3c_window_loss reads the targets it is handed
# rlx_nstep_q_window_loss: the targets horizon by the reference's name; TARGETS_GIVEN reads the targets it is handed
NSTEPQ_HORIZON = {"N-Step": CONSTANTS["RLX_NSTEPQ_N_STEP"], "1-Step": CONSTANTS["RLX_NSTEPQ_ONE_STEP"]}
NSTEPQ_TARGETS_GIVEN = CONSTANTS["RLX_NSTEPQ_TARGETS_GIVEN"]
# rlx_acer_window_loss's mode bits: the trust-region step on the gradient; the window's arrays are handed in, not computed
ACER_TRUST_REGION, ACER_TARGETS_GIVEN = CONSTANTS["RLX_ACER_TRUST_REGION"], CONSTANTS["RLX_ACER_TARGETS_GIVEN"]
ACT = {None: CONSTANTS["RLX_ACT_NONE"]}         # activation codes by name: {None: 0, "none": 0, "relu": 1, "tanh": 2}
ACT.update((k[len("RLX_ACT_"):].lower(), v) for k, v in CONSTANTS.items() if k.startswith("RLX_ACT_"))


def make_columns(pairs):
    """[(src_tensor, dst_tensor), ...] -> rlx_column[]; rows run along dim 0 of every tensor."""
    arr = (Column * len(pairs))()
    for i, (s, d) in enumerate(pairs):
        rb = (s[0].numel() if s.dim() > 1 else 1) * s.element_size()
        arr[i] = Column(s.data_ptr(), d.data_ptr(), rb)
    return arr


def splitk_reduce_jobs(jobs, stream=None, ppo_tail=None, per_tail=None):
    """sum the partials of the deferred products `jobs` (SplitkJob list) in one launch.
    ppo_tail: a PpoRowsDesc whose all-rows part (rlx_ppo_heads_tail) rides on the (last) launch as extra workgroups.
    per_tail: the argument tuple of rlx_per_update (without the stream) — the prioritized replay's priority update rides on
    the (last) launch as one workgroup (rlx_splitk_reduce_jobs_per_update)."""
    live = [j for j in jobs if j.splits > 1]
    s = current_stream() if stream is None else stream
    for i in range(0, len(live), MAX_SPLITK_JOBS):
        chunk = live[i:i + MAX_SPLITK_JOBS]
        arr = (SplitkJob * len(chunk))(*chunk)
        if per_tail is not None and ppo_tail is None and i + MAX_SPLITK_JOBS >= len(live):
            run = lambda a=arr, n=len(chunk), t=per_tail: lib().splitk_reduce_jobs_per_update(ctypes.byref(a), n, *t, s)
            per_tail = None
        elif ppo_tail is not None and i + MAX_SPLITK_JOBS >= len(live):
            run = lambda a=arr, n=len(chunk), t=ppo_tail: lib().splitk_reduce_jobs_ppo_tail(ctypes.byref(a), n, ctypes.byref(t), s)
            ppo_tail = None
        else:
            run = lambda a=arr, n=len(chunk): lib().splitk_reduce_jobs(ctypes.byref(a), n, s)
        _record((), run, flops=0.0)                # part of the GEMM family's time, no products of its own
        run()
    if ppo_tail is not None:                       # nothing to reduce: the tail as a launch of its own
        lib().ppo_heads_tail(ctypes.byref(ppo_tail), s)
    if per_tail is not None:
        lib().per_update(*per_tail, s)


def conv_input_grad(dz, weights, dx, x_out, deriv, tables, B, H, W, C, KH, KW, S, Co, towers, dy_stride, w_stride,
                    dx_stride, stream=None):
    """rlx_conv_input_grad; recorded with the flops of the product it replaces (dcol = dz W^T: 2*M*K*Co per tower)."""
    s = current_stream() if stream is None else stream
    OH, OW = (H - KH) // S + 1, (W - KW) // S + 1
    run = lambda: lib().conv_input_grad(dz, weights, dx, x_out, ACT[deriv], tables, B, H, W, C, KH, KW, S, Co, towers,
                                        dy_stride, w_stride, dx_stride, s)
    if GEMM_HOOK is not None:
        d = GemmDesc()
        d.M, d.N, d.K, d.batch = B * OH * OW, KH * KW * C, Co, towers
        _record((d,), run)
    run()


def per_update_desc(args):
    """PrioritizedExperienceReplay.priority_update_args() -> PerUpdateDesc"""
    sum_t, min_t, max_t, cap, idx, err, n, alpha, eps, maxp, status = args
    d = PerUpdateDesc()
    d.sum_tree, d.min_tree, d.max_tree, d.capacity = sum_t.data_ptr(), min_t.data_ptr(), max_t.data_ptr(), int(cap)
    d.idx, d.td_errors, d.n, d.alpha, d.epsilon = idx.data_ptr(), err.data_ptr(), int(n), float(alpha), float(eps)
    d.max_priority, d.status = maxp.data_ptr(), status.data_ptr()
    return d


def conv_dw_item(x, x_tower_stride, x_is_u8, a_div, dz, dz_tower_stride, B, H, W, C, KH, KW, S, Co, towers, dw, dw_tower_stride, db,
                 db_tower_stride, workspace):
    it = ConvDwItem()
    it.x, it.x_tower_stride, it.x_is_u8, it.a_div = x.data_ptr(), x_tower_stride, int(bool(x_is_u8)), float(a_div)
    it.dz, it.dz_tower_stride = dz.data_ptr(), dz_tower_stride
    it.B, it.H, it.W, it.C, it.KH, it.KW, it.S, it.filters, it.towers = B, H, W, C, KH, KW, S, Co, towers
    it.dw, it.dw_tower_stride, it.db, it.db_tower_stride = dw.data_ptr(), dw_tower_stride, _ptr(db), db_tower_stride
    it.workspace, it.workspace_floats = workspace.data_ptr(), workspace.numel()
    return it


def conv_dw_multi(items, jobs, stream=None, adam=None):
    """rlx_conv_dw_multi: the convolution layers' weight gradients of one backward pass as ONE launch; jobs[i] receives
    item i's outstanding reduction (the SAME SplitkJob objects the caller commits).
    adam = (AdamSplitDesc, riders, riders_first): rlx_conv_dw_multi_adam — the same launch also steps the early Adam blocks.
    Such a call changes weights, so it is never recorded for replay: not allowed while GEMM_HOOK is set."""
    s = current_stream() if stream is None else stream
    n = len(items)
    arr = (ConvDwItem * n)(*items)
    jarr = (SplitkJob * n)()

    def run():
        lib().conv_dw_multi(arr, jarr, n, s)
    if adam is not None:
        if GEMM_HOOK is not None:
            raise RuntimeError("rlx_conv_dw_multi_adam applies an Adam step: it cannot be recorded for replay")
        desc, riders, first = adam
        lib().conv_dw_multi_adam(arr, jarr, n, ctypes.byref(desc), int(riders), int(bool(first)), s)
        run = lambda: None
    if GEMM_HOOK is not None:
        descs = []
        for it in items:
            OH, OW = (it.H - it.KH) // it.S + 1, (it.W - it.KW) // it.S + 1
            d = GemmDesc()
            d.M, d.K = it.KH * it.KW * it.C, it.B * OH * OW
            d.N, d.batch, d.a_is_u8 = (it.towers * it.filters, 1, 1) if it.x_is_u8 else (it.filters, it.towers, 0)
            descs.append(d)
        _record(tuple(descs), run)
    run()
    for j, out in zip(jarr, jobs):
        ctypes.memmove(ctypes.byref(out), ctypes.byref(j), ctypes.sizeof(SplitkJob))


GEMM_HOOK = None   # bench.py sets this to record the descriptors issued by one update
CALL_COUNT = 0     # librlx entry points called so far (bench.py: launches of one eager update)


def _ptr(t):
    return None if t is None else (t.data_ptr() if hasattr(t, "data_ptr") else t)


def gemm(M, N, K, A, B, C, *, a_strides=None, a_tabs=None, a_u8=False, a_div=1.0,
         a_vec_along_k=1, a_tab_vec_ok=0, b_strides=None, ldc=None, bias=None, activation=None,
         deriv_aux=None, aux_ld=None, deriv_kind=None, accumulate=False, batch=1,
         a_batch_stride=0, b_batch_stride=0, c_batch_stride=0, bias_batch_stride=0,
         aux_batch_stride=0, workspace=None, colsum_out=None, colsum_batch_stride=0, stream=None,
         batch_inner=0, a_batch_stride2=0, b_batch_stride2=0, bias_batch_stride2=0, n_fold=0, launch=True,
         defer=None, row_heads=None, kw_min_tiles=0):
    """Thin wrapper building an rlx_gemm_desc.  a_strides=(row, k), b_strides=(k, n) in elements.
    launch=False: return the descriptor (for gemm_pair) instead of running it.
    defer: a SplitkJob — if K gets split over workgroups the reduction of the partials is left to
    splitk_reduce_jobs (rlx_gemm_defer); `workspace` must then stay untouched until that ran."""
    d = GemmDesc()
    d.M, d.N, d.K, d.batch = int(M), int(N), int(K), int(batch)
    d.A, d.B, d.C = _ptr(A), _ptr(B), _ptr(C)
    if a_tabs is not None:
        d.a_row_tab, d.a_k_tab = _ptr(a_tabs[0]), _ptr(a_tabs[1])
        d.a_row_stride, d.a_k_stride = 0, 0
    else:
        rs, ks = a_strides if a_strides is not None else (K, 1)
        d.a_row_stride, d.a_k_stride = int(rs), int(ks)
    ks, ns = b_strides if b_strides is not None else (N, 1)
    d.b_k_stride, d.b_n_stride = int(ks), int(ns)
    d.a_batch_stride, d.b_batch_stride = int(a_batch_stride), int(b_batch_stride)
    d.ldc = int(N if ldc is None else ldc)
    d.c_batch_stride, d.bias_batch_stride = int(c_batch_stride), int(bias_batch_stride)
    d.bias, d.deriv_aux = _ptr(bias), _ptr(deriv_aux)
    d.aux_ld = int(N if aux_ld is None else aux_ld)
    d.aux_batch_stride = int(aux_batch_stride)
    d.workspace = _ptr(workspace)
    d.colsum_out, d.colsum_batch_stride = _ptr(colsum_out), int(colsum_batch_stride)
    d.workspace_floats = int(workspace.numel()) if workspace is not None else 0
    d.a_is_u8, d.a_div = int(bool(a_u8)), float(a_div)
    d.a_vec_along_k, d.a_tab_vec_ok = int(a_vec_along_k), int(a_tab_vec_ok)
    d.activation, d.deriv_kind = ACT[activation], ACT[deriv_kind]
    d.accumulate = int(bool(accumulate))
    d.batch_inner = int(batch_inner)
    d.a_batch_stride2, d.b_batch_stride2 = int(a_batch_stride2), int(b_batch_stride2)
    d.bias_batch_stride2 = int(bias_batch_stride2)
    d.n_fold = int(n_fold)
    d.kw_min_tiles = int(kw_min_tiles)
    if row_heads is not None:                 # a ctypes array of SmallDenseProblem (kept alive by the descriptor)
        d._row_heads = row_heads
        d.row_heads, d.n_row_heads = ctypes.addressof(row_heads), len(row_heads)
    if not launch:
        return d
    s = current_stream() if stream is None else stream
    if defer is not None:
        run = lambda: lib().gemm_defer(ctypes.byref(d), ctypes.byref(defer), s)
    else:
        run = lambda: lib().gemm(ctypes.byref(d), s)
    _record((d,), run)
    run()


def _record(descs, run, flops=None):
    """bench.py's recorder: the products a launch stands for (their 2*M*N*K*batch are its algorithmic flops unless
    `flops` says otherwise) and a thunk that issues the same launch again."""
    if GEMM_HOOK is not None:
        GEMM_HOOK({"descs": tuple(GemmDesc.from_buffer_copy(x) for x in descs), "run": run, "flops": flops})


def gemm_pair_or_single(desc, stream=None):
    """run one descriptor built with gemm(..., launch=False)."""
    s = current_stream() if stream is None else stream
    run = lambda: lib().gemm(ctypes.byref(desc), s)
    _record((desc,), run)
    run()


def gemm_multi(descs, jobs, stream=None):
    """descriptors built with gemm(..., launch=False) of up to three weight-gradient products -> ONE launch
    (rlx_gemm_multi_defer); jobs: their SplitkJob objects (filled where a split-K reduction stays outstanding)."""
    s = current_stream() if stream is None else stream
    n = len(descs)
    darr = (GemmDesc * n)(*descs)
    jarr = (SplitkJob * n)()

    def run():
        lib().gemm_multi_defer(darr, n, jarr, s)
        for i, j in enumerate(jobs):
            ctypes.memmove(ctypes.addressof(j), ctypes.addressof(jarr[i]), ctypes.sizeof(SplitkJob))
    _record(tuple(descs), run)                     # one entry: the products go out as one launch
    run()


def gemm_pair(weight_grad, input_grad, stream=None, defer=None):
    """two descriptors built with gemm(..., launch=False): a layer's dW and dX products as one launch.
    defer: a SplitkJob for the weight gradient's split-K reduction (see gemm)."""
    s = current_stream() if stream is None else stream
    if defer is not None:
        run = lambda: lib().gemm_pair_defer(ctypes.byref(weight_grad), ctypes.byref(input_grad), ctypes.byref(defer), s)
    else:
        run = lambda: lib().gemm_pair(ctypes.byref(weight_grad), ctypes.byref(input_grad), s)
    _record((weight_grad, input_grad), run)        # one entry: the two products go out as one launch
    run()
