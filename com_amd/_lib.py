"""ctypes binding of ``libpcdops_hip.so`` (C ABI: ``include/pcd_ops.h``).

There is NO CPU fallback: if the shared library is missing or a call fails, this module raises.
Python passes raw device pointers (``tensor.data_ptr()``), element counts and the current HIP
stream; torch is only the owner of device memory and streams.
"""
import ctypes
import os
import re
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libpcdops_hip.so")
CSRC = os.path.join(_HERE, "csrc")

HEADER = os.path.join(os.path.dirname(_HERE), "include", "pcd_ops.h")


class PcdError(RuntimeError):
    pass


# The header is the one record of the ABI: prototypes and integer constants are parsed from it at import (plain `re` over
# the few shapes its declarations have -- regularise an odd declaration in the header rather than teach this C).
_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int, "size_t": ctypes.c_size_t, "float": ctypes.c_float,
            "double": ctypes.c_double, "long long": ctypes.c_longlong, "unsigned long long": ctypes.c_ulonglong,
            "uint64_t": ctypes.c_ulonglong}


def _strip_comments(text):
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def _ctype(c_type, decl):
    """ctypes type of one C return / parameter type (its name already removed); an unknown one is an error, never a guess."""
    words = [w for w in c_type.replace("*", " * ").replace("[", " * [").split() if w != "const"]
    if "*" in words:
        return ctypes.c_char_p if words == ["char", "*"] else ctypes.c_void_p
    try:
        return _SCALARS[" ".join(words)]
    except KeyError:
        raise PcdError(f"include/pcd_ops.h: unknown type '{c_type.strip()}' in declaration `{decl}`") from None


def parse_prototypes(text):
    """name -> (restype, argtypes) of every `ret pcd_name(args);` in the text of a C header."""
    text = re.sub(r"^[ \t]*#.*$", " ", _strip_comments(text), flags=re.M)              # preprocessor lines
    text = re.sub(r"\{[^{}]*\}", " ", text).replace('extern "C" {', " ")                 # struct / enum bodies
    protos = {}
    for stmt in text.split(";"):
        decl = " ".join(stmt.split()).lstrip("} ")
        m = re.fullmatch(r"(.*?)\b(pcd_\w+) ?\((.*)\)", decl)
        if m is None:
            if decl and decl.split()[0] not in ("typedef", "struct", "enum"):
                raise PcdError(f"include/pcd_ops.h: cannot parse `{decl}`")
            continue
        ret, name, params = m.groups()
        params = [] if params.strip() == "void" else [q.strip() for q in params.split(",")]
        # a parameter is `type name` or `type name[n]`: the last identifier is its name
        args = [_ctype(re.sub(r"\w+\s*(\[[^\]]*\])?$", r"\1", q), decl) for q in params]
        protos[name] = (None if ret.strip() == "void" else _ctype(ret, decl), args)
    return protos


def parse_constants(text):
    """name -> value of every `#define PCD_NAME <integer expression>` (literals, negatives, earlier PCD_ names)."""
    consts = {}
    for name, expr in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(PCD_\w+)[ \t]+(\S.*)$", _strip_comments(text), flags=re.M):
        try:
            if not re.fullmatch(r"[\w\s()+*-]+", expr):
                raise SyntaxError(expr)
            consts[name] = int(eval(expr, {"__builtins__": {}}, consts))
        except (SyntaxError, NameError, TypeError):
            raise PcdError(f"include/pcd_ops.h: #define {name} {expr.strip()} is not an integer expression") from None
    return consts


with open(HEADER) as _f:
    _header_text = _f.read()
PROTOTYPES = parse_prototypes(_header_text)      # name -> (restype, argtypes) of EVERY function include/pcd_ops.h declares
CONSTANTS = parse_constants(_header_text)        # ... and its integer #defines, also module attributes: _lib.PCD_BN_EXT_MID
globals().update(CONSTANTS)
del _f, _header_text
# the short names some of them had before they were read from the header
for _k in ("COLSUM_MAX_JOBS", "WGRAD_MAX_JOBS", "COUNT_CHECK_MAX", "POSTPROC_MAX_HEADS", "POSTPROC_MAX_CLASSES", "POSTPROC_MAX_K",
           "BN_MID_ROWS", "BN_EXT_MID", "BN_COUNTER_STRIDE"):
    globals()[_k] = CONSTANTS["PCD_" + _k]

_lib = None


class PcdColsumJob(ctypes.Structure):
    """include/pcd_ops.h: struct PcdColsumJob."""
    _fields_ = [("partial", ctypes.c_void_p), ("out", ctypes.c_void_p), ("rows", ctypes.c_int), ("c", ctypes.c_int)]


class PcdWgradReduceJob(ctypes.Structure):
    """include/pcd_ops.h: struct PcdWgradReduceJob."""
    _fields_ = [("workspace", ctypes.c_void_p), ("dweight", ctypes.c_void_p), ("kvol", ctypes.c_int),
                ("cin", ctypes.c_int), ("cout", ctypes.c_int), ("pmax", ctypes.c_int), ("splits", ctypes.c_int),
                ("layout", ctypes.c_int), ("cout_write", ctypes.c_int), ("cin_write", ctypes.c_int)]


class PcdCountCheck(ctypes.Structure):
    """include/pcd_ops.h: struct PcdCountCheck (static-shape overflow guard)."""
    _fields_ = [("count", ctypes.c_void_p * COUNT_CHECK_MAX), ("cap", ctypes.c_int32 * COUNT_CHECK_MAX)]


class PcdPostprocHead(ctypes.Structure):
    """include/pcd_ops.h: struct PcdPostprocHead (the maps of one centre head)."""
    _fields_ = [("map", ctypes.c_void_p * 6), ("strides", (ctypes.c_longlong * 4) * 6), ("dtype", ctypes.c_int * 6),
                ("num_class", ctypes.c_int), ("label", ctypes.c_int * POSTPROC_MAX_CLASSES)]


class PcdPostprocConfig(ctypes.Structure):
    """include/pcd_ops.h: struct PcdPostprocConfig (POST_PROCESSING of a centre head)."""
    _fields_ = [("batch", ctypes.c_int), ("num_heads", ctypes.c_int), ("height", ctypes.c_int), ("width", ctypes.c_int),
                ("max_obj", ctypes.c_int), ("nms_pre", ctypes.c_int), ("nms_post", ctypes.c_int), ("nms_normal", ctypes.c_int),
                ("use_score_thresh", ctypes.c_int), ("score_thresh", ctypes.c_float), ("nms_thresh", ctypes.c_float),
                ("limit", ctypes.c_float * 6), ("feature_map_stride", ctypes.c_float), ("voxel_x", ctypes.c_float),
                ("voxel_y", ctypes.c_float), ("pc_x", ctypes.c_float), ("pc_y", ctypes.c_float)]


class PcdComCurriculum(ctypes.Structure):
    """include/pcd_ops.h: struct PcdComCurriculum (LOSS_CURRICULUM of the COM head)."""
    _fields_ = [("ucl", ctypes.c_int), ("fix_threshold", ctypes.c_int), ("straight", ctypes.c_int),
                ("tuning", ctypes.c_int), ("only_center", ctypes.c_int), ("apply", ctypes.c_int), ("add", ctypes.c_int),
                ("radius", ctypes.c_int), ("k_straight", ctypes.c_double), ("elongation", ctypes.c_double),
                ("height", ctypes.c_double), ("alpha", ctypes.c_double), ("threshold", ctypes.c_double),
                ("conf_classes", ctypes.c_int), ("conf_groups", ctypes.c_int)]


class PcdAnchorCurriculum(ctypes.Structure):
    """include/pcd_ops.h: struct PcdAnchorCurriculum (LOSS_CURRICULUM of the anchor curriculum head)."""
    _fields_ = [("ucl", ctypes.c_int), ("oto", ctypes.c_int), ("sm", ctypes.c_int), ("sma", ctypes.c_int),
                ("norm", ctypes.c_int), ("smt", ctypes.c_float), ("pos_norm", ctypes.c_float), ("neg_norm", ctypes.c_float),
                ("offset", ctypes.c_double), ("ema", ctypes.c_double)]


class PcdRoiSampler(ctypes.Structure):
    """include/pcd_ops.h: struct PcdRoiSampler (TARGET_CONFIG of a RoI head as pcd_roi_head_sample_targets takes it)."""
    _fields_ = [("batch", ctypes.c_int), ("num_rois", ctypes.c_int), ("num_gt", ctypes.c_int), ("rois_per_image", ctypes.c_int),
                ("fg_rois_per_image", ctypes.c_int), ("score_type", ctypes.c_int), ("given_inds", ctypes.c_int),
                ("reg_fg_thresh", ctypes.c_float), ("cls_fg_thresh", ctypes.c_float), ("cls_bg_thresh", ctypes.c_float),
                ("cls_bg_thresh_lo", ctypes.c_float), ("cls_span", ctypes.c_float)]


class PcdBnReduce(ctypes.Structure):
    """include/pcd_ops.h: struct PcdBnReduce (conv-epilogue reductions for the BatchNorm beside the conv)."""
    _fields_ = [("mode", ctypes.c_int), ("relu", ctypes.c_int), ("x", ctypes.c_void_p), ("y", ctypes.c_void_p),
                ("mean", ctypes.c_void_p), ("invstd", ctypes.c_void_p), ("partial", ctypes.c_void_p),
                ("partial_rows", ctypes.c_int), ("mid", ctypes.c_void_p), ("counters", ctypes.c_void_p)]


def build(force=False):
    """hipcc --offload-arch=gfx950 -> com_amd/lib/libpcdops_hip.so (cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["make", "-C", CSRC, "-s", "clean"])
    subprocess.check_call(["make", "-C", CSRC, "-s", "-j4"])
    return LIB_PATH


def lib():
    """Load the HIP library; raise if it has not been built (no fallback path exists)."""
    global _lib
    if _lib is None:
        # torch bundles its own HIP runtime (libamdhip64); it must be loaded FIRST so that this library's
        # NEEDED entry binds to the same runtime instance (two runtimes in one process do not share devices,
        # streams or allocations).
        import torch  # noqa: F401
        if not os.path.exists(LIB_PATH):
            raise PcdError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C com_amd/csrc`. There is no CPU fallback for the hot path.")
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(handle, name)  # AttributeError if a declared symbol is not exported
            fn.restype = res
            fn.argtypes = args
        # (tuning options are set through set_option -- bench.py / tools/ forward PCD_OPT_<KEY> environment variables with
        #  tools/env_switches.py; neither this module nor the library reads the environment)
        _lib = handle
    return _lib


def use_experiments_library():
    """The second library of measured-slower kernels was retired: there is nothing to load.  Kept so
    that a caller that still asks for it (PCD_TEST_EXPERIMENTS=1 in tests/conftest.py) gets this error."""
    raise PcdError("the EXPERIMENTS build was retired: its kernels measured slower and are no longer compiled (DESIGN.md 4.4)")


def set_option(key, value):
    """PROCESS-WIDE (one table per loaded library, read at launch time without synchronisation): set options before
    the first launch, not from concurrent threads; tests restore what they change (tests/conftest.py::pcd_option)."""
    check(lib().pcd_set_option(key.encode(), int(value)), f"pcd_set_option({key})")


def get_option(key):
    v = ctypes.c_int(0)
    check(lib().pcd_get_option(key.encode(), ctypes.byref(v)), f"pcd_get_option({key})")
    return int(v.value)


def check(code, what):
    if code != 0:
        msg = lib().pcd_error_string(code).decode()
        if code == CONSTANTS["PCD_ERR_LAUNCH"]:
            msg += " [" + lib().pcd_last_hip_error_string().decode() + "]"
        raise PcdError(f"{what} failed: {msg} (code {code})")


def host_f32(values):
    arr = (ctypes.c_float * len(values))(*[float(v) for v in values])
    return arr


def host_i32(values):
    arr = (ctypes.c_int * len(values))(*[int(v) for v in values])
    return arr


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    if t is None:
        return None
    return ctypes.c_void_p(t.data_ptr())


def stream_ptr():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def workspace(nbytes, device, floor=256):
    """A scratch buffer of at least `floor` bytes (a zero-byte query still gets a valid pointer)."""
    import torch
    return torch.empty((max(int(nbytes), floor),), dtype=torch.uint8, device=device)


def dtype_code(t):
    """PCD_F32 / PCD_BF16 of a feature tensor."""
    import torch
    if t.dtype == torch.float32:
        return CONSTANTS["PCD_F32"]
    if t.dtype == torch.bfloat16:
        return CONSTANTS["PCD_BF16"]
    raise PcdError(f"unsupported feature dtype {t.dtype} (float32 / bfloat16 only)")


def require_device(what, *tensors, verb="needs", allow_none=False):
    """Raise unless every one of `tensors` is a HIP device tensor (allow_none: None entries pass); returns the first."""
    import torch
    for t in tensors:
        if not (isinstance(t, torch.Tensor) and t.is_cuda) and not (allow_none and t is None):
            noun = "a HIP device tensor" if len(tensors) == 1 else "HIP device tensors"
            raise PcdError(f"{what} {verb} {noun} (there is no CPU fallback)")
    return tensors[0] if tensors else None
