"""ctypes binding of ``libcft_hip.so`` (C ABI declared in ``include/cft_hip.h``).

There is deliberately NO fallback: if the library is missing or the device is not gfx950 every
op raises.  ``build()`` compiles the library in-tree with hipcc (cross-compiles without a GPU).
"""
import ctypes
import os
import re
import subprocess

# torch must be imported BEFORE the library is dlopen'ed: torch ships its own libamdhip64 and a
# process that first loads the system copy (through libcft_hip.so) and then torch's ends up with
# two HIP runtimes ("No HIP GPUs are available").  Loaded in this order both bind to torch's copy.
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CFT_HIP_LIB") or os.path.join(_HERE, "libcft_hip.so")      # (CFT_HIP_LIB: load another build of the library, e.g. one made with tools/build.sh and CFT_OUT)
CSRC = os.path.join(_HERE, "csrc")
SOURCES = ("runtime.hip", "conv_gemm.hip", "conv_gemm_asm.hip", "focus_conv.hip", "bottleneck.hip", "pointwise.hip", "attention.hip", "attention_tokens.hip", "nms.hip", "train.hip", "metrics.hip", "curves.hip", "confusion.hip", "loss.hip", "autoanchor.hip", "dataset.hip", "detect.hip", "optim.hip", "mosaic.hip", "augment.hip", "jpeg.hip", "jpeg_encode.hip", "tta.hip")

HEADER = os.path.join(_HERE, "..", "include", "cft_hip.h")
HEADERS = ("cft_common.h", "conv_common.h", "focus_common.h", "bneck_common.h", "metrics_common.h", "resize_common.h", "jpeg_common.h", "conv_gemm_asm.inc")

_SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "unsigned long long": ctypes.c_ulonglong}
_RETURNS = {"int": ctypes.c_int, "long": ctypes.c_long, "const char*": ctypes.c_char_p}
_TYPE_WORDS = frozenset("void char short int long float double signed unsigned const".split())


def parse_header(text):
    """``(signatures, constants)`` of a header in the dialect of include/cft_hip.h: ``ret cft_name(args);`` prototypes whose arguments
    are pointers (-> c_void_p, device and host alike: callers pass ``data_ptr()`` integers, arrays or ``byref``) or named int / long /
    float / unsigned long long scalars -> name: (restype, argtypes); ``CFT_X = n`` enumerators and ``#define CFT_X n`` -> name: n.
    Anything else in a prototype raises with the prototype's name: a type is never guessed."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    consts = {k: int(v) for k, v in re.findall(r"(?:#define\s+|\b)(CFT_\w+)\s*=?\s*(-?\d+)\b", text)}
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    sigs = {}
    for ret, name, args in re.findall(r"([\w\s*]+?)\b(cft_\w+)\s*\(([^()]*)\)\s*;", text):
        ret = re.sub(r"\s*\*", "*", " ".join(ret.split()))
        if ret not in _RETURNS:
            raise ValueError(f"{name}: unknown return type '{ret}'")
        argtypes = []
        for arg in ([] if args.strip() in ("", "void") else args.split(",")):
            *kind, pname = [w for w in arg.split() if w != "const"] or [""]
            if "*" in arg:
                argtypes.append(ctypes.c_void_p)
            elif " ".join(kind) in _SCALARS and pname not in _TYPE_WORDS:
                argtypes.append(_SCALARS[" ".join(kind)])
            else:
                raise ValueError(f"{name}: unknown parameter type in '{' '.join(arg.split())}' (scalars are named int / long / float / unsigned long long)")
        sigs[name] = (_RETURNS[ret], argtypes)
    return sigs, consts


# name -> (restype, argtypes) of every entry point, and the header's constants: include/cft_hip.h is the only description of the ABI
with open(HEADER) as _fh:
    SIGNATURES, _consts = parse_header(_fh.read())
ABI_VERSION = _consts["CFT_ABI_VERSION"]
CFT_BF16, CFT_F32, CFT_F16 = (_consts[k] for k in ("CFT_BF16", "CFT_F32", "CFT_F16"))
ACT_NONE, ACT_SILU, ACT_GELU = (_consts[k] for k in ("CFT_ACT_NONE", "CFT_ACT_SILU", "CFT_ACT_GELU"))

_lib = None


def missing_symbols():
    """The entry points of the header that the built library's bytes do not name (its dynamic string table holds every export): a
    library from before an entry point was added is stale whatever its timestamp says.  Nothing is loaded."""
    with open(LIB_PATH, "rb") as fh:
        blob = fh.read()
    return [name for name in SIGNATURES if name.encode() + b"\0" not in blob]


def build(verbose=False):
    """Compile every HIP source for gfx950 into ``libcft_hip.so`` next to this file."""
    srcs = [os.path.join(CSRC, s) for s in SOURCES]
    hdrs = [os.path.join(CSRC, h) for h in HEADERS] + [HEADER]
    newest = max(os.path.getmtime(p) for p in srcs + hdrs)
    if os.path.exists(LIB_PATH) and os.path.getmtime(LIB_PATH) >= newest and not missing_symbols():
        return LIB_PATH
    # one object per source, compiled concurrently (only the stale ones), then one link
    hdr_time = max(os.path.getmtime(h) for h in hdrs)
    obj_dir = os.path.join(_HERE, "build")
    os.makedirs(obj_dir, exist_ok=True)
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"]
    jobs, objs = [], []
    for src in srcs:
        obj = os.path.join(obj_dir, os.path.basename(src)[:-4] + ".o")
        objs.append(obj)
        if os.path.exists(obj) and os.path.getmtime(obj) >= max(os.path.getmtime(src), hdr_time):
            continue
        cmd = ["hipcc"] + flags + ["-c", src, "-o", obj]
        if verbose:
            print(" ".join(cmd))
        jobs.append((cmd, subprocess.Popen(cmd)))
    for cmd, p in jobs:
        if p.wait() != 0:
            raise subprocess.CalledProcessError(p.returncode, cmd)
    cmd = ["hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB_PATH] + objs
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    global _lib
    _lib = None
    return LIB_PATH


def load():
    """Return the loaded library (cached).  Raises RuntimeError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: the HIP kernels are the only execution path of this package. "
            "Build them with `python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc).")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError here = ABI mismatch, let it propagate
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


def check(status, what):
    if status != 0:
        msg = load().cft_last_error().decode(errors="replace")
        raise RuntimeError(f"{what} failed (status {status}): {msg}")
