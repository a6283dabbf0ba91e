"""ctypes binding of ``libcft_hip.so`` (C ABI declared in ``include/cft_hip.h``).

There is deliberately NO fallback: if the library is missing or the device is not gfx950 every
op raises.  ``build()`` compiles the library in-tree with hipcc (cross-compiles without a GPU).
"""
import ctypes
import functools
import glob
import os
import re
import shutil
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

# torch must be imported BEFORE the library is dlopen'ed: torch ships its own libamdhip64 and a
# process that first loads the system copy (through libcft_hip.so) and then torch's ends up with
# two HIP runtimes ("No HIP GPUs are available").  Loaded in this order both bind to torch's copy.
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
BUILT_LIB = os.path.join(_HERE, "libcft_hip.so")                  # what build() writes unless told otherwise
LIB_PATH = os.environ.get("CFT_HIP_LIB") or BUILT_LIB             # what load() loads (CFT_HIP_LIB: another build of the library, e.g. one made with tools/build.sh and CFT_OUT)
CSRC = os.path.join(_HERE, "csrc")
HEADER = os.path.join(_HERE, "..", "include", "cft_hip.h")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"]      # of every compile of the project: the library, the ISA listings of the tests and tools

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


def missing_symbols(path=None):
    """The entry points of the header that the built library's bytes do not name (its dynamic string table holds every export): a
    library from before an entry point was added is stale whatever its timestamp says.  Nothing is loaded."""
    with open(path or LIB_PATH, "rb") as fh:
        blob = fh.read()
    return [name for name in SIGNATURES if name.encode() + b"\0" not in blob]


def sources():
    """Every HIP source of the library: a file dropped into csrc/ is built."""
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")))


def staleness_inputs():
    """What every object depends on besides its own source: a file dropped into csrc/ rebuilds."""
    return sorted(glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.inc"))) + [HEADER]


SOURCES = tuple(os.path.basename(p) for p in sources())      # the names, for readers that ask "is x.hip built"; no list is kept by hand


def _compile(cmd):
    status = subprocess.Popen(cmd).wait()
    if status != 0:
        raise subprocess.CalledProcessError(status, cmd)


def build(verbose=False, out=None, extra_flags=()):
    """Compile every HIP source for gfx950 into ``libcft_hip.so`` next to this file (wherever CFT_HIP_LIB points: that is load()'s
    business), or into ``out``.  Another ``out`` or ``extra_flags`` compile everything afresh in an object directory of their own."""
    global _lib
    srcs, deps = sources(), staleness_inputs()
    in_tree = out is None and not extra_flags
    out = BUILT_LIB if out is None else os.path.abspath(out)
    newest = max(os.path.getmtime(p) for p in srcs + deps)
    if in_tree and os.path.exists(out) and os.path.getmtime(out) >= newest and not missing_symbols(out):
        return out
    # one object per source (in the tree's own cache only the stale ones), a bounded number of compiles at a time, then one link
    dep_time = max(os.path.getmtime(h) for h in deps)
    obj_dir = os.path.join(_HERE, "build") if in_tree else tempfile.mkdtemp(prefix="cft_build_")
    os.makedirs(obj_dir, exist_ok=True)
    cmds, objs = [], []
    for src in srcs:
        obj = os.path.join(obj_dir, os.path.basename(src)[:-4] + ".o")
        objs.append(obj)
        if not (os.path.exists(obj) and os.path.getmtime(obj) >= max(os.path.getmtime(src), dep_time)):
            cmds.append([HIPCC] + HIPCC_FLAGS + list(extra_flags) + ["-c", src, "-o", obj])
    cmds.append([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out] + objs + list(extra_flags))
    if verbose:
        print("\n".join(" ".join(cmd) for cmd in cmds))
    pool = ThreadPoolExecutor(max(1, min(16, int(os.environ.get("MAX_JOBS", 16)))))
    try:
        list(pool.map(_compile, cmds[:-1]))
        _compile(cmds[-1])
    finally:
        pool.shutdown(cancel_futures=True)
        if not in_tree:
            shutil.rmtree(obj_dir, ignore_errors=True)
    if in_tree:
        _lib = None          # load() opens the new library
    return out


def device_asm(src, extra=()):
    """The gfx950 assembly hipcc makes of a HIP source's device code, with the flags of the build (+ ``extra``); a source is
    compiled once per process.  FileNotFoundError without hipcc."""
    return _device_asm(os.path.abspath(src), tuple(extra))


@functools.lru_cache(maxsize=None)
def _device_asm(src, extra):
    cmd = [HIPCC] + HIPCC_FLAGS + ["-S", "--cuda-device-only", *extra, "-o", "-", src]
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def kernel_notes(asm):
    """{kernel name: {key: int}} of every integer key of the entries under ``amdhsa.kernels:`` in a listing.  An entry opens at
    ``  - .key:`` whichever key comes first, with a value on the line or not (``.args:``); its own keys sit four columns in, those of
    its arguments deeper."""
    entries = []
    for line in asm[asm.index("amdhsa.kernels:"):].split("\n")[1:]:
        if not line.startswith("  "):
            break
        m = re.match(r"(  - |    )\.(\w+):\s*(.*?)\s*$", line)
        if m and m.group(1) == "  - ":
            entries.append({})
        if m:
            entries[-1][m.group(2)] = m.group(3)
    return {e["name"]: {k: int(v) for k, v in e.items() if v.isdigit()} for e in entries}


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
