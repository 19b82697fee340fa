"""ctypes loader for libucnerf_march.so, bound from include/ucnerf_march.h itself.

The header is the only statement of the C ABI: `parse_header` reads its prototypes, its three descriptor structs and its
`#define UCN_X` constants, and this module's `SIGNATURES`, `UcnField` / `UcnSky` / `UcnSkyTrain` and `X` attributes are what it
found.  Adding an entry point is a header edit plus the `.hip`; nothing is restated here.  A declaration the parser does not know
raises ImportError with its text -- it never guesses.

The HIP library is the product: if it is missing or stale this module raises -- there is no
CPU or eager-PyTorch fallback anywhere in ucnerf_amd.
"""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# UCN_LIB_PATH: another build of the same ABI for A/B measurements; default = the in-tree product
LIB_PATH = os.environ.get("UCN_LIB_PATH") or os.path.join(_HERE, "csrc", "libucnerf_march.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ucnerf_march.h")

c_u32, c_u64, c_i32, c_f32, c_vp = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int, ctypes.c_float, ctypes.c_void_p
_SCALARS = {"uint32_t": c_u32, "uint64_t": c_u64, "int": c_i32, "int32_t": c_i32, "float": c_f32, "size_t": ctypes.c_size_t}
_BASE_TYPE = re.compile(r"(?:const\s+)?(\w+)\b\s*(.*)", re.S)                   # `[const] type` and its declarators
_DECLARATOR = re.compile(r"((?:\*\s*(?:const\b\s*)?)*)\b(\w+)(?:\[(\d+)\])?")      # `*name`, `*const *name`, `name[8]`
_INT_OPS = (("|", int.__or__), ("<<", int.__lshift__), ("*", int.__mul__))      # loosest first


def _unknown(text):
    return ImportError(f"include/ucnerf_march.h: no binding rule for `{' '.join(text.split())}`")


def _int_expr(expr, constants):
    """<int | hex | UCN_NAME> joined by * | << and parentheses."""
    toks = re.findall(r"0[xX][0-9a-fA-F]+|\d+|UCN_\w+|<<|[*|()]", expr)
    if "".join(toks) != "".join(expr.split()):
        raise _unknown(expr)

    def level(i):
        if i < len(_INT_OPS):
            v = level(i + 1)
            while toks and toks[0] == _INT_OPS[i][0]:
                toks.pop(0)
                v = _INT_OPS[i][1](v, level(i + 1))
            return v
        t = toks.pop(0)
        if t == "(":
            v = level(0)
            if toks.pop(0) != ")":
                raise ValueError(expr)
            return v
        return constants[t[4:]] if t.startswith("UCN_") else int(t, 0)

    try:
        v = level(0)
        if toks:
            raise ValueError(expr)
    except (IndexError, KeyError, ValueError):
        raise _unknown(expr) from None
    return v


def parse_header(text):
    """C text of the header's three kinds of declaration ->
    ({X: int} of `#define UCN_X`, {typedef name: ctypes.Structure class}, {entry point: (restype, [argtypes])})."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"#ifdef __cplusplus.*?#endif", " ", text, flags=re.S)             # the extern "C" braces
    constants, types, structs, protos = {}, dict(_SCALARS), {}, {}
    for line in re.findall(r"^#define[ \t]+UCN_(.*)$", text, re.M):
        m = re.fullmatch(r"(\w+)[ \t]+(\S.*?)\s*", line)
        if not m:
            raise _unknown("#define UCN_" + line)
        constants[m.group(1)] = _int_expr(m.group(2), constants)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)

    def declare(decl, member):
        """`[const] type a, *b, c[8]` -> [(name, ctypes type)]; AttributeError / KeyError on any other shape or type"""
        base, rest = _BASE_TYPE.fullmatch(decl.strip()).groups()
        out = []
        for d in rest.split(","):
            stars, name, count = _DECLARATOR.fullmatch(d.strip()).groups()
            if not stars:
                t = types[base]
            else:
                t = ctypes.POINTER(structs[base]) if base in structs and stars.count("*") == 1 else c_vp
            if count and not member:
                raise KeyError(d)                # an array parameter is a pointer in C: the header does not use the form
            out.append((name, t * int(count) if count else t))
        return out

    def struct(m):
        tag, body, name = m.groups()
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            try:
                fields += declare(decl, True)
            except (AttributeError, KeyError):
                raise _unknown(decl) from None
        cls = "".join(part.capitalize() for part in tag.split("_"))
        structs[name] = type(cls, (ctypes.Structure,), {"_fields_": fields, "__doc__": f"struct {tag} (include/ucnerf_march.h)."})
        return " "

    for m in re.finditer(r"typedef\s+void\s*\*\s*(\w+)\s*;", text):            # an opaque handle (ucn_stream_t)
        types[m.group(1)] = c_vp
    text = re.sub(r"typedef\s+void\s*\*\s*\w+\s*;", " ", text)
    text = re.sub(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", struct, text, flags=re.S)
    for decl in filter(None, (d.strip() for d in text.split(";"))):
        try:
            ret, name, params = re.fullmatch(r"(const\s+char\s*\*|\w+)\s*\b(ucn_\w+)\s*\((.*)\)", decl, re.S).groups()
            args = [declare(p, False)[0][1] for p in ([] if params.strip() == "void" else params.split(","))]
            protos[name] = (ctypes.c_char_p if "*" in ret else types[ret], args)
        except (AttributeError, KeyError):
            raise _unknown(decl) from None
    return constants, structs, protos


try:
    with open(HEADER_PATH) as _f:
        _CONSTANTS, _STRUCTS, _PROTOTYPES = parse_header(_f.read())
except FileNotFoundError:
    raise ImportError(f"{HEADER_PATH} not found: the bindings are read from it (it ships with the package's source tree). "
                      "ucnerf_amd has no CPU / eager fallback.") from None
globals().update(_CONSTANTS)        # UCN_TABLE_F16 -> TABLE_F16, ...; ABI_VERSION is UCN_ABI_VERSION
UcnField, UcnSky, UcnSkyTrain = _STRUCTS["ucn_field_t"], _STRUCTS["ucn_sky_t"], _STRUCTS["ucn_sky_train_t"]
SIGNATURES = {name: args for name, (_, args) in _PROTOTYPES.items()}      # name -> argtypes

# Entry points added without an ABI bump: a host-side probe that no product path calls, and the batch assembler of
# internal/datasets.py, which no earlier path calls.  An older build of the same ABI loaded through UCN_LIB_PATH may lack them
# (calling one there is an AttributeError, not a fallback); every other symbol is required.
_ADDED_WITHIN_ABI = {"ucn_level_groups_probe", "ucn_train_batch"}

_lib = None


def load():
    """dlopen the in-tree library and bind every symbol of the header (ImportError if absent)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with ucnerf_amd/csrc/build.sh (hipcc --offload-arch=gfx950). "
            "ucnerf_amd has no CPU / eager fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, args) in _PROTOTYPES.items():
        if name in _ADDED_WITHIN_ABI and not hasattr(lib, name):
            continue                     # an earlier build of the same ABI (UCN_LIB_PATH, A/B measurements)
        fn = getattr(lib, name)          # AttributeError = header/library mismatch: fail loudly
        fn.argtypes = args
        fn.restype = restype
    got = lib.ucn_abi_version()
    if got != ABI_VERSION:
        raise ImportError(f"libucnerf_march.so ABI {got} != expected {ABI_VERSION}: rebuild")
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        raise RuntimeError(load().ucn_last_error().decode())


def ptr(t):
    """Device/host address of a tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


def stream():
    """The current HIP stream handle (the reference launches on the default stream,
    gridencoder.cu:374-382; here the caller's current torch stream is honoured)."""
    return torch.cuda.current_stream().cuda_stream


def require_device(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"{what} must be a CUDA tensor")      # CHECK_CUDA, gridencoder.cu:15
