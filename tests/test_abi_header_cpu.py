"""The ctypes bindings are read from include/ucnerf_march.h (ucnerf_amd/_lib.py::parse_header).  Two checks that no second hand
copy can give: the parser on literal C of every declaration shape the header uses, and the derived descriptor structs against the
host C compiler's own sizeof / offsetof.  CPU only; nothing is launched."""
import ctypes
import os
import subprocess

import pytest

from ucnerf_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SNIPPET = """
/* a comment with a prototype in it: int ucn_not_declared(float x); */
#define UCN_B 24
#define UCN_A (UCN_B * 64)
#define UCN_FLAG 0x100
#define UCN_BOTH (UCN_FLAG | 1 << 4)
typedef void *ucn_stream_t; /* opaque */
typedef struct ucn_thing {
    /* pointers that share one declaration */
    const float *a, *b;
    const float *w[8];      /* an array of pointers */
    uint32_t n, m;
    float scale;
    void *packed;
} ucn_thing_t;
const char *ucn_message(void);
uint64_t ucn_thing_floats(const ucn_thing_t *t);
int ucn_broken_over_lines(const ucn_thing_t *t, const float *sdist /*[N,S+1]*/,
                          float *const *tensors_host /*HOST [count]*/,
                          uint32_t N, int32_t k, float lam /*read by one curve only*/,
                          size_t bytes, int flags /*1: a, b; 2: (c)*/,
                          float *out /*[N,S+1]*/, ucn_stream_t stream);
"""


def test_parser_on_literal_declarations():
    constants, structs, protos = _lib.parse_header(SNIPPET)
    assert constants == {"B": 24, "A": 24 * 64, "FLAG": 0x100, "BOTH": 0x110}
    assert list(structs) == ["ucn_thing_t"]
    thing = structs["ucn_thing_t"]
    assert thing.__name__ == "UcnThing" and issubclass(thing, ctypes.Structure)
    vp = _lib.c_vp
    assert thing._fields_ == [("a", vp), ("b", vp), ("w", vp * 8), ("n", _lib.c_u32), ("m", _lib.c_u32), ("scale", _lib.c_f32),
                              ("packed", vp)]
    assert list(protos) == ["ucn_message", "ucn_thing_floats", "ucn_broken_over_lines"]       # the commented one is not declared
    assert protos["ucn_message"] == (ctypes.c_char_p, [])                                     # (void)
    assert protos["ucn_thing_floats"] == (_lib.c_u64, [ctypes.POINTER(thing)])
    assert protos["ucn_broken_over_lines"] == (_lib.c_i32, [ctypes.POINTER(thing), vp, vp, _lib.c_u32, _lib.c_i32, _lib.c_f32,
                                                            ctypes.c_size_t, _lib.c_i32, vp, vp])


@pytest.mark.parametrize("text", [
    "int ucn_f(long n);",                           # a parameter type the table does not have
    "double ucn_f(void);",                          # ... a return type
    "int ucn_f(uint32_t);",                         # a parameter without a name
    "int ucn_f(int (*callback)(int));",             # a declarator shape the header does not use
    "int ucn_f(float x, ...);",
    "typedef struct ucn_s { double d; } ucn_s_t;",  # a member type
    "typedef struct ucn_s { float m[2][2]; } ucn_s_t;",
    "static const int ucn_k = 3;",                  # a declaration that is neither of the three kinds
    "#define UCN_X 1.5",
    "#define UCN_X (UCN_UNDEFINED * 2)",
    "#define UCN_X (1 + 2)",                        # an operator outside * | <<
    "#define UCN_F(x) (x)",
])
def test_parser_raises_on_what_it_does_not_know(text):
    with pytest.raises(ImportError, match="ucnerf_march.h"):
        _lib.parse_header(text)


def test_the_module_is_the_parsed_header():
    constants, structs, protos = _lib.parse_header(open(_lib.HEADER_PATH).read())
    assert os.path.samefile(_lib.HEADER_PATH, os.path.join(REPO, "include", "ucnerf_march.h"))
    assert len(protos) >= 116 and list(_lib.SIGNATURES) == list(protos)
    for name, value in constants.items():
        assert getattr(_lib, name) == value, name
    assert constants["ABI_VERSION"] == _lib.ABI_VERSION and constants["LEVEL_SCALE_WS_FLOATS"] == constants["MAX_LEVELS"] * 64
    assert list(structs) == ["ucn_field_t", "ucn_sky_t", "ucn_sky_train_t"]
    lib = _lib.load()
    for name, (restype, argtypes) in protos.items():
        fn = getattr(lib, name)
        assert fn.restype == restype and list(fn.argtypes) == _lib.SIGNATURES[name], name
        assert len(argtypes) == len(_lib.SIGNATURES[name]), name


def test_descriptor_layouts_are_the_c_compilers(tmp_path):
    """sizeof and every offsetof of the three descriptor structs, as the host C compiler lays out the header's own typedefs,
    against the ctypes classes the loader derived from the same text."""
    classes = {"ucn_field_t": _lib.UcnField, "ucn_sky_t": _lib.UcnSky, "ucn_sky_train_t": _lib.UcnSkyTrain}
    lines = ["#include <stdio.h>", '#include "ucnerf_march.h"', "int main(void) {"]
    want = {}
    for ctype, cls in classes.items():
        assert len(cls._fields_) >= 9
        lines.append(f'    printf("{ctype} %zu\\n", sizeof({ctype}));')
        want[ctype] = ctypes.sizeof(cls)
        for member, _ in cls._fields_:
            lines.append(f'    printf("{ctype}.{member} %zu\\n", offsetof({ctype}, {member}));')
            want[f"{ctype}.{member}"] = getattr(cls, member).offset
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(_lib.HEADER_PATH), "-o", str(exe), str(src)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert {k: int(v) for k, v in got.items()} == want
    # the members fill the struct: nothing the header declares is missing from the class
    for cls in classes.values():
        last, last_type = cls._fields_[-1]
        assert getattr(cls, last).offset + ctypes.sizeof(last_type) <= ctypes.sizeof(cls) < getattr(cls, last).offset + ctypes.sizeof(last_type) + 8
