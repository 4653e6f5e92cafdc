"""The ctypes structures, constants and the value-returning rule of coach_amd/_rlx.py are all read from include/rlx.h;
this pins them to what a C compiler makes of the same header (CPU only, no library call)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from coach_amd import _rlx, signals


def _compiler():
    for cc in ("cc", "/opt/rocm/llvm/bin/clang", "/opt/rocm/lib/llvm/bin/clang", "clang"):
        path = shutil.which(cc)
        if path:
            return path
    return None


def _flatten(cls, base=0, prefix=""):
    """[(dotted member path, offset, size, kind)] of every scalar of a structure, nested ones expanded."""
    out = []
    for name, ctype in cls._fields_:
        off = base + getattr(cls, name).offset
        if issubclass(ctype, ctypes.Structure):
            out += _flatten(ctype, off, prefix + name + ".")
        else:
            out.append((prefix + name, off, ctypes.sizeof(ctype), _CTYPES_KIND[ctype._type_]))
    return out


# the member's kind as the C compiler sees it — signed / unsigned integer, floating point, pointer (the size tells the
# rest) — so that a float mirrored as an int of the same size does not pass
_KIND = ('_Generic((%s), int: "i", long: "i", long long: "i", unsigned char: "u", unsigned: "u", unsigned long: "u", '
         'unsigned long long: "u", float: "f", double: "f", default: "p")')
_CTYPES_KIND = dict([(c, "i") for c in "bhilq"] + [(c, "u") for c in "BHILQ"] + [("f", "f"), ("d", "f"), ("P", "p")])


def test_every_structure_of_the_header_is_generated_and_named():
    raw = open(_rlx.HEADER).read()
    declared = re.findall(r"^\s*typedef struct (rlx_\w+)", raw, re.M)
    assert len(declared) == len(_rlx.STRUCTS) >= 16, (declared, list(_rlx.STRUCTS))
    assert declared == list(_rlx.STRUCTS)                         # declaration order, nothing missed by the parser
    assert set(_rlx.STRUCT_NAMES) == set(declared)                # no stale name in the table
    for c_name, cls in _rlx.STRUCTS.items():
        public = getattr(_rlx, _rlx.STRUCT_NAMES[c_name])
        assert issubclass(public, cls) and cls.__name__ == _rlx.STRUCT_NAMES[c_name]
        assert ctypes.sizeof(public) == ctypes.sizeof(cls) and public._fields_ is cls._fields_
    assert signals.SignalSource is _rlx.SignalSource
    assert _rlx.SplitkJob(M=3, N=5, batch=2, splits=4).workspace_floats() == (3 * 5 + 5) * 2 * 4
    assert _rlx.SplitkJob(M=3, N=5, batch=2, splits=1).workspace_floats() == 0


def test_layout_matches_the_c_compiler(tmp_path):
    cc = _compiler()
    if cc is None:
        pytest.skip("no C compiler (cc or ROCm's clang) on this machine")
    lines, expected = [], []
    for c_name, cls in _rlx.STRUCTS.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (c_name, c_name))
        expected.append("%s %d" % (c_name, ctypes.sizeof(cls)))
        for path, off, size, kind in _flatten(cls):
            member = "((%s *)0)->%s" % (c_name, path)
            lines.append('printf("%s.%s %%zu %%zu %%s\\n", offsetof(%s, %s), sizeof(%s), %s);'
                         % (c_name, path, c_name, path, member, _KIND % member))
            expected.append("%s.%s %d %d %s" % (c_name, path, off, size, kind))
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rlx.h"\nint main(void) {\n%s\nreturn 0;\n}\n'
                   % "\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run([cc, "-std=c11", "-I", os.path.dirname(_rlx.HEADER), "-o", str(exe), str(src)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    print("layout probe: %s, %d structures, %d scalar members" % (cc, len(_rlx.STRUCTS), len(got) - len(_rlx.STRUCTS)))
    assert len(got) > 16 * 4                                       # the probe printed something for every structure
    assert got == expected, [(g, e) for g, e in zip(got, expected) if g != e][:10]


def test_constants_come_from_the_header():
    raw = open(_rlx.HEADER).read()

    def define(name):
        return int(re.search(r"^#define %s\s+(-?\d+)\s*$" % name, raw, re.M).group(1))
    assert _rlx.NOISY_PASSES == define("RLX_NOISY_PASSES") == len(_rlx.NOISY_PASS)
    assert sorted(_rlx.NOISY_PASS.values()) == list(range(_rlx.NOISY_PASSES))
    assert _rlx.NOISY_MAX_LAYERS == define("RLX_NOISY_MAX_LAYERS")
    assert _rlx.ADAM_TICKET_WORDS == define("RLX_ADAM_TICKET_WORDS")
    assert _rlx.MAX_SPLITK_JOBS == define("RLX_MAX_SPLITK_JOBS")
    assert _rlx.MAX_COLUMNS == define("RLX_MAX_COLUMNS")
    assert _rlx.ABI_VERSION == define("RLX_ABI_VERSION")
    enum = dict(re.findall(r"\bRLX_ACT_(\w+)\s*=\s*(\d+)", raw))
    assert len(enum) >= 3
    assert _rlx.ACT == dict({None: int(enum["NONE"])}, **{k.lower(): int(v) for k, v in enum.items()})
    assert _rlx.ACT[None] == _rlx.ACT["none"] and {"relu", "tanh"} <= set(_rlx.ACT)
    # the status codes ride along: every enumerator of the header has an explicit value
    assert _rlx.CONSTANTS["RLX_OK"] == 0 and _rlx.CONSTANTS["RLX_ERR_INVALID_ARG"] == -1


def test_value_returning_rule_selects_the_supported_queries_and_the_version():
    declared = _rlx.parse_header()
    selected = {n for n in declared if _rlx.returns_value(n)}
    assert selected == {n for n in declared if n.endswith("_supported")} | {"rlx_abi_version"}
    assert len(selected) >= 12 and "rlx_abi_version" in declared
    for n in selected:                                             # an int, never a string
        assert declared[n][0] is ctypes.c_int, n
    assert not _rlx.returns_value("rlx_gemm") and not _rlx.returns_value("rlx_last_error")


@pytest.mark.parametrize("member, what", [
    ("float taps[4];", "taps"),                                    # array
    ("int flag : 1;", "flag"),                                     # bit-field
    ("union { int i; float f; } u;", "union"),
    ("int (*callback)(int);", "callback"),                         # function pointer
    ("short n;", "unknown type 'short'"),
    ("wchar_t *name;", "unknown type 'wchar_t'"),
    ("rlx_later later;", "unknown type 'rlx_later'"),              # a structure that is not defined yet
])
def test_struct_parser_refuses_what_is_outside_the_grammar(member, what):
    text = "typedef struct rlx_probe {\n    int n; const float *x, *y;\n    %s\n} rlx_probe;\n" % member
    with pytest.raises(ValueError, match=r"rlx_probe.*" + re.escape(what)):
        _rlx.parse_structs(text, {"rlx_probe": "Probe"})


def test_struct_parser_accepts_the_stated_grammar_and_needs_a_name():
    text = ("typedef struct rlx_inner { unsigned char *p; long long a, b; unsigned int u; uint32_t w; } rlx_inner;\n"
            "typedef struct rlx_outer { rlx_inner first, second; const struct rlx_fwd *next; const rlx_inner *same;\n"
            "    double d; int i; float f; } rlx_outer;\n")
    got = _rlx.parse_structs(text, {"rlx_inner": "Inner", "rlx_outer": "Outer"})
    inner, outer = got["rlx_inner"], got["rlx_outer"]
    assert [f[0] for f in inner._fields_] == ["p", "a", "b", "u", "w"] and ctypes.sizeof(inner) == 32
    assert [f[0] for f in outer._fields_] == ["first", "second", "next", "same", "d", "i", "f"]
    assert outer._fields_[0][1] is inner and outer._fields_[2][1] is ctypes.c_void_p and ctypes.sizeof(outer) == 96
    with pytest.raises(ValueError, match="rlx_outer has no class name"):
        _rlx.parse_structs(text, {"rlx_inner": "Inner"})
    with pytest.raises(ValueError, match="explicit integer value"):
        _rlx.parse_constants("enum { RLX_A = 0, RLX_B };")
