"""The one loader of the test side's native libraries: the CPU oracle (oracle/ow_oracle_capi.cpp) and the CPU restatements over its
headers (tests/c/*_ref.cpp), each plain or as one of the two sensitivity variants.

Building is make's job: load() asks oracle/Makefile for exactly the library it is about to open, once per process and library, so an
edited oracle header is noticed by the next process and an up-to-date library costs milliseconds.  The libraries live in oracle/_build.

Declaring is the source's job: after dlopen, every function the library exports gets its restype and argtypes from the text of its
definition -- the definitions at column 0 inside the source's `extern "C" { ... }` block.  The vocabulary is TYPES plus pointers (anything
with `*` or `[]`, as c_void_p).  A type outside it, or an exported function whose definition was not found (one made by a macro, say), is
refused with a message naming the library, the function and the parameter: no function is ever called with a guessed signature.
"""
import ctypes as C
import os
import re
import subprocess
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
VARIANTS = ("", "perturbed", "voice_perturbed")      # plain, -DOW_ORACLE_EXP_PERTURB, -DOW_ORACLE_VOICE_PERTURB (oracle/Makefile)
TYPES = {"void": None, "int": C.c_int, "unsigned": C.c_uint, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t,
         "long long": C.c_longlong, "unsigned long long": C.c_ulonglong}
_TYPE_WORDS = {"void", "char", "short", "int", "long", "signed", "unsigned", "float", "double", "size_t"}
_LIBS = {}
_LOCK = threading.Lock()
_NOT_CODE = re.compile(r'//[^\n]*|/\*.*?\*/|"(?:\\.|[^"\\\n])*"|\'(?:\\.|[^\'\\\n])*\'', re.S)
_DEFINITION = re.compile(r"^(?!static\b)((?:\w+[ \t*]+)+)(\w+)[ \t]*\(", re.M)


class Refused(Exception):
    pass


def _matching(text, at, opener, closer):
    """Index of the `closer` that matches the `opener` at text[at]."""
    depth = 0
    for i in range(at, len(text)):
        depth += (text[i] == opener) - (text[i] == closer)
        if depth == 0:
            return i
    raise Refused("unbalanced %s%s" % (opener, closer))


def prototypes(source_text):
    """{name: (return type text, [parameter text])} of the definitions at column 0 inside the extern "C" block; static ones are not
    exported and are left out."""
    m = re.search(r'^extern "C" \{', source_text, re.M)
    if m is None:
        return {}
    code = _NOT_CODE.sub(lambda c: " " if c.group().startswith("/") else '""', source_text[m.end() - 1:])
    block = code[1:_matching(code, 0, "{", "}")]
    out = {}
    for d in _DEFINITION.finditer(block):
        close = _matching(block, d.end() - 1, "(", ")")
        if block[close + 1:].lstrip()[:1] == "{":
            params = " ".join(block[d.end():close].split())
            out[d.group(2)] = (d.group(1), [] if params in ("", "void") else [p.strip() for p in re.split(r",(?![^()]*\))", params)])
    return out


def _ctype(text, where, parameter=False):
    """The ctypes type of a return type, or of a parameter with or without its name."""
    words = [w for w in text.split() if w != "const"]
    if "(" not in text and ("*" in text or "[" in text):
        return C.c_void_p
    if parameter and len(words) > 1 and words[-1] not in _TYPE_WORDS:
        words = words[:-1]                            # the name
    if " ".join(words) in TYPES and not (parameter and words == ["void"]):
        return TYPES[" ".join(words)]
    raise Refused("%s: `%s` is outside the vocabulary (%s, pointers)" % (where, text.strip(), ", ".join(TYPES)))


def exported_functions(so_path):
    """The function symbols the library defines for C: nm's T entries but the mangled ones and the linker's _init / _fini."""
    out = subprocess.check_output(["nm", "-D", "--defined-only", so_path], universal_newlines=True)
    return {f[2] for f in (line.split() for line in out.splitlines()) if len(f) == 3 and f[1] == "T" and not f[2].startswith("_")}


def declare(lib, so_path, source_path):
    """Set restype and argtypes of every function `lib` exports from its definition in the source; returns the names."""
    with open(source_path) as f:
        protos = prototypes(f.read())
    names = exported_functions(so_path)
    for name in sorted(names):
        where = "%s: %s" % (os.path.basename(so_path), name)
        if name not in protos:
            raise Refused("%s is exported, but %s defines no such function at column 0 of its extern \"C\" block" %
                          (where, os.path.relpath(source_path, ROOT)))
        ret, params = protos[name]
        fn = getattr(lib, name)
        fn.restype = _ctype(ret, where + ", return type")
        fn.argtypes = [_ctype(p, "%s, parameter %d (`%s`)" % (where, i + 1, _param_name(p)), parameter=True) for i, p in enumerate(params)]
    return names


def _param_name(text):
    """For the messages: the identifier of `(*name)(...)`, else the last one in front of any `[...]`."""
    m = re.search(r"\(\s*\*\s*(\w+)", text)
    return m.group(1) if m else re.findall(r"[A-Za-z_]\w*", text)[-1]


def target(name, variant=""):
    """(make target under oracle/, source path) of library `name` ("ow_oracle" or "<command>_ref") in one of VARIANTS."""
    assert variant in VARIANTS, variant
    source = os.path.join(ORACLE_DIR, "ow_oracle_capi.cpp") if name == "ow_oracle" else os.path.join(ROOT, "tests", "c", name + ".cpp")
    return "_build/lib%s%s.so" % (name, "_" + variant if variant else ""), source


def load(name, variant=""):
    """The library, brought up to date by make, opened and declared: once per process."""
    with _LOCK:
        if (name, variant) not in _LIBS:
            goal, source = target(name, variant)
            subprocess.check_call(["make", "-s", "-C", ORACLE_DIR, goal])
            path = os.path.join(ORACLE_DIR, goal)
            lib = C.CDLL(path)
            declare(lib, path, source)
            _LIBS[(name, variant)] = lib
        return _LIBS[(name, variant)]
