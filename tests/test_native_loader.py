"""tests/native.py, the loader of the oracle and of the CPU restatements: what it derives from a source's text, what it refuses, and that
every library of the suite builds through oracle/Makefile, loads, and has a declaration for exactly the functions it exports."""
import ctypes as C
import os
import subprocess

import pytest

import native

ADDRESS = 0x7f0012345678

SYNTHETIC = r"""
#include <cstddef>
namespace { double outside(double x) { return 2.0 * x; } }
double mangled(double x) { return outside(x); }
extern "C" {
// double syn_in_a_comment(long double x) { return x; }
/* int syn_in_a_block_comment(int x) { */
static double helper(double x) { return x; }
void syn_void(void) {}
int syn_int(int x) { return x; }
unsigned syn_unsigned(unsigned x) { return x; }
float syn_float(float x) { return x; }
double syn_double(double x) { return helper(x); }
size_t syn_size(size_t x) { return x; }
long long syn_ll(long long x) { return x; }
unsigned long long syn_ull(unsigned long long x) { return x; }
void* syn_ptr(void) { return (void*)0x7f0012345678; }
const double* syn_same(const double* p) { return p; }
int syn_is_ptr(const void* p) { return p == (const void*)0x7f0012345678 ? 1 : 0; }
double syn_broken(const double* in, double out[4], size_t n,      // a comment (with parentheses, a comma) and a brace {
                  float scale,
                  const unsigned long long seed) {
    for (size_t i = 0; i < 4; ++i) out[i] = i < n ? in[i] * scale : (double)seed;
    return out[0] + out[3];
}
}  // extern "C"
int after_the_block(int x) { return x; }
"""
PTR = C.c_void_p
EXPECTED = {
    "syn_void": (None, []), "syn_int": (C.c_int, [C.c_int]), "syn_unsigned": (C.c_uint, [C.c_uint]), "syn_float": (C.c_float, [C.c_float]),
    "syn_double": (C.c_double, [C.c_double]), "syn_size": (C.c_size_t, [C.c_size_t]), "syn_ll": (C.c_longlong, [C.c_longlong]),
    "syn_ull": (C.c_ulonglong, [C.c_ulonglong]), "syn_ptr": (PTR, []), "syn_same": (PTR, [PTR]), "syn_is_ptr": (C.c_int, [PTR]),
    "syn_broken": (C.c_double, [PTR, PTR, C.c_size_t, C.c_float, C.c_ulonglong]),
}
RESTATEMENTS = ("note_audit_ref", "bark_audit_ref", "centroid_track_ref", "render_poly_ref", "pump_ref", "calibrate_ref", "preamp_bench_ref",
                "mlp_eval_ref")
# every library the suite and the tools load: the oracle's three, the eight restatements, and the sensitivity variants their loaders name
LIBRARIES = ([("ow_oracle", v) for v in native.VARIANTS] + [(n, "") for n in RESTATEMENTS] +
             [("note_audit_ref", "voice_perturbed"), ("bark_audit_ref", "voice_perturbed"), ("centroid_track_ref", "perturbed"),
              ("render_poly_ref", "perturbed")])


def build(tmp_path, text, name="libsyn.so"):
    """`text` as a shared library with the compiler and the flags oracle/Makefile states: (library path, source path)."""
    flags = subprocess.check_output(["make", "-s", "-C", native.ORACLE_DIR, "flags"], universal_newlines=True).split()
    src, so = str(tmp_path / "syn.cpp"), str(tmp_path / name)
    with open(src, "w") as f:
        f.write(text)
    subprocess.check_call(flags + ["-shared", "-o", so, src])
    return so, src


def test_declarations_come_from_the_source_text(tmp_path):
    so, src = build(tmp_path, SYNTHETIC)
    L = C.CDLL(so)
    assert native.declare(L, so, src) == set(EXPECTED)
    for name, (res, args) in EXPECTED.items():
        assert getattr(L, name).restype is res and getattr(L, name).argtypes == args, name
    # values that survive only with the declarations
    assert L.syn_size(2 ** 40) == 2 ** 40
    assert L.syn_ull(2 ** 63 + 1) == 2 ** 63 + 1
    assert L.syn_ll(-3 * 2 ** 40) == -3 * 2 ** 40
    assert L.syn_float(0.1) == C.c_float(0.1).value != 0.1
    assert L.syn_double(0.1) == 0.1
    assert L.syn_double(3) == 3.0                          # a plain int for a double parameter is converted, not passed in an integer register
    assert L.syn_int(-7) == -7 and L.syn_unsigned(2 ** 32 - 1) == 2 ** 32 - 1
    assert L.syn_ptr() == ADDRESS and L.syn_is_ptr(L.syn_ptr()) == 1 and L.syn_is_ptr(None) == 0
    data, out = (C.c_double * 2)(1.5, 2.5), (C.c_double * 4)()
    assert L.syn_same(data) == C.addressof(data)
    assert L.syn_broken(data, out, 2, 2.0, 2 ** 53) == 3.0 + 2.0 ** 53 and list(out) == [3.0, 5.0, 2.0 ** 53, 2.0 ** 53]
    with pytest.raises(C.ArgumentError):
        L.syn_int(1.5)


@pytest.mark.parametrize("parameter, word", [("long double x", "x"), ("struct pair p", "p"), ("double (*fn)(double, int)", "fn"), ("char c", "c")])
def test_a_type_outside_the_vocabulary_is_refused(tmp_path, parameter, word):
    so, src = build(tmp_path, 'struct pair { int a, b; };\nextern "C" {\nint refused_one(int n, %s) { return n; }\n}\n' % parameter)
    with pytest.raises(native.Refused, match=r"libsyn\.so: refused_one, parameter 2 \(`%s`\)" % word):
        native.declare(C.CDLL(so), so, src)


def test_a_return_type_outside_the_vocabulary_is_refused(tmp_path):
    so, src = build(tmp_path, 'extern "C" {\nlong double refused_two(int n) { return n; }\n}\n')
    with pytest.raises(native.Refused, match=r"libsyn\.so: refused_two, return type"):
        native.declare(C.CDLL(so), so, src)


def test_an_export_without_a_parsed_definition_is_refused(tmp_path):
    so, src = build(tmp_path, '#define DEFINE(name) double name(double x) { return x; }\nextern "C" {\nDEFINE(by_macro)\n}\n')
    with pytest.raises(native.Refused, match=r"libsyn\.so: by_macro is exported"):
        native.declare(C.CDLL(so), so, src)


@pytest.mark.parametrize("name, variant", LIBRARIES, ids=["%s-%s" % (n, v or "plain") for n, v in LIBRARIES])
def test_library_builds_loads_and_is_declared(name, variant, monkeypatch):
    lib = native.load(name, variant)
    goal, source = native.target(name, variant)
    exported = native.exported_functions(os.path.join(native.ORACLE_DIR, goal))
    with open(source) as f:
        assert set(native.prototypes(f.read())) == exported and exported
    assert all(getattr(lib, n).argtypes is not None for n in exported)
    # a second load in this process does not start make again ...
    monkeypatch.setattr(native.subprocess, "check_call", lambda *a, **k: pytest.fail("make started again for %s" % goal))
    assert native.load(name, variant) is lib
    # ... and in another process make decides: nothing to do now, a rebuild once a header of the oracle is newer
    make = ["make", "-s", "-q", "-C", native.ORACLE_DIR]
    assert subprocess.call(make + [goal]) == 0
    assert subprocess.call(make + ["-W", "ow_chain.hpp", goal]) == 1
