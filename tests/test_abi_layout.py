"""The C-ABI's records, constants and prototypes, stated once in Python (openwurli_amd/binding.py), against include/openwurli_hip.h and
include/openwurli_hip_test.h: no GPU needed.

One C program, generated from the binding's `_fields_` and compiled once, prints sizeof / offsetof of every struct and field and the value
of every constant as a C compiler sees the headers.  What that program cannot see (it is generated from the binding) comes from the
headers' text: which structs and constants exist, the order of each struct's declarators, how many parameters a prototype has.  A struct,
constant or parameter added to a header without its binding fails here.  SIZES and VALUES pin this header's layouts as literals: a change
to either table is a change of OW_ABI_VERSION."""
import ctypes as C
import importlib
import os
import pkgutil
import re
import subprocess

import numpy as np
import pytest

import openwurli_amd
from openwurli_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = {h: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S) for h in ("openwurli_hip.h", "openwurli_hip_test.h")}
TEXT = "\n".join(HEADERS.values())

snake = lambda camel: re.sub(r"(?<!^)([A-Z])", r"_\1", camel).lower()                       # OwMidiEvent -> ow_midi_event
STRUCTS = {snake(n): c for n, c in vars(binding).items() if isinstance(c, type) and issubclass(c, C.Structure)}
names = lambda cls: [f[0] for f in cls._fields_]
# every struct's declarators in order: `double w1[16][2], b1[16]` -> w1, b1; `const double* decay_rate` -> decay_rate
DECLARED = {s: [re.search(r"(\w+)\s*(?:\[[^\]]*\]\s*)*$", d).group(1) for decl in body.split(";") if decl.strip() for d in decl.split(",")]
            for s, body in re.findall(r"typedef struct (ow_\w+) \{(.*?)\} \1;", TEXT, flags=re.S)}
CONSTANTS = set(re.findall(r"#define (OW_\w+)", TEXT)) | {k for body in re.findall(r"enum \{(.*?)\}", TEXT, flags=re.S) for k in re.findall(r"(OW_\w+) =", body)}
NO_MIRROR = {     # constants the binding does not restate, and why
    r"OW_TEST_\w+": "indices into the debug dumps of openwurli_hip_test.h; the tests that read a dump name them themselves",
    r"OW_VOICE_\w+": "slot states come back as plain ints (ow_engine_slot_state); engine.py names them where it reports them",
    r"OW_(PREAMP|POWER_AMP|TREMOLO)_\w+": "the *_kind arguments are plain ints; each wrapper names the kinds it accepts beside its defaults",
}
MIRRORED = sorted(k for k in CONSTANTS if not any(re.fullmatch(p, k) for p in NO_MIRROR))

SIZES = {     # sizeof, in bytes
    "ow_diag": 56, "ow_power_amp_diag": 56, "ow_job": 48, "ow_mlp_weights": 4232, "ow_mlp_corrections": 88, "ow_mlp_train_model": 56,
    "ow_mlp_train_cfg": 32, "ow_mlp_train_result": 48, "ow_midi_event": 12, "ow_batch_cfg": 40, "ow_alias_audit_result": 232, "ow_timed_event": 16,
    "ow_midi_render_cfg": 56, "ow_midi_render_stats": 24, "ow_calib_point": 56, "ow_calibrate_cfg": 40, "ow_calibrate_row": 152, "ow_preamp_point": 32,
    "ow_preamp_measure_cfg": 32, "ow_preamp_measure_row": 96, "ow_poly_chord": 96, "ow_poly_cfg": 32, "ow_poly_row": 120, "ow_centroid_job": 40,
    "ow_centroid_cfg": 56, "ow_centroid_row": 88, "ow_note_job": 8, "ow_intermod_product": 56, "ow_intermod_report": 376, "ow_intermod_cfg": 24,
    "ow_intermod_detail": 64, "ow_intermod_row": 456, "ow_overshoot_cfg": 24, "ow_overshoot_row": 80, "ow_bark_cfg": 32, "ow_bark_row": 104,
    "ow_pump_point": 88, "ow_pump_cfg": 32, "ow_pump_row": 120, "ow_segment": 24, "ow_harmonics_cfg": 40, "ow_iso_note": 56, "ow_iso_cfg": 48,
}
VALUES = {
    "OW_ABI_VERSION": 8, "OW_MLP_HIDDEN": 16, "OW_MLP_OUTPUTS": 11, "OW_MLP_TRAIN_MAX_ROW_EPOCHS": 1 << 26, "OW_WAV_NONE": -1, "OW_WAV_ROUND": 0,
    "OW_WAV_TRUNCATE": 1, "OW_MAX_HARMONICS": 8, "OW_GOERTZEL_OFFSETS": 11, "OW_NOISE_MAX_BAND_BINS": 4096, "OW_AUDIT_HARMONICS": 12,
    "OW_CALIB_SAMPLES": 22050, "OW_PBENCH_SAMPLES": 22050, "OW_PBENCH_GAIN_LO": 13230, "OW_PBENCH_HARM_LO": 16537, "OW_POLY_MAX_NOTES": 31,
    "OW_CENTROID_MAX_WINDOW": 4096, "OW_CENTROID_NO_DATA": 0, "OW_CENTROID_OK": 1, "OW_CENTROID_MISS": 2, "OW_INTERMOD_MAX_PROBES": 75,
    "OW_INTERMOD_DIRTY": 0, "OW_INTERMOD_MARGINAL": 1, "OW_INTERMOD_OK": 2, "OW_INTERMOD_CLEAN": 3, "OW_PUMP_STATIC": 0, "OW_PUMP_STEP": 1,
    "OW_PUMP_RAMP": 2, "OW_PUMP_LOGCOS": 3,
}


@pytest.fixture(scope="session")
def compiled(tmp_path_factory):
    """{"S": {struct: size}, "F": {(struct, field): (offset, size)}, "K": {constant: value}} as gcc sees the headers."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "openwurli_hip_test.h"', 'int main(void) {']
    for s, cls in STRUCTS.items():
        lines.append(f'    printf("S {s} . %zu 0\\n", sizeof({s}));')
        lines += [f'    printf("F {s} {f} %zu %zu\\n", offsetof({s}, {f}), sizeof((({s}*)0)->{f}));' for f in names(cls)]
    lines += [f'    printf("K {k} . %lld 0\\n", (long long)({k}));' for k in MIRRORED]
    d = tmp_path_factory.mktemp("abi")
    (d / "layout.c").write_text("\n".join(lines + ["    return 0;", "}"]))
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(d / "layout"), str(d / "layout.c")])
    out = {"S": {}, "F": {}, "K": {}}
    for kind, a, b, x, y in (ln.split() for ln in subprocess.check_output([str(d / "layout")], text=True).splitlines()):
        out[kind][(a, b) if kind == "F" else a] = (int(x), int(y)) if kind == "F" else int(x)
    return out


# ---- completeness --------------------------------------------------------------------------------------------------------------------
def test_every_header_struct_has_a_binding_and_the_reverse():
    assert len(STRUCTS) == 43 and set(STRUCTS) == set(DECLARED) == set(SIZES)


def test_every_header_constant_is_mirrored_or_listed(compiled, hiplib):
    assert set(MIRRORED) == set(VALUES) and len(MIRRORED) < len(CONSTANTS)
    for k in MIRRORED:
        assert compiled["K"][k] == getattr(binding, k[3:]) == VALUES[k], k
    assert VALUES["OW_ABI_VERSION"] == binding.ABI_VERSION == hiplib.ow_abi_version() == 8      # SIZES and VALUES change with it, never alone


# ---- layouts -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", sorted(STRUCTS))
def test_struct_layout_header_compiler_binding(compiled, s):
    cls = STRUCTS[s]
    assert names(cls) == DECLARED[s], (s, [pair for pair in zip(names(cls), DECLARED[s]) if pair[0] != pair[1]])
    assert compiled["S"][s] == C.sizeof(cls) == SIZES[s], s
    for f in names(cls):
        assert compiled["F"][s, f] == (getattr(cls, f).offset, getattr(cls, f).size), (s, f)


def test_row_field_tuples_are_the_rows_doubles():
    for cls, lead, fields in ((binding.OwCalibrateRow, 3, binding.CALIBRATE_ROW_FIELDS), (binding.OwOvershootRow, 3, binding.OVERSHOOT_ROW_FIELDS),
                              (binding.OwBarkRow, 5, binding.BARK_ROW_FIELDS)):
        assert DECLARED[snake(cls.__name__)][lead:] == list(fields)


def test_every_dtype_is_its_struct(compiled):
    of_struct = {s: np.dtype(cls) for s, cls in STRUCTS.items() if not any(issubclass(t, C._Pointer) for _, t in cls._fields_)}
    assert set(STRUCTS) - set(of_struct) == {"ow_mlp_train_cfg", "ow_iso_cfg"}                  # by-pointer only: nobody needs an array of them
    seen = {}
    for m in pkgutil.iter_modules(openwurli_amd.__path__):
        mod = importlib.import_module("openwurli_amd." + m.name)
        for name, dt in vars(mod).items():
            if not name.endswith("DTYPE"):
                continue
            where = f"{m.name}.{name}"
            match = [s for s, d in of_struct.items() if isinstance(dt, np.dtype) and d == dt]
            assert len(match) == 1, (where, match)
            s = seen[where] = match[0]
            assert dt.itemsize == compiled["S"][s] and list(dt.names) == DECLARED[s], (where, s)
            for f in dt.names:
                assert (dt.fields[f][1], dt.fields[f][0].itemsize) == compiled["F"][s, f], (where, s, f)
    assert len(seen) == 26 and len(set(seen.values())) == 23, seen      # re-exported: NOTE_JOB_DTYPE by overshoot and bark_audit, TIMED_EVENT_DTYPE by midi_render
    assert seen["binding.MIDI_DTYPE"] == "ow_midi_event" and seen["intermod_audit.ROW_DTYPE"] == "ow_intermod_row"


# ---- prototypes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("header,table", [("openwurli_hip.h", binding.SYMBOLS), ("openwurli_hip_test.h", binding.TEST_SYMBOLS)])
def test_argtypes_count_the_prototypes_parameters(header, table):
    protos = dict(re.findall(r"\b(ow_\w+)\s*\(([^()]*)\)\s*;", HEADERS[header]))
    assert sorted(protos) == sorted(table)
    for fn, params in protos.items():
        n = 0 if params.strip() == "void" else params.count(",") + 1
        assert len(table[fn][1]) == n, (fn, params)


# ---- loading -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("version,needles", [(binding.ABI_VERSION + 1, ("OW_ABI_VERSION 9", "rebuild with ./build.sh")),
                                             (binding.ABI_VERSION, ("does not export ow_last_error",))])
def test_a_stale_library_is_refused_by_name(tmp_path, monkeypatch, version, needles):
    """A library that exports ow_abi_version alone: another version is refused as such before any other symbol is resolved, and with the
    right version the first missing symbol is named.  OwError both times, never a bare AttributeError."""
    (tmp_path / "stub.c").write_text("int ow_abi_version(void) { return %d; }\n" % version)
    so = str(tmp_path / "libstub.so")
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-o", so, str(tmp_path / "stub.c")])
    monkeypatch.setenv("OPENWURLI_HIP_LIB", so)
    monkeypatch.setattr(binding, "_LIB", None)
    with pytest.raises(binding.OwError) as e:
        binding.load_library()
    assert so in str(e.value) and all(s in str(e.value) for s in needles), str(e.value)
    assert binding._LIB is None
