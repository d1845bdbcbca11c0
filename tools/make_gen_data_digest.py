#!/usr/bin/env python3
"""Record what tools/extract_constants.py makes of the reference's literals, as tests/golden/gen_data_digest.json: the SHA-256 of the
whole generated header and, per table, its value count and the SHA-256 of its literal tokens.  Runs only where the reference tree
the generator reads exists; tests/test_oracle_baked_matrices.py then holds data/ow_gen_data.h to the record anywhere."""
import hashlib
import importlib.util
import json
import os
import re
import sys
import tempfile
from pathlib import Path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "gen_data_digest.json")
ENTRY_RE = re.compile(r"^OW_DATA_DECL double (\w+)((?:\[\w+\])*) = (\{.*?\}|[^;{]+);|^#define (\w+) (\S+)$", re.S | re.M)


def digest(text):
    """{"sha256": of the text, "tables": name -> {"count", "sha256" of the tokens joined by ','}} for every table / scalar / #define."""
    tables = {}
    for m in ENTRY_RE.finditer(text):
        name, body = (m.group(1), m.group(3)) if m.group(1) else (m.group(4), m.group(5))
        toks = [t for t in re.split(r"[\s,{}]+", body) if t]
        tables[name] = {"count": len(toks), "sha256": hashlib.sha256(",".join(toks).encode()).hexdigest()}
    return {"sha256": hashlib.sha256(text.encode()).hexdigest(), "tables": tables}


def main():
    spec = importlib.util.spec_from_file_location("extract_constants", os.path.join(ROOT, "tools", "extract_constants.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with tempfile.TemporaryDirectory() as td:
        mod.OUT = Path(td) / "ow_gen_data.h"
        mod.main()
        rec = digest(mod.OUT.read_text())
    with open(OUT, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {OUT} ({len(rec['tables'])} tables)")


if __name__ == "__main__":
    sys.exit(main())
