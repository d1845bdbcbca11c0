#!/usr/bin/env python3
"""Record tests/golden/chain_bits_parent.npz, tests/golden/power_amp_cases_parent.npz and tests/golden/job_chain_bits_parent.npz: the
renders of tests/chain_bits_cases.py with ONE build of the library, against which tests/test_gpu_chain_bits.py,
tests/test_gpu_power_amp_cases.py and tests/test_gpu_job_chain_bits.py compare the current build bit for bit.  Run it on an MI355X with
the library of the commit to pin (a scratch worktree of it, built with build.sh):

    OPENWURLI_HIP_LIB=<worktree>/openwurli_amd/lib/libopenwurli_hip.so python tools/record_chain_bits.py --commit <hash> --box <name>

The commit and the box go into the files (`meta`).  --only takes the names of the files to write (default: all three).  In the job
fixture an array that equals one already in the file, bit for bit, is kept as the other's name ("=<name>"): the forms of one kernel give
the same rows."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", required=True, help="commit the library was built from")
    ap.add_argument("--box", required=True, help="machine the renders ran on")
    ap.add_argument("--only", nargs="*", help="files to record (default: all)")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    import chain_bits_cases as cases
    import openwurli_amd as ow
    meta = np.array([f"commit={args.commit}", f"box={args.box}", f"library={os.path.basename(ow.library_path())}"])
    for fname, table, run in (("chain_bits_parent.npz", cases.CHAIN_CASES, cases.run_chain),
                              ("power_amp_cases_parent.npz", cases.PA_CASES, cases.run_power_amp),
                              ("job_chain_bits_parent.npz", cases.JOB_CASES, cases.run_job_case)):
        if args.only and fname not in args.only:
            continue
        arrays, seen = {"meta": meta}, {}
        for name in table:
            t0 = time.perf_counter()
            first = run(ow, name)
            t1 = time.perf_counter()
            again = run(ow, name)
            for key, a in first.items():
                assert a.tobytes() == again[key].tobytes(), f"{name}/{key}: two renders of one build differ"
                same = seen.setdefault((a.dtype.str, a.shape, a.tobytes()), f"{name}/{key}")
                alias = table is cases.JOB_CASES and same != f"{name}/{key}" and a.nbytes >= 256      # only test_gpu_job_chain_bits.py resolves these
                arrays[f"{name}/{key}"] = np.array("=" + same) if alias else a
            print(name, "%.2f s" % (t1 - t0), "resets", int(first["resets"].sum()) if "resets" in first else "-",
                  {k: v.tolist() for k, v in first.items() if k in ("peak", "tap_absmin_nonzero")},
                  ("tap max %.3g" % first["tap_absmax"].max()) if "tap_absmax" in first else "", flush=True)
        path = os.path.join(args.out_dir, fname)
        np.savez_compressed(path, **arrays)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
