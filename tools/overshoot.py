"""`preamp-bench overshoot` on the device (tools/preamp-bench/src/main.rs:2137-2247): the reference's flags and defaults, its stdout.

  python tools/overshoot.py [--notes 36,48,60,72,84] [--velocities 64,127] [--device N]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--notes", default="36,48,60,72,84")
    ap.add_argument("--velocities", default="64,127")
    ap.add_argument("--device", type=int, default=0)
    return ap.parse_args(argv)


def main(argv=None):
    from openwurli_amd import overshoot as ov
    a = parse_args(argv)
    sys.stdout.write(ov.report(ov.parse_csv_u8(a.notes), ov.parse_csv_u8(a.velocities), device=a.device))


if __name__ == "__main__":
    main()
