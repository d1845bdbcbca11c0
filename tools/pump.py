"""`preamp-bench pump-sweep` / `pump-trace` / `pump-spike` / `pump-step` / `pump-sinusoid` on the device
(tools/preamp-bench/src/main.rs:2329-3063): the reference's flags and defaults, its CSV files and its stderr report.

  python tools/pump.py pump-sweep    [--ldr-min 1000] [--ldr-max 1000000] [--points 256] [--settle 60000] [--avg 4096]
                                     [--sample-rate 48000] [--csv FILE]
  python tools/pump.py pump-trace    [--ldr 1000000] [--settle 400000] [--samples 131072] [--csv FILE]
  python tools/pump.py pump-spike    [--csv-prefix /tmp/pump_spike] [--settle 400000] [--avg 8192]
  python tools/pump.py pump-step     [--ldr-from 1000000] [--ldr-to 19000] [--sample-rate 88200] [--settle 750000] [--samples 720000]
                                     [--csv FILE]
  python tools/pump.py pump-sinusoid [--ldr-min 19000] [--ldr-max 1000000] [--freq 5.6] [--cycles 10] [--sample-rate 88200]
                                     [--settle 750000] [--csv FILE]
  all: [--device N]; --csv defaults to pump_<command>.csv in the system's temporary directory, as the reference's temp_default
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _count(text):
    """parse_flag(...) as usize (main.rs:98-105): a float, truncated; NaN and negatives give 0."""
    from openwurli_amd._rust_text import as_usize
    return as_usize(float(text))


def main(argv=None):
    from openwurli_amd import pump
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="command", required=True)

    def command(name, **flags):
        p = sub.add_parser(name)
        for flag, (typ, default) in flags.items():
            p.add_argument("--" + flag.replace("_", "-"), type=typ, default=default)
        p.add_argument("--device", type=int, default=0)
        return p
    command("pump-sweep", ldr_min=(float, 1_000.0), ldr_max=(float, 1_000_000.0), points=(_count, 256), settle=(_count, 60_000), avg=(_count, 4_096),
            sample_rate=(float, 48_000.0), csv=(str, None))
    command("pump-trace", ldr=(float, 1_000_000.0), settle=(_count, 400_000), samples=(_count, 131_072), csv=(str, None))
    command("pump-spike", csv_prefix=(str, "/tmp/pump_spike"), settle=(_count, 400_000), avg=(_count, 8_192))
    command("pump-step", ldr_from=(float, 1_000_000.0), ldr_to=(float, 19_000.0), sample_rate=(float, 88_200.0), settle=(_count, 750_000),
            samples=(_count, 720_000), csv=(str, None))
    command("pump-sinusoid", ldr_min=(float, 19_000.0), ldr_max=(float, 1_000_000.0), freq=(float, 5.6), cycles=(float, 10.0), sample_rate=(float, 88_200.0),
            settle=(_count, 750_000), csv=(str, None))
    a = vars(ap.parse_args(argv))
    fn = getattr(pump, a.pop("command").replace("-", "_"))
    sys.stderr.write(fn(**a)["report"])


if __name__ == "__main__":
    main()
