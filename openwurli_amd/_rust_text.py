"""What the preamp-bench command modules share: the reference's base rate, Rust's number conversions and number formatting."""
import math

BASE_SR = 44100.0                                           # main.rs:27


def midi_note_name(note: int) -> str:
    """main.rs:666-673."""
    return "%s%d" % (("C", "C#", "D", "D#", "E", "F", "F#", "G", "G#", "A", "A#", "B")[note % 12], note // 12 - 1)


def parse_csv_u8(text: str) -> list:
    """parse_csv_list::<u8> (main.rs:907-910): comma-separated, trimmed, items that are no u8 are dropped."""
    out = []
    for item in text.split(","):
        item = item.strip()
        digits = item[1:] if item[:1] == "+" else item
        if digits.isascii() and digits.isdigit() and int(digits) <= 255:
            out.append(int(digits))
    return out


def as_usize(x: float) -> int:
    """Rust's `f64 as usize`: NaN and negatives give 0."""
    return int(x) if x > 0 and math.isfinite(x) else 0


def samples(duration: float) -> int:
    """(duration * BASE_SR) as usize."""
    return as_usize(float(duration) * BASE_SR)


def to_dbfs(val: float) -> float:
    """main.rs:2241-2247."""
    return 20.0 * math.log10(val) if val > 1e-15 else -120.0


def _f(x, spec):
    """Rust's {:spec}: it rounds the exact binary value half to even, as Python's %-format does, but prints NaN as "NaN" (padded to the
    width, without a sign) where Python prints "nan"; inf is "inf" in both."""
    x = float(x)
    if math.isnan(x):
        return ("%" + spec.split(".")[0].lstrip("+") + "s") % "NaN"
    return ("%" + spec) % x


def _e(x, prec, plus=False):
    """Rust's {:.<prec>e} ({:+.<prec>e} with plus): the exponent carries neither padding nor a plus sign -- 1.000000e3, 8.540763e0,
    2.5e-7 -- where Python prints 1.000000e+03.  NaN and inf as in _f."""
    x = float(x)
    if math.isnan(x):
        return "NaN"
    if math.isinf(x):
        return ("+" if plus and x > 0 else "") + ("inf" if x > 0 else "-inf")
    mant, exp = ((("%+." if plus else "%.") + str(int(prec)) + "e") % x).split("e")
    return mant + "e" + str(int(exp))
