"""TEST INFRASTRUCTURE: the numbers that cross the text boundary, at the cases where hand-written arithmetic goes wrong.

Seeded generators, no file: ``decimal_texts()`` (JSON number spellings of at most 19 significant digits: what the
Eisel-Lemire parser of ``surge_amd/csrc/f64_parse.h`` must decide alone), ``long_texts()`` (20 .. 399 bytes with a
non-zero digit beyond the 19th: what it hands to an exact method), ``double_bits()`` (bit patterns for the writer of
``f64_text.h``) and ``integer_texts()``.  ``tests/test_number_text_cases.py`` holds every one of them to its own claims on
the CPU; ``tests/test_number_text_gpu.py`` runs them through the device kernels."""
import functools
import random

import numpy as np

EXPONENTS = range(-345, 312)                # every decimal exponent the parser's table covers, and a few on either side
SIGNIFICAND_DIGITS = (1, 2, 9, 15, 16, 17, 18, 19)
SPECIALS = ["2.4703282292062327e-324", "2.4703282292062328e-324",      # half of the smallest subnormal: down to 0 (a tie, to even), and just above it
            "2.2250738585072011e-308", "2.2250738585072014e-308",      # the largest subnormal | the smallest normal
            "1.7976931348623157e308", "1.7976931348623158e308", "1.7976931348623159e308",  # the largest double | still it | infinity
            "1e309", "0e999", "1e-400", "9999999999999999999e-343",
            "0", "-0", "0.0", "-0.0", "1", "-1", "4.9e-324", "5e-324", "1e-323", "1e308", "1e-308"]


def bits_of(x: float) -> int:
    return int(np.float64(x).view(np.uint64))


def shortest(bits: int) -> str:
    """The shortest spelling that reads back as this double (Python's repr: David Gay's algorithm)."""
    return repr(float(np.uint64(bits).view(np.float64)))


def _digits(rnd, n):
    return str(rnd.randint(1, 9)) + "".join(rnd.choice("0123456789") for _ in range(n - 1))


def tie_significands(n=1500, seed=52):
    rnd = random.Random(seed)
    return [rnd.randint(2 ** 52, 2 ** 53 - 1) for _ in range(n)]


@functools.lru_cache(maxsize=None)
def decimal_classes():
    """The corpus by class: name -> list of texts (``decimal_texts()`` is their concatenation)."""
    rnd = random.Random(19)
    out = {}
    out["every exponent"] = [f"{_digits(rnd, nd)}e{e}" for e in EXPONENTS for nd in SIGNIFICAND_DIGITS for _ in range(2)]
    ms = tie_significands()
    # m + 1/2 lies exactly between the doubles m and m + 1; an odd integer below 2^54 between two even ones
    out["ties"] = [f"{m}.5" for m in ms] + [str(2 * m + 1) for m in ms]
    # ... and one unit of the 19th digit below and above each of them
    beside = lambda n, up: f"{n}.{'0' * (18 - len(str(n)))}1" if up else f"{n - 1}.{'9' * (19 - len(str(n - 1)))}"  # noqa: E731
    out["beside a tie"] = ([f"{m}.499" for m in ms] + [f"{m}.501" for m in ms] + [beside(2 * m + 1, False) for m in ms] + [beside(2 * m + 1, True) for m in ms])
    out["first subnormals"] = [shortest(b) for b in range(1, 201)]
    out["subnormal boundary"] = [shortest(b) for b in (2 ** 52 - 1, 2 ** 52, 2 ** 52 + 1)]
    out["specials"] = list(SPECIALS)
    p2 = []
    for k in range(-1074, 1024, 3):
        b = bits_of(2.0 ** k)
        p2 += [shortest(x) for x in (b - 1, b, b + 1) if 0 < x < 0x7FF0000000000000]
    out["powers of two"] = p2
    variants = []
    for _ in range(400):
        ds, e = _digits(rnd, rnd.choice(SIGNIFICAND_DIGITS)), rnd.randint(-330, 290)
        variants += ["0" * rnd.randint(1, 5) + f"{ds}e{e}",                                # leading zeros
                     f"{ds}E+{abs(e)}" if len(ds) + abs(e) < 300 else f"{ds}E+7", f"{ds}e-{abs(e)}", f"-{ds}E{e}",
                     f"{ds[0]}.{ds[1:] or '0'}e{e}", f"{ds}.0e{e}", f"{ds}e{'-' if e < 0 else ''}00{abs(e)}"]
        d19 = _digits(rnd, 19)
        z = "0" * rnd.randint(1, 40)
        variants += [f"{d19}{z}e{rnd.randint(-340, 250)}", f"{d19}.{z}", f"{d19[:7]}.{d19[7:]}{z}E{rnd.randint(-300, 290)}"]  # the dropped digits are all zero
    for zeros in (1, 5, 20, 100, 300, 306, 323, 340):
        for nd in SIGNIFICAND_DIGITS:
            variants.append("0." + "0" * zeros + _digits(rnd, nd))                                                             # 0.000...ddd
    out["spellings"] = variants
    return out


def decimal_texts():
    return [t for texts in decimal_classes().values() for t in texts]


@functools.lru_cache(maxsize=None)
def _long_texts():
    from fractions import Fraction

    rnd = random.Random(20)
    out = ["0.1000000000000000055511151231257827021181583404541015625", "9007199254740993.00000000000000000001",
           "123456789012345678901234567890", "-12345678901234567890123.5E-3", "12345678901234567891", "1" + "0" * 18 + "1", "1." + "0" * 396 + "1"]  # (20 bytes ... 399 bytes)
    for m in tie_significands(60, seed=53):   # a tie, and the digit far behind it that breaks it
        out += [f"{m}.5" + "0" * rnd.randint(2, 60) + "1", f"{m}.4" + "9" * rnd.randint(18, 60), f"{2 * m + 1}." + "0" * rnd.randint(3, 40) + "3"]
    for _ in range(60):                    # a double's exact decimal expansion (up to some hundred digits), cut to the limit
        v = float(np.uint64(rnd.randrange(0x3000000000000000, 0x4FF0000000000000)).view(np.float64))
        f = Fraction(v)
        whole, rest = divmod(f.numerator, f.denominator)
        frac = ""
        while rest and len(frac) < 360:
            rest *= 10
            d, rest = divmod(rest, f.denominator)
            frac += str(d)
        t = (f"{whole}.{frac}" if frac else str(whole))[:399].rstrip(".")
        if len(t.replace(".", "").lstrip("0")) > 19 and t.replace(".", "").lstrip("0")[19:].strip("0"):
            out.append(t)
    for total in (20, 21, 25, 40, 100, 200, 300, 390, 398, 399):  # random digits, the whole spelling `total` bytes long
        for _ in range(8):
            exp = f"e{rnd.randint(-320, 300 - total)}" if total <= 200 and rnd.random() < 0.6 else ""
            point = rnd.random() < 0.5
            if total - len(exp) - point < 20:  # (fewer digits than the fast path takes: digits only)
                exp, point = "", False
            n = total - len(exp) - point
            ds = _digits(rnd, n - 1) + str(rnd.randint(1, 9))
            pos = rnd.randint(1, n - 1)
            out.append((ds[:pos] + "." + ds[pos:] if point else ds) + exp)
    return [t for t in out if 20 <= len(t) <= 399]


def long_texts():
    return list(_long_texts())


@functools.lru_cache(maxsize=None)
def bit_classes():
    """name -> uint64 array: the structured sets of tests/test_f64_text.py, and the longest texts."""
    rng = np.random.default_rng(1)
    rnd = random.Random(2)
    out = {}
    out["powers of two"] = np.concatenate([(2.0 ** np.arange(-1074, 1024)).view(np.uint64),
                                           (2.0 ** np.arange(-1022, 1024)).view(np.uint64) - np.uint64(1),
                                           (2.0 ** np.arange(-1022, 1023)).view(np.uint64) + np.uint64(1)])
    out["powers of ten"] = np.array([float(f"1e{e}") for e in range(-323, 309)]).view(np.uint64)
    out["families"] = np.array([float(f"{m}e{e}") for e in range(-30, 40)
                                for m in (9.999999999999999, 9.999999999999998, 1.0000000000000002, 5.5, 2.5)]).view(np.uint64)
    m = np.arange(1, 5001, dtype=np.uint64)
    out["mantissas 1 to 5000"] = np.concatenate([m, m | np.uint64(1 << 63)])  # the two-digit rule's product and divisions
    out["subnormals"] = rng.integers(1, 1 << 52, size=3000, dtype=np.uint64)
    r = rng.integers(0, 1 << 64, size=6000, dtype=np.uint64)
    out["random"] = r[(r & np.uint64(0x7FF0000000000000)) != np.uint64(0x7FF0000000000000)]  # finite only
    edge = []
    for adj in (-7, -6, -1, 0, 19, 20):  # the adjusted exponents where BigDecimal.toString changes form
        for _ in range(40):
            one = float(f"{rnd.randint(1, 9)}e{adj}")
            edge += [one, -one]
            for _ in range(20):
                v = float(f"{rnd.randint(1, 9)}.{_digits(rnd, 16)}e{adj}")
                if len(repr(v).split("e")[0].replace(".", "").strip("0")) == 17:  # 17 digits are the shortest: the longest text
                    edge += [v, -v]
                    break
    out["longest texts"] = np.array(edge, dtype=np.float64).view(np.uint64)
    out["zeros"] = np.array([0.0, -0.0], dtype=np.float64).view(np.uint64)
    return out


def double_bits():
    return np.concatenate(list(bit_classes().values()))


INT_RANGES = {"I32": (-(2 ** 31), 2 ** 31 - 1), "U32": (0, 2 ** 32 - 1), "I64": (-(2 ** 63), 2 ** 63 - 1)}


def integer_texts(kind: str):
    lo, hi = INT_RANGES[kind]
    return [str(lo), str(hi), str(lo - 1), str(hi + 1), "-0", "00", "01", "1.0", "1e0", "12345678901234567890", "0", "-1", "7"]


def int_or_none(text: str):
    """What Python reads the spelling as when it is an integer literal of digits with an optional minus, else None."""
    body = text[1:] if text.startswith("-") else text
    return int(text) if body.isdigit() else None
