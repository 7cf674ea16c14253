"""x = s / 32767 in two FP64 instructions (scale_sample in sela_encode.hip): q = s * C1 with C1 = 2^-15 + 2^-30 + 2^-45, which is
exact for a 17-bit s, then x = fma(s, C2, q) with C2 = RN(1/32767 - C1).  Checked here with exact rationals for EVERY s the fast
kernels can meet -- 16-bit samples and the difference of two, [-65536, 65536] -- against the correctly rounded quotient the
reference computes (src/lpc/residue_generator.cpp:12-18).  No GPU: the constants are read from the kernel source.
"""
import os
import re
from fractions import Fraction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C1_HEX, C2_HEX = "0x1.0002000400000p-15", "0x1.0002000400080p-60"
DOMAIN = range(-65536, 65537)


def _rn(q: Fraction) -> float:
    """the double nearest to a rational, ties to even (int / int in Python is correctly rounded)"""
    return q.numerator / q.denominator


def test_the_kernel_source_holds_these_constants():
    text = open(os.path.join(ROOT, "sela_amd", "csrc", "sela_encode.hip")).read()
    body = text[text.index("double scale_sample(int32_t s)"):]
    body = body[: body.index("\n}\n")]
    m = re.search(r"c1 = (0x[0-9a-fA-F.]+p-?\d+), c2 = (0x[0-9a-fA-F.]+p-?\d+);", body)
    assert m, body
    assert float.fromhex(m.group(1)) == float.fromhex(C1_HEX) and float.fromhex(m.group(2)) == float.fromhex(C2_HEX)
    assert "__builtin_fma(x, c2, q)" in body and "x * c1" in body, body


def test_the_constants_are_what_the_derivation_says():
    c1, c2 = Fraction(float.fromhex(C1_HEX)), Fraction(float.fromhex(C2_HEX))
    assert c1 == Fraction(1, 2**15) + Fraction(1, 2**30) + Fraction(1, 2**45)
    assert float.fromhex(C2_HEX) == _rn(Fraction(1, 32767) - c1)
    assert c2 > 0 and abs(c1 + c2 - Fraction(1, 32767)) < Fraction(1, 2**112)


def test_two_instructions_give_the_quotient_for_every_17_bit_sample():
    c1, c2 = Fraction(float.fromhex(C1_HEX)), Fraction(float.fromhex(C2_HEX))
    wrong = []
    for s in DOMAIN:
        q = s * c1
        assert Fraction(_rn(q)) == q, ("s * C1 is not exact", s)  # the multiply rounds nothing away
        x = _rn(s * c2 + q)                                       # the fma: one rounding of the exact sum
        if x != s / 32767.0 or (s == 0 and str(x) != "0.0"):
            wrong.append(s)
    assert not wrong, (len(wrong), wrong[:8])


def test_the_product_alone_is_not_exact():
    """s * RN(1/32767) without a correction step differs from the quotient for 1280 of the 131,073 values: the second
    instruction cannot be dropped."""
    r = 1.0 / 32767.0
    wrong = [s for s in DOMAIN if s * r != s / 32767.0]
    assert len(wrong) == 1280, len(wrong)
