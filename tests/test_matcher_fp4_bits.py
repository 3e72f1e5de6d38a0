"""The FP4 expansion rule of the matrix-core matcher (fp4_word, putslam_amd/csrc/ps_matcher_mfma.h), restated in plain Python
and read back from the header: nibble i of output dword j takes descriptor bit 4 i + j as its sign, every nibble's low three
bits are 0b110 (magnitude 4.0), and the 32 bits of a descriptor dword go to the 32 nibbles of its four output dwords one to one.
The header's static_asserts check the same at compile time; this test keeps the two statements of the rule together."""
import os
import re

M32 = 0xFFFFFFFF
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "putslam_amd", "csrc", "ps_matcher_mfma.h")


def fp4_word(w, j, sign=0x88888888, fill=0x66666666):
    return ((sign & (w << (3 - j))) | (~sign & fill)) & M32


def header_rule():
    """fp4_word's return expression as the header states it (C and Python agree on its operators), defaults included."""
    text = open(HEADER).read()
    m = re.search(r"constexpr uint32_t fp4_word\(uint32_t w, int j, uint32_t sign = (0x[0-9A-Fa-f]+)u, uint32_t fill = (0x[0-9A-Fa-f]+)u\)"
                  r"\s*\{\s*return ([^;]+);\s*\}", text)
    assert m, "fp4_word not found in ps_matcher_mfma.h"
    sign, fill, expr = int(m.group(1), 16), int(m.group(2), 16), m.group(3)
    assert re.fullmatch(r"[\s()&|~<>\-0-9a-z]+", expr) and set(re.findall(r"[a-z]+", expr)) <= {"w", "j", "sign", "fill"}
    return lambda w, j: eval(expr, {"__builtins__": {}}, dict(w=w, j=j, sign=sign, fill=fill)) & M32


WORDS = [0, M32, 0x80000001, 0xDEADBEEF, 0x01234567, 0xA5A5C3C3, 0x0F0F00FF, 0x13579BDF] + [1 << b for b in range(32)] + \
        [M32 ^ (1 << b) for b in range(32)]


def signs(words4):
    """{descriptor bit position the rule assigns: sign bit} over the 32 nibbles of four output dwords"""
    return {4 * i + j: (words4[j] >> (4 * i + 3)) & 1 for j in range(4) for i in range(8)}


def test_restated_rule_is_a_bijection_with_magnitude_four():
    for w in WORDS:
        out = [fp4_word(w, j) for j in range(4)]
        assert all(o & 0x77777777 == 0x66666666 for o in out), hex(w)
        s = signs(out)
        assert sorted(s) == list(range(32)) and all(s[b] == (w >> b) & 1 for b in range(32)), hex(w)
    for b in range(32):  # bit b alone: exactly one nibble of the 32 is negative, nibble b // 4 of dword b % 4
        out = [fp4_word(1 << b, j) for j in range(4)]
        neg = [(j, i) for j in range(4) for i in range(8) if (out[j] >> (4 * i)) & 0xF == 0xE]
        assert neg == [(b % 4, b // 4)] and sum(bin(o & 0x88888888).count("1") for o in out) == 1


def test_header_states_the_same_rule():
    rule = header_rule()
    for w in WORDS:
        assert [rule(w, j) for j in range(4)] == [fp4_word(w, j) for j in range(4)], hex(w)


def test_both_operand_sides_give_exact_distances():
    """What the contraction needs: with the same rule on both sides, sum over the 32 FP4 products of two dwords is
    16 * (32 - 2 * popcount(a ^ b))."""
    val = {0x6: 4.0, 0xE: -4.0}
    for a, b in zip(WORDS, reversed(WORDS)):
        pa = [val[(fp4_word(a, j) >> (4 * i)) & 0xF] for j in range(4) for i in range(8)]
        pb = [val[(fp4_word(b, j) >> (4 * i)) & 0xF] for j in range(4) for i in range(8)]
        assert sum(x * y for x, y in zip(pa, pb)) == 16 * (32 - 2 * bin(a ^ b).count("1"))
