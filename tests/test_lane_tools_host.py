"""The host-callable part of uzkge_amd/csrc/lane_tools.hpp (the lane-serial tools the modules around the MSMs share) on the CPU: the
header's plain C++ has no HIP in it, so g++ builds tests/cpp/lane_tools_host.cpp as a stand-alone program -- once plain, once under
Address- and UndefinedBehaviorSanitizer -- and its answers are held to Python integers: a word against either modulus at 0, M - 1, M,
M + 1 and 2^256 - 1; the big-endian word codec on the same words; the curve equation at (1, 2) and (1, 3); the inversions in both
fields and the square root candidate, whose exponents the header derives from the moduli."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "lane_tools_host.cpp")
P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
MOD = {"q": P, "r": R}
FIXED = 0x2A5F1C3B9D7E604812F3A6B5C4D3E2F1A0B9C8D7E6F5041322314051607F8E9D          # 254 bits, below both moduli
assert FIXED.bit_length() == 254 and FIXED < R < P
H = lambda v: "%064x" % v


@pytest.fixture(scope="module", params=[[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def ask(request, tmp_path_factory):
    """the program, built once per flavour: ask(lines) -> the answers, one per line"""
    exe = os.path.join(str(tmp_path_factory.mktemp("lane_tools")), "lane_tools_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", *request.param, "-o", exe, SRC], check=True)

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "Sanitizer" not in r.stderr, r.stdout + r.stderr[:4000]
        out = r.stdout.split("\n")[:-1]
        assert len(out) == len(lines), r.stdout
        return out
    return run


def _edge_words(m):
    return [0, m - 1, m, m + 1, 2**256 - 1]


def test_below_modulus(ask):
    cases = [(f, v) for f in "qr" for v in _edge_words(MOD[f])]
    got = ask(["below %s %s" % (f, H(v)) for f, v in cases])
    assert got == ["1" if v < MOD[f] else "0" for f, v in cases]


def test_word_codec(ask):
    words = sorted(set(_edge_words(P) + _edge_words(R) + [1, FIXED]))
    got = ask(["be %s" % H(v) for v in words])
    for v, line in zip(words, got):
        raw, back = line.split()
        assert bytes.fromhex(raw) == v.to_bytes(32, "big"), H(v)
        assert int(back, 16) == v
    assert got[words.index(1)].split()[0] == "00" * 31 + "01"


def test_g1_on_curve(ask):
    assert ask(["curve %s %s" % (H(1), H(2)), "curve %s %s" % (H(1), H(3))]) == ["1", "0"]


def test_wire_pow_inverts(ask):
    cases = [(f, a) for f in "qr" for a in (1, 2, MOD[f] - 1, FIXED)]
    got = ask(["inv %s %s" % (f, H(a)) for f, a in cases])
    for (f, a), line in zip(cases, got):
        inv = int(line, 16)
        assert inv < MOD[f] and a * inv % MOD[f] == 1, (f, H(a), line)
        assert inv == pow(a, MOD[f] - 2, MOD[f])


def test_sqrt_candidate(ask):
    four, fixed = (int(x, 16) for x in ask(["sqrt %s" % H(4), "sqrt %s" % H(FIXED)]))
    assert four < P and four * four % P == 4
    assert fixed == pow(FIXED, (P + 1) // 4, P)
