"""The bound mappings of comdb2_amd/csrc/hsc_reldiff.h on the host: the
register form rel_diff_w and the locate's short form rel_short against the
general rel_diff, which is the definition ((X - B) >> shift over the
composite key's limbs, saturated, with the remainder flag).

A stand-alone program (its own main) includes the header and is built twice:
plain, and with -fsanitize=address,undefined.  Shapes: W = 1 and 2, every lw
in 0 .. W, tz in {0, 1, 8, 56, 63}.  For every shape and several bases B:

  placed   X = B + m * 2^shift + off for m in {0, 1, kSat - 1, kSat, kSat + 1}
           and off in {-1, 0, +1} (shift = tz + 64 (W - lw)): around the base,
           and around saturation;
           a borrow out of each limb (limb j of X one below B's, the limb above
           one more), each limb differing by +-1 alone, the largest and the
           smallest key
  random   10^6 per shape: a third with every limb random, a third with B's
           gid and word 0 within a few 2^tz of B's, a third with B's gid and
           word 0 equal to B's or +-1 -- so the short form's precondition
           (rel_short_ok) holds for some and fails for others

rel_diff_w must agree with rel_diff on every input (the return value, and v
and rem when it is true: together they fix both the ceil and the floor code).
On shapes with lw == W, rel_short must agree wherever rel_short_ok holds; the
program counts both sides of the precondition and the test asserts that each
occurred on every such shape.
"""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "comdb2_amd", "csrc")

PROG = r"""
#include "hsc_reldiff.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace hsc;
typedef unsigned __int128 u128;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// keys as limbs, most significant first: k[0] = gid, k[1 ..] = words
struct Key { uint64_t k[3]; };

// x + (sign) d over n limbs (wrapping), d given least significant limb first
static Key add(const Key &x, int n, const uint64_t (&d)[4], bool neg)
{
    Key r = x;
    uint64_t carry = 0;
    for (int i = n - 1, j = 0; i >= 0; --i, ++j) {
        const uint64_t dj = neg ? ~d[j] : d[j];
        const u128 s = (u128)x.k[i] + dj + (j == 0 ? (neg ? 1 : 0) : carry);
        r.k[i] = (uint64_t)s;
        carry = (uint64_t)(s >> 64);
    }
    return r;
}

// m << shift + off as limbs (least significant first); off in {-1, 0, 1}
static Key placed(const Key &b, int n, uint64_t m, int shift, int off)
{
    uint64_t d[4] = {0, 0, 0, 0};
    const int q = shift / 64, r = shift % 64;
    d[q] = m << r;
    if (r && q + 1 < 4) d[q + 1] = m >> (64 - r);
    Key x = add(b, n, d, false);
    const uint64_t one[4] = {1, 0, 0, 0};
    if (off > 0) x = add(x, n, one, false);
    if (off < 0) x = add(x, n, one, true);
    return x;
}

static unsigned long long n_cases = 0, n_short = 0, n_general = 0;

template <int W>
static void check(int lw, int tz, const Key &x, const Key &b)
{
    uint64_t v0 = 0, v1 = 0, v2 = 0;
    bool r0 = false, r1 = false, r2 = false;
    const bool ok0 = rel_diff(W, lw, tz, x.k[0], x.k + 1, 1, b.k[0], b.k + 1, 1, kSat, v0, r0);
    uint64_t xw[W];
    for (int i = 0; i < W; ++i) xw[i] = x.k[1 + i];
    const bool ok1 = rel_diff_w<W>(lw, tz, x.k[0], xw, b.k[0], b.k + 1, kSat, v1, r1);
    ++n_cases;
    if (ok0 != ok1 || (ok0 && (v0 != v1 || r0 != r1))) {
        std::printf("rel_diff_w W=%d lw=%d tz=%d x=%llx.%llx.%llx b=%llx.%llx.%llx: %d %llx %d vs %d %llx %d\n",
                    W, lw, tz, (unsigned long long)x.k[0], (unsigned long long)x.k[1],
                    (unsigned long long)x.k[2], (unsigned long long)b.k[0], (unsigned long long)b.k[1],
                    (unsigned long long)b.k[2], ok1, (unsigned long long)v1, r1, ok0,
                    (unsigned long long)v0, r0);
        std::exit(1);
    }
    if (lw != W) return;
    if (!rel_short_ok<W>(tz, x.k[0], xw, b.k[0], b.k + 1)) {
        ++n_general;
        return;
    }
    ++n_short;
    const bool ok2 = rel_short<W>(tz, xw, b.k + 1, kSat, v2, r2);
    if (ok0 != ok2 || (ok0 && (v0 != v2 || r0 != r2))) {
        std::printf("rel_short W=%d tz=%d x=%llx.%llx.%llx b=%llx.%llx.%llx: %d %llx %d vs %d %llx %d\n", W,
                    tz, (unsigned long long)x.k[0], (unsigned long long)x.k[1],
                    (unsigned long long)x.k[2], (unsigned long long)b.k[0], (unsigned long long)b.k[1],
                    (unsigned long long)b.k[2], ok2, (unsigned long long)v2, r2, ok0,
                    (unsigned long long)v0, r0);
        std::exit(1);
    }
}

template <int W>
static void shape(int lw, int tz, long n_random)
{
    const int n = W + 1;
    const int shift = tz + 64 * (W - lw);
    const unsigned long long s0 = n_short, g0 = n_general;
    const Key bases[] = {
        {{5, 0x0880000000000000ull, 0x4000000000000000ull}},
        {{5, 0, 0}},
        {{0, 0, 0}},
        {{7, ~0ull, ~0ull}},
        {{~0ull, ~0ull, ~0ull}},
        {{3, 0x8000000000000000ull, 0}},
        {{9, 0x0123456789ABCDEFull, 0xFEDCBA9876543210ull}},
    };
    const uint64_t ms[] = {0, 1, kSat - 1, kSat, kSat + 1};
    for (const Key &b0 : bases) {
        Key b = b0;
        for (int i = n; i < 3; ++i) b.k[i] = 0;
        for (uint64_t m : ms)
            for (int off = -1; off <= 1; ++off) check<W>(lw, tz, placed(b, n, m, shift, off), b);
        for (int j = 0; j < n; ++j) {
            for (int s = -1; s <= 1; s += 2) {  // limb j alone differs by +-1
                Key x = b;
                x.k[j] += (uint64_t)s;
                check<W>(lw, tz, x, b);
            }
            if (j > 0) {  // a borrow out of limb j: one below there, one more above
                Key x = b;
                x.k[j] -= 1;
                x.k[j - 1] += 1;
                check<W>(lw, tz, x, b);
                x.k[j] = 0;  // and limb j wrapping from the smallest value
                check<W>(lw, tz, x, b);
            }
        }
        Key big, small;
        for (int i = 0; i < 3; ++i) big.k[i] = i < n ? ~0ull : 0, small.k[i] = 0;
        check<W>(lw, tz, big, b);
        check<W>(lw, tz, small, b);
    }
    const uint64_t near = tz >= 62 ? ~0ull : (4ull << tz) - 1;
    for (long i = 0; i < n_random; ++i) {
        Key b = bases[rnd() % 7], x;
        if (rnd() & 1)
            for (int j = 0; j < n; ++j) b.k[j] = rnd();
        for (int j = n; j < 3; ++j) b.k[j] = 0;
        for (int j = 0; j < 3; ++j) x.k[j] = j < n ? rnd() : 0;
        const int kind = (int)(rnd() % 3);
        if (kind >= 1) {
            x.k[0] = b.k[0];
            if (kind == 1)
                x.k[1] = b.k[1] + (rnd() & near) - (rnd() & 1 ? (rnd() & near) : 0);
            else
                x.k[1] = b.k[1] + (rnd() % 3) - 1;
        }
        check<W>(lw, tz, x, b);
    }
    if (lw == W && (n_short == s0 || n_general == g0)) {
        std::printf("W=%d tz=%d: one side of the precondition never occurred\n", W, tz);
        std::exit(1);
    }
}

int main(int argc, char **argv)
{
    const long n_random = argc > 1 ? std::atol(argv[1]) : 1000000;
    const int tzs[] = {0, 1, 8, 56, 63};
    for (int tz : tzs) {
        for (int lw = 0; lw <= 1; ++lw) shape<1>(lw, tz, n_random);
        for (int lw = 0; lw <= 2; ++lw) shape<2>(lw, tz, n_random);
    }
    std::printf("ok %llu %llu %llu\n", n_cases, n_short, n_general);
    return 0;
}
"""


def _compiler():
    for cxx in ("g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = shutil.which(cxx)
        if path:
            return path
    pytest.fail("no host C++ compiler")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined",
                                            "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "sanitized"])
def test_short_and_register_forms_match_rel_diff(tmp_path, flags):
    src = tmp_path / "locate_codes.cpp"
    exe = tmp_path / "locate_codes"
    src.write_text(PROG)
    subprocess.run([_compiler(), "-std=c++17", "-Wall", "-I", CSRC, *flags, str(src), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    word, n_cases, n_short, n_general = r.stdout.split()
    assert word == "ok"
    # 25 shapes of 10^6 random inputs each; 10 of them (lw == W) reach the short form's test
    assert int(n_cases) > 25 * 1000000
    assert int(n_short) > 0 and int(n_general) > 0
    assert int(n_short) + int(n_general) > 10 * 1000000
