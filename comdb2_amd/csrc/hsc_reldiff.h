// hsc_reldiff.h -- a probe bound as a narrow-window code: (X - B) >> shift
// for composite keys, in the general form (rel_diff), the register form for
// one or two key words (rel_diff_w) and the short form of the locate's fast
// instances (rel_short).  Plain C++: hipcc compiles it for host and device,
// a host compiler for the stand-alone model check (tests/test_locate_codes.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define HSC_HD __host__ __device__
#else
#define HSC_HD
#endif
#define HSC_HD_INLINE HSC_HD inline __attribute__((always_inline))

namespace hsc {

constexpr uint64_t kSat = 1ull << 62;    // saturated code: above every key

// (X - B) >> shift for composite keys X = (xg, xw[j * xs]) and B = (bg,
// bw[j * bs]), limbs most significant first: limb 0 = gid, limb j + 1 = word
// j.  shift = tz bits of limb lw plus every limb after lw (the window's rows
// agree on all of those bits).  Returns false if X < B.  Otherwise v =
// min((X - B) >> shift, sat) and rem = whether the shifted-out bits of X - B
// are nonzero.
HSC_HD inline bool rel_diff(int W, int lw, int tz, uint64_t xg, const uint64_t *xw, size_t xs,
                            uint64_t bg, const uint64_t *bw, size_t bs, uint64_t sat, uint64_t &v,
                            bool &rem)
{
    uint64_t borrow = 0, d_last = 0, d_prev = 0, high = 0, below = 0;
    for (int i = W; i >= 0; --i) {
        const uint64_t x = i ? xw[(size_t)(i - 1) * xs] : xg;
        const uint64_t b = i ? bw[(size_t)(i - 1) * bs] : bg;
        const uint64_t d = x - b - borrow;
        borrow = (x < b) | ((x == b) & (borrow != 0));
        if (i > lw)
            below |= d;
        else if (i == lw)
            d_last = d;
        else if (i == lw - 1)
            d_prev = d;
        else
            high |= d;
    }
    if (borrow) return false;
    rem = (below != 0) | (tz ? (d_last & ((1ull << tz) - 1)) != 0 : false);
    const uint64_t top = tz ? d_prev >> tz : d_prev;
    const uint64_t low = tz ? (d_last >> tz) | (d_prev << (64 - tz)) : d_last;
    v = (high | top) ? sat : (low < sat ? low : sat);
    return true;
}

// rel_diff for W = 1 or 2 key words held in registers: the words subtract as
// one 128-bit borrow chain, the gid limb after it; the limb roles come from
// uniform branches on lw and the shift by tz (< 64) is a funnel shift whose
// tz = 0 case needs no branch ((d << 1) << 63 = 0).
template <int W>
HSC_HD_INLINE bool rel_diff_w(int lw, int tz, uint64_t xg, const uint64_t (&xw)[W], uint64_t bg,
                              const uint64_t *bw, uint64_t sat, uint64_t &v, bool &rem)
{
    static_assert(W == 1 || W == 2, "register form for 1 or 2 words");
    typedef unsigned __int128 u128;
    uint64_t d[W + 1];
    bool borrow;
    if constexpr (W == 2) {
        const u128 x = (u128)xw[0] << 64 | xw[1], b = (u128)bw[0] << 64 | bw[1];
        const u128 dd = x - b;
        d[1] = (uint64_t)(dd >> 64);
        d[2] = (uint64_t)dd;
        borrow = x < b;
    } else {
        d[1] = xw[0] - bw[0];
        borrow = xw[0] < bw[0];
    }
    d[0] = xg - bg - (borrow ? 1 : 0);
    if (xg < bg || (xg == bg && borrow)) return false;
    uint64_t below, d_last, d_prev, high;
    if (W == 2 && lw == 2) {
        below = 0, d_last = d[W], d_prev = d[W - 1], high = d[0];
    } else if (lw == 1) {
        below = d[W] & (W == 2 ? ~0ull : 0), d_last = d[1], d_prev = d[0], high = 0;
    } else {
        below = d[1] | d[W], d_last = d[0], d_prev = 0, high = 0;
    }
    const uint64_t top = d_prev >> tz;
    const uint64_t low = (d_last >> tz) | ((d_prev << 1) << (63 - tz));
    rem = (below | (d_last & ((1ull << tz) - 1))) != 0;
    v = (high | top) ? sat : (low < sat ? low : sat);
    return true;
}

// The short form, for windows whose last key word is the last limb that
// varies (lw == W, W = 1 or 2: shift = tz, no limb below lw).
//
// Precondition (rel_short_ok): xg == bg and, for W = 2, xw[0] >= bw[0] with
// e = xw[0] - bw[0] below 2^tz (tz = 0 leaves xw[0] == bw[0]; the test of
// xw[0] >= bw[0] is needed, the wrapping difference alone is also small when
// xw[0] is just below bw[0] modulo 2^64).
//
// Then rel_short returns what rel_diff(W, W, tz, ...) and rel_diff_w<W>(W,
// tz, ...) return, v and rem included:
//  - The gid limbs are equal, so X < B <=> words(X) < words(B).  For W = 1
//    that is xw[0] < bw[0]; for W = 2, with xw[0] >= bw[0], it is e == 0 and
//    xw[1] < bw[1].  rel_short returns false in exactly these cases, and
//    rel_diff's final borrow is set in exactly these cases.
//  - Otherwise X >= B and the chain ends without a borrow, so the gid limb's
//    difference is xg - bg - 0 = 0.  W = 1: d_last = xw[0] - bw[0], d_prev =
//    the gid limb = 0, high = 0, so top = 0 and low = d_last >> tz.  W = 2:
//    d_last = xw[1] - bw[1] (wrapping), d_prev = e - c with c = (xw[1] <
//    bw[1]), high = the gid limb = 0; 0 <= d_prev <= e < 2^tz, so top =
//    d_prev >> tz = 0 and low = d_last >> tz | d_prev << (64 - tz), which is
//    (d_prev << 1) << (63 - tz) for every tz < 64 (0 when tz = 0, where
//    d_prev = 0 anyway).  With high | top = 0, v = min(low, sat): the
//    saturation rel_diff applies to low is kept, the one it applies through
//    top cannot occur.
//  - below is empty (no limb after lw), so rem = (d_last & (2^tz - 1)) != 0.
// What is left out is the gid limb's subtraction and compare, the borrow
// into it and the test of high | top.
template <int W>
HSC_HD_INLINE bool rel_short_ok(int tz, uint64_t xg, const uint64_t (&xw)[W], uint64_t bg,
                                const uint64_t *bw)
{
    static_assert(W == 1 || W == 2, "short form for 1 or 2 words");
    if constexpr (W == 2)
        return xg == bg && xw[0] >= bw[0] && xw[0] - bw[0] < (1ull << tz);
    else
        return xg == bg;
}

template <int W>
HSC_HD_INLINE bool rel_short(int tz, const uint64_t (&xw)[W], const uint64_t *bw, uint64_t sat,
                             uint64_t &v, bool &rem)
{
    static_assert(W == 1 || W == 2, "short form for 1 or 2 words");
    uint64_t d_last, d_prev;
    if constexpr (W == 2) {
        const uint64_t e = xw[0] - bw[0];
        const bool c = xw[1] < bw[1];
        if (e == 0 && c) return false;
        d_last = xw[1] - bw[1];
        d_prev = e - (c ? 1 : 0);
    } else {
        if (xw[0] < bw[0]) return false;
        d_last = xw[0] - bw[0];
        d_prev = 0;
    }
    const uint64_t low = (d_last >> tz) | ((d_prev << 1) << (63 - tz));
    rem = (d_last & ((1ull << tz) - 1)) != 0;
    v = low < sat ? low : sat;
    return true;
}

}  // namespace hsc
