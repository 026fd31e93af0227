// wsg_utf8.h — well-formed UTF-8 (RFC 3629) as a position-local rule, shared
// by the host helper wsg_utf8_valid_up_to and the gfx950 kernels k_utf8_scan and k_utf8_wire
// (one source of truth, as wsg_frame.h is for the frame arithmetic).
//
// RFC 6455 5.6 / 8.1 want a text message, taken over all its fragments, to be
// valid UTF-8, and 7.1.6 the same of a close reason; the endpoint fails the
// connection with status 1007 otherwise.  The reference does not validate.
//
// valid_up_to(b) is the length of the longest well-formed prefix of b:
// shortest form only, no surrogates U+D800-DFFF, nothing above U+10FFFF, the
// bytes C0, C1 and F5-FF never valid, a sequence cut off by the end of b
// invalid.  It is the smallest position i that is bad (utf8_bad_at), or the
// length when there is none.  Every byte outside the string counts as 00,
// before it and after it, so the rule needs no bounds: a position's verdict
// depends on at most the 3 bytes before it and the 3 after.
#pragma once

#include <stdint.h>

#include "wsg_frame.h"

namespace wsg {

WSG_HD bool utf8_is_cont(uint32_t b) { return (b & 0xC0u) == 0x80u; }

// Length a non-continuation byte declares: 1 for 00-7F, 2 for C2-DF, 3 for
// E0-EF, 4 for F0-F4; 0 for C0, C1 and F5-FF (and for a continuation byte).
WSG_HD uint32_t utf8_len(uint32_t b)
{
    return b < 0x80u ? 1u : b < 0xC2u ? 0u : b < 0xE0u ? 2u : b < 0xF0u ? 3u : b < 0xF5u ? 4u : 0u;
}

// The byte after a lead of length >= 2: A0-BF after E0 (no overlong), 80-9F
// after ED (no surrogate), 90-BF after F0 (no overlong), 80-8F after F4
// (nothing above U+10FFFF), 80-BF otherwise.
WSG_HD bool utf8_second_ok(uint32_t lead, uint32_t s)
{
    const uint32_t lo = lead == 0xE0u ? 0xA0u : lead == 0xF0u ? 0x90u : 0x80u;
    const uint32_t hi = lead == 0xEDu ? 0x9Fu : lead == 0xF4u ? 0x8Fu : 0xBFu;
    return s >= lo && s <= hi;
}

// Is position i bad?  at(j) is byte j of the string and 00 for every j outside
// it (j from i - 3 to i + 3 is asked for, only as far as the verdict needs).
template <class At>
WSG_HD bool utf8_bad_at(At at, int64_t i)
{
    const uint32_t b = at(i);
    if (utf8_is_cont(b)) {
        // the nearest non-continuation byte before it, at distance k <= 3,
        // must declare more than k bytes
        const uint32_t p1 = at(i - 1);
        if (!utf8_is_cont(p1))
            return utf8_len(p1) <= 1u;
        const uint32_t p2 = at(i - 2);
        if (!utf8_is_cont(p2))
            return utf8_len(p2) <= 2u;
        const uint32_t p3 = at(i - 3);
        if (!utf8_is_cont(p3))
            return utf8_len(p3) <= 3u;
        return true;
    }
    const uint32_t len = utf8_len(b);
    if (len <= 1u)
        return len == 0u;
    // (a sequence cut off by the string's end meets a 00 here)
    if (!utf8_second_ok(b, at(i + 1)))
        return true;
    if (len >= 3u && !utf8_is_cont(at(i + 2)))
        return true;
    return len == 4u && !utf8_is_cont(at(i + 3));
}

// ---- the same rule word-wise: 4 positions per 32-bit word ---------------------
// A little-endian word holds 4 consecutive bytes; a class of bytes is a word
// with bit 7 of a byte set where the byte is in the class (additions below stay
// inside their byte: no carry crosses).  utf8_words_bad asks the rule about 16
// positions at once; the kernel runs it as a filter (valid text, the common
// case, ends here) and utf8_bad_at over the positions of a word that has a
// flag.  tests/test_utf8_host.py holds the two forms against each other.
constexpr uint32_t UTF8_H = 0x80808080u;

// lane j of the result = lane j - k of the 8 bytes lo:w (k = 1..3 positions up)
WSG_HD uint32_t utf8_up(uint32_t lo, uint32_t w, uint32_t k) { return (w << (8u * k)) | (lo >> (32u - 8u * k)); }
// lane j of the result = lane j + k of the 8 bytes w:hi
WSG_HD uint32_t utf8_down(uint32_t w, uint32_t hi, uint32_t k) { return (w >> (8u * k)) | (hi << (32u - 8u * k)); }

struct Utf8Classes {
    uint32_t cont;         // 80-BF
    uint32_t g2, g3, g4;   // valid leads that declare >= 2, >= 3, 4 bytes
    uint32_t nv;           // C0, C1, F5-FF
    uint32_t l3, l4;       // E0-FF, F0-FF (with the never-valid ones)
};

WSG_HD Utf8Classes utf8_classes(uint32_t x)
{
    const uint32_t b6 = x << 1, b5 = x << 2, b4 = x << 3;   // bit 6 / 5 / 4 of a byte at its bit 7
    const uint32_t hi = x & UTF8_H;
    Utf8Classes c;
    c.cont = hi & ~b6;
    const uint32_t l2 = hi & b6;
    c.l3 = l2 & b5;
    c.l4 = c.l3 & b4;
    const uint32_t le1 = ~((x & 0x0E0E0E0Eu) + 0x7F7F7F7Fu);   // low nibble <= 1
    const uint32_t ge5 = (x & 0x0F0F0F0Fu) + 0x7B7B7B7Bu;      // low nibble >= 5
    c.nv = (l2 & ~b5 & ~b4 & le1) | (c.l4 & ge5);
    c.g2 = l2 & ~c.nv;
    c.g3 = c.l3 & ~c.nv;
    c.g4 = c.l4 & ~c.nv;
    return c;
}

// d[0..6): the positions -4..19 (bytes outside the string 00).  bad[w], w =
// 0..3: bit 7 of byte j set exactly when position 4 w + j is bad.
WSG_HD void utf8_words_bad(const uint32_t d[6], uint32_t bad[4])
{
    Utf8Classes before = utf8_classes(d[0]);
    Utf8Classes here = utf8_classes(d[1]);
    for (int w = 1; w <= 4; ++w) {
        const uint32_t x = d[w], nx = d[w + 1];
        const Utf8Classes after = utf8_classes(nx);
        // a lead: its second byte's range, then continuation bytes
        const uint32_t n = x & 0x0F0F0F0Fu;
        const uint32_t is0 = ~(n + 0x7F7F7F7Fu), is4 = ~((n ^ 0x04040404u) + 0x7F7F7F7Fu),
                       isD = ~((n ^ 0x0D0D0D0Du) + 0x7F7F7F7Fu);
        const uint32_t e = here.l3 & ~here.l4;                   // E0-EF
        const uint32_t next = utf8_down(x, nx, 1);
        const uint32_t nb5 = next << 2, nb54 = nb5 | (next << 3);
        const uint32_t special = (e & is0 & ~nb5) | (e & isD & nb5) | (here.l4 & is0 & ~nb54) | (here.l4 & is4 & nb54);
        const uint32_t c1 = utf8_down(here.cont, after.cont, 1), c2 = utf8_down(here.cont, after.cont, 2),
                       c3 = utf8_down(here.cont, after.cont, 3);
        const uint32_t lead_bad = here.nv | (here.g2 & (~c1 | special)) | (here.g3 & ~c2) | (here.g4 & ~c3);
        // a continuation byte: the nearest non-continuation byte before it declares enough
        const uint32_t p1 = utf8_up(before.cont, here.cont, 1), p2 = utf8_up(before.cont, here.cont, 2);
        const uint32_t ok = utf8_up(before.g2, here.g2, 1) | (utf8_up(before.g3, here.g3, 2) & p1) |
                            (utf8_up(before.g4, here.g4, 3) & p1 & p2);
        bad[w - 1] = (lead_bad | (here.cont & ~ok)) & UTF8_H;
        before = here;
        here = after;
    }
}

// valid_up_to of buf[0, len); reads no byte outside it.
inline uint64_t utf8_valid_up_to(const uint8_t* buf, uint64_t len)
{
    auto at = [&](int64_t j) -> uint32_t { return j < 0 || uint64_t(j) >= len ? 0u : buf[j]; };
    for (uint64_t i = 0; i < len; ++i)
        if (buf[i] >= 0x80u && utf8_bad_at(at, int64_t(i)))   // (an ASCII position is never bad)
            return i;
    return len;
}

} // namespace wsg
