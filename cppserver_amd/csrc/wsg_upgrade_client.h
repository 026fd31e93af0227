// wsg_upgrade_client.h — the client's half of the upgrade handshake as
// WSClient::onReceived (ws_api.cpp), HTTPResponse::Parse (http.cpp) and
// WebSocket::PerformClientUpgrade (ws.cpp) judge a connection's first bytes,
// shared by the host helper wsg_upgrade_client_judge and the gfx950 kernels of
// wsg_upgrade_client_streams, as wsg_upgrade.h is for the server's half.  It
// restates the classes; it does not repair them.
//
// The header block, the line split, the trimming and the Content-Length fold
// are the server's (up_line of wsg_upgrade.h, position-local as described
// there).  New here: the status line (uc_status), the Base64 decoder that skips
// foreign bytes with strncmp's compare behind it (uc_accept_ok), the expected
// digest of a nonce (uc_expect: two SHA-1 blocks over a fixed 60 bytes), the
// client's fold and its outcome, and the request's key (uc_key_char).
// An accept line's pass or fail depends on the line and the stream's digest
// alone, so the lane that owns the line's first byte judges it like any other.
#pragma once

#include "wsg_upgrade.h"

namespace wsg {

enum : uint32_t { UC_CONNECTION = 1, UC_UPGRADE = 2, UC_ACCEPT = 4, UC_ALL = 7 };

// ---- the status line ----------------------------------------------------------
struct UcStatus {
    bool ok;           // a space behind at least one byte, then exactly three digits up to the next space or the end
    uint32_t status;   // the three digits
};

// The line [0, eol).  (HTTPResponse::Parse sums the digits before it counts
// them; only a run of three is well-formed, so nothing is summed for another.)
template <class Src>
WSG_HD UcStatus uc_status(Src src, uint64_t eol)
{
    UcStatus st{};
    uint64_t s1 = 0;
    while (s1 < eol && src(s1) != ' ')
        ++s1;
    if (s1 == 0 || s1 >= eol)
        return st;
    uint64_t s2 = s1 + 1;
    while (s2 < eol && src(s2) != ' ')
        ++s2;
    if (s2 - s1 - 1 != 3)
        return st;
    uint32_t v = 0;
    for (uint64_t i = s1 + 1; i < s2; ++i) {
        const uint32_t c = src(i);
        if (c < '0' || c > '9')
            return st;
        v = v * 10 + (c - '0');
    }
    st.ok = true;
    st.status = v;
    return st;
}

// ---- the key a client sends and the digest it expects ---------------------------
// Character t < 24 of Base64(nonce); nb(i): byte i < 16 of the nonce.
template <class Nonce>
WSG_HD uint32_t uc_key_char(Nonce nb, uint32_t t)
{
    if (t >= 22)
        return '=';
    const uint32_t i = 3 * (t >> 2), k = t & 3;
    const uint32_t v = (nb(i) << 16) | ((i + 1 < 16 ? nb(i + 1) : 0u) << 8) | (i + 2 < 16 ? nb(i + 2) : 0u);
    return up_b64((v >> (18 - 6 * k)) & 63u);
}

// SHA-1(Base64(nonce) || GUID): 60 bytes, so the padding and the length take a
// block of their own.  n: the nonce as four words in memory order (little
// endian); h: the digest, byte i at bits 24 - 8 * (i & 3) of h[i >> 2].  Every
// index is a constant once the loops are unrolled.
WSG_HD void uc_expect(const uint32_t n[4], uint32_t h[5])
{
    const char* guid = "258EAFA5-E914-47DA-95CA-C5AB0DC85B11";   // RFC 6455 1.3
    uint32_t w[16];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int g = 0; g < 6; ++g) {
        uint32_t v = 0;
        for (int k = 0; k < 3; ++k) {
            const int i = 3 * g + k;
            v = (v << 8) | (i < 16 ? (n[i >> 2] >> (8 * (i & 3))) & 0xFFu : 0u);
        }
        w[g] = (up_b64(v >> 18) << 24) | (up_b64((v >> 12) & 63u) << 16) |
               ((g == 5 ? uint32_t('=') : up_b64((v >> 6) & 63u)) << 8) | (g == 5 ? uint32_t('=') : up_b64(v & 63u));
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < 9; ++k)
        w[6 + k] = (uint32_t(uint8_t(guid[4 * k])) << 24) | (uint32_t(uint8_t(guid[4 * k + 1])) << 16) |
                   (uint32_t(uint8_t(guid[4 * k + 2])) << 8) | uint32_t(uint8_t(guid[4 * k + 3]));
    w[15] = 0x80000000u;
    h[0] = 0x67452301u;
    h[1] = 0xEFCDAB89u;
    h[2] = 0x98BADCFEu;
    h[3] = 0x10325476u;
    h[4] = 0xC3D2E1F0u;
    up_sha1_block(h, w);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < 15; ++k)
        w[k] = 0;
    w[15] = 60 * 8;
    up_sha1_block(h, w);
}

// ---- the accept value -----------------------------------------------------------
WSG_HD int32_t uc_b64_val(uint32_t c)   // WS::Base64Decode: -1 for a byte outside the alphabet
{
    return c >= 'A' && c <= 'Z'   ? int32_t(c - 'A')
           : c >= 'a' && c <= 'z' ? int32_t(c - 'a') + 26
           : c >= '0' && c <= '9' ? int32_t(c - '0') + 52
           : c == '+'             ? 62
           : c == '/'             ? 63
                                  : -1;
}

// src[s, s + n) decoded as WS::Base64Decode does (bytes outside the alphabet
// are skipped, a byte comes out whenever eight bits are held), the decoded
// bytes `got` compared with the digest as strncmp(got, expect, min(|got|, 20))
// does: in order, unequal bytes fail, equal NUL bytes pass at once, and so do
// the end of either.  expect(i): byte i < 20 of the digest.
template <class Src, class Expect>
WSG_HD bool uc_accept_ok(Src src, uint64_t s, uint64_t n, Expect expect)
{
    uint32_t acc = 0, bits = 0, i = 0;
    for (uint64_t k = 0; k < n && i < 20; ++k) {
        const int32_t v = uc_b64_val(src(s + k));
        if (v < 0)
            continue;
        acc = ((acc << 6) | uint32_t(v)) & 0xFFFFu;   // (at most 7 bits are held over)
        bits += 6;
        if (bits >= 8) {
            bits -= 8;
            const uint32_t got = (acc >> bits) & 0xFFu;
            if (got != expect(i))
                return false;
            if (got == 0)
                return true;
            ++i;
        }
    }
    return true;
}

// ---- one header line --------------------------------------------------------------
struct UcLine {
    bool open, malformed, has_clen;   // as UpLine's
    uint32_t name;                    // UC_* of the three, or 0
    uint32_t fail;                    // the WSG_UC_* code the line fails with, or 0
    uint64_t clen;
    uint64_t val_off, val_len;        // the trimmed value
};

// The line's name is Sec-WebSocket-Accept: behind the blanks at `start` the 20
// letters without case, then blanks up to the line's first ':' (a well-formed
// line: up_line found that ':' behind `start`).
template <class Src>
WSG_HD bool uc_names_accept(Src src, uint64_t start)
{
    // "sec-websocket-accept", eight letters to a word: the loop stays a loop on the device (unrolled, its
    // twenty early exits nest twenty saved exec masks and the kernel runs out of scalar registers)
    const uint64_t lit[3] = {0x736265772D636573ull, 0x63612D74656B636Full, 0x74706563ull};
    uint64_t i = start;
    while (up_trimmed(src(i)))
        ++i;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (uint32_t k = 0; k < 20; ++k, ++i) {
        const uint64_t word = k < 8 ? lit[0] : k < 16 ? lit[1] : lit[2];
        if (up_lower(src(i)) != (uint32_t(word >> (8 * (k & 7))) & 0xFFu))
            return false;
    }
    while (up_trimmed(src(i)))
        ++i;
    return src(i) == ':';
}

// The line that starts at `start`: up_line's split, trimming and
// Content-Length, the three names judged by the client's rule.
template <class Src, class Expect>
WSG_HD UcLine uc_line(Src src, uint64_t start, uint64_t limit, Expect expect)
{
    const UpLine b = up_line(src, start, limit);
    UcLine ln{};
    ln.open = b.open;
    ln.malformed = b.malformed;
    ln.has_clen = b.has_clen;
    ln.clen = b.clen;
    ln.val_off = b.val_off;
    ln.val_len = b.val_len;
    if (b.open || b.malformed || b.has_clen || b.val_off <= start)   // (val_off 0: an empty line)
        return ln;
    if (b.name == UP_CONNECTION) {   // no keep-alive form on this side
        ln.name = UC_CONNECTION;
        ln.fail = up_ieq(src, b.val_off, b.val_len, "upgrade", 7) ? 0 : WSG_UC_BAD_CONNECTION;
    } else if (b.name == UP_UPGRADE) {
        ln.name = UC_UPGRADE;
        ln.fail = b.fail ? WSG_UC_BAD_UPGRADE : 0;
    } else if (b.name == 0 && uc_names_accept(src, start)) {
        ln.name = UC_ACCEPT;
        ln.fail = uc_accept_ok(src, b.val_off, b.val_len, expect) ? 0 : WSG_UC_BAD_ACCEPT;
    }
    return ln;
}

// ---- the reduction over lines, in position order -----------------------------------
struct UcFold {
    bool malformed, has_clen;
    bool judged;      // an accept line in front of the walk's end, the failing one included
    uint32_t fail;    // the first failing line's code
    uint32_t seen;    // the names in front of it
    uint64_t clen;    // the last Content-Length
    uint64_t acc_off, acc_len;   // the last accept value judged
};

// acc, then the line behind it.
WSG_HD void uc_fold(UcFold& acc, const UcLine& ln)
{
    acc.malformed = acc.malformed || ln.malformed;
    if (ln.has_clen) {
        acc.has_clen = true;
        acc.clen = ln.clen;
    }
    if (acc.fail || !ln.name)
        return;
    if (ln.name == UC_ACCEPT) {
        acc.judged = true;
        acc.acc_off = ln.val_off;
        acc.acc_len = ln.val_len;
    }
    if (ln.fail) {
        acc.fail = ln.fail;
        return;
    }
    acc.seen |= ln.name;
}

// ---- the outcome ---------------------------------------------------------------------
struct UcOutcome {
    uint64_t accept_off, body_off;   // absolute
    uint32_t accept_len, body_len, status, code;
    uint64_t consumed, need;
};

// found: the response has a header end, hend bytes from its start; `off` the
// response's wire offset, len its bytes.
WSG_HD UcOutcome uc_outcome(bool found, uint64_t hend, const UcStatus& st, const UcFold& f, uint64_t off, uint64_t len,
                            uint64_t max_response)
{
    UcOutcome o{};
    const uint32_t unfinished = max_response && len >= max_response ? WSG_UC_TOO_LONG : WSG_UC_INCOMPLETE;
    o.code = unfinished;
    if (!found)
        return o;
    if (!st.ok || f.malformed) {
        o.code = WSG_UC_BAD_HTTP;
        o.consumed = hend;
        return o;
    }
    const uint64_t clen = f.has_clen ? f.clen : 0;
    if (len - hend < clen) {
        o.need = hend + clen < hend ? UINT64_MAX : hend + clen;
        return o;
    }
    o.consumed = hend + clen;
    o.body_off = off + hend;
    o.body_len = up_sat32(clen);
    o.status = st.status;
    if (st.status != 101) {   // the headers are not walked
        o.code = WSG_UC_NOT_101;
        return o;
    }
    if (f.judged) {
        o.accept_off = off + f.acc_off;
        o.accept_len = up_sat32(f.acc_len);
    }
    // (as PerformClientUpgrade ends: the three flags first, the failing header only between them)
    o.code = f.seen == UC_ALL ? WSG_UC_ACCEPTED : f.fail ? f.fail : WSG_UC_MISSING;
    return o;
}

// The record's four 8-byte words (the kernel stores it that way).
WSG_HD void uc_record(const UcOutcome& o, uint64_t w[4])
{
    w[0] = o.accept_off;
    w[1] = o.body_off;
    w[2] = uint64_t(o.accept_len) | (uint64_t(o.body_len) << 32);
    w[3] = (uint64_t(o.status) << 32) | (uint64_t(o.code) << 48);
}

} // namespace wsg
