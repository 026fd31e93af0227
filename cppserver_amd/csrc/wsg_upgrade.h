// wsg_upgrade.h — the WebSocket upgrade handshake as WSSession::onReceived,
// HTTPRequest::Parse (http.cpp) and WebSocket::PerformServerUpgrade (ws.cpp)
// judge a connection's first bytes, shared by the host helper
// wsg_upgrade_judge and the gfx950 kernels of wsg_upgrade_streams (one source
// of truth, as wsg_utf8.h and wsg_proto.h are for their rules).  SHA-1 and
// Base64 are written here: no OpenSSL on either side.
//
// Position-local form.  With p the first "\r\n\r\n" and eol the first "\r\n",
// a header line starts at every i < p whose two bytes in front are "\r\n"
// (the first such i is eol + 2) and ends at the next "\r\n", so a line is
// judged from its first byte alone (up_line) and no line is empty.  The
// request's outcome is a reduction over the lines in position order
// (up_fold within one owner, the kernel's ballots across owners): any
// malformed line, the last Content-Length, the first failing line, the names
// seen and the last key in front of it.  up_outcome turns the reduced facts
// into the record, consumed and need.
#pragma once

#include <stdint.h>

#include "wsg_frame.h"

namespace wsg {

enum : uint32_t { UP_CONNECTION = 1, UP_UPGRADE = 2, UP_KEY = 4, UP_VERSION = 8, UP_ALL = 15 };

// ---- the responses, exactly as HTTPResponse serialises them -----------------
#define WSG_UP_400(n, body) \
    "HTTP/1.1 400 Bad Request\r\nContent-Type: text/plain; charset=UTF-8\r\nContent-Length: " n "\r\n\r\n" body
#define WSG_UP_101_HEAD \
    "HTTP/1.1 101 Switching Protocols\r\nConnection: Upgrade\r\nUpgrade: websocket\r\nSec-WebSocket-Accept: "
// (28 bytes of room for the accept value)
#define WSG_UP_T_ACCEPTED WSG_UP_101_HEAD "============================" "\r\nContent-Length: 0\r\n\r\n"
#define WSG_UP_T_BAD_HTTP WSG_UP_400("20", "Invalid HTTP request")
#define WSG_UP_T_BAD_CONNECTION                                                                                  \
    WSG_UP_400("106", "Invalid WebSocket handshaked request: 'Connection' header value must be 'Upgrade' or "    \
                      "'keep-alive, Upgrade'")
#define WSG_UP_T_BAD_UPGRADE \
    WSG_UP_400("80", "Invalid WebSocket handshaked request: 'Upgrade' header value must be 'websocket'")
#define WSG_UP_T_EMPTY_KEY \
    WSG_UP_400("88", "Invalid WebSocket handshaked request: 'Sec-WebSocket-Key' header value must be non empty")
#define WSG_UP_T_BAD_VERSION \
    WSG_UP_400("87", "Invalid WebSocket handshaked request: 'Sec-WebSocket-Version' header value must be '13'")
#define WSG_UP_T_MISSING WSG_UP_400("26", "Invalid WebSocket response")

constexpr uint32_t UP_ACCEPT_AT = sizeof(WSG_UP_101_HEAD) - 1;   // the accept value's place in the 101
constexpr uint32_t UP_ACCEPT_LEN = 28;
constexpr uint32_t UP_TEMPLATES = WSG_UP_MISSING + 1;   // indexed by code; INCOMPLETE has none
constexpr uint32_t UP_HEAD_400 = sizeof(WSG_UP_400("20", "")) - 1;

// Response bytes of an outcome (0: none).
WSG_HD uint32_t up_resp_len(uint32_t code)
{
    switch (code) {
    case WSG_UP_ACCEPTED: return sizeof(WSG_UP_T_ACCEPTED) - 1;
    case WSG_UP_BAD_HTTP: return sizeof(WSG_UP_T_BAD_HTTP) - 1;
    case WSG_UP_BAD_CONNECTION: return sizeof(WSG_UP_T_BAD_CONNECTION) - 1;
    case WSG_UP_BAD_UPGRADE: return sizeof(WSG_UP_T_BAD_UPGRADE) - 1;
    case WSG_UP_EMPTY_KEY: return sizeof(WSG_UP_T_EMPTY_KEY) - 1;
    case WSG_UP_BAD_VERSION: return sizeof(WSG_UP_T_BAD_VERSION) - 1;
    case WSG_UP_MISSING: return sizeof(WSG_UP_T_MISSING) - 1;
    default: return 0;
    }
}
static_assert(sizeof(WSG_UP_T_ACCEPTED) - 1 == 148 && sizeof(WSG_UP_T_BAD_CONNECTION) - 1 == WSG_UPGRADE_RESP_MAX &&
                  sizeof(WSG_UP_T_BAD_HTTP) - 1 == UP_HEAD_400 + 20 &&
                  sizeof(WSG_UP_T_BAD_CONNECTION) - 1 == UP_HEAD_400 + 1 + 106 &&
                  sizeof(WSG_UP_T_BAD_UPGRADE) - 1 == UP_HEAD_400 + 80 &&
                  sizeof(WSG_UP_T_EMPTY_KEY) - 1 == UP_HEAD_400 + 88 &&
                  sizeof(WSG_UP_T_BAD_VERSION) - 1 == UP_HEAD_400 + 87 &&
                  sizeof(WSG_UP_T_MISSING) - 1 == UP_HEAD_400 + 26 && WSG_UPGRADE_RESP_MAX >= 177,
              "every Content-Length is its body's, and WSG_UPGRADE_RESP_MAX the longest response's");

// ---- bytes ------------------------------------------------------------------
WSG_HD uint32_t up_lower(uint32_t c) { return c >= 'A' && c <= 'Z' ? c + 32u : c; }
WSG_HD bool up_trimmed(uint32_t c) { return c == ' ' || c == '\t'; }                     // http.cpp: trim
WSG_HD bool up_blank(uint32_t c) { return c == ' ' || (c >= '\t' && c <= '\r'); }        // isspace, C locale

// src[s, s + n) equals `lit` (lower case, n bytes) without case.
template <class Src>
WSG_HD bool up_ieq(Src src, uint64_t s, uint64_t n, const char* lit, uint32_t lit_len)
{
    if (n != lit_len)
        return false;
    for (uint32_t i = 0; i < lit_len; ++i)
        if (up_lower(src(s + i)) != uint32_t(uint8_t(lit[i])))
            return false;
    return true;
}

// ---- one header line --------------------------------------------------------
struct UpLine {
    bool open;        // no "\r\n" behind it below `limit`: the request has no header end either
    bool malformed;
    bool has_clen;
    uint32_t name;    // UP_* of the four, or 0
    uint32_t fail;    // the WSG_UP_* code the line fails with, or 0
    uint64_t clen;
    uint64_t val_off, val_len;   // the trimmed value
};

// The line that starts at `start` (src indexes the request from 0, `limit`
// bytes of it exist).
template <class Src>
WSG_HD UpLine up_line(Src src, uint64_t start, uint64_t limit)
{
    UpLine ln{};
    uint64_t e = start, colon = UINT64_MAX;
    bool ended = false;
    for (; e + 1 < limit; ++e) {
        const uint32_t c = src(e);
        if (c == '\r' && src(e + 1) == '\n') {
            ended = true;
            break;
        }
        if (c == ':' && colon == UINT64_MAX)
            colon = e;
    }
    if (!ended) {
        ln.open = true;
        return ln;
    }
    if (e == start)   // (an empty line is skipped; none exists in front of the header end)
        return ln;
    if (colon == UINT64_MAX || colon == start) {
        ln.malformed = true;
        return ln;
    }
    uint64_t ks = start, ke = colon, vs = colon + 1, ve = e;
    while (ks < ke && up_trimmed(src(ks)))
        ++ks;
    while (ke > ks && up_trimmed(src(ke - 1)))
        --ke;
    while (vs < ve && up_trimmed(src(vs)))
        ++vs;
    while (ve > vs && up_trimmed(src(ve - 1)))
        --ve;
    const uint64_t kn = ke - ks, vn = ve - vs;
    ln.val_off = vs;
    ln.val_len = vn;
    if (up_ieq(src, ks, kn, "content-length", 14)) {
        ln.has_clen = true;
        for (uint64_t i = vs; i < ve; ++i) {
            const uint32_t c = src(i);
            if (c < '0' || c > '9') {
                ln.malformed = true;
                return ln;
            }
            ln.clen = ln.clen * 10 + (c - '0');   // mod 2^64
        }
    } else if (up_ieq(src, ks, kn, "connection", 10)) {
        ln.name = UP_CONNECTION;
        bool ok = up_ieq(src, vs, vn, "upgrade", 7);
        if (!ok) {   // "keep-alive,Upgrade" once the blanks are gone
            const char* lit = "keep-alive,upgrade";
            uint32_t j = 0;
            ok = true;
            for (uint64_t i = vs; i < ve && ok; ++i) {
                const uint32_t c = src(i);
                if (up_blank(c))
                    continue;
                ok = j < 18 && up_lower(c) == uint32_t(uint8_t(lit[j]));
                ++j;
            }
            ok = ok && j == 18;
        }
        ln.fail = ok ? 0 : WSG_UP_BAD_CONNECTION;
    } else if (up_ieq(src, ks, kn, "upgrade", 7)) {
        ln.name = UP_UPGRADE;
        ln.fail = up_ieq(src, vs, vn, "websocket", 9) ? 0 : WSG_UP_BAD_UPGRADE;
    } else if (up_ieq(src, ks, kn, "sec-websocket-key", 17)) {
        ln.name = UP_KEY;
        ln.fail = vn ? 0 : WSG_UP_EMPTY_KEY;
    } else if (up_ieq(src, ks, kn, "sec-websocket-version", 21)) {
        ln.name = UP_VERSION;
        ln.fail = up_ieq(src, vs, vn, "13", 2) ? 0 : WSG_UP_BAD_VERSION;
    }
    return ln;
}

// ---- the reduction over lines, in position order ------------------------------
struct UpFold {
    bool malformed;
    bool has_clen;
    uint32_t fail;    // the first failing line's code
    uint32_t seen;    // the names in front of it
    uint64_t clen;    // the last Content-Length
    uint64_t key_off, key_len;   // the last key line's value in front of it (seen & UP_KEY)
};

// acc, then the line behind it.
WSG_HD void up_fold(UpFold& acc, const UpLine& ln)
{
    acc.malformed = acc.malformed || ln.malformed;
    if (ln.has_clen) {
        acc.has_clen = true;
        acc.clen = ln.clen;
    }
    if (acc.fail || !ln.name)
        return;
    if (ln.fail) {
        acc.fail = ln.fail;
        return;
    }
    acc.seen |= ln.name;
    if (ln.name == UP_KEY) {
        acc.key_off = ln.val_off;
        acc.key_len = ln.val_len;
    }
}

// ---- the request line ---------------------------------------------------------
struct UpStart {
    bool ok;       // two spaces at least
    bool get;      // the method is exactly "GET"
    uint64_t url_off, url_len;
};

template <class Src>
WSG_HD UpStart up_start(Src src, uint64_t eol)
{
    uint64_t s1 = UINT64_MAX, s2 = 0;
    for (uint64_t i = 0; i < eol; ++i)
        if (src(i) == ' ') {
            if (s1 == UINT64_MAX)
                s1 = i;
            s2 = i;
        }
    UpStart st{};
    st.ok = s1 != UINT64_MAX && s1 != s2;
    if (st.ok) {
        st.get = s1 == 3 && src(0) == 'G' && src(1) == 'E' && src(2) == 'T';
        st.url_off = s1 + 1;
        st.url_len = s2 - s1 - 1;
    }
    return st;
}

// ---- the outcome ----------------------------------------------------------------
WSG_HD uint32_t up_sat32(uint64_t v) { return v > UINT32_MAX ? UINT32_MAX : uint32_t(v); }

struct UpOutcome {
    uint64_t key_off, url_off;   // absolute
    uint32_t key_len, url_len, resp_len, status, code;
    uint64_t consumed, need;
};

// found: the request has a header end, hend bytes from its start; `off` the
// request's wire offset, len its bytes.
WSG_HD UpOutcome up_outcome(bool found, uint64_t hend, const UpStart& st, const UpFold& f, uint64_t off, uint64_t len,
                            uint64_t max_request)
{
    UpOutcome o{};
    const uint32_t unfinished = max_request && len >= max_request ? WSG_UP_TOO_LONG : WSG_UP_INCOMPLETE;
    if (!found) {
        o.code = unfinished;
        return o;
    }
    if (!st.ok || f.malformed) {
        o.code = WSG_UP_BAD_HTTP;
        o.consumed = hend;
    } else if (f.has_clen && len - hend < f.clen) {
        o.code = unfinished;
        o.need = hend + f.clen < hend ? UINT64_MAX : hend + f.clen;
        return o;
    } else {
        o.consumed = hend + (f.has_clen ? f.clen : 0);
        o.url_off = off + st.url_off;
        o.url_len = up_sat32(st.url_len);
        if (!st.get) {
            o.code = WSG_UP_NOT_GET;
        } else {
            if (f.seen & UP_KEY) {
                o.key_off = off + f.key_off;
                o.key_len = up_sat32(f.key_len);
            }
            // (as PerformServerUpgrade ends: the flags first, the failing header only between them)
            o.code = f.seen == 0        ? WSG_UP_NOT_WEBSOCKET
                     : f.seen == UP_ALL ? WSG_UP_ACCEPTED
                     : f.fail           ? f.fail
                                        : WSG_UP_MISSING;
        }
    }
    o.resp_len = up_resp_len(o.code);
    o.status = o.code == WSG_UP_ACCEPTED ? 101u : o.resp_len ? 400u : 0u;
    return o;
}

// The record's four 8-byte words (the kernel stores it that way).
WSG_HD void up_record(const UpOutcome& o, uint64_t w[4])
{
    w[0] = o.key_off;
    w[1] = o.url_off;
    w[2] = uint64_t(o.key_len) | (uint64_t(o.url_len) << 32);
    w[3] = uint64_t(o.resp_len) | (uint64_t(o.status) << 32) | (uint64_t(o.code) << 48);
}

// ---- SHA-1 (FIPS 180-4) and Base64 (RFC 4648) -----------------------------------
WSG_HD uint32_t up_rol(uint32_t x, uint32_t n) { return (x << n) | (x >> (32u - n)); }

// One block: every index is a constant once the loops are unrolled, so h and
// w stay in registers on the device.
WSG_HD void up_sha1_block(uint32_t h[5], uint32_t w[16])
{
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int t = 0; t < 80; ++t) {
        if (t >= 16)
            w[t & 15] = up_rol(w[(t + 13) & 15] ^ w[(t + 8) & 15] ^ w[(t + 2) & 15] ^ w[t & 15], 1);
        const uint32_t f = t < 20 ? (b & c) | (~b & d) : t < 40 ? b ^ c ^ d : t < 60 ? (b & c) | (b & d) | (c & d) : b ^ c ^ d;
        const uint32_t k = t < 20 ? 0x5A827999u : t < 40 ? 0x6ED9EBA1u : t < 60 ? 0x8F1BBCDCu : 0xCA62C1D6u;
        const uint32_t tmp = up_rol(a, 5) + f + e + k + w[t & 15];
        e = d;
        d = c;
        c = up_rol(b, 30);
        b = a;
        a = tmp;
    }
    h[0] += a;
    h[1] += b;
    h[2] += c;
    h[3] += d;
    h[4] += e;
}

// SHA-1 of the n bytes msg(0 .. n - 1).
template <class Msg>
WSG_HD void up_sha1(Msg msg, uint64_t n, uint32_t h[5])
{
    h[0] = 0x67452301u;
    h[1] = 0xEFCDAB89u;
    h[2] = 0x98BADCFEu;
    h[3] = 0x10325476u;
    h[4] = 0xC3D2E1F0u;
    const uint64_t blocks = (n + 9 + 63) / 64;
    const uint64_t bits = n * 8;
    const auto padded = [&](uint64_t t) -> uint32_t { return t < n ? msg(t) & 0xFFu : t == n ? 0x80u : 0u; };
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (uint64_t b = 0; b < blocks; ++b) {
        uint32_t w[16];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int k = 0; k < 16; ++k) {
            const uint64_t t = b * 64 + uint64_t(k) * 4;
            w[k] = (padded(t) << 24) | (padded(t + 1) << 16) | (padded(t + 2) << 8) | padded(t + 3);
        }
        if (b + 1 == blocks) {   // the length: no message byte reaches the last eight
            w[14] = uint32_t(bits >> 32);
            w[15] = uint32_t(bits);
        }
        up_sha1_block(h, w);
    }
}

WSG_HD uint32_t up_b64(uint32_t v)   // v < 64
{
    return v < 26 ? 'A' + v : v < 52 ? 'a' + (v - 26) : v < 62 ? '0' + (v - 52) : v == 62 ? '+' : '/';
}

// Base64 of the 20 digest bytes: 28 characters, four to a word in memory order.
WSG_HD void up_base64_digest(const uint32_t h[5], uint32_t out[7])
{
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int g = 0; g < 7; ++g) {
        uint32_t v = 0;
        for (int k = 0; k < 3; ++k) {
            const int i = 3 * g + k;
            v = (v << 8) | (i < 20 ? (h[i >> 2] >> (24 - 8 * (i & 3))) & 0xFFu : 0u);
        }
        out[g] = up_b64(v >> 18) | (up_b64((v >> 12) & 63u) << 8) | (up_b64((v >> 6) & 63u) << 16) |
                 ((g == 6 ? uint32_t('=') : up_b64(v & 63u)) << 24);
    }
}

// Base64(SHA-1(key || GUID)): key(0 .. key_len - 1) the trimmed value.
template <class Key>
WSG_HD void up_accept(Key key, uint64_t key_len, uint32_t out[7])
{
    const char* guid = "258EAFA5-E914-47DA-95CA-C5AB0DC85B11";   // RFC 6455 1.3
    uint32_t h[5];
    up_sha1([&](uint64_t t) -> uint32_t { return t < key_len ? key(t) : uint32_t(uint8_t(guid[t - key_len])); },
            key_len + 36, h);
    up_base64_digest(h, out);
}

} // namespace wsg
