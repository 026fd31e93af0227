// wsg_upgrade_client_host.cpp — wsg_upgrade_client_judge and
// wsg_upgrade_request: one upgrade response judged, one upgrade request
// built, on the host by the rule of wsg_upgrade_client.h, the one the kernels
// of wsg_upgrade_client_streams and wsg_upgrade_requests run, with the lines
// folded in one owner's order.  Host-only C++ (no HIP, no OpenSSL), so the
// sanitizer build of tests/cpp compiles it as it is.
#include "wsg_upgrade_client.h"

#include <string.h>

extern "C" int wsg_upgrade_client_judge(const uint8_t* buf, uint64_t len, const uint8_t nonce[16],
                                        uint64_t max_response, wsg_upgrade_reply* out, uint64_t* consumed,
                                        uint64_t* need)
{
    if ((len && !buf) || !nonce || !out)
        return WSG_EINVAL;
    const auto src = [buf](uint64_t r) -> uint32_t { return buf[r]; };
    uint32_t n[4], h[5];
    for (int k = 0; k < 4; ++k)
        n[k] = uint32_t(nonce[4 * k]) | uint32_t(nonce[4 * k + 1]) << 8 | uint32_t(nonce[4 * k + 2]) << 16 |
               uint32_t(nonce[4 * k + 3]) << 24;
    wsg::uc_expect(n, h);
    const auto expect = [&h](uint32_t i) -> uint32_t { return (h[i >> 2] >> (24 - 8 * (i & 3))) & 0xFFu; };
    // the header end, the first line end
    bool found = false;
    uint64_t p = 0;
    for (uint64_t i = 0; i + 4 <= len && !found; ++i)
        if (buf[i] == '\r' && buf[i + 1] == '\n' && buf[i + 2] == '\r' && buf[i + 3] == '\n') {
            found = true;
            p = i;
        }
    wsg::UcFold f{};
    wsg::UcStatus st{};
    if (found) {
        uint64_t eol = p;
        bool first = true;
        // a line starts behind every "\r\n" in front of the header end
        for (uint64_t i = 2; i < p; ++i) {
            if (buf[i - 2] != '\r' || buf[i - 1] != '\n')
                continue;
            if (first) {
                first = false;
                eol = i - 2;
            }
            const wsg::UcLine ln = wsg::uc_line(src, i, len, expect);
            if (!ln.open)
                wsg::uc_fold(f, ln);
        }
        st = wsg::uc_status(src, eol);
    }
    const wsg::UcOutcome o = wsg::uc_outcome(found, p + 4, st, f, 0, len, max_response);
    uint64_t w[4];
    wsg::uc_record(o, w);
    memcpy(out, w, sizeof(w));
    if (consumed)
        *consumed = o.consumed;
    if (need)
        *need = o.need;
    return WSG_OK;
}

extern "C" int wsg_upgrade_request(const uint8_t* tpl, uint32_t tpl_len, uint32_t key_at, const uint8_t nonce[16],
                                   uint8_t* out)
{
    if (!tpl || !nonce || !out || uint64_t(key_at) + 24 > tpl_len)
        return WSG_EINVAL;
    memcpy(out, tpl, tpl_len);
    const auto nb = [nonce](uint32_t i) -> uint32_t { return nonce[i]; };
    for (uint32_t t = 0; t < 24; ++t)
        out[key_at + t] = uint8_t(wsg::uc_key_char(nb, t));
    return WSG_OK;
}
