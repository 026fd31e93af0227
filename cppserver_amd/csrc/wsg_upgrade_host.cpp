// wsg_upgrade_host.cpp — wsg_upgrade_judge: one upgrade request judged on the
// host by the rule of wsg_upgrade.h, the one k_upgrade_parse runs, with the
// lines folded in one owner's order.  Host-only C++ (no HIP, no OpenSSL), so
// the sanitizer build of tests/cpp compiles it as it is.
#include "wsg_upgrade.h"

#include <string.h>

extern "C" int wsg_upgrade_judge(const uint8_t* buf, uint64_t len, uint64_t max_request, wsg_upgrade* out,
                                 uint8_t* resp, uint32_t resp_cap, uint64_t* consumed, uint64_t* need)
{
    if ((len && !buf) || !out || (resp_cap && !resp))
        return WSG_EINVAL;
    const auto src = [buf](uint64_t r) -> uint32_t { return buf[r]; };
    // the header end, the first line end
    bool found = false;
    uint64_t p = 0;
    for (uint64_t i = 0; i + 4 <= len && !found; ++i)
        if (buf[i] == '\r' && buf[i + 1] == '\n' && buf[i + 2] == '\r' && buf[i + 3] == '\n') {
            found = true;
            p = i;
        }
    wsg::UpFold f{};
    wsg::UpStart st{};
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
            const wsg::UpLine ln = wsg::up_line(src, i, len);
            if (!ln.open)
                wsg::up_fold(f, ln);
        }
        st = wsg::up_start(src, eol);
    }
    const wsg::UpOutcome o = wsg::up_outcome(found, p + 4, st, f, 0, len, max_request);
    uint64_t w[4];
    wsg::up_record(o, w);
    memcpy(out, w, sizeof(w));
    if (consumed)
        *consumed = o.consumed;
    if (need)
        *need = o.need;
    if (o.resp_len > resp_cap)
        return WSG_ENOMEM;
    static const char* const tpl[wsg::UP_TEMPLATES] = {
        "", WSG_UP_T_ACCEPTED, WSG_UP_T_BAD_HTTP, WSG_UP_T_BAD_CONNECTION, WSG_UP_T_BAD_UPGRADE, WSG_UP_T_EMPTY_KEY,
        WSG_UP_T_BAD_VERSION, WSG_UP_T_MISSING};
    if (o.resp_len) {
        memcpy(resp, tpl[o.code], o.resp_len);
        if (o.code == WSG_UP_ACCEPTED) {
            const uint8_t* key = buf + o.key_off;
            uint32_t a[7];
            wsg::up_accept([key](uint64_t t) -> uint32_t { return key[t]; }, o.key_len, a);
            for (uint32_t k = 0; k < wsg::UP_ACCEPT_LEN; ++k)
                resp[wsg::UP_ACCEPT_AT + k] = uint8_t(a[k >> 2] >> (8 * (k & 3)));
        }
    }
    return WSG_OK;
}
