// wsg_proto_judge (csrc/wsg_proto_host.cpp over csrc/wsg_proto.h, the rule
// the kernels run) under AddressSanitizer + UndefinedBehaviorSanitizer, no GPU:
// every combination of opcode, fin, masked, RSV, length, open and role against
// a second, straight-line statement of the rule table of include/wsg_capi.h.
// The wire block of each call is a heap block exactly as long as the frame, so
// a read outside the frame is an error of the run.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "wsg_capi.h"

namespace {

struct Want {
    int code;
    unsigned status;
    uint64_t bytes;
    unsigned open;
};

bool legal(unsigned s) { return (s >= 1000 && s <= 1003) || (s >= 1007 && s <= 1014) || (s >= 3000 && s <= 4999); }

// The table, row by row.
Want table(unsigned op, bool fin, bool masked, unsigned rsv, uint64_t len, bool open, uint64_t bytes, unsigned role,
           uint64_t max_message, unsigned carried)
{
    const bool control = (op & 8) != 0;
    const bool reserved = (op >= 3 && op <= 7) || (op >= 0xB && op <= 0xF);
    Want w{0, 0, bytes, open ? 1u : 0u};
    if (!control && !reserved) {
        w.bytes = op == 0 ? (bytes + len < bytes ? UINT64_MAX : bytes + len) : len;
        w.open = fin ? 0 : 1;
    }
    if (rsv != 0)
        w.code = WSG_PV_RSV;
    else if (reserved)
        w.code = WSG_PV_OPCODE;
    else if ((role == WSG_PROTO_SERVER && !masked) || (role == WSG_PROTO_CLIENT && masked))
        w.code = WSG_PV_MASK;
    else if (control && !fin)
        w.code = WSG_PV_CTRL_FRAGMENT;
    else if (control && len > 125)
        w.code = WSG_PV_CTRL_LONG;
    else if (op == 0 && !open)
        w.code = WSG_PV_CONT;
    else if ((op == 1 || op == 2) && open)
        w.code = WSG_PV_DATA;
    else if (op == 8 && len == 1)
        w.code = WSG_PV_CLOSE_LEN;
    else if (op == 8 && len >= 2 && !legal(carried))
        w.code = WSG_PV_CLOSE_CODE;
    else if (op <= 2 && max_message != 0 && w.bytes > max_message)
        w.code = WSG_PV_TOO_BIG;
    else if (op == 8)
        w.code = WSG_PV_CLOSED;
    if (w.code == WSG_PV_CLOSED)
        w.status = len == 0 ? 1005 : carried;
    else if (w.code == WSG_PV_TOO_BIG)
        w.status = 1009;
    else if (w.code != 0)
        w.status = 1002;
    return w;
}

int failures = 0;

void fail(const char* what, unsigned op, bool fin, bool masked, unsigned rsv, uint64_t len, bool open, unsigned role,
          uint64_t max_message, unsigned carried)
{
    if (++failures <= 20)
        std::fprintf(stderr, "%s: op %u fin %d masked %d rsv %#x len %llu open %d role %u max %llu status %u\n", what,
                     op, fin, masked, rsv, static_cast<unsigned long long>(len), open, role,
                     static_cast<unsigned long long>(max_message), carried);
}

} // namespace

int main()
{
    const uint64_t lens[] = {0, 1, 2, 125, 126};
    const unsigned rsvs[] = {0, 0x40};
    const unsigned statuses[] = {1000, 1005, 999, 4999};
    const uint64_t limits[] = {0, 100, 130};
    const uint32_t key = 0xA1B2C3D4u;
    long calls = 0;
    for (unsigned op = 0; op < 16; ++op)
        for (int fin = 0; fin < 2; ++fin)
            for (int masked = 0; masked < 2; ++masked)
                for (unsigned rsv : rsvs)
                    for (uint64_t len : lens)
                        for (int open = 0; open < 2; ++open)
                            for (unsigned role = 0; role < 3; ++role)
                                for (unsigned carried : statuses)
                                    for (uint64_t max_message : limits) {
                                        // the frame, exactly: header (length byte form; 126 takes the 2-byte form), key, payload
                                        const unsigned hdr = (len < 126 ? 2u : 4u) + (masked ? 4u : 0u);
                                        std::vector<uint8_t> wire(hdr + len);   // a heap block of exactly the frame
                                        uint8_t* w = wire.data();
                                        w[0] = uint8_t((fin ? 0x80 : 0) | rsv | op);
                                        w[1] = uint8_t((masked ? 0x80 : 0) | (len < 126 ? len : 126));
                                        if (len >= 126) {
                                            w[2] = uint8_t(len >> 8);
                                            w[3] = uint8_t(len);
                                        }
                                        if (masked)
                                            std::memcpy(w + hdr - 4, &key, 4);   // little-endian hosts: the key's bytes 0..3
                                        for (uint64_t t = 0; t < len; ++t) {
                                            const uint8_t plain = t == 0 ? uint8_t(carried >> 8) : t == 1 ? uint8_t(carried) : 0x55;
                                            w[hdr + t] = masked ? uint8_t(plain ^ uint8_t(key >> (8 * (t & 3)))) : plain;
                                        }
                                        wsg_recv_info info;
                                        std::memset(&info, 0, sizeof(info));
                                        info.payload_off = hdr;
                                        info.len = len;
                                        info.key = masked ? key : 0;
                                        info.opcode = uint8_t(op);
                                        info.fin = uint8_t(fin);
                                        info.masked = uint8_t(masked);
                                        info.hdr_len = uint8_t(hdr);
                                        info.b0 = w[0];
                                        wsg_proto_state before, after;
                                        std::memset(&before, 0, sizeof(before));
                                        std::memset(&after, 0xEE, sizeof(after));
                                        before.bytes = 90;
                                        before.open = uint8_t(open);
                                        uint16_t status = 0xEEEE;
                                        const int code = wsg_proto_judge(&info, w, &before, role, max_message, &after, &status);
                                        const Want want = table(op, fin, masked, rsv, len, open, 90, role, max_message,
                                                                len >= 2 ? carried : 0);
                                        ++calls;
                                        static const uint8_t zero[7] = {0};
                                        if (code != want.code || status != want.status || after.bytes != want.bytes ||
                                            after.open != want.open || std::memcmp(after._pad, zero, 7) != 0)
                                            fail("mismatch", op, fin, masked, rsv, len, open, role, max_message, carried);
                                    }
    // a frame error: code 2 whatever else the record says, the state kept
    {
        wsg_recv_info info;
        std::memset(&info, 0, sizeof(info));
        info.error = WSG_ETRUNC;
        wsg_proto_state before, after;
        std::memset(&before, 0, sizeof(before));
        before.bytes = 7;
        before.open = 1;
        uint16_t status = 0;
        if (wsg_proto_judge(&info, nullptr, &before, WSG_PROTO_SERVER, 1, &after, &status) != WSG_PV_FRAME ||
            status != 1002 || after.bytes != 7 || after.open != 1)
            fail("frame error", 0, 0, 0, 0, 0, 1, 1, 1, 0);
        // the saturating sum
        info.error = 0;
        info.len = 10;
        before.bytes = UINT64_MAX - 3;
        if (wsg_proto_judge(&info, nullptr, &before, WSG_PROTO_ANY, 0, &after, nullptr) != 0 ||
            after.bytes != UINT64_MAX || after.open != 1)
            fail("saturation", 0, 0, 0, 0, 10, 1, 0, 0, 0);
        if (wsg_proto_judge(nullptr, nullptr, &before, 0, 0, nullptr, nullptr) != WSG_EINVAL ||
            wsg_proto_judge(&info, nullptr, nullptr, 0, 0, nullptr, nullptr) != WSG_EINVAL ||
            wsg_proto_judge(&info, nullptr, &before, 3, 0, nullptr, nullptr) != WSG_EINVAL)
            fail("arguments", 0, 0, 0, 0, 0, 0, 3, 0, 0);
    }
    if (failures) {
        std::fprintf(stderr, "test_proto_host: %d of %ld calls differ\n", failures, calls);
        return 1;
    }
    std::printf("test_proto_host: %ld calls ok\n", calls);
    return 0;
}
