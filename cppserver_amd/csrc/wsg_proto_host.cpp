// wsg_proto_host.cpp — wsg_proto_judge: one frame judged on the host by the rule
// of wsg_proto.h, the one k_proto_judge runs.  Host-only C++ (no HIP), so the
// sanitizer build of tests/cpp compiles it as it is.
#include "wsg_proto.h"

extern "C" int wsg_proto_judge(const wsg_recv_info* info, const uint8_t* wire, const wsg_proto_state* before,
                               uint32_t role, uint64_t max_message, wsg_proto_state* after, uint16_t* status)
{
    if (!info || !before || role > WSG_PROTO_CLIENT)
        return WSG_EINVAL;
    wsg::ProtoFrame f;
    f.payload_off = info->payload_off;
    f.len = info->len;
    f.key = info->key;
    f.op = info->opcode;
    f.rsv = info->b0 & 0x70u;
    f.fin = info->fin != 0;
    f.masked = info->masked != 0;
    f.error = info->error != 0;
    const bool open = before->open != 0;
    const wsg::ProtoStep next = wsg::proto_then(wsg::proto_seed(before->bytes, open), wsg::proto_step(f));
    bool no_wire = false;
    uint32_t st = 0;
    const uint32_t code = wsg::proto_code(
        f, open, next.bytes, role, max_message,
        [&]() -> uint32_t {
            if (!wire) {
                no_wire = true;
                return 0;
            }
            return wsg::proto_wire_status(wire[f.payload_off], wire[f.payload_off + 1], f);
        },
        &st);
    if (no_wire)
        return WSG_EINVAL;
    if (after) {
        *after = wsg_proto_state{};
        after->bytes = next.bytes;
        after->open = uint8_t(next.open);
    }
    if (status)
        *status = uint16_t(st);
    return int(code);
}
