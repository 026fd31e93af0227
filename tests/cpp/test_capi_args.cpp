// The argument checks of the device entry points (cppserver_amd/csrc/wsg_args.h)
// without a device: every entry point's operands as literal rows — name, bytes
// at the shape below, alignment, kind — transcribed from the conditions the
// entry points spelled out before the tables (wsg_capi_device.cpp of the
// revision before wsg_args.h) and the contract text of wsg_capi.h, never from
// the tables under test.  For a _streams form the rows are the union of what
// its own checks, wsg_frame_streams inside it and its inner call ask.
//
// Pointers are addresses inside one static buffer, 64 bytes apart, and are
// never dereferenced (reply_op and relay_op, host memory the check reads, are
// real arrays).  in_alloc is this program's: it records every query and can
// refuse the k-th.  Built with AddressSanitizer + UndefinedBehaviorSanitizer
// (make sanitize).
#include "wsg_args.h"

#include <algorithm>
#include <cstdio>
#include <functional>
#include <string_view>
#include <utility>
#include <vector>

namespace {

int failures = 0;

#define CHECK(cond)                                                                                          \
    do {                                                                                                     \
        if (!(cond)) {                                                                                       \
            ++failures;                                                                                      \
            std::printf("FAIL %s:%d: %s  [%s %s]\n", __FILE__, __LINE__, #cond, what, detail);               \
        }                                                                                                    \
    } while (0)

using uc = unsigned char;
using Query = std::pair<const void*, uint64_t>;

std::vector<Query> asked;
int refuse_at = -1;   // the index of the query in_alloc refuses (-1: none)

alignas(64) uc arena[64 * 32];
uc* slot(size_t i) { return arena + 64 * i; }

} // namespace

bool in_alloc(const void* p, uint64_t bytes)
{
    asked.push_back({p, bytes});
    return int(asked.size()) - 1 != refuse_at;
}

namespace {

template <class T>
T* as(uc* p)
{
    return reinterpret_cast<T*>(p);
}

// The shape of a call.  full: the smallest non-trivial one; none: no frame, no
// stream, no byte.  (n_groups is 1 in both.)
struct Z {
    uint32_t n, ns;       // frames (or frame_cap, msg_room), streams
    uint64_t len, cap;    // wire_len (and new_len), every capacity (and a fan-out's total)
    uint32_t k, m;        // fan-out keys and messages
};
constexpr Z full{1, 1, 16, 16, 1, 1};
constexpr Z none{0, 0, 0, 0, 0, 0};

// A: always required.  S: required when its bytes are not 0.  O: optional.
// H: host memory, always required (never aligned, never looked up).
// h: host memory, required when the shape has messages.
struct Row {
    const char* name;
    uint64_t bytes;   // at `full`
    uint32_t align;
    char kind;
};

using P = const std::vector<uc*>&;
struct Entry {
    const char* name;
    std::vector<Row> rows;
    std::function<int(P, const Z&, bool)> call;   // p[i]: the operand of rows[i]
};

const uint8_t relay_none[5] = {0, 0, 0, 0, 0};
const uint8_t reply_echo[5] = {0, WSG_REPLY_SAME, WSG_REPLY_SAME, 0, 0};

wsg::Batch batch(uc* wire, uc* fs, uc* sf, const Z& z)
{
    return wsg::Batch{wire, z.len, as<const uint64_t>(fs), z.n, as<const uint32_t>(sf), z.ns};
}
wsg::MsgOut out(uc* msgs, uc* count, uc* info)
{
    return wsg::MsgOut{as<wsg_msg>(msgs), as<uint64_t>(count), as<wsg_recv_info>(info)};
}
wsg::Framed framed(uc* span, uc* fs, uc* sf, uc* nfo, const Z& z)
{
    return wsg::Framed{as<wsg_stream_span>(span), as<uint64_t>(fs), z.n, as<uint32_t>(sf), as<uint32_t>(nfo)};
}
wsg::ReplyOut reply(uc* op, uc* key, uc* rep, uc* off, uc* sr, uc* close, const Z& z)
{
    return wsg::ReplyOut{op, 0, as<const uint32_t>(key), rep, z.cap, as<uint64_t>(off), as<uint64_t>(sr),
                         as<uint64_t>(close)};
}
wsg::ProtoOps proto(uc* pr, uc* also, uc* verdict, uc* result, uint32_t role = WSG_PROTO_SERVER)
{
    return wsg::ProtoOps{as<wsg_proto_state>(pr), role, 0, as<const wsg_proto_verdict>(also),
                         as<wsg_proto_verdict>(verdict), as<uint64_t>(result)};
}
wsg::Utf8Inside utf8(uc* valid, uc* result) { return wsg::Utf8Inside{1, as<uint64_t>(valid), as<uint64_t>(result), nullptr, 1, 1}; }
wsg::RelayArgs relay(uc* op, uc* order, uc* gf, uc* rel, uc* off, uc* gr, const Z& z, uint32_t n_groups = 1)
{
    return wsg::RelayArgs{op, as<const uint32_t>(order), as<const uint32_t>(gf), n_groups, rel, z.cap, as<uint64_t>(off),
                          as<uint64_t>(gr)};
}

// ---- the rows, by entry point ---------------------------------------------------
// The checked reply's, shared by its five forms as literal pieces: direct
// (with d_frame_start, d_also) or _streams (with d_span, n_frames_out).
std::vector<Row> checked_rows(bool streams, bool validated, bool relays)
{
    std::vector<Row> r = {
        {"d_wire", 16, 16, 'S'},        {"d_frame_start", 8, 8, 'S'}, {"d_stream_first", 8, 4, 'A'},
        {"d_state", 8, 8, 'S'},         {"d_proto", 16, 8, 'A'},      {"d_send_key", 4, 4, 'O'},
        {"d_reply", 16, 16, 'S'},       {"d_reply_off", 16, 8, 'A'},  {"d_stream_reply", 16, 8, 'A'},
        {"d_close_off", 8, 8, 'A'},     {"d_verdict", 8, 8, 'A'},     {"d_result", 24, 8, 'A'},
        {"d_msgs", 40, 8, 'S'},         {"d_count", relays ? 64u : 40u, 8, 'A'},
        {"d_info", 32, 8, 'S'},
    };
    if (streams) {
        r.push_back({"d_span", 32, 1, 'S'});
        r.push_back({"n_frames_out", 0, 1, 'H'});
    } else {
        r.push_back({"d_also", 8, 8, 'O'});
    }
    if (validated) {
        r.push_back({"d_valid", 8, 8, 'S'});
        r.push_back({"d_utf8_result", 32, 8, 'A'});
    }
    if (relays) {
        r.push_back({"relay_op", 0, 1, 'H'});
        r.push_back({"d_order", 4, 4, 'O'});
        r.push_back({"d_group_first", 8, 4, 'O'});
        r.push_back({"d_relay", 16, 16, 'S'});
        r.push_back({"d_relay_off", 8, 8, 'S'});
        r.push_back({"d_group_relay", 16, 8, 'A'});
    }
    r.push_back({"reply_op", 0, 1, 'H'});
    return r;
}

// ... and the call that goes with them (the operands in the rows' order).
int checked_call(bool streams, bool validated, bool relays, P p, const Z& z, bool check, uint32_t n_groups = 1,
                 uint32_t role = WSG_PROTO_SERVER)
{
    const wsg::Batch b = batch(p[0], p[1], p[2], z);
    const wsg::MsgOut o = out(p[12], p[13], p[14]);
    const wsg::ReplyOut r = reply(p.back(), p[5], p[6], p[7], p[8], p[9], z);
    size_t at = 15;
    wsg::Framed f{};
    uc* also = nullptr;
    if (streams) {
        f = framed(p[at], p[1], p[2], p[at + 1], z);
        at += 2;
    } else {
        also = p[at++];
    }
    const wsg::ProtoOps pr = proto(p[4], also, p[10], p[11], role);
    wsg::Utf8Inside u{};
    if (validated) {
        u = utf8(p[at], p[at + 1]);
        at += 2;
    }
    wsg::RelayArgs q{};
    if (relays)
        q = relay(p[at], p[at + 1], p[at + 2], p[at + 3], p[at + 4], p[at + 5], z, n_groups);
    return wsg::args_messages(b, p[3], nullptr, 0, &r, o, &pr, validated ? &u : nullptr, relays ? &q : nullptr,
                              streams ? &f : nullptr, check);
}

Entry checked_entry(const char* name, bool streams, bool validated, bool relays)
{
    return Entry{name, checked_rows(streams, validated, relays), [=](P p, const Z& z, bool check) {
                     return checked_call(streams, validated, relays, p, z, check);
                 }};
}

std::vector<Entry> entries()
{
    std::vector<Entry> e;
    e.push_back({"wsg_decode_batch",
                 {{"d_wire", 16, 16, 'S'}, {"d_frame_start", 8, 1, 'S'}, {"d_out", 16, 16, 'S'}, {"d_info", 32, 1, 'S'}},
                 [](P p, const Z& z, bool check) {
                     return wsg::args_decode_batch(p[0], z.len, p[1], z.n, p[2], p[3], check);
                 }});
    e.push_back({"wsg_decode_messages",
                 {{"d_wire", 16, 16, 'S'},
                  {"d_frame_start", 8, 1, 'S'},
                  {"d_stream_first", 8, 1, 'A'},
                  {"d_state", 8, 1, 'S'},
                  {"d_msg", 16, 16, 'S'},
                  {"d_msgs", 40, 1, 'S'},
                  {"d_count", 16, 1, 'A'},
                  {"d_info", 32, 1, 'S'}},
                 [](P p, const Z& z, bool check) {
                     return wsg::args_messages(batch(p[0], p[1], p[2], z), p[3], p[4], z.cap, nullptr, out(p[5], p[6], p[7]), nullptr,
                                               nullptr, nullptr, nullptr, check);
                 }});
    e.push_back({"wsg_check_utf8",
                 {{"d_msg", 16, 16, 'S'},
                  {"d_msgs", 40, 8, 'S'},
                  {"d_count", 16, 8, 'A'},
                  {"d_valid", 8, 8, 'S'},
                  {"d_result", 32, 8, 'A'}},
                 [](P p, const Z& z, bool check) {
                     return wsg::args_check_utf8(p[0], z.cap, p[1], p[2], z.n, p[3], p[4], check);
                 }});
    e.push_back({"wsg_check_utf8_wire",
                 {{"d_wire", 16, 16, 'S'},
                  {"d_frame_start", 8, 8, 'S'},
                  {"d_stream_first", 8, 4, 'A'},
                  {"d_state", 8, 8, 'S'},
                  {"d_msgs", 40, 8, 'S'},
                  {"d_count", 16, 8, 'A'},
                  {"d_info", 32, 8, 'S'},
                  {"d_valid", 8, 8, 'S'},
                  {"d_result", 32, 8, 'A'}},
                 [](P p, const Z& z, bool check) {
                     const wsg::Utf8Inside u = utf8(p[7], p[8]);
                     return wsg::args_messages(batch(p[0], p[1], p[2], z), p[3], nullptr, 0, nullptr, out(p[4], p[5], p[6]),
                                               nullptr, &u, nullptr, nullptr, check);
                 }});
    // d_info, d_proto and d_verdict required whatever n and n_streams; the wire by the byte
    e.push_back({"wsg_check_protocol",
                 {{"d_wire", 16, 1, 'S'},
                  {"d_info", 32, 8, 'A'},
                  {"d_stream_first", 8, 4, 'A'},
                  {"d_state", 8, 8, 'O'},
                  {"d_proto", 16, 8, 'A'},
                  {"d_verdict", 8, 8, 'A'},
                  {"d_result", 24, 8, 'A'}},
                 [](P p, const Z& z, bool check) {
                     return wsg::args_check_protocol(batch(p[0], nullptr, p[2], z), p[1], p[3],
                                                     proto(p[4], nullptr, p[5], p[6]), check);
                 }});
    e.push_back({"wsg_frame_streams",
                 {{"d_wire", 16, 16, 'S'},
                  {"d_span", 32, 1, 'S'},
                  {"d_frame_start", 8, 1, 'S'},
                  {"d_stream_first", 8, 1, 'A'},
                  {"d_count", 16, 1, 'A'}},
                 [](P p, const Z& z, bool check) {
                     return wsg::args_frame_streams(p[0], z.len, p[1], z.ns, p[2], z.n, p[3], p[4], check);
                 }});
    e.push_back({"wsg_upgrade_streams",
                 {{"d_wire", 16, 16, 'S'},
                  {"d_span", 32, 8, 'S'},
                  {"d_up", 32, 8, 'S'},
                  {"d_resp", 16, 16, 'S'},
                  {"d_resp_off", 16, 8, 'A'},
                  {"d_count", 32, 8, 'A'}},
                 [](P p, const Z& z, bool check) {
                     return wsg::args_upgrade_streams(p[0], z.len, p[1], z.ns, p[2], p[3], z.cap, p[4], p[5], check);
                 }});
    e.push_back({"wsg_carry_streams",
                 {{"d_wire", 16, 16, 'S'},
                  {"d_span", 32, 8, 'S'},
                  {"d_close_off", 8, 8, 'O'},
                  {"d_new", 16, 16, 'S'},
                  {"d_read", 16, 8, 'O'},
                  {"d_next", 16, 16, 'S'},
                  {"d_next_span", 32, 8, 'S'},
                  {"d_count", 32, 8, 'A'}},
                 [](P p, const Z& z, bool check) {
                     return wsg::args_carry_streams(p[0], z.len, p[1], z.ns, p[2], p[3], z.len, p[4], p[5], z.cap, p[6],
                                                    p[7], check);
                 }});
    e.push_back({"wsg_decode_streams",
                 {{"d_wire", 16, 16, 'S'},
                  {"d_frame_start", 8, 1, 'S'},
                  {"d_stream_first", 8, 1, 'A'},
                  {"d_state", 8, 1, 'S'},
                  {"d_msg", 16, 16, 'S'},
                  {"d_msgs", 40, 1, 'S'},
                  {"d_count", 16, 1, 'A'},
                  {"d_info", 32, 1, 'S'},
                  {"d_span", 32, 1, 'S'},
                  {"n_frames_out", 0, 1, 'H'}},
                 [](P p, const Z& z, bool check) {
                     const wsg::Framed f = framed(p[8], p[1], p[2], p[9], z);
                     return wsg::args_messages(batch(p[0], p[1], p[2], z), p[3], p[4], z.cap, nullptr, out(p[5], p[6], p[7]), nullptr,
                                               nullptr, nullptr, &f, check);
                 }});
    // the unchecked replies: 16-byte operands alone aligned, 4 words of d_count
    const std::vector<Row> reply_rows = {
        {"d_wire", 16, 16, 'S'},  {"d_frame_start", 8, 1, 'S'}, {"d_stream_first", 8, 1, 'A'},  {"d_state", 8, 1, 'S'},
        {"d_send_key", 4, 1, 'O'}, {"d_reply", 16, 16, 'S'},    {"d_reply_off", 16, 1, 'A'},    {"d_stream_reply", 16, 1, 'A'},
        {"d_msgs", 40, 1, 'S'},   {"d_count", 32, 1, 'A'},      {"d_info", 32, 1, 'S'},
    };
    const Row reply_op_row = {"reply_op", 0, 1, 'H'};   // (last in every list of rows that has it)
    std::vector<Row> reply_messages_rows = reply_rows;
    reply_messages_rows.push_back(reply_op_row);
    e.push_back({"wsg_reply_messages", reply_messages_rows, [](P p, const Z& z, bool check) {
                     const wsg::ReplyOut r = reply(p.back(), p[4], p[5], p[6], p[7], nullptr, z);
                     return wsg::args_messages(batch(p[0], p[1], p[2], z), p[3], nullptr, 0, &r, out(p[8], p[9], p[10]),
                                               nullptr, nullptr, nullptr, nullptr, check);
                 }});
    std::vector<Row> reply_streams_rows = reply_rows;
    reply_streams_rows.push_back({"d_span", 32, 1, 'S'});
    reply_streams_rows.push_back({"n_frames_out", 0, 1, 'H'});
    reply_streams_rows.push_back(reply_op_row);
    e.push_back({"wsg_reply_streams", reply_streams_rows, [](P p, const Z& z, bool check) {
                     const wsg::Framed f = framed(p[11], p[1], p[2], p[12], z);
                     const wsg::ReplyOut r = reply(p.back(), p[4], p[5], p[6], p[7], nullptr, z);
                     return wsg::args_messages(batch(p[0], p[1], p[2], z), p[3], nullptr, 0, &r, out(p[8], p[9], p[10]),
                                               nullptr, nullptr, nullptr, &f, check);
                 }});
    e.push_back(checked_entry("wsg_reply_checked", false, false, false));
    e.push_back(checked_entry("wsg_reply_validated", false, true, false));
    e.push_back(checked_entry("wsg_reply_checked_streams", true, false, false));
    e.push_back(checked_entry("wsg_reply_validated_streams", true, true, false));
    e.push_back(checked_entry("wsg_relay_validated", false, true, true));
    e.push_back(checked_entry("wsg_relay_validated_streams", true, true, true));
    e.push_back({"wsg_utf8_verdicts",
                 {{"d_msgs", 40, 8, 'S'}, {"d_count", 16, 8, 'A'}, {"d_valid", 8, 8, 'S'}, {"d_also", 8, 8, 'S'}},
                 [](P p, const Z& z, bool check) {
                     return wsg::args_utf8_verdicts(p[0], p[1], z.n, p[2], z.ns, p[3], check);
                 }});
    // (d_wire by n, its bytes wire_cap; the payload ranges are the descriptors')
    e.push_back({"wsg_encode_batch",
                 {{"d_desc", 32, 1, 'S'}, {"d_wire", 16, 16, 'S'}, {"d_wire_off", 16, 1, 'A'}},
                 [](P p, const Z& z, bool check) {
                     return wsg::args_encode_batch(p[0], z.n, p[1], z.cap, p[2], check);
                 }});
    e.push_back({"wsg_fanout_encode",
                 {{"d_payload", 16, 1, 'S'}, {"d_keys", 4, 1, 'S'}, {"d_wire", 16, 16, 'S'}},
                 [](P p, const Z& z, bool check) {
                     return wsg::args_fanout_encode(p[0], z.len, p[1], z.k, p[2], z.cap, check);
                 }});
    e.push_back({"wsg_fanout_encode_many",
                 {{"src_off", 0, 1, 'h'},
                  {"len", 0, 1, 'h'},
                  {"opcode", 0, 1, 'h'},
                  {"d_keys", 4, 1, 'S'},
                  {"d_wire", 16, 16, 'S'},
                  {"wire_off", 0, 1, 'H'}},
                 [](P p, const Z& z, bool check) {
                     return wsg::args_fanout_encode_many(p[0], p[1], p[2], z.m, p[3], z.k, p[4], z.cap, p[5], check);
                 }});
    return e;
}

std::vector<uc*> operands(const Entry& e)
{
    std::vector<uc*> p(e.rows.size());
    for (size_t i = 0; i < p.size(); ++i)
        p[i] = slot(i);
    for (size_t i = 0; i < p.size(); ++i)
        if (std::string_view(e.rows[i].name) == "relay_op")
            p[i] = const_cast<uc*>(relay_none);
        else if (std::string_view(e.rows[i].name) == "reply_op")
            p[i] = const_cast<uc*>(reply_echo);
    return p;
}

int call(const Entry& e, P p, const Z& z, bool check, int refuse = -1)
{
    asked.clear();
    refuse_at = refuse;
    const int rc = e.call(p, z, check);
    refuse_at = -1;
    return rc;
}

bool device(char kind) { return kind == 'A' || kind == 'S' || kind == 'O'; }

void run(const Entry& e)
{
    const char* what = e.name;
    const char* detail = "";
    const std::vector<uc*> good = operands(e);

    CHECK(call(e, good, full, false) == WSG_OK);
    CHECK(asked.empty());                                   // without `check`, nothing is looked up

    for (size_t i = 0; i < good.size(); ++i) {
        const Row& r = e.rows[i];
        detail = r.name;
        std::vector<uc*> p = good;
        p[i] = nullptr;                                     // each operand null in turn
        CHECK(call(e, p, full, false) == (r.kind == 'O' ? WSG_OK : WSG_EINVAL));
        CHECK(asked.empty());
        if (!device(r.kind))
            continue;
        for (uint64_t off : {1, 4, 8}) {                    // ... and off its alignment
            p[i] = good[i] + off;
            CHECK(call(e, p, full, false) == (off % r.align ? WSG_EINVAL : WSG_OK));
        }
    }

    // no frame, no stream, no byte: what is required by a size may be null, the rest may not
    std::vector<uc*> bare = good;
    for (size_t i = 0; i < bare.size(); ++i)
        if (e.rows[i].kind == 'S' || e.rows[i].kind == 'h')
            bare[i] = nullptr;
    detail = "none";
    CHECK(call(e, bare, none, false) == WSG_OK);
    CHECK(call(e, good, none, false) == WSG_OK);
    for (size_t i = 0; i < bare.size(); ++i) {
        if (e.rows[i].kind != 'A' && e.rows[i].kind != 'H')
            continue;
        detail = e.rows[i].name;
        std::vector<uc*> p = bare;
        p[i] = nullptr;
        CHECK(call(e, p, none, false) == WSG_EINVAL);
    }

    // under `check`: every device operand looked up once with its bytes, and a refusal of any of them
    std::vector<Query> want;
    for (size_t i = 0; i < good.size(); ++i)
        if (device(e.rows[i].kind))
            want.push_back({good[i], e.rows[i].bytes});
    detail = "check";
    CHECK(call(e, good, full, true) == WSG_OK);
    std::vector<Query> got = asked;
    std::sort(got.begin(), got.end());
    std::sort(want.begin(), want.end());
    CHECK(got == want);
    if (got != want)
        for (const Query& q : got)
            std::printf("    asked slot %td: %llu bytes\n", (static_cast<const uc*>(q.first) - arena) / 64,
                        static_cast<unsigned long long>(q.second));
    for (int k = 0; k < int(got.size()); ++k)
        CHECK(call(e, good, full, true, k) == WSG_EINVAL);
    // an optional operand that is not given is not looked up
    for (size_t i = 0; i < good.size(); ++i) {
        if (e.rows[i].kind != 'O')
            continue;
        detail = e.rows[i].name;
        std::vector<uc*> p = good;
        p[i] = nullptr;
        CHECK(call(e, p, full, true) == WSG_OK);
        CHECK(asked.size() + 1 == want.size());
    }
}

// What is not one operand's, and the sizes the shape above cannot show.
void others()
{
    const char* what = "others";
    const char* detail = "";
    std::vector<uc*> p(32);
    for (size_t i = 0; i < p.size(); ++i)
        p[i] = slot(i);
    const auto has = [](const void* q, uint64_t bytes) {
        return std::find(asked.begin(), asked.end(), Query{q, bytes}) != asked.end();
    };

    // a wire's allocation holds its last 16-byte chunk whole; wsg_check_protocol reads it by the byte
    detail = "wire rounding";
    Z z = full;
    z.len = 10;
    asked.clear();
    CHECK(wsg::args_decode_batch(p[0], z.len, p[1], z.n, p[2], p[3], true) == WSG_OK);
    CHECK(has(p[0], 16) && has(p[2], 10));
    asked.clear();
    CHECK(wsg::args_check_protocol(batch(p[0], nullptr, p[2], z), p[1], p[3], proto(p[4], nullptr, p[5], p[6]), true) ==
          WSG_OK);
    CHECK(has(p[0], 10));
    CHECK(wsg::args_check_protocol(batch(p[0] + 1, nullptr, p[2], z), p[1], p[3], proto(p[4], nullptr, p[5], p[6]),
                                   false) == WSG_OK);

    // (n_streams + 1) * 4, (n + 1) * 8 and the tables at three frames in two streams
    detail = "sizes";
    z = Z{3, 2, 16, 16, 1, 1};
    asked.clear();
    const wsg::ReplyOut three = reply(p[11], p[4], p[5], p[6], p[7], nullptr, z);
    CHECK(wsg::args_messages(batch(p[0], p[1], p[2], z), p[3], nullptr, 0, &three, out(p[8], p[9], p[10]), nullptr,
                             nullptr, nullptr, nullptr, true) == WSG_OK);
    CHECK(has(p[1], 24) && has(p[2], 12) && has(p[3], 16) && has(p[4], 8) && has(p[6], 32) && has(p[7], 24) &&
          has(p[8], 120) && has(p[9], 32) && has(p[10], 96));

    // the counts
    detail = "counts";
    const auto decode = [&](const Z& s, const wsg::Framed* f) {
        return wsg::args_messages(batch(p[0], p[1], p[2], s), p[3], p[4], s.cap, nullptr, out(p[5], p[6], p[7]), nullptr,
                                               nullptr, nullptr, f, false);
    };
    const wsg::Framed f = framed(p[8], p[1], p[2], p[9], full);
    z = full;
    z.n = UINT32_MAX;
    CHECK(decode(z, nullptr) == WSG_EINVAL);
    CHECK(decode(z, &f) == WSG_OK);             // a frame_cap, not a count
    z = full;
    z.ns = UINT32_MAX;
    CHECK(decode(z, nullptr) == WSG_EINVAL);
    CHECK(decode(z, &f) == WSG_EINVAL);
    z = full;
    z.ns = 0;
    CHECK(decode(z, nullptr) == WSG_EINVAL);    // frames in no stream
    CHECK(decode(z, &f) == WSG_OK);             // room for frames and no stream: none is found
    CHECK(wsg::args_check_protocol(batch(p[0], nullptr, p[2], z), p[1], p[3], proto(p[4], nullptr, p[5], p[6]), false) ==
          WSG_OK);                              // judged as they are
    z = full;
    z.n = UINT32_MAX;
    CHECK(wsg::args_check_protocol(batch(p[0], nullptr, p[2], z), p[1], p[3], proto(p[4], nullptr, p[5], p[6]), false) ==
          WSG_EINVAL);
    CHECK(wsg::args_frame_streams(p[0], 16, p[1], UINT32_MAX, p[2], 1, p[3], p[4], false) == WSG_EINVAL);
    CHECK(wsg::args_frame_streams(p[0], 16, p[1], 1, p[2], UINT32_MAX, p[3], p[4], false) == WSG_OK);
    CHECK(wsg::args_upgrade_streams(p[0], 16, p[1], UINT32_MAX, p[2], p[3], 16, p[4], p[5], false) == WSG_EINVAL);
    CHECK(wsg::args_utf8_verdicts(p[0], p[1], 1, p[2], UINT32_MAX, p[3], false) == WSG_EINVAL);

    // the role
    detail = "role";
    CHECK(wsg::args_check_protocol(batch(p[0], nullptr, p[2], full), p[1], p[3],
                                   proto(p[4], nullptr, p[5], p[6], WSG_PROTO_CLIENT + 1), false) == WSG_EINVAL);
    const Entry relayed = checked_entry("wsg_relay_validated", false, true, true);
    std::vector<uc*> q = operands(relayed);
    CHECK(checked_call(false, true, true, q, full, false, 1, WSG_PROTO_CLIENT) == WSG_OK);
    CHECK(checked_call(false, true, true, q, full, false, 1, WSG_PROTO_CLIENT + 1) == WSG_EINVAL);

    // the relay's groups, and a kind both replied to and relayed
    detail = "relay";
    const size_t op = 18, gf = 20;   // relay_op, d_group_first among its rows
    CHECK(std::string_view(relayed.rows[op].name) == "relay_op" && std::string_view(relayed.rows[gf].name) == "d_group_first");
    CHECK(checked_call(false, true, true, q, full, false, 2) == WSG_OK);
    CHECK(checked_call(false, true, true, q, full, false, 0) == WSG_EINVAL);            // streams in no group
    CHECK(checked_call(false, true, true, q, none, false, 0) == WSG_OK);
    CHECK(checked_call(false, true, true, q, full, false, UINT32_MAX) == WSG_EINVAL);
    std::vector<uc*> one = q;
    one[gf] = nullptr;                                                                   // no table: one group
    CHECK(checked_call(false, true, true, one, full, false, 1) == WSG_OK);
    CHECK(checked_call(false, true, true, one, full, false, 2) == WSG_EINVAL);
    asked.clear();
    CHECK(checked_call(false, true, true, q, full, true, 2) == WSG_OK);
    CHECK(has(q[gf], 12) && has(q[gf + 3], 24));                                         // (n_groups + 1) * 4 and * 8
    const uint8_t relay_text[5] = {0, WSG_REPLY_SAME, 0, 0, 0};                          // reply_echo replies to text
    const uint8_t relay_close[5] = {0, 0, 0, 0x88, 0};
    q[op] = const_cast<uc*>(relay_text);
    CHECK(checked_call(false, true, true, q, full, false) == WSG_EINVAL);
    std::vector<uc*> qs = operands(checked_entry("wsg_relay_validated_streams", true, true, true));
    CHECK(checked_call(true, true, true, qs, full, false) == WSG_OK);
    qs[19] = const_cast<uc*>(relay_text);                                                // relay_op of the _streams rows
    CHECK(checked_call(true, true, true, qs, full, false) == WSG_EINVAL);
    q[op] = const_cast<uc*>(relay_close);
    CHECK(checked_call(false, true, true, q, full, false) == WSG_OK);

    // the carry: the next wire apart from both sources, the next spans not the spans
    detail = "carry";
    const auto carry = [&](uc* wire, uc* span, uc* fresh, uc* next, uc* next_span, uint32_t ns) {
        return wsg::args_carry_streams(wire, 16, span, ns, nullptr, fresh, 16, nullptr, next, 16, next_span, p[7], false);
    };
    CHECK(carry(p[0], p[1], p[2], p[3], p[4], 1) == WSG_OK);
    CHECK(carry(p[0], p[1], p[2], p[3], p[1], 1) == WSG_EINVAL);
    CHECK(carry(p[0], p[1], p[2], p[3], p[1], 0) == WSG_OK);
    CHECK(carry(p[0], p[1], p[2], p[0], p[4], 1) == WSG_EINVAL);
    CHECK(carry(p[0], p[1], p[2], p[2], p[4], 1) == WSG_EINVAL);
    CHECK(carry(arena, p[1], p[2], arena + 16, p[4], 1) == WSG_OK);     // end to end
    CHECK(wsg::args_carry_streams(arena, 32, p[1], 1, nullptr, p[2], 16, nullptr, arena + 16, 16, p[4], p[7], false) ==
          WSG_EINVAL);

    // wsg_encode_batch of no frame touches one word: nothing looked up; a wire of no capacity is still required
    detail = "encode";
    asked.clear();
    CHECK(wsg::args_encode_batch(p[0], 0, p[1], 16, p[2], true) == WSG_OK);
    CHECK(asked.empty());
    CHECK(wsg::args_encode_batch(p[0], 1, nullptr, 0, p[2], false) == WSG_EINVAL);
    CHECK(wsg::args_encode_batch(p[0], 0, p[1] + 1, 16, p[2], false) == WSG_EINVAL);   // aligned whatever n

    // the fan-outs: keys and wire by k (and m), the wire aligned when given
    detail = "fanout";
    CHECK(wsg::args_fanout_encode(nullptr, 0, nullptr, 0, nullptr, 0, false) == WSG_OK);
    CHECK(wsg::args_fanout_encode(nullptr, 0, nullptr, 0, p[0] + 8, 0, false) == WSG_EINVAL);
    CHECK(wsg::args_fanout_encode_many(p[0], p[1], p[2], 1, nullptr, 0, nullptr, 0, p[5], false) == WSG_OK);
    CHECK(wsg::args_fanout_encode_many(nullptr, nullptr, nullptr, 0, nullptr, 1, nullptr, 0, p[5], false) == WSG_OK);
    CHECK(wsg::args_fanout_encode_many(p[0], p[1], p[2], 1, p[3], 0, p[4] + 8, 0, p[5], false) == WSG_EINVAL);
}

} // namespace

int main()
{
    const std::vector<Entry> all = entries();
    for (const Entry& e : all)
        run(e);
    others();
    std::printf("%zu entry points, %d failures\n", all.size(), failures);
    return failures ? 1 : 0;
}
