// wsg_ctx.h — the context behind include/wsg_capi.h and what its four host
// sources share: wsg_capi.cpp (context, knobs, timing, header helpers),
// wsg_lane.cpp (the resident lane), wsg_capi_device.cpp (the device-resident
// entry points) and wsg_capi_host.cpp (the host-staged ones).  No kernel.
#pragma once

#include <hip/hip_runtime.h>

#include "wsg_internal.h"
#include "wsg_lane_plan.h"

#include <algorithm>
#include <vector>

// Encode scratch (scan partials, piece starts, piece -> frame map); the ctx
// has one for wsg_encode_batch and every pipeline slot its own.
struct wsg_enc_scratch {
    uint64_t* d_scan = nullptr;          // sums | piece sums | prefixes | piece prefixes
    uint64_t scan_cap = 0;               // entries
    uint32_t* d_piece_start = nullptr;   // n + 1 piece starts
    uint64_t piece_start_cap = 0;
    uint32_t* d_piece_frame = nullptr;   // piece -> frame
    uint64_t piece_frame_cap = 0;
};

// The users of one per-context scratch, in the order of their calls: the
// stream of the last of them and an event recorded behind it, so that a call
// on another stream waits for it on the device (scratch_enter / scratch_leave).
struct wsg_scratch_order {
    hipStream_t last = nullptr;
    hipEvent_t done = nullptr;   // timing disabled; made by the first call
    bool recorded = false;
};

// Every knob's default stands here, once; wsg_create overrides them from the
// environment ($WSG_*), once per context and never on a data path.
struct wsg_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    int num_cus = 256;
    int blocks_per_cu = 32;       // encode / fan-out / xor grids
    // k_encode_mask grid: one wave per piece up to 2^31 threads (137 GB of
    // frames), grid-stride beyond.  A grid capped at 1024 blocks/CU dealt C5's
    // 5.2 M pieces five per wave, grid-stride, so resident waves streamed five
    // regions GiB apart: 6.12 vs 5.43 ms for the 16 GiB job (tools/enc_ab.py,
    // round 3); at or under a grid's worth of pieces the two are the same
    int enc_blocks_per_cu = 32768;        // $WSG_ENC_BLOCKS_PER_CU (tests: grid-stride launch shapes)
    // k_encode_mask: pieces per launch (0: all in one); $WSG_ENC_LAUNCH_PIECES (tests: split launches)
    uint64_t enc_launch_pieces = 0;
    uint64_t xor_direct_max = 64 << 10;   // per-call XOR off the lane: kernel on the pinned stage up to this size
    uint64_t seg_bytes = 32ull << 20;     // staged host pipelines: segment of about this many wire bytes ($WSG_STAGE_MB)
    // multi-context splits keep several contexts of one device
    // ($WSG_HOST_MULTI_SHARE=1, one-GPU tests of the split)
    bool multi_share = false;
    // host batches up to this many wire bytes whose buffers are page-locked:
    // the kernels read and write them in place (one launch sequence and one
    // synchronize, no staging copies); $WSG_HOST_DIRECT_MAX
    uint64_t host_direct_max = 4 << 20;   // 1-4 MB batches 1.6-2x faster direct, 16 MB even (profiles/r3/host_direct_sizes.log)
    bool check = false;            // $WSG_CHECK=1: operand ranges validated before every device launch (debug, see in_alloc)
    int dec_blocks_per_cu = 4096;  // k_decode grid cap: one 16 KiB tile per block up to 16 GiB of wire (tools/tune.py, round 2: C2 84.3 vs 85.1 us at 48 blocks/CU, 88.1 at two tiles per block; C3 ragged 0.685 vs 0.705 ms at 256, 0.783 at 48)
                                   // $WSG_DEC_BLOCKS_PER_CU (tests: several tiles per block)
    // k_utf8_scan grid cap (a block takes 4 KiB per pass); $WSG_UTF8_BLOCKS_PER_CU (tests: several passes per block)
    int utf8_blocks_per_cu = 32;
    // k_utf8_wire grid cap (a wave takes one 4 KiB piece per pass and its loads wait for its record: with every
    // piece in a wave of its own C2 / ASCII took 50.2 us, at k_utf8_scan's cap 59.6; tools/validbench.py);
    // $WSG_UTF8_WIRE_BLOCKS_PER_CU (tests: several pieces per wave)
    int utf8_wire_blocks_per_cu = 128;
    int fan_waves_per_cu = 6;    // fan-out period path: waves per CU (tools/c4_ab.py, graph-replayed C4: 6 -> 8.10 us, 4 -> 8.16, 8 -> 8.32)
    // fan-out period path: waves per workgroup (A/B $WSG_FAN_WPB; one-wave
    // workgroups measured best: C4 8.5 us against 9.3 at 4 and 9.0 at 8-16,
    // tools/c4_ab.py with graph-replayed launches; an empty kernel of that
    // grid is 1.65 us either way)
    int fan_wpb = 1;
    uint64_t small_avg = wsg::SMALL_AVG;   // batch encode: k_encode_small when wire_cap <= n * small_avg
    unsigned long long* d_err = nullptr;        // latch of the caller-visible async entry points (wsg_sync)
    // latches of the host-staged pipelines (their own status): [0] the
    // decodes' (read back, re-armed after an error), [1] the encodes' (their
    // capacity is checked on the host, so nothing they latch is read: apart,
    // so that it never disables the decodes' latch read-back)
    unsigned long long* d_err_host = nullptr;
    unsigned long long* h_err_copy = nullptr;   // page-locked: d_err_host after a large in-place decode
    // scratch
    wsg_enc_scratch enc;
    wsg_scratch_order enc_order;   // wsg_encode_batch calls
    // wsg_decode_messages: the plan block (wsg::msg_plan_layout, wsg::rfc_plan_layout behind it) and the gather's piece records
    int assembly = WSG_ASSEMBLY_REFERENCE;   // wsg_set_assembly: the rule of the calls that run the message plan
    uint8_t* d_msg_plan = nullptr;
    uint64_t msg_plan_cap = 0;
    wsg::MsgPiece* d_msg_pieces = nullptr;
    uint64_t msg_pieces_cap = 0;
    // wsg_relay_validated: its plan block (wsg::relay_plan_layout) and the piece records of its gather, under msg_order
    uint8_t* d_relay_plan = nullptr;
    uint64_t relay_plan_cap = 0;
    wsg::MsgPiece* d_relay_pieces = nullptr;
    uint64_t relay_pieces_cap = 0;
    wsg_scratch_order msg_order;   // wsg_decode_messages calls
    // wsg_frame_streams: per-stream counts and scan partials (wsg::frame_plan_layout); wsg_upgrade_streams and
    // wsg_carry_streams: their plans (wsg::upgrade_plan_layout, wsg::carry_plan_layout) in the same array, under the
    // same order
    uint64_t* d_frame_plan = nullptr;
    uint64_t frame_plan_cap = 0;
    wsg_scratch_order frame_order;   // wsg_frame_streams calls
    // wsg_check_protocol: the frames' streams, scan partials, per-stream states (wsg::proto_plan_layout)
    uint8_t* d_proto_plan = nullptr;
    uint64_t proto_plan_cap = 0;
    wsg_scratch_order proto_order;   // wsg_check_protocol calls
    // staging of the per-call XOR (wsg_xor_host)
    uint8_t* d_stage = nullptr;
    uint64_t d_stage_cap = 0;
    uint8_t* h_stage = nullptr;
    uint64_t h_stage_cap = 0;
    // pipelined host paths (wsg_decode_batch_host, wsg_encode_batch_host): staging per slot
    struct Slot {
        // carries no work; kept, and made before the role streams: without it
        // (or made after them) bench.py --full read the page-locked staged
        // legs 38.7 / 37.9 against 39.7 / 39.8 GiB/s (profiles/r14)
        hipStream_t stream = nullptr;
        hipEvent_t done = nullptr;       // the segment's last copy back has finished
        hipEvent_t h2d_done = nullptr;   // inputs are in HBM
        hipEvent_t k_done = nullptr;     // kernels have finished
        uint8_t* d_wire = nullptr;       // segment, decoded in place
        uint64_t wire_cap = 0;
        uint8_t* h_in = nullptr;         // pinned staging for pageable callers
        uint64_t h_in_cap = 0;
        uint8_t* h_out = nullptr;
        uint64_t h_out_cap = 0;
        uint64_t* h_fs = nullptr;        // rebased frame starts (pinned)
        uint64_t h_fs_cap = 0;
        wsg_recv_info* h_info = nullptr; // info staging (pinned)
        uint64_t h_info_cap = 0;
        uint64_t* d_fs = nullptr;
        uint64_t d_fs_cap = 0;
        wsg_recv_info* d_info = nullptr;
        uint64_t d_info_cap = 0;
        // encode (wsg_encode_batch_host): payload in, frames out in d_wire
        uint8_t* d_payload = nullptr;
        uint64_t payload_cap = 0;
        wsg_send_desc* d_desc = nullptr;
        uint64_t desc_cap = 0;
        wsg_send_desc* h_desc = nullptr;  // rebased descriptors (pinned)
        uint64_t h_desc_cap = 0;
        uint64_t* d_woff = nullptr;
        uint64_t woff_cap = 0;
        wsg_enc_scratch enc;
        // work to finish on the host once `done` has fired
        bool busy = false;
        uint8_t* out_dst = nullptr;      // pageable destination of h_out (null: DMA'd directly)
        uint64_t out_len = 0;
        wsg_recv_info* info_dst = nullptr;
        uint32_t info_n = 0;
        uint64_t base = 0;               // wire offset of the segment's first byte
    };
    static constexpr int kSlots = 3;
    Slot slots[kSlots];
    // role streams of the host pipelines: every H2D copy on one stream, every
    // kernel on another, every D2H copy on a third, so the two copy directions
    // run concurrently while kernels run between them
    hipStream_t s_h2d = nullptr, s_kern = nullptr, s_d2h = nullptr;
    // the host lane (wsg_internal.h): page-locked host batches of at most
    // lane_max wire bytes (and per-call XORs of at most that many bytes) go to
    // the device's resident lane, shared by every context of the process,
    // through its mailboxes instead of a launch + synchronize ($WSG_LANE_MAX,
    // 0 = never: the launch paths only; tools/lane_ab.py sweep)
    struct LaneServer* lane = nullptr;   // the device's (made on first use)
    uint64_t lane_max = 512 << 10;
    uint32_t lane_groups = wsg::LANE_GROUPS_MAX;   // most frame groups of one request ($WSG_LANE_GROUPS)
    uint64_t lane_requests = 0;          // requests this context put on the lane (wsg_lane_stats)
    bool dead = false;                   // a lane request neither answered nor drained: buffers may still be written
    // timing of the dominant kernel
    struct EvPair {
        hipEvent_t a, b;
    };
    int timing = 0;            // 0 off; k > 0: time every k-th dominant-kernel launch
    uint64_t timing_seq = 0;
    std::vector<EvPair> pending, pool;
    double acc_ms = 0.0;
    uint64_t launches = 0;
    double min_ms = 0.0, max_ms = 0.0;   // extremes of the launches since the last reset
};

#define WSG_HIP(expr)                                                                                        \
    do {                                                                                                     \
        if ((expr) != hipSuccess)                                                                            \
            return WSG_EHIP;                                                                                 \
    } while (0)

// Everything below is the library's own: none of it is exported.
#pragma GCC visibility push(hidden)

#include "wsg_args.h"   // the entry points' argument checks (declares in_alloc)

constexpr unsigned long long kNoError = ~0ull;

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
// The `stream` argument of an entry point: NULL selects HIP's default (null)
// stream, as in every HIP API.
inline hipStream_t as_stream(void* s) { return static_cast<hipStream_t>(s); }
inline uint64_t ceil_div(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

inline int grid_for(const wsg_ctx* c, uint64_t tiles, int blocks_per_cu = 0)
{
    const uint64_t cap = uint64_t(c->num_cus) * uint64_t(blocks_per_cu ? blocks_per_cu : c->blocks_per_cu);
    return int(std::max<uint64_t>(1, std::min(tiles, cap)));
}

// grow a device array of T to at least `want` entries
template <class T>
int ensure_array(T*& ptr, uint64_t& cap, uint64_t want)
{
    want = std::max<uint64_t>(want, 1);
    if (want <= cap)
        return WSG_OK;
    WSG_HIP(hipDeviceSynchronize());
    if (ptr)
        WSG_HIP(hipFree(ptr));
    ptr = nullptr;
    cap = 0;
    if (hipMalloc(&ptr, want * sizeof(T)) != hipSuccess)
        return WSG_ENOMEM;
    cap = want;
    return WSG_OK;
}

// ... and a page-locked host array (flags: hipHostMalloc's), whose users have
// drained before it grows
template <class T>
int ensure_pinned(T*& ptr, uint64_t& cap, uint64_t want, unsigned flags)
{
    want = std::max<uint64_t>(want, 1);
    if (want <= cap)
        return WSG_OK;
    if (ptr)
        (void)hipHostFree(ptr);
    ptr = nullptr;
    cap = 0;
    if (hipHostMalloc(&ptr, want * sizeof(T), flags) != hipSuccess)
        return WSG_ENOMEM;
    cap = want;
    return WSG_OK;
}

// Record the start event of a timed kernel; returns the pair index or -1.
inline int timing_begin(wsg_ctx* c, hipStream_t s)
{
    if (c->timing <= 0 || (c->timing_seq++ % uint64_t(c->timing)) != 0)
        return -1;
    wsg_ctx::EvPair ev;
    if (!c->pool.empty()) {
        ev = c->pool.back();
        c->pool.pop_back();
    } else {
        if (hipEventCreate(&ev.a) != hipSuccess || hipEventCreate(&ev.b) != hipSuccess)
            return -1;
    }
    (void)hipEventRecord(ev.a, s);
    c->pending.push_back(ev);
    return int(c->pending.size()) - 1;
}

inline void timing_end(wsg_ctx* c, hipStream_t s, int idx)
{
    if (idx >= 0)
        (void)hipEventRecord(c->pending[size_t(idx)].b, s);
}

// ---- wsg_capi.cpp ------------------------------------------------------------
// Before a call on `s` touches the scratch `o` orders: wait on the device for
// the last call that used it if that ran on another stream (no host
// synchronisation).  *ordered = false while `s` is capturing: a captured call
// neither waits nor records (the event would become a node of the graph, and a
// wait on an event recorded outside the capture is not capturable).
int scratch_enter(wsg_scratch_order& o, hipStream_t s, bool* ordered);
// Behind the call's last launch on `s`.
int scratch_leave(wsg_scratch_order& o, hipStream_t s, bool ordered);
void free_enc(wsg_enc_scratch& e);
// in_alloc (declared in wsg_args.h, whose rows ask it).  Checked launches
// ($WSG_CHECK=1, a debug mode): [p, p + bytes) must lie in ONE device
// allocation (hipMemGetAddressRange), which every access of the kernel to that
// operand stays inside when the sizes passed are right.  GPU address
// sanitizers are not available on the target pool; this catches a short
// buffer or a wrong size on the host, before the kernel runs.

// ---- wsg_capi_device.cpp -----------------------------------------------------
// Device decode: one k_decode launch (the pipelined host path runs several
// of these concurrently, one per slot).
int decode_launch(wsg_ctx* c, const uint8_t* d_wire, uint64_t wire_len, const uint64_t* d_frame_start, uint32_t n,
                  uint8_t* d_out, wsg_recv_info* d_info, hipStream_t s, unsigned long long* err);
// scratch for either encode path (the piece map only for the piece kernel;
// for both when c is null)
int ensure_enc(const wsg_ctx* c, wsg_enc_scratch& e, uint32_t n, uint64_t wire_cap);
int encode_launch(wsg_ctx* c, hipStream_t s, const uint8_t* d_payload, const wsg_send_desc* d_desc, uint32_t n,
                  uint8_t* d_wire, uint64_t wire_cap, uint64_t* d_wire_off, wsg_enc_scratch& e,
                  unsigned long long* err);

// ---- wsg_capi_host.cpp -------------------------------------------------------
// [p, p + bytes) lies in a block wsg_host_alloc made (no runtime query).
bool in_host_block(const void* p, uint64_t bytes = 1);
bool host_pinned(const void* p);
// Page-locked AND mapped at the same address on the device, so a kernel may
// take the host pointer as it is (hipHostMalloc memory).  Memory registered
// with hipHostRegister can have another device address; such buffers take
// the staged pipeline (hipMemcpyAsync handles any host pointer).
bool host_direct(const void* p);
// Everything slot_reserve / slot_reserve_enc gave a slot (wsg_destroy).
void slot_free(wsg_ctx::Slot& sl);

// ---- wsg_lane.cpp: the host lane (wsg_internal.h) ----------------------------
// The lane for this context's request, or nullptr (lane off for the context,
// the lane given up, or it cannot be made).
LaneServer* lane_for(wsg_ctx* c);
// The groups a request asks lane_plan for: about as many as the lane has idle
// workgroups (W shared among the requests in flight), at most the context's
// lane_groups.
uint32_t lane_want(const wsg_ctx* c, const LaneServer* s);

// One group's task words (w[LANE_WORDS]); lo, hi of an encode: the payload
// span of the group's frames.
void lane_task_decode(uint64_t* w, uint32_t n, const uint8_t* wire, uint64_t wire_len, const uint64_t* frame_start,
                      uint8_t* out, wsg_recv_info* info, const LaneGroup& g);
void lane_task_encode(uint64_t* w, uint32_t n, const uint8_t* payload, const wsg_send_desc* desc,
                      const uint64_t* wire_off, uint8_t* wire, const LaneGroup& g, uint64_t lo, uint64_t hi);
// inline_src: the payload of at most LANE_INLINE bytes travels in the task
// (null: `stage` is XORed in place)
void lane_task_xor(uint64_t* w, uint8_t* stage, uint64_t len, uint32_t key, uint32_t phase, const void* inline_src);

enum LaneResult { LANE_DONE = 0, LANE_FALLBACK = 1, LANE_LOST = 2 };

// Post a request's groups (task words words[k], w[0] = op | n << 32) and wait
// for every answer.  LANE_DONE: answered (*errs: the frames with an error).
// LANE_FALLBACK: not done by the lane, which has left: the caller does the
// request on the launch path (*answered: groups the lane did finish before it
// was given up — their outputs are written).  LANE_LOST: given up and the lane
// did not leave in time: it may still write the request's buffers, so the
// caller must not reuse them (the context is marked dead).
// xwords > 0: one inline-XOR task, answered by its self-tagged units
// (wsg::LaneXres), whose dwords go to xout.
LaneResult lane_run(wsg_ctx* c, LaneServer* s, const uint64_t (*words)[wsg::LANE_WORDS], uint32_t groups,
                    uint64_t* errs, uint32_t* answered, uint32_t xwords = 0, uint32_t* xout = nullptr);

#pragma GCC visibility pop
