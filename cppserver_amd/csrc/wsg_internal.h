// wsg_internal.h — kernel geometry and kernel declarations shared by the
// kernel sources (wsg_decode.hip, wsg_encode.hip, wsg_fanout.hip,
// wsg_lane_device.hip, wsg_misc.hip, wsg_messages.hip, wsg_frames.hip,
// wsg_utf8.hip, wsg_proto.hip, wsg_assembly.hip, wsg_upgrade.hip, wsg_upgrade_client.hip, wsg_carry.hip, wsg_relay.hip) and the C-ABI implementation (wsg_ctx.h).
// The launchers take the operand groups of wsg_operands.h by const reference
// and unpack them at the <<<>>> call: no kernel sees a group.
#pragma once

#include "wsg_frame.h"
#include "wsg_lane_plan.h"   // LANE_THREADS, LANE_GROUPS_MAX
#include "wsg_operands.h"    // the operand groups the launchers take: Batch, MsgOut, ReplyOut, ProtoOps, ...

namespace wsg {

constexpr int BLOCK = 256;                  // 4 wave64s
constexpr int CHUNK = 16;                   // bytes per lane per step (dwordx4)
#ifndef WSG_UNROLL
#define WSG_UNROLL 4
#endif
constexpr int UNROLL = WSG_UNROLL;          // steps per lane per tile
constexpr uint64_t TILE = uint64_t(BLOCK) * CHUNK * UNROLL;   // 16 KiB of output
#ifndef WSG_EU
#define WSG_EU 4
#endif
constexpr int EU = WSG_EU;                              // encode: 16-B steps per lane per piece
constexpr uint64_t PIECE = uint64_t(64) * CHUNK * EU;   // encode work piece: 4 KiB of one frame
// Pieces start on 128-byte line boundaries of the OUTPUT, so every 1 KiB
// store row of a wave writes whole lines (a 16-B-aligned but line-misaligned
// streaming store costs 6-16 %: tools/membench.hip explore, delta 16/80).
constexpr uint64_t PIECE_ALIGN = 128;
#ifndef WSG_FAN_UNITS
#define WSG_FAN_UNITS 4
#endif
constexpr int FAN_UNITS = WSG_FAN_UNITS;                 // fan-out: 16-B chunks per lane per pass
constexpr uint32_t SMALL_F = BLOCK;                      // small-frame encode: most frames per block
                                                         // (512/1024 measured 10-40 % slower)
#ifndef WSG_SMALL_AVG
#define WSG_SMALL_AVG 4096
#endif
constexpr uint64_t SMALL_AVG = WSG_SMALL_AVG;            // ... used when wire_cap <= n * SMALL_AVG
#ifndef WSG_SMALL_RANGE
#define WSG_SMALL_RANGE 32768
#endif
constexpr uint64_t SMALL_RANGE = WSG_SMALL_RANGE;        // ... wire bytes per block (sets frames per block)
#ifndef WSG_SCAN_PER_LANE
#define WSG_SCAN_PER_LANE 4
#endif
constexpr int SCAN_PER_LANE = WSG_SCAN_PER_LANE;   // encode scan: frames per lane
constexpr uint64_t SCAN_ITEMS = uint64_t(BLOCK) * SCAN_PER_LANE;   // frames per scan block

// Host launchers, each defined next to its kernels in the source its section names.
// ---- one-launch decode (wsg_decode_batch; wsg_decode.hip) -------------------
// k_decode: grid blocks over the wire's tiles, per-frame info and the error
// latch from the same launch.
hipError_t launch_decode(hipStream_t s, int grid, const uint8_t* wire, uint8_t* out, uint64_t wire_len,
                         const uint64_t* fs, uint32_t n, wsg_recv_info* info, unsigned long long* err);

// ---- batch encode (wsg_encode_batch; wsg_encode.hip) ------------------------
// Sizes + piece counts scan (scan: 4 * ceil(n / SCAN_ITEMS) words), wire
// offsets, piece starts (n + 1 each) and the piece -> frame map.
hipError_t launch_encode_scan(hipStream_t s, const wsg_send_desc* desc, uint32_t n, uint64_t* wire_off,
                              uint32_t* piece_start, uint64_t* scan, uint32_t* piece_frame, uint64_t pieces_cap,
                              uint64_t wire_cap, unsigned long long* err);
hipError_t launch_encode_mask(hipStream_t s, int grid, const uint8_t* payload, const wsg_send_desc* desc, uint32_t n,
                              const uint64_t* wire_off, const uint32_t* piece_start, const uint32_t* piece_frame,
                              uint8_t* wire, uint64_t wire_cap, uint32_t q_begin, uint32_t q_end);
// Small-frame batch encode: block-local sizes scan (scan: ceil(n /
// SCAN_ITEMS) block totals), then k_encode_small, which adds the block
// prefixes, writes the final wire_off[0..n] and latches capacity errors.
hipError_t launch_encode_scan_small(hipStream_t s, const wsg_send_desc* desc, uint32_t n, uint64_t* wire_off,
                                    uint64_t* scan);
hipError_t launch_encode_small(hipStream_t s, const uint8_t* payload, const wsg_send_desc* desc, uint32_t n,
                               uint64_t* wire_off, const uint64_t* scan, uint8_t* wire, uint64_t wire_cap,
                               unsigned long long* err);

// ---- message assembly (wsg_decode_messages; wsg_messages.hip) ---------------
// Plan scratch of one call, carved by the host out of one device block
// (msg_plan_layout): per-frame scan results, per-block partials (one block =
// BLOCK frames), the totals.
struct MsgPlan {
    uint64_t* dst;        // n: offset in d_msg of each frame's payload (delivered bytes before it)
    uint64_t* bbytes;     // nb: block sums of delivered bytes, then their exclusive prefixes
    uint64_t* bbytes_pre;
    uint64_t* bpc;        // nb: block sums of pieces, then their exclusive prefixes
    uint64_t* bpc_pre;
    uint64_t* tot;        // [0] FIN frames, [1] last FIN frame + 1, [2] delivered bytes, [3] pieces
    // per frame, block-local: the batch-wide value is the entry combined with
    // its block's prefix (the kernels never rewrite an entry in place, so a
    // lane may read any frame's while others run)
    uint32_t* finx;       // n: FIN frames before frame i
    uint32_t* pinc;       // n: 1 + last frame <= i that heads a stream or names an opcode (0: none)
    uint32_t* qx;         // n: 1 + last FIN frame < i (0: none)
    uint32_t* sidx;       // n: the frame's stream
    uint32_t* pstart;     // n: pieces before frame i
    uint32_t* bfin;       // nb each: block partials and their exclusive prefixes
    uint32_t* bfin_pre;
    uint32_t* bp;
    uint32_t* bp_pre;
    uint32_t* bq;
    uint32_t* bq_pre;
    // wsg_reply_messages only
    uint64_t* rex;        // n: block-local reply bytes of the FIN frames before frame i
    uint64_t* brep;       // nb: block sums of reply bytes, then their exclusive prefixes
    uint64_t* brep_pre;
    uint64_t* brn;        // nb: block sums of reply frames
    uint64_t* rtot;       // tot as the gather of a reply reads it: [2] reply bytes, [3] pieces
};
// Bytes of that block for n frames; plan (or null) gets the pointers into base.
uint64_t msg_plan_layout(uint8_t* base, uint32_t n, MsgPlan* plan);
// What WSG_ASSEMBLY_RFC adds to that scratch (wsg_assembly.hip), behind the
// MsgPlan block.  A frame is of class D (a data frame: opcode 0-7, no error),
// DF (D with FIN), C (a FIN control frame without error) or of none, and H
// when it heads a stream; a run is the D frames from the first one behind a DF
// frame or at or behind a stream's head to the next DF frame of that stream.
// The frames' kernels know the streams through H alone, so every frame of a
// run derives the same run from the same scans.  They share MsgPlan's sidx,
// rex, brep*, brn, tot ([0] messages, [2] delivered bytes, [3] pieces) and
// rtot with the reply kernels and the gather.
struct RfcPlan {
    // per frame, block-local (the batch-wide value: combined with the block's prefix)
    uint32_t* cnt;        // n: frames before i of class D | DF << 8 | C << 16 | H << 24
    uint32_t* qd;         // n: 1 + last DF frame < i (0: none)
    uint32_t* hq;         // n: 1 + last H frame <= i (0: none)
    uint32_t* pop;        // n: 1 + last D frame <= i that names an opcode (0: none)
    uint32_t* ex;         // n: message-ending frames delivered before i
    uint64_t* ab;         // n: delivered payload bytes before i
    uint64_t* cb;         // n: ... of control frames
    uint64_t* pc;         // n: pieces of the delivered frames before i | of the control frames among them << 32
    // per frame, batch-wide
    uint32_t* ff;         // n: a C frame inside a run, a DF frame: the run's first frame; else i
    uint32_t* eo;         // n: the frame that ends frame i's message (i itself for a C frame); UINT32_MAX: not delivered
    // nb each: block partials and their exclusive prefixes
    uint32_t* bD;
    uint32_t* bD_pre;
    uint32_t* bDF;
    uint32_t* bDF_pre;
    uint32_t* bC;
    uint32_t* bC_pre;
    uint32_t* bH;
    uint32_t* bH_pre;
    uint32_t* bqd;
    uint32_t* bqd_pre;
    uint32_t* bhq;
    uint32_t* bhq_pre;
    uint32_t* bpop;
    uint32_t* bpop_pre;
    uint32_t* bex;
    uint32_t* bex_pre;
    uint64_t* bab;
    uint64_t* bab_pre;
    uint64_t* bcb;
    uint64_t* bcb_pre;
    uint64_t* bpc;
    uint64_t* bpc_pre;
    uint64_t* tot;        // [0] D frames, [1] DF frames, [2] C frames, [3] H frames, [4] last DF frame + 1
};
uint64_t rfc_plan_layout(uint8_t* base, uint32_t n, RfcPlan* plan);
// Both plans of one call and the rule that picks between them (the context's
// mode, read on the host when the call is made).
struct MsgPlans {
    MsgPlan ref;
    RfcPlan rfc;
    int assembly;         // WSG_ASSEMBLY_*
};
// One work piece of the gather, everything its wave needs in one 32-byte
// scalar load (a piece -> frame map as the encode's put three dependent
// loads between a wave's start and its first data load).
struct alignas(32) MsgPiece {
    uint64_t poff;   // wire offset of the frame's payload
    uint64_t d0;     // offset in d_msg of the payload's first byte
    uint64_t len;    // payload bytes
    uint32_t key;
    uint32_t k;      // piece of the frame: [A + k * PIECE, A + (k + 1) * PIECE) of d_msg, A = d0 & ~(PIECE_ALIGN - 1)
};
// The scratch of a call that runs the message plan, and its error latch: what
// the entry points' msg_scratch() fills.
struct MsgScratch {
    MsgPlans plans;
    MsgPiece* pieces;
    uint64_t pieces_cap;
    unsigned long long* err;
};
// The plan pass: d_info, d_msgs, d_count, d_state, the plan and the piece
// records (pieces_cap entries); latches frame errors and WSG_ENOMEM.
// state null (wsg_check_utf8_wire, with msg_cap UINT64_MAX): d_state is only
// read, as `seed` (the sticky opcodes), and k_msg_state is left out; else seed is state.
hipError_t launch_msg_plan(hipStream_t s, const Batch& b, wsg_stream_state* state, const wsg_stream_state* seed,
                           uint64_t msg_cap, const MsgOut& o, const MsgScratch& x);
// The gather pass over piece records, a wave per piece: every payload byte of
// the pieces below tot[3] to its place in dst.  tot: MsgPlan::tot (the
// delivered payloads, unmasked, to d_msg), MsgPlan::rtot (a reply's, re-keyed,
// to the reply wire) or RelayPlan::gtot (the relayed ones, unmasked, to d_relay).
hipError_t launch_gather(hipStream_t s, int grid, const uint8_t* wire, const uint64_t* tot, const MsgPiece* pieces,
                         uint64_t pieces_cap, uint8_t* dst, uint64_t dst_cap);

// ---- replies (wsg_reply_messages; wsg_messages.hip) -------------------------
// The plan pass of a reply: launch_msg_plan's outputs but the d_msg layout's
// capacity check, and d_reply_off, d_stream_reply, d_count[2..3], every reply
// frame's header and status prefix, and piece records whose destination is
// the reply wire; latches frame errors and WSG_ENOMEM (reply_cap).
hipError_t launch_reply_plan(hipStream_t s, const Batch& b, wsg_stream_state* state, const ReplyOut& r,
                             const MsgOut& o, const MsgScratch& x);
// wsg_reply_checked's plan pass: launch_reply_plan with the protocol kernels
// (launch_proto_* below, d_state's consumed written ahead of them) and the
// merge with `also` (or null) between the message plan and the reply kernels,
// whose checked instantiations stop every stream's replies at its terminal
// frame and put its close frame there; d_close_off, d_verdict, d_proto,
// d_result and d_count[0..5) besides launch_reply_plan's outputs.
// stream_grid: blocks of the per-stream kernels (grid-stride).
// utf8 (wsg_reply_validated, or null): Utf8Inside of wsg_operands.h.
struct ProtoPlan;
hipError_t launch_reply_checked_plan(hipStream_t s, int stream_grid, const Batch& b, wsg_stream_state* state,
                                     const ProtoOps& p, const ProtoPlan& pplan, const ReplyOut& r, const MsgOut& o,
                                     const MsgScratch& x, const Utf8Inside* utf8 = nullptr);

// ---- relays (wsg_relay_validated; wsg_relay.hip) -----------------------------
// Scratch of one call, carved by the host out of one device block
// (relay_plan_layout; one block = BLOCK messages, frames or positions).
struct RelayPlan {
    // per message m (the first d_count[0] of n), block-local
    uint64_t* mex;      // n: relay bytes of the messages before m
    // per frame i, block-local but fmsg
    uint64_t* fex;      // n: data bytes of the relayed frames before i (under WSG_ASSEMBLY_RFC: of data frames)
    uint32_t* fpc;      // n: pieces of the relayed frames before i
    uint32_t* fmsg;     // n: the relayed message whose data frame i holds (UINT32_MAX: none)
    // per position p, block-local
    uint64_t* pex;      // ns: relay bytes of the streams at the positions before p
    // per stream j
    uint32_t* mfirst;   // ns: its first message and one past its last (both 0: none)
    uint32_t* mend;
    uint32_t* inv;      // ns: the lowest position that names j (UINT32_MAX: none)
    // block partials and their exclusive prefixes
    uint64_t* bm;       // nb: relay bytes
    uint64_t* bm_pre;
    uint64_t* bn;       // nb: relay frames
    uint64_t* bw;       // nb: data bytes
    uint64_t* bw_pre;
    uint64_t* bp;       // nb: pieces
    uint64_t* bp_pre;
    uint64_t* bs;       // nbs: relay bytes by position
    uint64_t* bs_pre;
    uint64_t* tot;      // [0] relay bytes, [1] relay frames, [2] pieces, whatever the tables hold
    uint64_t* gtot;     // [0] the tables keep their rules; as the gather reads it: [2] relay bytes, [3] pieces
    uint64_t* bad;      // the lowest offending position (n_streams + g: entry g of d_group_first); UINT64_MAX: none
};
// Bytes of that block for n frames in ns streams; plan (or null) gets the pointers into base.
uint64_t relay_plan_layout(uint8_t* base, uint32_t n, uint32_t ns, RelayPlan* plan);
// Behind launch_reply_checked_plan (d_info, d_msgs, d_verdict and plans.ref.tot
// final): d_relay_off, d_group_relay, d_count[5..8), every relay frame's header
// and status prefix and the piece records of the relayed frames, whose
// destination is d_relay and whose key is the receive key; latches WSG_EINVAL
// (order, group_first; index n + 1 + the plan's `bad`) and WSG_ENOMEM
// (relay_cap; index n + 1).  A relay frame is unmasked: the kernels size it by relay.relay_op and
// no mask.  x: the message plan's as it stands, with the relay's own piece records.
hipError_t launch_relay_plan(hipStream_t s, const Batch& b, const MsgOut& o, const wsg_proto_verdict* verdict,
                             const RelayArgs& relay, const RelayPlan& Q, const MsgScratch& x);

// ---- WSG_ASSEMBLY_RFC (wsg_set_assembly; wsg_assembly.hip) ------------------
// The plan kernels of RFC 6455 5.4's rule, in the places the launchers of
// wsg_messages.hip run the reference rule's (n > 0 but for launch_rfc_state).
// The four scan kernels: d_info and the error latch, P.sidx, R, P.tot,
// d_count[0..1], WSG_ENOMEM (msg_cap); d_state[j].ahead is read.
hipError_t launch_rfc_scans(hipStream_t s, const Batch& b, const wsg_stream_state* state, uint64_t msg_cap,
                            const MsgOut& o, const MsgScratch& x);
// k_msg_finalize's part: d_msgs and the gather's piece records, in dense order.
hipError_t launch_rfc_finalize(hipStream_t s, const Batch& b, const MsgOut& o, const MsgScratch& x);
// k_msg_state's part (consumed, opcode 0, ahead), or k_msg_consumed's (consumed alone); n == 0 allowed.
hipError_t launch_rfc_state(hipStream_t s, uint32_t n, const uint32_t* stream_first, uint32_t n_streams,
                            wsg_stream_state* state, const RfcPlan& R, bool consumed_only);
// k_reply_local's and k_reply_finalize's parts, around k_reply_blocks
// (verdict: d_verdict as words when checked, null and r.close_off null otherwise).
hipError_t launch_rfc_reply_local(hipStream_t s, bool checked, const Batch& b, const MsgOut& o, const MsgScratch& x,
                                  const ReplyRule& rule, const uint64_t* verdict);
hipError_t launch_rfc_reply_finalize(hipStream_t s, bool checked, const Batch& b, const MsgOut& o, const MsgScratch& x,
                                     const ReplyOut& r, const ReplyRule& rule, const uint64_t* verdict);

// ---- the device framer (wsg_frame_streams; wsg_frames.hip) -----------------
// Scratch of one call, carved out of one device array of uint64 (one block =
// BLOCK streams).
struct FramePlan {
    uint64_t* cnt;     // ns: whole frames of each stream (k_frame_count)
    uint64_t* ex;      // ns: block-local exclusive prefix of cnt
    uint64_t* bcnt;    // nb: block sums of cnt
    uint64_t* bpre;    // nb: their exclusive prefixes
    uint64_t* bcons;   // nb: block sums of the spans' consumed bytes
    uint64_t* tot;     // [0] frames found, [1] bytes consumed
};
// Entries of that array for ns streams; plan (or null) gets the pointers into base.
uint64_t frame_plan_layout(uint64_t* base, uint32_t ns, FramePlan* plan);
// Count walk, scan, write walk: the spans' consumed / need, stream_first
// (ns + 1), count, and, when they fit, the frame_start entries; latches span
// and capacity errors.  grid: blocks of the two walks (one wave per stream,
// grid-stride).
hipError_t launch_frame_streams(hipStream_t s, int grid, const uint8_t* wire, uint64_t wire_len, wsg_stream_span* span,
                                uint32_t ns, uint64_t* frame_start, uint32_t frame_cap, uint32_t* stream_first,
                                uint64_t* count, const FramePlan& plan, unsigned long long* err);
// wsg_decode_streams: every span's consumed lowered to the start of the
// stream's first frame that wsg_decode_messages left in the tail.
hipError_t launch_frame_tail(hipStream_t s, wsg_stream_span* span, uint32_t ns, const uint64_t* frame_start,
                             const uint32_t* stream_first, const wsg_stream_state* state, uint32_t n);

// ---- the upgrade handshake (wsg_upgrade_streams; wsg_upgrade.hip) -----------
// Scratch of one call, carved out of the framer's device array (one block =
// BLOCK streams).
struct UpgradePlan {
    uint64_t* ex;       // ns: block-local exclusive prefix of the streams' response bytes
    uint64_t* bsum;     // 4 * nb: block sums of response bytes, accepted, rejected, incomplete streams
    uint64_t* bpre;     // nb: exclusive prefixes of the first of those
    uint64_t* tot;      // [0] response bytes
    uint32_t* accept;   // 8 * ns: each accepted stream's 28 accept bytes
};
uint64_t upgrade_plan_layout(uint64_t* base, uint32_t ns, UpgradePlan* plan);
// Parse (one wave per stream, grid-stride over `grid` blocks), scan, accept
// values, responses: d_up, the spans' consumed / need, resp_off (ns + 1),
// count (4) and, when they fit, the responses; latches span and capacity errors.
hipError_t launch_upgrade_streams(hipStream_t s, int grid, const uint8_t* wire, uint64_t wire_len,
                                  wsg_stream_span* span, uint32_t ns, uint64_t max_request, wsg_upgrade* up,
                                  uint8_t* resp, uint64_t resp_cap, uint64_t* resp_off, uint64_t* count,
                                  const UpgradePlan& plan, unsigned long long* err);

// ---- the client's upgrade (wsg_upgrade_client_streams; wsg_upgrade_client.hip) ----
// Scratch of one call, carved out of the framer's device array (one block =
// BLOCK streams).
struct UpClientPlan {
    uint32_t* digest;   // 8 * ns: each stream's 20 expected digest bytes, in memory order, and 12 of zero
    uint64_t* bsum;     // 3 * nb: block sums of accepted, whole but not accepted, incomplete streams
};
uint64_t upclient_plan_layout(uint64_t* base, uint32_t ns, UpClientPlan* plan);
// Digests (one lane per stream), parse (one wave per stream, grid-stride over
// `grid` blocks), counts: d_up, the spans' consumed / need, count (3); latches
// span errors.
hipError_t launch_upgrade_client_streams(hipStream_t s, int grid, const uint8_t* wire, uint64_t wire_len,
                                         wsg_stream_span* span, uint32_t ns, const uint8_t* nonce,
                                         uint64_t max_response, wsg_upgrade_reply* up, uint64_t* count,
                                         const UpClientPlan& plan, unsigned long long* err);
// k_upgrade_requests (total = n * tpl_len > 0): every byte of req below total,
// a 16-byte block per lane, grid-stride over `grid` blocks.
hipError_t launch_upgrade_requests(hipStream_t s, int grid, const uint8_t* tpl, uint32_t tpl_len, uint32_t key_at,
                                   const uint8_t* nonce, uint8_t* req, uint64_t total);

// ---- the carry between two rounds (wsg_carry_streams; wsg_carry.hip) --------
// Scratch of one call, carved out of the framer's device array (one block =
// BLOCK streams).
struct CarryPlan {
    uint64_t* tsrc;    // ns: wire offset of the stream's tail
    uint64_t* tlen;    // ns: its bytes
    uint64_t* nsrc;    // ns: offset in d_new of the stream's read
    uint64_t* nlen;    // ns: its bytes
    uint64_t* ex;      // ns: block-local exclusive prefix of the streams' padded sizes
    uint64_t* off;     // ns + 1: the streams' offsets in d_next; [ns] its bytes used
    uint64_t* bsum;    // 4 * nb: block sums of padded sizes, tail bytes, read bytes, dropped streams
    uint64_t* bpre;    // nb: exclusive prefixes of the first of those
};
uint64_t carry_plan_layout(uint64_t* base, uint32_t ns, CarryPlan* plan);
// Sizes, scan, offsets: next_span (ns), count (4), the plan's runs; latches
// the streams' errors and the capacity.
hipError_t launch_carry_plan(hipStream_t s, uint64_t wire_len, const wsg_stream_span* span, uint32_t ns,
                             const uint64_t* close_off, uint64_t new_len, const wsg_stream_read* read, uint64_t next_cap,
                             wsg_stream_span* next_span, uint64_t* count, const CarryPlan& plan, unsigned long long* err);
// k_carry_copy (ns > 0): every chunk of next below the plan's total, when that
// fits next_cap; grid blocks of four waves, a PIECE per wave and pass.
hipError_t launch_carry_copy(hipStream_t s, int grid, const uint8_t* wire, const uint8_t* fresh, uint32_t ns,
                             const CarryPlan& plan, uint8_t* next, uint64_t next_cap);

// ---- UTF-8 on the device (wsg_check_utf8; wsg_utf8.hip) ---------------------
// k_utf8_init: d_valid[m] = len for m < min(d_count[0], msg_room), and
// d_result = {0, UINT64_MAX, 0, 0} (grid >= 1 also when msg_room == 0).
hipError_t launch_utf8_init(hipStream_t s, int grid, const wsg_msg* msgs, const uint64_t* count, uint32_t msg_room,
                            uint64_t* valid, uint64_t* result);
// The payload kernel: every 16-byte chunk of d_msg below min(msg_cap,
// d_count[1]) once, grid-stride (a block takes BLOCK chunks, 4 KiB, per pass);
// the lowest bad position of a checked message into d_valid by atomicMin.
hipError_t launch_utf8_scan(hipStream_t s, int grid, const uint8_t* msg, uint64_t msg_cap, const wsg_msg* msgs,
                            const uint64_t* count, uint32_t msg_room, uint32_t which, uint64_t* valid);
// d_result: the records with d_valid[m] < len, the lowest of them, the
// records checked and their bytes.
hipError_t launch_utf8_count(hipStream_t s, int grid, const wsg_msg* msgs, const uint64_t* count, uint32_t msg_room,
                             uint64_t msg_cap, uint32_t which, const uint64_t* valid, uint64_t* result);

// wsg_utf8_verdicts: also[j] all 0xFF, then the lowest {WSG_PV_UTF8, 1007,
// FIN frame} over stream j's selected records with d_valid[m] < len.
hipError_t launch_utf8_verdicts(hipStream_t s, int rec_grid, int stream_grid, const wsg_msg* msgs,
                                const uint64_t* count, uint32_t msg_room, uint32_t which, const uint64_t* valid,
                                uint32_t n_streams, wsg_proto_verdict* also);

// ---- UTF-8 from the masked wire (wsg_check_utf8_wire; wsg_utf8.hip) ---------
// The payload kernel over the message plan's piece records (launch_msg_plan's,
// read as 4 KiB pieces of the wire), one wave per record, grid-stride: every
// payload byte of a delivered frame loaded once and unmasked in registers;
// d_valid as launch_utf8_scan leaves it for the dense layout of the same
// messages.  Between launch_utf8_init and launch_utf8_count (msg_cap
// UINT64_MAX: every record lies inside the layout).
// (msg_room is b.n: a message ends in a frame.)
hipError_t launch_utf8_wire(hipStream_t s, int grid, const Batch& b, const MsgOut& o, const MsgScratch& x,
                            uint32_t which, uint64_t* valid);
// wsg_reply_validated: launch_utf8_verdicts over a seed that is also_in[j]
// (null: none) where that names a frame of stream j, all 0xFF otherwise.
// (over the b.n records u.valid has; the merged verdicts into u.also)
hipError_t launch_utf8_verdicts_over(hipStream_t s, int stream_grid, const Batch& b,
                                     const wsg_proto_verdict* also_in, const MsgOut& o, const Utf8Inside& u);

// ---- protocol rules on the device (wsg_check_protocol; wsg_proto.hip) -------
struct ProtoStep;   // wsg_proto.h
// Scratch of one call, carved by the host out of one device block
// (proto_plan_layout; one block = BLOCK frames).
struct ProtoPlan {
    ProtoStep* part;   // nb: the blocks' composed steps
    ProtoStep* pre;    // nb: their exclusive prefixes
    uint64_t* out;     // 2 * ns: the state d_proto[j] gets, as its two words (k_proto_judge to k_proto_finish)
    uint32_t* sidx;    // n: the frame's stream
};
// Bytes of that block for n frames in ns streams; plan (or null) gets the pointers into base.
uint64_t proto_plan_layout(uint8_t* base, uint32_t n, uint32_t ns, ProtoPlan* plan);
// k_proto_local and k_proto_blocks: d_verdict and d_result seeded (all 0xFF;
// {0, UINT64_MAX, 0}), the frames' streams and the scanned block partials in
// the plan.  At least one block, also for n == 0 or n_streams == 0.
// (The protocol launchers read b.n, b.stream_first, b.n_streams and, the judge, the wire; info: the decode's.)
hipError_t launch_proto_scan(hipStream_t s, const Batch& b, const wsg_recv_info* info, const ProtoOps& p,
                             const ProtoPlan& plan);
// The per-frame judging kernel (n > 0 and n_streams > 0): every frame's code,
// the first of each stream into d_verdict by atomicMin; the state d_proto asks
// for into the plan.
hipError_t launch_proto_judge(hipStream_t s, const Batch& b, const wsg_recv_info* info,
                              const wsg_stream_state* state, const ProtoOps& p, const ProtoPlan& plan);
// wsg_reply_checked: d_verdict[j] replaced by also[j] where that comes first (one lane per stream, grid-stride).
hipError_t launch_proto_merge(hipStream_t s, int grid, uint32_t n, const uint32_t* stream_first, uint32_t n_streams,
                              const wsg_proto_verdict* also, wsg_proto_verdict* verdict);
// One lane per stream (grid-stride): d_proto and d_result's counts.
hipError_t launch_proto_finish(hipStream_t s, int grid, const Batch& b, const wsg_stream_state* state,
                               const ProtoOps& p, const ProtoPlan& plan);

// ---- fan-out (wsg_fanout_encode, wsg_fanout_encode_many; wsg_fanout.hip) ----
// Messages of one fan-out launch (blockIdx.y): payload and output offsets.
constexpr int FAN_MSGS = 32;
struct FanMsgs {
    uint64_t src[FAN_MSGS];   // message payload offset from the payload base
    uint64_t dst[FAN_MSGS];   // wire offset of the message's first frame
};
// Period-path fan-out of nmsgs (<= FAN_MSGS) messages of one geometry; false:
// the frame size does not suit it (the caller takes launch_fanout per message).
bool launch_fanout_period(hipStream_t s, int cus, int waves_per_cu, int wpb, const uint8_t* payload, uint64_t len,
                          const uint32_t* keys, uint32_t k, uint8_t opcode, uint32_t mask, uint64_t fsize,
                          uint8_t* wire, const FanMsgs& msgs, uint32_t nmsgs, hipError_t* err);
hipError_t launch_fanout(hipStream_t s, int grid, const uint8_t* payload, uint64_t len, const uint32_t* keys,
                         uint32_t k, uint8_t opcode, uint32_t mask, uint64_t fsize, uint8_t* wire);

// ---- single-buffer XOR, offset rebase, test hook (wsg_misc.hip) -------------
hipError_t launch_xor(hipStream_t s, int grid, const uint8_t* src, uint8_t* dst, uint64_t len, uint32_t key,
                      uint32_t phase);
// Multi-GPU gather (wsg_mgpu.cpp): the job's wire offsets from the ranks'
// local offsets, staged rank by rank at rank_base[r] (chunk c of the job is
// rank c % world's local chunk c / world, placed at goff[c]);
// out_off[n_total] = total.
hipError_t launch_rebase_offsets(hipStream_t s, const uint64_t* stage, const uint64_t* goff, const uint64_t* rank_base,
                                 uint64_t n_total, uint32_t chunk, uint32_t world, uint64_t* out_off, uint64_t total);
// Test hook only: one wave waiting `us` microseconds (at most 0.2 s) on `s`.
hipError_t launch_test_spin(hipStream_t s, uint32_t us);

// ---- the host lane (wsg_lane_device.hip; host side: wsg_lane.cpp) -----------
// One resident kernel per device for small host batches.
// A host batch of a few KiB (an echo's read: ~1000 frames of 38 B) costs a
// launch and a synchronize per pass (10 us for an empty kernel on MI355X,
// tools/smallpass.hip) on top of its PCIe round trips.  The lane is launched
// once per device and shared by every context of the process: W workgroups,
// each with a mailbox of LANE_RING task slots in page-locked host memory.
// A request is cut into frame groups; group k gets the ticket x + k of a
// process-wide ticket counter, i.e. slot (x + k) / W of workgroup (x + k) % W,
// so consecutive requests spread over the workgroups and one request's groups
// run side by side.  The host writes a slot's units (each value, then its
// tag = ticket + 1; the first unit last), the workgroup polls its next slot
// (every unit in one read), does the group on the host buffers in place and answers
// in the slot's response.  Every workgroup ends: on `stop` (teardown, or a
// request that timed out), or after idle_ticks without a task / yield_ticks of
// running, announced in `closing` so that the others follow at their next
// check; a caller waiting on an answer launches the next generation, which
// resumes each mailbox where the last one left it (next_j).
enum : uint32_t { LANE_DECODE = 1, LANE_ENCODE = 2, LANE_XOR = 3, LANE_XOR_INLINE = 4 };
constexpr uint64_t LANE_INLINE = 40;     // xor: payloads up to this size travel in the task (w[4..8])
constexpr uint64_t LANE_STAGE = 64 << 10;  // decode: wire bytes staged in LDS (one group's range limit)
constexpr uint64_t LANE_PSTAGE = 64 << 10; // encode: payload arena staged in LDS when its 16-B blocks fit
// LDS of the lane (one layout per op, the larger sized):
//   decode: staged wire | info blocks (32 B) | payload bounds (2 x 8 B), key (4 B), frame starts (8 B) per frame
//   encode: offsets (8 B) | heads (16 B) | records (16 B) | descriptors (32 B) per frame | staged payload
constexpr uint64_t LANE_LDS_DECODE = LANE_STAGE + 60 * LANE_THREADS + 64;
constexpr uint64_t LANE_LDS_ENCODE = 72 * LANE_THREADS + 64 + LANE_PSTAGE;
constexpr uint64_t LANE_LDS = LANE_LDS_DECODE > LANE_LDS_ENCODE ? LANE_LDS_DECODE : LANE_LDS_ENCODE;
static_assert(LANE_LDS <= 160 * 1024 - 1024, "the lane's workgroup LDS");
constexpr uint32_t LANE_WGS_MAX = 32;          // workgroups of the lane (each a CU's worth of LDS)
constexpr uint32_t LANE_RING = 64;             // task slots per workgroup mailbox
constexpr uint32_t LANE_WORDS = 9;             // task units (w[])
// A task word and the ticket it belongs to, + 1 (the host stores v, then
// tag; the lane reads the 16 bytes in one request).
struct alignas(16) LaneUnit {
    uint64_t v, tag;
};
// One frame group of a request (the host's, read by one workgroup):
//   w[0] = op | n << 32 (posted last: the workgroup polls its tag)
//   decode: w[1..5] = wire, wire_len, frame_start, out, info;
//           w[6] = f_lo | cnt << 32 (the group's frames [f_lo, f_lo + cnt));
//           w[7], w[8] = the group's wire range [lo, hi): its first start (0
//           for the first group) to the next group's (wire_len after the last),
//           clamped to wire_len — bit-identical to k_decode there; the table
//           strictly increasing (the caller checks), hi - lo + 64 <= LANE_STAGE
//   encode: w[1..4] = payload, desc, wire_off (n + 1, host-computed), wire;
//           w[6] = f_lo | cnt << 32; w[7], w[8] = the group's payload span
//           [lo, hi) ({0, 0}: none)
//   xor:    w[1..3] = buffer, length, key | phase << 32 (n = 1): the
//           page-locked buffer XORed in place, byte i with key byte
//           (phase + i) % 4; LANE_XOR_INLINE: the payload (<= LANE_INLINE
//           bytes) in w[4..8], the result in the slot's LaneXres (no write
//           to the buffer, no fence, no `done`)
struct LaneTask {
    LaneUnit w[LANE_WORDS];
    uint64_t pad[2];
};
// The lane's answer to a task: errs (decode: frames with an error), then
// done = the task's tag (release).
struct alignas(16) LaneResp {
    uint64_t done, errs;
};
// The answer of an inline XOR: result dword k beside the low 32 bits of the
// task's tag, one 8-byte unit each, written by one lane with one store and
// read by the host with one load — a unit showing the tag holds its dword,
// so the answer needs no release fence before it (the fence waits for the
// stores to be acknowledged over PCIe).
struct alignas(16) LaneXres {
    uint64_t u[LANE_INLINE / 4];
};
struct alignas(16) LaneCtl {
    uint32_t stop;      // host: every workgroup leaves at its next check
    uint32_t closing;   // lane: launch `closing` is ending (its workgroups leave at their next check)
    uint64_t pad;
};
struct LaneBell {
    LaneCtl ctl;
    uint64_t next_j[LANE_WGS_MAX];             // lane: workgroup g's next mailbox position (stored as it leaves)
    LaneResp resp[LANE_WGS_MAX][LANE_RING];    // lane: answers
    LaneXres xres[LANE_WGS_MAX][LANE_RING];    // lane: inline XOR answers
    LaneTask box[LANE_WGS_MAX][LANE_RING];     // host: mailboxes (ticket x: box[x % W][(x / W) % LANE_RING])
};
// A launch of `workgroups` (the server's W) workgroups of generation `gen`
// (>= 1): each leaves after idle_ticks without a task, after yield_ticks of
// running (at a task boundary), on `stop`, or when `closing` names its
// generation.  delay_ticks: a test hook, the workgroups wait that long before
// their first poll (a lane that starts late).
hipError_t launch_lane(hipStream_t s, LaneBell* bell, uint32_t workgroups, uint64_t idle_ticks,
                       uint64_t yield_ticks, uint32_t gen, uint64_t delay_ticks);

} // namespace wsg
