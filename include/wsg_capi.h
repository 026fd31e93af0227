/*
 * wsg_capi.h — C-ABI boundary of the MI355X WebSocket frame codec.
 *
 * This is the drop-in boundary for CppServer's per-byte WebSocket hot path
 * (reference: chronoxor/CppServer 1.0.5.0, class CppServer::WS::WebSocket,
 * include/server/ws/ws.h:29, source/server/ws/ws.cpp:212-498).
 *
 * Plain C types only: pointers, sizes, fixed-layout structs.  No C++ types and
 * no torch types cross this boundary; no C++ exception ever leaves it.  Every
 * entry point returns an int status (WSG_OK = 0, negative on failure).
 *
 * Device ("d_") buffers are caller-owned and must already be resident in HBM.
 * Batch entry points are asynchronous on the given HIP stream (NULL = HIP's
 * default stream, as everywhere in HIP; wsg_stream() returns a non-blocking
 * stream owned by the context); the caller synchronizes (wsg_sync) before
 * reading outputs.  Data-dependent errors (a frame that overruns the wire, overlapping
 * frames) are latched in the context and reported by wsg_sync.
 *
 * Thread-safety: one wsg_ctx per host thread.  A ctx is not thread-safe.
 *
 * Streams: one thread may drive a ctx on several streams.  wsg_encode_batch
 * calls share one scratch of the ctx (scan partials, piece starts, piece ->
 * frame map), wsg_decode_messages and wsg_reply_messages calls another (plan
 * block, piece records) and wsg_frame_streams calls a third (per-stream frame
 * counts, scan partials; wsg_decode_streams and wsg_reply_streams are one
 * call of each of the last two) and wsg_check_protocol calls a fourth (the
 * frames' streams, scan partials, per-stream states; wsg_reply_checked and
 * wsg_reply_validated use the second and the fourth and are ordered with the
 * users of both; wsg_check_utf8_wire uses the second);
 * wsg_decode_batch, wsg_check_utf8, wsg_utf8_verdicts and the fan-out calls use none.  The calls that
 * share a scratch are ordered across streams on the device, in the order they
 * were made: a call on another stream than the previous one first waits
 * (hipStreamWaitEvent, no host synchronisation) for an event recorded behind
 * that one, so two batches double-buffered on two streams run their
 * wsg_encode_batch kernels one after the other.  A call made while its stream
 * is capturing is not ordered: it neither waits nor records, so the caller
 * keeps other users of that scratch off the device while the graph runs.  A
 * graph holding wsg_encode_batch / wsg_decode_messages / wsg_reply_messages /
 * wsg_frame_streams / wsg_check_protocol / wsg_reply_checked launches (the _streams
 * forms synchronise and cannot be captured) names the
 * scratch addresses it was captured with; a later call that needs a larger
 * scratch frees them (after a device synchronise), and the graph must not be
 * replayed after that: give such a graph a ctx of its own.  Capture no call
 * that has to grow a scratch: run it once with the same n and capacity first.
 *
 * Debug: with $WSG_CHECK=1 at wsg_create, the device entry points check
 * before every launch that each operand range lies inside one device
 * allocation (encode: every descriptor's payload range too, read back from
 * the device) and return WSG_EINVAL instead of launching otherwise.
 */
#ifndef WSG_CAPI_H
#define WSG_CAPI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WSG_ABI_VERSION 3

/* ---- status codes ------------------------------------------------------ */
#define WSG_OK          0
#define WSG_EINVAL    (-22)  /* bad argument: NULL pointer, misaligned buffer, overlapping frames */
#define WSG_ETRUNC    (-61)  /* a frame header/payload runs past the end of the wire */
#define WSG_ENOMEM    (-12)  /* device or pinned allocation failed / output capacity too small */
#define WSG_EHIP      (-5)   /* HIP runtime error (no device, launch failure, ...) */

/* ---- opcode byte values (reference ws.h:33-43) ------------------------- */
#define WSG_FIN    0x80
#define WSG_TEXT   0x01
#define WSG_BINARY 0x02
#define WSG_CLOSE  0x08
#define WSG_PING   0x09
#define WSG_PONG   0x0A

/* Required alignment of wire/output device buffers in the batch decode/encode
 * entry points (hipMalloc and torch allocations satisfy it). */
#define WSG_ALIGN 16

/* One frame to encode (a batched PrepareSendFrame call, ws.cpp:212).
 * key is _ws_send_mask[0..3] read as a little-endian uint32, i.e.
 * byte j of the key is (key >> 8*j) & 0xFF (ws.cpp:244-247, :270). */
typedef struct wsg_send_desc {
    uint64_t src_off;   /* payload offset inside d_payload                    */
    uint64_t len;       /* payload length in bytes (excluding close status)   */
    uint32_t key;       /* per-connection send mask (ws.cpp:97 / :206)       */
    int32_t  status;    /* close status, ws.cpp:215 (0 = none)                */
    uint8_t  opcode;    /* whole first header byte, e.g. WSG_FIN|WSG_BINARY   */
    uint8_t  mask;      /* nonzero: set MASK bit and emit the 4 key bytes     */
    uint8_t  _pad[6];
} wsg_send_desc;        /* 32 bytes */

/* One decoded frame (the per-frame arithmetic of PrepareReceiveFrame,
 * ws.cpp:320-386). */
typedef struct wsg_recv_info {
    uint64_t payload_off; /* absolute offset of the payload in wire and output */
    uint64_t len;         /* payload length                                    */
    uint32_t key;         /* receive mask (little-endian), 0 if unmasked       */
    uint8_t  opcode;      /* b0 & 0x0F (raw; 0 = continuation, ws.cpp:320)     */
    uint8_t  fin;         /* b0 >> 7 (ws.cpp:321)                              */
    uint8_t  masked;      /* b1 >> 7 (ws.cpp:322)                              */
    uint8_t  hdr_len;     /* 2/4/10 (+4 when masked), ws.cpp:331/349/367       */
    uint8_t  b0;          /* raw first header byte (RSV bits kept)             */
    int8_t   error;       /* 0, or WSG_ETRUNC / WSG_EINVAL for this frame      */
    uint8_t  _pad[6];
} wsg_recv_info;        /* 32 bytes */

typedef struct wsg_ctx wsg_ctx;

/* ---- context ------------------------------------------------------------ */
/* Bind to HIP device `device`, create a non-blocking stream, small scratch.   */
int wsg_create(int device, wsg_ctx** out);
int wsg_destroy(wsg_ctx* ctx);
/* Synchronize `stream` (NULL = default stream) and return one data-dependent
 * error latched since the last wsg_sync (then clear the latch): over all the
 * calls since then, on any stream, the error of the lowest frame index (the
 * latch is an atomic minimum of frame << 8 | code), not the first in time.   */
int wsg_sync(wsg_ctx* ctx, void* stream);
/* HIP stream owned by the context (a hipStream_t). */
void* wsg_stream(wsg_ctx* ctx);
int wsg_abi_version(void);
/* Human-readable name of a status code. */
const char* wsg_strerror(int code);

/* ---- batch decode: unmask (PrepareReceiveFrame over many frames) -------- */
/* d_wire: `wire_len` bytes of concatenated frames.  d_frame_start[i]: wire
 * offset of frame i (strictly increasing, frames must not overlap; the host
 * framer produces it with RequiredReceiveFrameSize semantics, ws.cpp:458).
 * d_out: wire_len bytes; on return it is the wire with every frame's payload
 * unmasked in place (ws.cpp:399-406); header and gap bytes are copied
 * unchanged.  d_out may equal d_wire (in-place).  d_info[i] describes frame i
 * (payload at d_out + d_info[i].payload_off).  d_wire/d_out 16-byte aligned;
 * the kernel reads d_wire in whole 16-byte blocks, so the block holding the
 * last wire byte must be readable (hipMalloc / torch allocations are).       */
int wsg_decode_batch(wsg_ctx* ctx, const uint8_t* d_wire, uint64_t wire_len,
                     const uint64_t* d_frame_start, uint32_t n,
                     uint8_t* d_out, wsg_recv_info* d_info, void* stream);

/* ---- batch decode to messages (the second half of PrepareReceiveFrame) --- */
/* (Added without an ABI bump: WSG_ABI_VERSION stays 3, the change only adds
 * symbols and structs; nothing existing moved.)
 * One assembled message: what the session would hand to onWSReceived /
 * onWSClose / onWSPing / onWSPong at a FIN frame (ws.cpp:411-452). */
typedef struct wsg_msg {
    uint64_t off;          /* offset of the callback's data in d_msg (past a close status) */
    uint64_t len;          /* the callback's size (close: without the 2 status bytes)     */
    uint32_t stream;       /* index of the stream                                          */
    uint32_t first_frame;  /* index in d_frame_start of the message's first frame         */
    uint32_t nframes;      /* frames accumulated into it (>= 1); WSG_ASSEMBLY_RFC: the span
                              first_frame .. its FIN frame, control frames inside it counted */
    int32_t  status;       /* close: ws.cpp:431-439 (1000 when < 2 bytes); otherwise 0     */
    uint8_t  kind;         /* WSG_CB_*; 0 = no callback (unknown sticky opcode, Q6)        */
    uint8_t  opcode;       /* _ws_opcode at the FIN frame; WSG_ASSEMBLY_RFC: the message's own */
    uint8_t  _pad[6];      /* written as 0 */
} wsg_msg;                 /* 40 bytes */

typedef struct wsg_stream_state {
    uint32_t consumed;     /* out: frames of this stream that went into messages          */
    uint8_t  opcode;       /* WSG_ASSEMBLY_REFERENCE: in: _ws_opcode before the stream's
                              first frame; out: _ws_opcode after its last consumed frame.
                              WSG_ASSEMBLY_RFC: ignored, written as 0 (the resubmitted
                              tail begins with the frame that names its opcode)            */
    uint8_t  _pad;         /* written as 0 */
    uint8_t  ahead[2];     /* a 16-bit count, little-endian, at offset 6 (two bytes, so that
                              the struct names only the types it named before; a caller
                              that carries the record from call to call never reads it, and
                              WSG_STREAM_AHEAD does for one that wants to).
                              WSG_ASSEMBLY_RFC: in: FIN control frames behind the first
                              frame of the resubmitted tail that an earlier call delivered;
                              out: those behind the first frame of the tail this call
                              leaves (at most 65535).  WSG_ASSEMBLY_REFERENCE: ignored,
                              written as 0                                                  */
} wsg_stream_state;        /* 8 bytes */
#define WSG_STREAM_AHEAD(s) ((uint16_t)((s).ahead[0] | ((s).ahead[1] << 8)))

/* ---- the assembly rule: which frames make a message ------------------------ */
/* (Added without an ABI bump: symbols only, and a field in what was padding.)
 * WSG_ASSEMBLY_REFERENCE, the default: ws.cpp:399-452 bit for bit.  Every FIN
 * frame ends a message made of all its stream's frames since the previous FIN
 * frame, control frames included, under the sticky _ws_opcode.
 * WSG_ASSEMBLY_RFC: RFC 6455 5.4.  A FIN control frame is a message of its own
 * (buffer: its payload; first_frame: itself; nframes 1; opcode: its own; kind
 * by that opcode, 0 for a reserved one; a close's status, off and len by the
 * two-byte rule of its own payload), also between the fragments of a data
 * message.  A data message is the payloads of its run's data frames alone: the
 * run is the non-control frames from the first one behind the previous data
 * FIN frame to the next data FIN frame.  first_frame is the run's first frame,
 * nframes the span up to its FIN frame (control frames inside it count, so
 * first_frame + nframes - 1 is the FIN frame), opcode the last non-zero opcode
 * among the run's frames (the first fragment's on a legal stream), kind
 * WSG_CB_RECEIVED for opcodes 1 and 2, else 0.  A frame with an error, and a
 * control frame without FIN, lie in no message and end none.  Messages,
 * buffers and replies are in the order of the frames that end them, so a ping
 * inside a message comes in front of it.
 * Carry-over.  When a stream ends inside a run, consumed stops at the run's
 * first frame; the control frames behind it were delivered in this call (the
 * first 65535 of them: `ahead` counts no further, and the rest wait for the
 * call that holds the run's FIN frame) and are skipped, by their count in
 * d_state[j].ahead, when the tail comes back.  Without an open run every frame
 * of the stream is consumed and ahead is 0.
 * The mode is the context's, read on the host when a call is made; a captured
 * graph keeps the mode it was captured under.  It is honoured by
 * wsg_decode_messages, wsg_decode_streams, wsg_reply_messages,
 * wsg_reply_streams, wsg_check_utf8_wire, wsg_reply_checked(_streams) and
 * wsg_reply_validated(_streams); the calls that work on tables
 * (wsg_check_utf8, wsg_utf8_verdicts, wsg_check_protocol, wsg_frame_streams)
 * take either mode's.                                                        */
#define WSG_ASSEMBLY_REFERENCE 0
#define WSG_ASSEMBLY_RFC       1
int wsg_set_assembly(wsg_ctx* ctx, int mode);   /* WSG_EINVAL for any other mode */
int wsg_get_assembly(wsg_ctx* ctx);             /* the mode; WSG_EINVAL without a context */

/* wsg_decode_batch's frames, assembled into messages (ws.cpp:399-452) and
 * packed densely: the layout wsg_encode_batch takes its payloads in.
 * d_wire / wire_len / d_frame_start / n / d_info: as wsg_decode_batch (d_info
 * gets the same records; d_wire is only read).  d_stream_first[0..n_streams]:
 * non-decreasing, [0] = 0, [n_streams] = n; frames [d_stream_first[j],
 * d_stream_first[j+1]) are connection j's frames in arrival order (empty
 * streams allowed).  Within a stream every FIN frame ends a message whose
 * buffer is the unmasked payloads of all the stream's frames since its
 * previous FIN frame (control frames included, as the reference appends
 * them); its opcode is the last non-zero b0 & 0x0F of the stream so far,
 * seeded from d_state[j].opcode and never reset between messages.  Message
 * buffers lie back to back in d_msg (16-byte aligned, msg_cap bytes; wire_len
 * always suffices) in the order of their FIN frames; d_msgs[0..d_count[0])
 * describes them (room for n), d_count[1] = bytes used in d_msg.  Frames
 * after a stream's last FIN frame are its tail: no byte of theirs is written,
 * d_state[j].consumed says where it begins, and the caller resubmits them at
 * the head of stream j in its next call with the returned d_state[j] (its
 * opcode; under WSG_ASSEMBLY_RFC, which replaces the rule of this paragraph
 * by the one stated at wsg_set_assembly, its ahead).
 * Asynchronous on `stream`.  Latched for wsg_sync: a frame error (as
 * wsg_decode_batch; the frame then counts as an empty non-FIN continuation),
 * or WSG_ENOMEM when the messages need more than msg_cap bytes: then no byte
 * of d_msg is written and d_count still holds the size needed.             */
int wsg_decode_messages(wsg_ctx* ctx, const uint8_t* d_wire, uint64_t wire_len,
                        const uint64_t* d_frame_start, uint32_t n,
                        const uint32_t* d_stream_first, uint32_t n_streams,
                        wsg_stream_state* d_state,
                        uint8_t* d_msg, uint64_t msg_cap,
                        wsg_msg* d_msgs, uint64_t* d_count,
                        wsg_recv_info* d_info, void* stream);

/* ---- the device framer: raw stream bytes to a frame table ----------------- */
/* (Added without an ABI bump, as wsg_decode_messages was: symbols and structs
 * only.)  One connection's bytes in a batch. */
typedef struct wsg_stream_span {
    uint64_t off;       /* in:  wire offset of the stream's first unparsed byte        */
    uint64_t len;       /* in:  bytes of this stream in the batch                      */
    uint64_t consumed;  /* out: bytes covered by whole frames (resubmit from off+consumed) */
    uint64_t need;      /* out: size the partial frame at the tail is known to have    */
} wsg_stream_span;      /* 32 bytes */

/* Find the frame boundaries of n_streams connections on the device: the
 * d_frame_start / d_stream_first tables wsg_decode_batch and
 * wsg_decode_messages take, without a host framer.
 * Whole frames.  Stream j is d_wire[off, off + len).  Its frames are parsed
 * from `off`, each header exactly as one delivered whole (wsg_header_unpack,
 * ws.cpp:320-386).  A frame is whole when its header is complete and hdr_len +
 * payload length fits in the bytes that remain (compared without forming a sum
 * that could wrap); the walk stops at the first frame that is not.
 * consumed: the bytes of the stream's whole frames.
 * need, with rem = len - consumed: 0 when rem == 0; 2 when rem == 1; the
 * header's length (known from its second byte) while the header is
 * incomplete; hdr_len + payload length, saturating at UINT64_MAX, once it is
 * complete.  The 127 form is taken as the reference takes it, all 64 bits, no
 * MSB check: a length of 2^63 or 2^64 - 1 is a frame that never completes, not
 * an error.
 * Outputs.  d_stream_first[0..n_streams]: the exclusive prefix of the streams'
 * frame counts ([n_streams] = frames found).  d_frame_start[d_stream_first[j]
 * ..): stream j's frame starts, absolute wire offsets (frame_cap entries of
 * room).  d_count[0] = frames found, d_count[1] = the sum of `consumed`.
 * Span order.  Spans are given in increasing, non-overlapping wire order, so
 * the table is strictly increasing, as wsg_decode_batch requires; bytes
 * between spans and partial tails are gaps, which both decode calls allow.
 * Latched for wsg_sync, under the key stream << 8 | code (the same atomic
 * minimum, the stream index where the decodes put the frame index):
 * WSG_EINVAL for a span that runs past wire_len, or that starts before the
 * end of the span before it (when that one lies inside the wire): that stream
 * yields no frames, consumed 0 and need 0, the other streams are unaffected;
 * WSG_ENOMEM for more than frame_cap frames: d_count, d_stream_first and the
 * spans are still written, not one entry of d_frame_start is; WSG_EINVAL for
 * more than UINT32_MAX - 1 frames (likewise; d_stream_first saturates).  The
 * last two are latched under the key n_streams << 8 | code.
 * Arguments.  d_wire 16-byte aligned and readable to the end of its last
 * 16-byte block, as for wsg_decode_batch; span offsets of any alignment;
 * n_streams == 0 is valid (d_stream_first[0] = 0, d_count = {0, 0}).
 * Asynchronous on `stream`.
 * Relation to SURVEY Q7.  A stream is parsed as if it arrived unsplit, and a
 * tail is resubmitted from off + consumed, never continued in the middle of a
 * header: this is the whole-frame contract wsg_decode_batch already has, not
 * the reference's mis-parse of a header split across two reads (which
 * wsg_rx_feed reproduces).
 * Streams: the calls share a scratch of the ctx (per-stream counts, scan
 * partials) and are ordered across streams on the device like the
 * wsg_encode_batch and wsg_decode_messages calls (see "Streams" above), with
 * the same capture rule: a captured call is not ordered, and a call that has
 * to grow the scratch must not be captured: run it once with the same
 * n_streams first.                                                          */
int wsg_frame_streams(wsg_ctx* ctx, const uint8_t* d_wire, uint64_t wire_len,
                      wsg_stream_span* d_span, uint32_t n_streams,
                      uint64_t* d_frame_start, uint32_t frame_cap,
                      uint32_t* d_stream_first, uint64_t* d_count, void* stream);

/* Raw bytes to messages: wsg_frame_streams, one synchronisation of `stream`
 * to read the frame count (*n_frames_out), wsg_decode_messages with that n.
 * d_msgs and d_info need room for frame_cap records; d_count ends as
 * wsg_decode_messages leaves it (messages, bytes of d_msg).  Then
 * d_span[j].consumed is lowered to the start of stream j's first tail frame
 * (the first frame behind the stream's last FIN frame that went into a
 * message; `need` is left as the framer wrote it), so a connection's whole
 * carry-over to its next call is: the bytes from off + consumed, and
 * d_state[j].opcode.  Returns WSG_EINVAL while `stream` is capturing;
 * WSG_ENOMEM (WSG_EINVAL), with nothing decoded, when the framer found more
 * than frame_cap (UINT32_MAX - 1) frames (the latch holds it too).  Errors of
 * single spans and frames are latched as by the two calls.                  */
int wsg_decode_streams(wsg_ctx* ctx, const uint8_t* d_wire, uint64_t wire_len,
                       wsg_stream_span* d_span, uint32_t n_streams,
                       wsg_stream_state* d_state,
                       uint64_t* d_frame_start, uint32_t frame_cap, uint32_t* d_stream_first,
                       uint8_t* d_msg, uint64_t msg_cap, wsg_msg* d_msgs, uint64_t* d_count,
                       wsg_recv_info* d_info, uint32_t* n_frames_out, void* stream);

/* ---- replies: received messages to frames to send, on the device ---------- */
/* (Added without an ABI bump, as wsg_decode_messages was: symbols only.)
 *
 * What an echo server does with a batch (performance/ws_echo_server.cpp:
 * onWSReceived -> SendBinaryAsync, ws_session.h: onWSPing -> SendPongAsync)
 * in one asynchronous call: the arguments, message rules, d_msgs, d_info,
 * d_state and frame errors of wsg_decode_messages, but instead of a dense
 * d_msg the reply frames, ready to send.  Every payload byte is read once
 * from d_wire and written once into d_reply; d_msgs[m].off / len and
 * d_count[1] describe the dense layout that wsg_decode_messages would have
 * produced (no such buffer is written).
 *
 * reply_op (host array, read during the call) is indexed by WSG_CB_*; entry
 * 0 is ignored (a kind-0 message is never answered).  0: no reply to that
 * kind; WSG_REPLY_SAME: WSG_FIN | the message's opcode; anything else: the
 * reply's whole first header byte.  The reference echo server is
 * {0, WSG_FIN|WSG_BINARY, 0, WSG_FIN|WSG_PONG, 0}.
 *
 * The reply to message m of stream j is what a session whose _ws_send_mask
 * is d_send_key[j] (little-endian, as wsg_send_desc.key; NULL: every key 0,
 * a server) leaves in _ws_send_buffer after PrepareSendFrame(op, mask, data,
 * size, 0) with the callback's data, or, for a WSG_CB_CLOSE message, after
 * PrepareSendFrame(op, mask, NULL, 0, msg.status).  Byte-exact with
 * ws.cpp:212-271 as wsg_encode_batch is: one frame per message however many
 * fragments it came in, the two-byte prefix on CLOSE/PING/PONG opcodes (a
 * pong to a non-empty ping carries 00 00 ahead of its data), the XOR with
 * the send key when mask == 0 too.
 *
 * Reply frames lie back to back in d_reply (16-byte aligned, reply_cap
 * bytes, not overlapping d_wire; wire_len + 14 * n always suffices) in
 * message order:
 *   d_reply_off[0..d_count[0]]   (room for n + 1) message m's frame is
 *                                d_reply[d_reply_off[m], d_reply_off[m+1]),
 *                                empty when it gets no reply
 *   d_stream_reply[0..n_streams] connection j's replies are the one range
 *                                d_reply[d_stream_reply[j], d_stream_reply[j+1])
 *   d_count[0..4)                messages, bytes of the dense layout, reply
 *                                bytes, reply frames
 * When the replies need more than reply_cap bytes no byte of d_reply is
 * written and wsg_sync reports WSG_ENOMEM (behind every frame error);
 * everything else is final.
 * Streams: the call uses the scratch of wsg_decode_messages and is ordered
 * with those calls across streams (see "Streams" above); the same capture
 * rule holds: run it once with the same n first.
 * Under WSG_ASSEMBLY_RFC the messages are that rule's (wsg_set_assembly): a
 * reply belongs to the frame that ends its message, so a ping between
 * fragments is answered ahead of the echo of the message around it, and that
 * echo carries the data frames' bytes alone; run the uncaptured call under
 * the mode the capture will use.                                             */
#define WSG_REPLY_SAME 0xFF   /* reply opcode byte: WSG_FIN | the message's opcode */

int wsg_reply_messages(wsg_ctx* ctx, const uint8_t* d_wire, uint64_t wire_len,
                       const uint64_t* d_frame_start, uint32_t n,
                       const uint32_t* d_stream_first, uint32_t n_streams,
                       wsg_stream_state* d_state,
                       const uint8_t reply_op[5], int mask, const uint32_t* d_send_key,
                       uint8_t* d_reply, uint64_t reply_cap,
                       uint64_t* d_reply_off, uint64_t* d_stream_reply,
                       wsg_msg* d_msgs, uint64_t* d_count,
                       wsg_recv_info* d_info, void* stream);

/* Raw bytes to reply frames: wsg_decode_streams with wsg_reply_messages in
 * the place of wsg_decode_messages (the framer, one synchronisation of
 * `stream`, the replies, d_span[j].consumed lowered to the first tail
 * frame); the same returns.  An echo server's loop is this call, then one
 * send per d_stream_reply range.                                            */
int wsg_reply_streams(wsg_ctx* ctx, const uint8_t* d_wire, uint64_t wire_len,
                      wsg_stream_span* d_span, uint32_t n_streams, wsg_stream_state* d_state,
                      uint64_t* d_frame_start, uint32_t frame_cap, uint32_t* d_stream_first,
                      const uint8_t reply_op[5], int mask, const uint32_t* d_send_key,
                      uint8_t* d_reply, uint64_t reply_cap, uint64_t* d_reply_off, uint64_t* d_stream_reply,
                      wsg_msg* d_msgs, uint64_t* d_count, wsg_recv_info* d_info,
                      uint32_t* n_frames_out, void* stream);

/* ---- UTF-8: text messages and close reasons checked on the device --------- */
/* (Added without an ABI bump, as wsg_decode_messages was: symbols and
 * constants only.)
 *
 * RFC 6455 5.6 / 8.1 require a text message, taken over all its fragments,
 * to be valid UTF-8, and 7.1.6 the same of a close frame's reason; the
 * endpoint fails the connection with status 1007 otherwise.  The reference
 * does not validate (it hands the bytes to onWSReceived as they are), so this
 * is a call of its own behind wsg_decode_messages / wsg_decode_streams, whose
 * d_msg holds every message unmasked with its fragments joined.
 *
 * valid_up_to(b) of a byte string is the length of its longest prefix that is
 * well-formed UTF-8 (RFC 3629: shortest form only, no surrogates
 * U+D800-DFFF, nothing above U+10FFFF, the bytes C0, C1 and F5-FF never
 * valid, a sequence cut off by the end of b invalid): len(b) when b is valid.
 *
 * Inputs.  d_msg (16-byte aligned, msg_cap bytes), d_msgs and d_count as the
 * decode left them on the device: d_count[0] the message count, d_count[1]
 * the bytes used, both read on the device, so the two calls need no
 * synchronisation between them on one stream.  M = min(d_count[0], msg_room)
 * records are looked at; d_valid has room for msg_room words.
 * What is checked.  Message m < M is selected by `which` (the WSG_UTF8_* bits
 * or'ed), from its record's kind and opcode alone (a fragmented message whose
 * sticky opcode at its FIN frame is WSG_TEXT counts as text).  A selected
 * message is checked when off + len <= min(msg_cap, d_count[1]) (compared
 * without forming a sum that could wrap); no byte of d_msg at or past that
 * bound is ever read.  A decode that latched WSG_ENOMEM wrote no byte of
 * d_msg and left d_count[1] > msg_cap: the caller sees that status at its
 * wsg_sync and drops the verdicts of that batch.
 * Outputs.  d_valid[m] for m < M: valid_up_to of d_msg[off, off + len) when
 * message m is checked, len otherwise; entries at M and beyond are not
 * written.  d_result[0..4): the checked messages with d_valid[m] < len, the
 * lowest such m (UINT64_MAX when there is none), the messages checked, the
 * bytes checked (the sum of their len).  Minima and counts: deterministic.
 * Asynchronous on `stream`.  Latches nothing: invalid UTF-8 is a result, not
 * an error of the call, and wsg_sync is unaffected.  Uses no scratch of the
 * context: it is ordered against nothing (see "Streams" above) and can be
 * captured without a first plain run.  msg_room == 0, which == 0 and
 * d_count[0] == 0 are valid.  WSG_EINVAL for a NULL or misaligned operand.  */
#define WSG_UTF8_TEXT   1u  /* kind == WSG_CB_RECEIVED && opcode == WSG_TEXT            */
#define WSG_UTF8_CLOSE  2u  /* kind == WSG_CB_CLOSE: the reason, d_msg[off, off + len)  */
#define WSG_UTF8_EVERY  4u  /* every record, whatever its kind and opcode               */

int wsg_check_utf8(wsg_ctx* ctx, const uint8_t* d_msg, uint64_t msg_cap,
                   const wsg_msg* d_msgs, const uint64_t* d_count, uint32_t msg_room,
                   uint32_t which, uint64_t* d_valid, uint64_t* d_result, void* stream);

/* ---- UTF-8 checked from the masked wire: no d_msg --------------------------- */
/* (Added without an ABI bump: symbols only.)
 *
 * wsg_check_utf8 over the messages of a frame table, read where they lie in
 * d_wire: masked, cut into fragments, with other frames between them.  The
 * call runs the message plan of wsg_decode_messages itself and unmasks in
 * registers; there is no dense message buffer.
 *
 * Inputs.  d_wire, wire_len, d_frame_start, n, d_stream_first, n_streams as
 * wsg_decode_messages takes them.  d_state is read and NOT written: each
 * stream's sticky opcode is the seed, and a reply call behind this one sees
 * the same seed.  `which`: the WSG_UTF8_* bits.
 * Outputs of the plan.  d_info, d_msgs, d_count[0..1] and the frame-error
 * latch are exactly what wsg_decode_messages writes for the same arguments
 * (with a msg_cap that holds everything: WSG_ENOMEM is never latched);
 * d_msgs[m].off / len describe the dense layout, although no such buffer
 * exists.
 * UTF-8 outputs.  d_valid[0..d_count[0]) (room for n words) and
 * d_result[0..4) are exactly what wsg_check_utf8 writes for that dense layout
 * with msg_room = n and a msg_cap that holds everything: the same selection
 * by `which` from kind and opcode, valid_up_to over the message's callback
 * data, every byte outside [off, off + len) counting as 00 (a close message's
 * two status bytes and the neighbouring message's bytes too), d_valid[m] of
 * an unselected message its len, d_result = {invalid, lowest, checked,
 * bytes}.  Deterministic.
 * Bytes read.  Every payload byte of a delivered frame is loaded once, as
 * part of its aligned 16-byte block; beside that only the up-to-3 message
 * bytes either side of a 4 KiB piece of a frame, where a sequence can cross
 * that edge.  No byte of d_wire at or past the end of its last 16-byte block
 * is read, and bytes at or past wire_len never influence a result.  A frame
 * with an error contributes no bytes, as in the plan.
 * Asynchronous on `stream`.  Nothing but frame errors is latched: invalid
 * text is a result.  The call uses the message plan's scratch of the ctx, so
 * it enters and leaves that order (see "Streams" above), with the usual
 * capture rule: run it once uncaptured with the same n and wire_len first.
 * n == 0, n_streams == 0, which == 0 and empty streams are valid.  WSG_EINVAL
 * for a NULL operand (d_wire when wire_len, the tables when n, d_state when
 * n_streams, d_count, d_result, d_stream_first), d_wire not 16-byte aligned,
 * any other operand not 8-byte aligned (4 for d_stream_first), and under
 * WSG_CHECK=1 for an operand too short for its allocation.  The timing hook
 * brackets the payload kernel.
 * Under WSG_ASSEMBLY_RFC the messages are that rule's: a text message is
 * checked over its own fragments' bytes, whatever control frames lie between
 * them, and d_state[j].ahead is read in the place of its opcode.             */
int wsg_check_utf8_wire(wsg_ctx* ctx, const uint8_t* d_wire, uint64_t wire_len,
                        const uint64_t* d_frame_start, uint32_t n,
                        const uint32_t* d_stream_first, uint32_t n_streams,
                        const wsg_stream_state* d_state, uint32_t which,
                        wsg_msg* d_msgs, uint64_t* d_count /* 2 words */, wsg_recv_info* d_info,
                        uint64_t* d_valid /* n words */, uint64_t* d_result /* 4 words */, void* stream);

/* Length of the longest well-formed UTF-8 prefix of buf[0..len) (RFC 3629);
 * len when the whole buffer is valid.  Host; the rule the kernel runs. */
uint64_t wsg_utf8_valid_up_to(const uint8_t* buf, uint64_t len);

/* ---- protocol: the frame-sequence rules of RFC 6455 checked on the device -- */
/* (Added without an ABI bump, as wsg_decode_messages was: symbols, structs and
 * constants only.)
 *
 * RFC 6455 5.1, 5.2, 5.4, 5.5 and 7.4 (Autobahn groups 2-5 and 7): an endpoint
 * fails a connection with status 1002 for RSV bits without an extension, a
 * reserved opcode, a client frame that is not masked (a server frame that is),
 * a fragmented or over-long control frame, a continuation with nothing to
 * continue, a new data frame inside a message, a close frame with a 1-byte
 * body or an illegal status; with 1009 when a message outgrows its limit.  The
 * reference accepts all of these, so this is a call of its own behind a decode
 * (wsg_decode_batch, wsg_decode_messages, wsg_reply_messages or the _streams
 * forms), from the d_info and d_stream_first it left on the device and two
 * wire bytes per close frame; no synchronisation is needed in between on one
 * stream.
 *
 * State.  Before a frame a stream is (open, bytes): a data message (opcode 1
 * or 2) has begun and not had its FIN frame, and that message's payload bytes
 * so far.  With op = opcode, rsv = b0 & 0x70, a frame leaves the state
 * unchanged when error != 0, op & 8 (control) or op is reserved (3-7, 0xB-0xF);
 * op 1 or 2: bytes = len, open = !fin; op 0: bytes += len (saturating at
 * UINT64_MAX), open = !fin.  The transition applies whether or not the frame
 * violates a rule.
 * Judgement.  A frame's code is the lowest-numbered WSG_PV_* below that
 * applies (a violation wins over WSG_PV_CLOSED); the status is 1002 for codes
 * 2-11, 1009 for WSG_PV_TOO_BIG and for WSG_PV_CLOSED the status the close
 * frame carries (1005 when it is empty): d_wire[payload_off] and
 * d_wire[payload_off + 1], each XOR the key's bytes 0 and 1 when masked, taken
 * big-endian; the legal ones are 1000-1003, 1007-1014 and 3000-4999.  A
 * stream's terminal frame is its first frame with any code; frames behind it
 * are not judged.
 * Outputs.  d_verdict[j]: stream j's terminal frame (`frame` its index in the
 * frame table), all eight bytes 0xFF when it has none (frame == UINT32_MAX,
 * code == WSG_PV_NONE).  d_proto[j] is read as the state before the stream's
 * first frame (open: non-zero) and written as the state after its last frame,
 * or, with d_state (as wsg_decode_messages left it), after frame
 * d_stream_first[j] + d_state[j].consumed - 1, the incoming state when
 * consumed == 0: the state at the point from which the caller resubmits the
 * tail.  Every frame of the stream is judged all the same, and judging the
 * tail again in the next call gives the same verdicts.  d_result[0..3): the
 * streams whose terminal frame is a violation (code >= 2), the lowest such
 * stream (UINT64_MAX when there is none), the streams that closed cleanly.
 * Minima and counts: deterministic.
 * role: WSG_PROTO_ANY (no mask rule), WSG_PROTO_SERVER (judging frames a client
 * sent) or WSG_PROTO_CLIENT.  max_message: 0 for no limit.
 * Asynchronous on `stream`.  Latches nothing: a violation is a result, and
 * wsg_sync is unaffected.  n == 0, n_streams == 0 and empty streams are valid
 * (an empty stream keeps its state and gets the all-0xFF verdict; with
 * n_streams == 0 no frame is judged).  A close status whose two bytes do not
 * lie below wire_len is read as 0.  WSG_EINVAL for a NULL operand other than
 * d_state (d_wire may be NULL when wire_len == 0), a misaligned one (8 bytes;
 * d_stream_first 4) or a role above 2.
 * Streams: the calls share a scratch of the ctx (the frames' streams, scan
 * partials, per-stream states) and are ordered across streams on the device
 * like the wsg_encode_batch and wsg_decode_messages calls (see "Streams"
 * above), with the same capture rule: a captured call is not ordered, and a
 * call that has to grow the scratch must not be captured: run it once with
 * the same n and n_streams first.                                           */
#define WSG_PV_CLOSED         1   /* a legal close frame: not a violation     */
#define WSG_PV_FRAME          2   /* d_info[i].error != 0                     */
#define WSG_PV_RSV            3
#define WSG_PV_OPCODE         4
#define WSG_PV_MASK           5
#define WSG_PV_CTRL_FRAGMENT  6
#define WSG_PV_CTRL_LONG      7
#define WSG_PV_CONT           8
#define WSG_PV_DATA           9
#define WSG_PV_CLOSE_LEN      10
#define WSG_PV_CLOSE_CODE     11
#define WSG_PV_TOO_BIG        12
#define WSG_PV_NONE           0xFF  /* d_verdict: the stream has no terminal frame */

#define WSG_PROTO_ANY     0u
#define WSG_PROTO_SERVER  1u  /* the frames came from a client: they must be masked */
#define WSG_PROTO_CLIENT  2u  /* the frames came from a server: they must not be    */

typedef struct wsg_proto_state {   /* 16 bytes */
    uint64_t bytes;        /* payload bytes of the open message so far               */
    uint8_t  open;         /* a data message has begun and not had its FIN frame     */
    uint8_t  _pad[7];      /* written as 0 */
} wsg_proto_state;

typedef struct wsg_proto_verdict { /* 8 bytes; as one little-endian uint64 it orders by frame first */
    uint8_t  code;         /* WSG_PV_*                                               */
    uint8_t  _pad;
    uint16_t status;       /* the close status the endpoint answers with             */
    uint32_t frame;        /* index of the terminal frame in the frame table         */
} wsg_proto_verdict;

int wsg_check_protocol(wsg_ctx* ctx, const uint8_t* d_wire, uint64_t wire_len,
                       const wsg_recv_info* d_info, uint32_t n,
                       const uint32_t* d_stream_first, uint32_t n_streams,
                       const wsg_stream_state* d_state /* or NULL */,
                       wsg_proto_state* d_proto, uint32_t role, uint64_t max_message,
                       wsg_proto_verdict* d_verdict, uint64_t* d_result, void* stream);

/* One frame judged on the host by the rule the kernel runs: info its record,
 * wire the buffer info->payload_off indexes (read only for a close frame's
 * status; may be NULL otherwise), before the stream's state in front of it.
 * Returns the frame's code (0: none) or WSG_EINVAL; *after (or NULL) gets the
 * state behind the frame, *status (or NULL) the status that goes with the
 * code (0 with code 0).                                                     */
int wsg_proto_judge(const wsg_recv_info* info, const uint8_t* wire, const wsg_proto_state* before,
                    uint32_t role, uint64_t max_message, wsg_proto_state* after, uint16_t* status);

/* ---- the upgrade handshake: a connection's first bytes on the device ------- */
/* (Added without an ABI bump, as wsg_decode_messages was: symbols, a struct
 * and constants only.)
 *
 * A connection's first bytes are its HTTP upgrade request.  wsg_upgrade_streams
 * judges one request per stream exactly as WSSession::onReceived,
 * HTTPRequest::Parse and WebSocket::PerformServerUpgrade do (csrc/wsg_upgrade.h
 * restates them) and writes the bytes to send back.
 * The rule.  The header block ends behind the first "\r\n\r\n" (hend); without
 * one the request is incomplete.  The request line runs to the first "\r\n";
 * with no space in it, or one only, the request is malformed.  The header
 * lines in between are split at "\r\n" (a lone '\r' or '\n' is an ordinary
 * byte); a line with no ':' or with ':' first is malformed; key and value are
 * trimmed of space and tab.  Content-Length (name compared without case, the
 * last one wins, a non-digit is malformed, the value taken mod 2^64) gives
 * clen.  Malformed: 400 "Invalid HTTP request", consumed = hend, decided before
 * the body's completeness.  Fewer than clen bytes behind hend: incomplete.
 * Else consumed = hend + clen, and the bytes behind it are the connection's
 * first frames.  A method other than "GET" gets no response.  Then the headers
 * in order, names compared without case (ASCII): Connection must be "Upgrade",
 * or "keep-alive,Upgrade" once space, \t, \n, \v, \f and \r are removed;
 * Upgrade must be "websocket"; Sec-WebSocket-Key non-empty;
 * Sec-WebSocket-Version "13".  The first failing header ends the walk.  Of
 * the four, counting those in front of it: none seen, not a WebSocket request,
 * no response (whatever failed); all four seen, the 101 response (a failing
 * header behind them no longer counts), its accept value
 * Base64(SHA-1(key || GUID)) over the last Sec-WebSocket-Key value in front of
 * the end of the walk, of any length; otherwise a 400, with the failing
 * header's text, or "Invalid WebSocket response" when none failed.           */
#define WSG_UP_INCOMPLETE      0   /* no header end yet, or the body is short: resubmit with more bytes */
#define WSG_UP_ACCEPTED        1   /* 101 */
#define WSG_UP_BAD_HTTP        2   /* 400: malformed request line or header line */
#define WSG_UP_BAD_CONNECTION  3   /* 400 */
#define WSG_UP_BAD_UPGRADE     4   /* 400 */
#define WSG_UP_EMPTY_KEY       5   /* 400 */
#define WSG_UP_BAD_VERSION     6   /* 400 */
#define WSG_UP_MISSING         7   /* 400: some of the four headers, not all */
#define WSG_UP_NOT_GET         8   /* no response: the HTTP layer's */
#define WSG_UP_NOT_WEBSOCKET   9   /* no response: none of the four headers in front of the walk's end */
#define WSG_UP_TOO_LONG       10   /* incomplete at max_request bytes or more: no response, disconnect */
#define WSG_UPGRADE_RESP_MAX 196   /* the longest response (the 'Connection' 400); the 101 has 148 bytes */

typedef struct wsg_upgrade {      /* 32 bytes */
    uint64_t key_off;   /* absolute wire offset of the trimmed Sec-WebSocket-Key value hashed; 0 if none */
    uint64_t url_off;   /* absolute offset of the request target (for routing / onWSConnecting)          */
    uint32_t key_len, url_len;
    uint32_t resp_len;  /* bytes of this stream's response, 0 when it gets none                          */
    uint16_t status;    /* 101, 400 or 0                                                                 */
    uint8_t  code;      /* WSG_UP_*                                                                      */
    uint8_t  _pad;      /* written as 0 */
} wsg_upgrade;

/* Stream j is d_wire[off, off + len) of d_span[j], one request per stream per
 * call: whatever follows `consumed` is not looked at.  d_up[j]: the outcome;
 * url_off / url_len are set when the request is whole and well-formed HTTP
 * (codes other than INCOMPLETE, TOO_LONG and BAD_HTTP), key_off / key_len when
 * the header walk met a key in front of its end; a length saturates at
 * UINT32_MAX.  d_span[j].consumed: 0 while the request is incomplete (or too
 * long), hend for BAD_HTTP, hend + clen otherwise.  d_span[j].need: hend +
 * clen, saturating, when only the body is missing, else 0.
 * max_request: 0 for no limit; otherwise an incomplete request of len >=
 * max_request gets WSG_UP_TOO_LONG.
 * Responses lie in stream order in d_resp; d_resp_off[0..n_streams] is the
 * exclusive prefix of resp_len.  n_streams * WSG_UPGRADE_RESP_MAX always
 * suffices for resp_cap.  When the total exceeds resp_cap no byte of d_resp
 * is written and WSG_ENOMEM is latched (key n_streams << 8 | code); every
 * table is still final.  d_count[0..4): streams accepted, answered with a
 * 400, WSG_UP_INCOMPLETE, and the response bytes.
 * A span past wire_len, or one that starts before the end of the span before
 * it, is latched as wsg_frame_streams latches it (WSG_EINVAL under stream <<
 * 8 | code); that stream gets WSG_UP_INCOMPLETE, consumed 0 and no response.
 * n_streams == 0 and empty streams are valid.  WSG_EINVAL for a NULL operand,
 * d_wire or d_resp not 16-byte aligned (d_wire readable to the end of its
 * last 16-byte block), another operand not 8-byte aligned.
 * Asynchronous on `stream`.  The call uses wsg_frame_streams' scratch of the
 * ctx and is ordered across streams with those calls, under the same capture
 * rule: run it once uncaptured with the same n_streams before capturing.
 * The onWSConnecting veto stays the caller's: drop the response and route by
 * url_off / url_len.                                                         */
int wsg_upgrade_streams(wsg_ctx* ctx, const uint8_t* d_wire, uint64_t wire_len,
                        wsg_stream_span* d_span, uint32_t n_streams, uint64_t max_request,
                        wsg_upgrade* d_up, uint8_t* d_resp, uint64_t resp_cap,
                        uint64_t* d_resp_off /* n_streams + 1 */, uint64_t* d_count /* 4 */, void* stream);

/* One request judged on the host by the rule the kernels run (host memory, no
 * ctx, no OpenSSL): buf[0, len) as one stream at offset 0.  *out as d_up[j],
 * the response to resp (resp_cap bytes of room; WSG_ENOMEM, with *out,
 * *consumed and *need still written, when it is longer), *consumed and *need
 * as the span's.  resp may be NULL with resp_cap 0.                          */
int wsg_upgrade_judge(const uint8_t* buf, uint64_t len, uint64_t max_request, wsg_upgrade* out,
                      uint8_t* resp, uint32_t resp_cap, uint64_t* consumed, uint64_t* need);

/* ---- the client's half of the upgrade handshake on the device -------------- */
/* (Added without an ABI bump: symbols, a struct and constants only.)
 *
 * A client connection's first bytes are the server's answer to its upgrade
 * request.  wsg_upgrade_client_streams judges one response per stream exactly
 * as WSClient::onReceived, HTTPResponse::Parse and
 * WebSocket::PerformClientUpgrade do (csrc/wsg_upgrade_client.h restates them;
 * DESIGN §26), against the 16-byte nonce the client sent as its key.
 * The rule.  The header block ends behind the first "\r\n\r\n" (hend); without
 * one the response is incomplete.  The status line runs to the first "\r\n".
 * With s1 its first space and s2 the next space behind s1 (or the line's
 * end), it is well-formed only when s1 exists, s1 > 0 and (s1, s2) is exactly
 * three ASCII digits, the status; a reason phrase may be missing.  The header
 * lines are split, trimmed and checked as wsg_upgrade_streams' are, and
 * Content-Length (without case, the last one wins, a non-digit is malformed,
 * mod 2^64) gives clen.  Malformed: WSG_UC_BAD_HTTP, consumed = hend, decided
 * before the body's completeness.  Fewer than clen bytes behind hend:
 * incomplete.  Else consumed = hend + clen, and the bytes behind it are the
 * connection's first frames.  A status other than 101: WSG_UC_NOT_101, the
 * headers are not walked.  Then the headers in order, names compared without
 * case (ASCII): Connection must be "Upgrade" (no keep-alive form on this
 * side); Upgrade must be "websocket"; Sec-WebSocket-Accept is decoded as
 * WS::Base64Decode does (a byte outside the 64-letter alphabet, '=' and
 * blanks among them, is skipped; six bits a letter, a byte whenever eight are
 * held) into `got`, which is compared with expect = SHA-1(Base64(nonce) ||
 * GUID) as strncmp(got, expect, min(|got|, 20)) does: in order, unequal bytes
 * fail and equal NUL bytes pass at once.  So an empty value, a value that
 * decodes to a prefix of the digest, one with more than 20 bytes behind a
 * right digest and one that agrees up to a NUL byte of the digest all pass,
 * as they do in the classes and the reference.  The first failing header ends
 * the walk.  All three seen in front of the walk's end: accepted (a failing
 * header behind them no longer counts); otherwise the failing header's code,
 * or WSG_UC_MISSING when none failed.                                        */
#define WSG_UC_INCOMPLETE      0   /* no header end yet, or the body is short: resubmit with more bytes */
#define WSG_UC_ACCEPTED        1   /* handshaked */
#define WSG_UC_BAD_HTTP        2   /* malformed status line or header line ("Invalid HTTP response") */
#define WSG_UC_BAD_CONNECTION  3
#define WSG_UC_BAD_UPGRADE     4
#define WSG_UC_BAD_ACCEPT      5
#define WSG_UC_MISSING         6   /* some of the three headers missing, none failing ("Invalid WebSocket response") */
#define WSG_UC_NOT_101         7   /* a whole response with another status: no error text, not handshaked */
#define WSG_UC_TOO_LONG        8   /* incomplete at max_response bytes or more: disconnect */

typedef struct wsg_upgrade_reply {   /* 32 bytes */
    uint64_t accept_off;   /* absolute wire offset of the trimmed value of the last Sec-WebSocket-Accept
                              line the walk judged (a failing one is judged); 0 if none */
    uint64_t body_off;     /* absolute offset of the body (hend); set with body_len for a whole, well-formed response */
    uint32_t accept_len, body_len;   /* saturating at UINT32_MAX */
    uint32_t _zero;        /* written as 0 */
    uint16_t status;       /* the three digits, 0 while incomplete / malformed / too long */
    uint8_t  code;         /* WSG_UC_* */
    uint8_t  _pad;         /* written as 0 */
} wsg_upgrade_reply;

/* Stream j is d_wire[off, off + len) of d_span[j], one response per stream per
 * call, judged against d_nonce[16j, 16j + 16): whatever follows `consumed` is
 * not looked at.  d_span[j].consumed: 0 while the response is incomplete (or
 * too long), hend for BAD_HTTP, hend + clen otherwise.  d_span[j].need: hend +
 * clen, saturating, when only the body is missing, else 0.
 * max_response: 0 for no limit; otherwise an incomplete response of len >=
 * max_response gets WSG_UC_TOO_LONG.
 * d_count[0..3): streams accepted, whole but not accepted (codes 2-7),
 * WSG_UC_INCOMPLETE.
 * A span past wire_len, or one that starts before the end of the span before
 * it, is latched as wsg_frame_streams latches it (WSG_EINVAL under stream <<
 * 8 | code); that stream gets WSG_UC_INCOMPLETE, consumed 0 and an otherwise
 * zero record.  n_streams == 0 and empty streams are valid.  WSG_EINVAL for a
 * NULL operand, d_wire or d_nonce not 16-byte aligned (d_wire readable to the
 * end of its last 16-byte block), another operand not 8-byte aligned.
 * Asynchronous on `stream`.  The call uses wsg_frame_streams' scratch of the
 * ctx and is ordered across streams with those calls, under the same capture
 * rule: run it once uncaptured with the same n_streams before capturing.     */
int wsg_upgrade_client_streams(wsg_ctx* ctx, const uint8_t* d_wire, uint64_t wire_len,
                               wsg_stream_span* d_span, uint32_t n_streams,
                               const uint8_t* d_nonce /* 16 * n_streams */, uint64_t max_response,
                               wsg_upgrade_reply* d_up, uint64_t* d_count /* 3 */, void* stream);

/* The requests that go with those nonces.  d_tpl[0, tpl_len) is a request with
 * a 24-byte hole at key_at (what onWSConnecting followed by SetBody()
 * produces, the key's value aside); request j is d_req[j * tpl_len, (j + 1) *
 * tpl_len): the template with Base64(d_nonce[16j, 16j + 16)) in the hole.  No
 * byte of d_req at or behind n * tpl_len is written.
 * WSG_EINVAL for key_at + 24 > tpl_len (so for tpl_len below 24), a NULL
 * operand that n > 0 needs, d_req, d_tpl or d_nonce not 16-byte aligned
 * (d_tpl readable to the end of its last 16-byte block); WSG_ENOMEM, decided
 * on the host with nothing launched, when n * tpl_len > req_cap.
 * Asynchronous on `stream`; no scratch.                                      */
int wsg_upgrade_requests(wsg_ctx* ctx, const uint8_t* d_tpl, uint32_t tpl_len, uint32_t key_at,
                         const uint8_t* d_nonce /* 16 * n */, uint32_t n, uint8_t* d_req, uint64_t req_cap,
                         void* stream);

/* One response judged on the host by the rule the kernels run (host memory, no
 * ctx, no OpenSSL): buf[0, len) as one stream at offset 0 against nonce[16].
 * *out as d_up[j], *consumed and *need (or NULL) as the span's.              */
int wsg_upgrade_client_judge(const uint8_t* buf, uint64_t len, const uint8_t nonce[16], uint64_t max_response,
                             wsg_upgrade_reply* out, uint64_t* consumed, uint64_t* need);

/* One request on the host: out[0, tpl_len) = the template with Base64(nonce)
 * at key_at.  WSG_EINVAL for key_at + 24 > tpl_len or a NULL operand.        */
int wsg_upgrade_request(const uint8_t* tpl, uint32_t tpl_len, uint32_t key_at, const uint8_t nonce[16], uint8_t* out);

/* ---- checked replies: an echo server that fails connections on the device -- */
/* (Added without an ABI bump, as wsg_decode_messages was: symbols and
 * constants only.)
 *
 * wsg_reply_messages with wsg_check_protocol run inside it, in one
 * asynchronous call with no host round trip: replies stop at a stream's
 * terminal frame, a close frame carrying the verdict's status is appended to
 * that stream's range of d_reply, and the peer's own close is answered with a
 * close.  Every payload byte is still read once and written once; the header
 * pass and the protocol check share one d_info.
 *
 * What it runs.  The protocol check runs on the d_info that the plan's header
 * pass has just written, before any reply is sized.  d_info, d_msgs, d_state,
 * d_count[0..1], the frame-error latch and the reply_op / mask / d_send_key
 * rules are exactly those of wsg_reply_messages; every message record is
 * still written, answered or not.
 * d_verdict, d_proto, d_result are as wsg_check_protocol writes them when
 * given this call's d_state (d_proto[j] comes out as the state behind the
 * stream's last consumed frame), d_verdict and d_result taken over the
 * effective verdicts: with d_also == NULL the effective verdict of stream j
 * is the protocol's; otherwise whichever of the two has the lower `frame`,
 * and at equal frames the protocol's unless its code is WSG_PV_CLOSED and
 * d_also[j].code >= 2 (a violation beats a clean close).  An all-0xFF entry
 * of d_also means none.  d_also entries name frames of this call's frame
 * table; an entry whose frame lies outside stream j's range is ignored.
 * Terminal frame.  Let t be the `frame` of stream j's effective verdict, if
 * it has one.  A message of stream j whose FIN frame has an index below t is
 * answered as by wsg_reply_messages; one whose FIN frame is t or behind it
 * gets no reply.  The stream gets one close frame:
 * PrepareSendFrame(WSG_FIN | WSG_CLOSE, mask, NULL, 0, status) with
 * _ws_send_mask = d_send_key[j], status the verdict's with 1005 replaced by
 * 1000 (1005 never goes on the wire, RFC 6455 7.4.1): 4 bytes, 8 when masked
 * (2 and 6 for a d_also entry of status 0, which has no prefix).  It is
 * emitted even when t lies in the stream's tail and the stream has no message
 * at all.  reply_op[WSG_CB_CLOSE] still applies to close-kind messages in
 * front of t; the legal close frame itself is t, so it is answered by this
 * close frame and not twice.
 * Layout.  Every reply belongs to its message's FIN frame, every close frame
 * to its terminal frame, and d_reply holds them in frame order, so a stream's
 * close frame is the last thing in its range.
 *   d_stream_reply[0..n_streams] as wsg_reply_messages; range j includes the
 *                                close frame
 *   d_reply_off[0..d_count[0]]   the reply bytes, close frames included, that
 *                                belong to frames in front of message m's FIN
 *                                frame: the start of an answered message's
 *                                frame, whose length is the frame's own (a
 *                                close frame may lie between it and
 *                                d_reply_off[m+1]); [d_count[0]] is the total
 *   d_close_off[0..n_streams)    the offset of stream j's close frame,
 *                                UINT64_MAX when it has none
 *   d_count[0..5)                messages, bytes of the dense layout, reply
 *                                bytes and reply frames (both with the close
 *                                frames), close frames
 * Sums and counts: deterministic.  wire_len + 14 * n still suffices for
 * reply_cap: the frames of the unanswered message that holds t (or t itself,
 * in the tail) pay for the close frame.  When the total exceeds reply_cap no
 * byte of d_reply is written and WSG_ENOMEM is latched behind every frame
 * error; all tables are final either way.
 * Arguments: checked like both calls' together (WSG_EINVAL for a NULL operand
 * other than d_also and d_send_key, d_wire / d_reply not 16-byte aligned, any
 * other operand not 8-byte aligned (4 for d_stream_first and d_send_key),
 * role > 2).  n == 0, n_streams == 0 and empty streams are valid: no close
 * frame, all-0xFF verdicts, d_close_off all UINT64_MAX.
 * Streams: the call uses two scratches of the ctx, the message plan's and the
 * protocol plan's, and enters and leaves both orders, so it is ordered
 * against every other user of either (see "Streams" above); the capture rule
 * is the usual one: run it once uncaptured with the same n and n_streams
 * first.  The timing hook brackets the gather, as in wsg_reply_messages.
 * Under WSG_ASSEMBLY_RFC the messages and replies are that rule's; the
 * terminal-frame cut, the close frame, d_stream_reply, d_close_off and the
 * wire_len + 14 * n bound mean what they mean above (a message is answered
 * when the frame that ends it lies in front of the terminal frame).          */
#define WSG_PV_UTF8           13  /* wsg_utf8_verdicts: an invalid text message or close reason (1007) */

int wsg_reply_checked(wsg_ctx* ctx, const uint8_t* d_wire, uint64_t wire_len,
                      const uint64_t* d_frame_start, uint32_t n,
                      const uint32_t* d_stream_first, uint32_t n_streams,
                      wsg_stream_state* d_state,
                      wsg_proto_state* d_proto, uint32_t role, uint64_t max_message,
                      const wsg_proto_verdict* d_also /* or NULL */,
                      const uint8_t reply_op[5], int mask, const uint32_t* d_send_key,
                      uint8_t* d_reply, uint64_t reply_cap,
                      uint64_t* d_reply_off, uint64_t* d_stream_reply, uint64_t* d_close_off,
                      wsg_proto_verdict* d_verdict, uint64_t* d_result,
                      wsg_msg* d_msgs, uint64_t* d_count /* 5 words */,
                      wsg_recv_info* d_info, void* stream);

/* Raw bytes to checked replies: wsg_reply_streams with wsg_reply_checked in
 * the place of wsg_reply_messages (no d_also: the frame table does not exist
 * before the call); the same returns and the same lowering of
 * d_span[j].consumed.  An echo server's loop is this call, one send per
 * d_stream_reply range, and a disconnect of every stream whose d_close_off is
 * not UINT64_MAX.                                                            */
int wsg_reply_checked_streams(wsg_ctx* ctx, const uint8_t* d_wire, uint64_t wire_len,
                              wsg_stream_span* d_span, uint32_t n_streams, wsg_stream_state* d_state,
                              uint64_t* d_frame_start, uint32_t frame_cap, uint32_t* d_stream_first,
                              wsg_proto_state* d_proto, uint32_t role, uint64_t max_message,
                              const uint8_t reply_op[5], int mask, const uint32_t* d_send_key,
                              uint8_t* d_reply, uint64_t reply_cap,
                              uint64_t* d_reply_off, uint64_t* d_stream_reply, uint64_t* d_close_off,
                              wsg_proto_verdict* d_verdict, uint64_t* d_result,
                              wsg_msg* d_msgs, uint64_t* d_count, wsg_recv_info* d_info,
                              uint32_t* n_frames_out, void* stream);

/* The result of wsg_check_utf8 as a d_also of wsg_reply_checked, behind
 * wsg_decode_messages + wsg_check_utf8 on the same frame table: every
 * d_also[j] is set to all 0xFF, then to the minimum, as one little-endian
 * word, of {code WSG_PV_UTF8, status 1007, frame = first_frame + nframes - 1}
 * over the stream's messages m < min(d_count[0], msg_room) that `which`
 * selects (the rule of wsg_check_utf8) and whose d_valid[m] < len: the
 * stream's first invalid message fails it at its FIN frame.  Uses no scratch,
 * latches nothing; asynchronous on `stream`.  A validating echo server is
 * wsg_decode_messages -> wsg_check_utf8 -> wsg_utf8_verdicts ->
 * wsg_reply_checked(d_also), all on one stream with no synchronisation.  Its
 * cost: the payload is moved twice, once into d_msg for the check and once
 * into the reply, and the plan runs twice; wsg_reply_validated below is the
 * same server in one call that validates straight from the masked wire.      */
int wsg_utf8_verdicts(wsg_ctx* ctx, const wsg_msg* d_msgs, const uint64_t* d_count, uint32_t msg_room,
                      uint32_t which, const uint64_t* d_valid, uint32_t n_streams,
                      wsg_proto_verdict* d_also, void* stream);

/* ---- validated replies: the checked, validating echo in one call ------------ */
/* (Added without an ABI bump: symbols only.)
 *
 * wsg_reply_checked with the UTF-8 check inside it.  Every output equals what
 * this chain writes on one stream:
 *   wsg_check_utf8_wire(which) -> wsg_utf8_verdicts(which) -> wsg_reply_checked(d_also')
 * where d_also'[j] is the UTF-8 verdict of stream j, or the caller's d_also[j]
 * when d_also is given, the entry is not all 0xFF and names a frame inside
 * stream j's range, or, when both exist, the lower of the two as one
 * little-endian word.  A caller entry outside its stream's range is dropped
 * before that comparison: it never shadows a UTF-8 verdict.  The plan runs
 * once, the payload is read once for the check and once for the reply and
 * written once; no d_msg exists.
 * Arguments: those of wsg_reply_checked, `which` (WSG_UTF8_* bits) behind
 * d_also, and d_valid (n words) and d_utf8_result (4 words) behind d_result,
 * written as wsg_check_utf8_wire writes them; they are final also when the
 * replies latch WSG_ENOMEM.  d_verdict / d_result count the effective
 * verdicts as in wsg_reply_checked: a stream failed for its text shows
 * {WSG_PV_UTF8, 1007, the FIN frame of its first invalid message} and gets
 * the 1007 close frame there, unless the protocol or the caller fails it at
 * an earlier frame.  which == 0 is wsg_reply_checked, byte for byte.
 * WSG_EINVAL as wsg_reply_checked, and for d_utf8_result NULL, d_valid NULL
 * with n > 0, or either not 8-byte aligned.  Streams: as wsg_reply_checked
 * (both scratches of the ctx; the merged verdicts live in the protocol
 * plan's); the timing hook brackets the reply gather.                        */
int wsg_reply_validated(wsg_ctx* ctx, const uint8_t* d_wire, uint64_t wire_len,
                        const uint64_t* d_frame_start, uint32_t n,
                        const uint32_t* d_stream_first, uint32_t n_streams,
                        wsg_stream_state* d_state,
                        wsg_proto_state* d_proto, uint32_t role, uint64_t max_message,
                        const wsg_proto_verdict* d_also /* or NULL */, uint32_t which,
                        const uint8_t reply_op[5], int mask, const uint32_t* d_send_key,
                        uint8_t* d_reply, uint64_t reply_cap,
                        uint64_t* d_reply_off, uint64_t* d_stream_reply, uint64_t* d_close_off,
                        wsg_proto_verdict* d_verdict, uint64_t* d_result,
                        uint64_t* d_valid /* n words */, uint64_t* d_utf8_result /* 4 words */,
                        wsg_msg* d_msgs, uint64_t* d_count /* 5 words */,
                        wsg_recv_info* d_info, void* stream);

/* Raw bytes to validated replies: wsg_reply_checked_streams with
 * wsg_reply_validated (d_also NULL) in the place of wsg_reply_checked; the
 * same returns, the same lowering of d_span[j].consumed and the same refusal
 * while capturing; d_valid has room for frame_cap words.  An echo server's
 * loop is this call and one wsg_sync.  Under WSG_ASSEMBLY_RFC that server is
 * RFC 6455 conformant for control frames between fragments too: a ping inside
 * a fragmented message is answered in the round it arrives, ahead of the
 * echo, the echo holds the message's bytes alone under the message's opcode,
 * and text is validated over those bytes.  Under the default,
 * WSG_ASSEMBLY_REFERENCE, such a ping's bytes join the message (the
 * reference's behaviour).                                                    */
int wsg_reply_validated_streams(wsg_ctx* ctx, const uint8_t* d_wire, uint64_t wire_len,
                                wsg_stream_span* d_span, uint32_t n_streams, wsg_stream_state* d_state,
                                uint64_t* d_frame_start, uint32_t frame_cap, uint32_t* d_stream_first,
                                wsg_proto_state* d_proto, uint32_t role, uint64_t max_message,
                                uint32_t which,
                                const uint8_t reply_op[5], int mask, const uint32_t* d_send_key,
                                uint8_t* d_reply, uint64_t reply_cap,
                                uint64_t* d_reply_off, uint64_t* d_stream_reply, uint64_t* d_close_off,
                                wsg_proto_verdict* d_verdict, uint64_t* d_result,
                                uint64_t* d_valid, uint64_t* d_utf8_result,
                                wsg_msg* d_msgs, uint64_t* d_count, wsg_recv_info* d_info,
                                uint32_t* n_frames_out, void* stream);

/* ---- the carry: the next round's wire built on the device ------------------ */
/* (Added without an ABI bump: one struct and one symbol.)
 *
 * Every _streams call returns d_span[j].consumed and leaves the rest of the
 * stream, a partial frame and the fragments of a message whose FIN frame has
 * not arrived, to be submitted again in front of the connection's next bytes.
 * wsg_carry_streams does that on the device: the last round's wire and span
 * table stay where they are, the host uploads only what it has just read, and
 * one asynchronous call writes the next round's wire and span table.
 *
 * Stream j of the next round is stream j of this one, for every j: no index is
 * compacted, a dropped or finished connection is an empty stream, and the
 * d_state / d_proto tables stay in place from round to round.  Its bytes are
 * tail || new: tail = d_wire[off + consumed, off + len) of d_span[j], new =
 * d_new[off, off + len) of d_read[j] (d_read NULL: no stream has new bytes).
 * d_close_off: NULL, or n_streams words as wsg_reply_checked* /
 * wsg_reply_validated* write them; any value other than UINT64_MAX drops
 * stream j, both parts empty and d_read[j] not looked at.
 *
 * d_next: the streams in index order, stream 0 at 0, each at the next multiple
 * of 16 behind the one before it; the padding up to that multiple, behind the
 * last stream too, is written as 0, so every byte of d_next[0, d_count[0]) is
 * defined, d_count[0] is a multiple of 16, and no byte from d_count[0] on is
 * written.  d_next_span[j] = {off, len = tail + new, consumed 0, need 0} for
 * every j (a dropped stream: len 0, off where it would lie).  d_count[0..4):
 * the bytes of d_next used (the next wire_len), the tail bytes carried, the
 * new bytes taken, the streams dropped.
 *
 * Latched for wsg_sync as wsg_frame_streams latches: WSG_EINVAL under stream
 * << 8 | code for a span wsg_frame_streams would refuse, consumed > len, or,
 * on a stream that is not dropped, a read that runs past new_len; that stream
 * is empty in d_next and the others are unaffected.  WSG_ENOMEM under
 * n_streams << 8 | code when d_count[0] > next_cap: no byte of d_next is
 * written, d_next_span and d_count are final.
 *
 * d_wire, d_new and d_next 16-byte aligned, the sources readable and d_next
 * writable to the end of their last 16-byte block, the tables 8-byte aligned;
 * d_next overlaps neither source and d_next_span is not d_span.  d_wire may be
 * NULL when wire_len is 0, d_new when new_len is 0, d_next when next_cap is 0.
 * n_streams == 0 and a first round over a zeroed span table are valid.
 * WSG_EINVAL for a NULL or misaligned operand or an overlap.  Asynchronous on
 * `stream`, no host synchronisation.  The call uses wsg_frame_streams'
 * scratch of the ctx and is ordered across streams with those calls, under
 * the same capture rule: run it once uncaptured with the same n_streams
 * before capturing.                                                          */
typedef struct wsg_stream_read {
    uint64_t off;   /* stream j's new bytes are d_new[off, off + len) */
    uint64_t len;
} wsg_stream_read;      /* 16 bytes */

int wsg_carry_streams(wsg_ctx* ctx, const uint8_t* d_wire, uint64_t wire_len,
                      const wsg_stream_span* d_span, uint32_t n_streams,
                      const uint64_t* d_close_off /* or NULL */,
                      const uint8_t* d_new, uint64_t new_len, const wsg_stream_read* d_read /* or NULL */,
                      uint8_t* d_next, uint64_t next_cap, wsg_stream_span* d_next_span,
                      uint64_t* d_count /* 4 */, void* stream);

/* ---- relays: a chat server's round, one buffer per room ---------------------- */
/* (Added without an ABI bump: symbols only.)
 *
 * The reference's other server, ws_chat_server / ws_multicast_server, sends
 * every received message to every session (WSServer::MulticastText,
 * ws_server.h:50).  A server's frames are unmasked, so every recipient gets
 * the same bytes: wsg_relay_validated writes a round's received messages,
 * checked and validated as wsg_reply_validated does, once, as unmasked server
 * frames, into one range of d_relay per room.
 *
 * The reply side is wsg_reply_validated's, byte for byte.  d_reply,
 * d_reply_off, d_stream_reply, d_close_off, d_verdict, d_result, d_valid,
 * d_utf8_result, d_msgs, d_info, d_state, d_proto, d_count[0..5) and the
 * latches are what wsg_reply_validated writes for the same arguments; the
 * terminal-frame rule, the close frames and both WSG_ASSEMBLY_* modes are
 * unchanged.  mask and d_send_key belong to the reply side only.
 * relay_op: five bytes indexed by WSG_CB_*, with reply_op's meaning: 0 none,
 * WSG_REPLY_SAME relays under the message's own opcode, any other value is
 * the whole first header byte.  A kind is replied to or relayed, not both:
 * relay_op[k] and reply_op[k] both non-zero is WSG_EINVAL at once (every
 * payload byte is read once for the check, once for the move, written once).
 * With relay_op all zero the call is wsg_reply_validated: d_relay is
 * untouched, d_count[5..8) are 0, every d_relay_off[m] is UINT64_MAX and
 * every d_group_relay entry 0.  The reference's chat server is
 *   reply_op = {0, 0, 0, WSG_FIN | WSG_PONG, 0}
 *   relay_op = {0, WSG_FIN | WSG_TEXT, 0, 0, 0}
 * A conformant server relays with WSG_REPLY_SAME: a binary message sent on as
 * text has not been validated under WSG_UTF8_TEXT.
 * Which messages.  Message m of stream j is relayed when relay_op[kind] is
 * non-zero and the frame that ends the message lies in front of the stream's
 * terminal frame (the rule by which wsg_reply_checked answers).  So an
 * invalid text message is never relayed (its FIN frame is the terminal
 * frame), nor anything of a failed stream behind its failure.
 * The relay frame is what MulticastText / MulticastBinary leave in the
 * server's _ws_send_buffer: PrepareSendFrame(op, false, data, size) with
 * _ws_send_mask 0; for a close-kind message PrepareSendFrame(op, false, NULL,
 * 0, status); the two-byte prefix on control opcodes as wsg_reply_messages
 * writes it.
 * Rooms.  d_order (n_streams 32-bit words, or NULL: the identity) is a
 * permutation of the stream indices; group g is the streams d_order[p] for p
 * in [d_group_first[g], d_group_first[g+1]).  d_group_first (n_groups + 1
 * 32-bit words) starts at 0, ends at n_streams and does not decrease; empty
 * groups are allowed.  d_group_first NULL needs n_groups == 1 and means one
 * room of everyone; n_groups == 0 needs n_streams == 0 (both WSG_EINVAL at
 * once otherwise).
 * Layout.  d_relay (16-byte aligned, overlapping no other operand) holds the
 * relay frames back to back with no padding, ordered by position p and,
 * within a stream, by message.
 *   d_group_relay[0..n_groups]  group g's bytes, which the host sends to every
 *                               member of g, are the one range
 *                               d_relay[d_group_relay[g], d_group_relay[g+1]);
 *                               [n_groups] is the total
 *   d_relay_off[0..d_count[0])  the start of message m's relay frame,
 *                               UINT64_MAX when m is not relayed; nothing
 *                               behind d_count[0] is written
 *   d_count[5..8)               relay bytes, relay frames, 0
 * wire_len + 14 * n always suffices for relay_cap.
 * Errors, latched for wsg_sync behind every frame error (and behind the reply
 * side's WSG_ENOMEM):
 *   WSG_EINVAL  d_order is not a permutation or d_group_first breaks its
 *               rule, keyed by the lowest offending position: a position p
 *               whose entry is >= n_streams or names a stream that a lower
 *               position names; behind every position, an entry g of
 *               d_group_first that is not 0 at g == 0, is below entry g - 1,
 *               or is not n_streams at g == n_groups.  Then no byte of
 *               d_relay is written, d_count[5..8) are 0, every d_relay_off is
 *               UINT64_MAX and every d_group_relay 0; the whole reply side is
 *               final and unaffected.
 *   WSG_ENOMEM  d_count[5] > relay_cap: no byte of d_relay is written and
 *               every table is final.
 * The two capacities are independent: a short reply_cap does not stop the
 * relay, nor the reverse.
 * Arguments: checked as wsg_reply_validated's; in addition WSG_EINVAL for
 * NULL relay_op, NULL d_relay with relay_cap > 0, NULL d_relay_off with
 * n > 0, NULL d_group_relay, d_relay not 16-byte aligned, d_relay_off or
 * d_group_relay not 8-byte aligned, d_order or d_group_first not 4-byte
 * aligned.
 * Streams, capture, timing: as wsg_reply_validated (both scratches, both
 * orders; the relay's plan and piece records live beside the message plan's,
 * under its order); run it once uncaptured with the same n, n_streams and
 * n_groups before capturing.  The timing hook brackets each of the two
 * gathers, the reply's and the relay's: a call counts as two launches (one
 * when relay_op is all zero, none when n == 0: a gather that has nothing to
 * move is not launched).
 * Send order.  To connection j the host sends its group's relay range first,
 * then d_reply[d_stream_reply[j], d_stream_reply[j+1]): a stream's close frame
 * is the last thing in that range, and no data frame may follow a close.     */
int wsg_relay_validated(wsg_ctx* ctx, const uint8_t* d_wire, uint64_t wire_len,
                        const uint64_t* d_frame_start, uint32_t n,
                        const uint32_t* d_stream_first, uint32_t n_streams,
                        wsg_stream_state* d_state,
                        wsg_proto_state* d_proto, uint32_t role, uint64_t max_message,
                        const wsg_proto_verdict* d_also /* or NULL */, uint32_t which,
                        const uint8_t reply_op[5], int mask, const uint32_t* d_send_key,
                        const uint8_t relay_op[5],
                        const uint32_t* d_order /* n_streams, or NULL */,
                        const uint32_t* d_group_first /* n_groups + 1, or NULL */, uint32_t n_groups,
                        uint8_t* d_reply, uint64_t reply_cap,
                        uint64_t* d_reply_off, uint64_t* d_stream_reply, uint64_t* d_close_off,
                        uint8_t* d_relay, uint64_t relay_cap,
                        uint64_t* d_relay_off /* n words */, uint64_t* d_group_relay /* n_groups + 1 words */,
                        wsg_proto_verdict* d_verdict, uint64_t* d_result,
                        uint64_t* d_valid /* n words */, uint64_t* d_utf8_result /* 4 words */,
                        wsg_msg* d_msgs, uint64_t* d_count /* 8 words */,
                        wsg_recv_info* d_info, void* stream);

/* Raw bytes to a chat round: wsg_reply_validated_streams with
 * wsg_relay_validated (d_also NULL) in the place of wsg_reply_validated; the
 * same returns, the same lowering of d_span[j].consumed and the same refusal
 * while capturing; d_relay_off has room for frame_cap words.  A chat server's
 * loop is one upload, wsg_carry_streams, this call and one wsg_sync.         */
int wsg_relay_validated_streams(wsg_ctx* ctx, const uint8_t* d_wire, uint64_t wire_len,
                                wsg_stream_span* d_span, uint32_t n_streams, wsg_stream_state* d_state,
                                uint64_t* d_frame_start, uint32_t frame_cap, uint32_t* d_stream_first,
                                wsg_proto_state* d_proto, uint32_t role, uint64_t max_message,
                                uint32_t which,
                                const uint8_t reply_op[5], int mask, const uint32_t* d_send_key,
                                const uint8_t relay_op[5],
                                const uint32_t* d_order, const uint32_t* d_group_first, uint32_t n_groups,
                                uint8_t* d_reply, uint64_t reply_cap,
                                uint64_t* d_reply_off, uint64_t* d_stream_reply, uint64_t* d_close_off,
                                uint8_t* d_relay, uint64_t relay_cap,
                                uint64_t* d_relay_off, uint64_t* d_group_relay,
                                wsg_proto_verdict* d_verdict, uint64_t* d_result,
                                uint64_t* d_valid, uint64_t* d_utf8_result,
                                wsg_msg* d_msgs, uint64_t* d_count, wsg_recv_info* d_info,
                                uint32_t* n_frames_out, void* stream);

/* ---- batch encode: header pack + mask (PrepareSendFrame over many frames) */
/* Frames are written back to back into d_wire (16-byte aligned, capacity
 * wire_cap bytes).  d_wire_off[0..n] receives each frame's offset;
 * d_wire_off[n] is the total wire length.  Byte-exact with ws.cpp:212-271,
 * including the close-status prefix on CLOSE/PING/PONG opcodes (ws.cpp:215)
 * and the XOR applied even when mask == 0 (ws.cpp:269-270).                  */
int wsg_encode_batch(wsg_ctx* ctx, const uint8_t* d_payload,
                     const wsg_send_desc* d_desc, uint32_t n,
                     uint8_t* d_wire, uint64_t wire_cap,
                     uint64_t* d_wire_off, void* stream);

/* ---- fan-out: one payload, k client keys (k x client-style SendBinary) -- */
/* Frame j = PrepareSendFrame(opcode, mask, payload, len) with
 * _ws_send_mask = d_keys[j]; frames back to back in d_wire, each
 * wsg_frame_size(opcode, mask, len, 0) bytes.  d_wire 16-byte aligned.        */
int wsg_fanout_encode(wsg_ctx* ctx, const uint8_t* d_payload, uint64_t len,
                      const uint32_t* d_keys, uint32_t k, uint8_t opcode,
                      int mask, uint8_t* d_wire, uint64_t wire_cap, void* stream);

/* ---- many messages x k keys in one call (a ws_multicast tick) ----------- */
/* The multicast driver sends `messages_rate` messages per tick to every
 * client (reference performance/ws_multicast_server.cpp:104-114, each through
 * WSServer::Multicast, source/server/ws/ws_server.cpp:36-64); this encodes
 * m messages for k client keys at once.  Frame (i, j) =
 * PrepareSendFrame(opcode[i], mask, message i, len[i]) with _ws_send_mask =
 * d_keys[j]; message i's payload is d_payload + src_off[i].  The k frames of
 * message i lie back to back from wire_off[i] (128-byte aligned; frame j at
 * wire_off[i] + j * wsg_frame_size(opcode[i], mask, len[i], 0)).
 * src_off / len / opcode are HOST arrays of m entries; wire_off (host, m + 1
 * entries) is filled, wire_off[m] = bytes used (checked against wire_cap).   */
int wsg_fanout_encode_many(wsg_ctx* ctx, const uint8_t* d_payload, const uint64_t* src_off, const uint64_t* len,
                           const uint8_t* opcode, uint32_t m, const uint32_t* d_keys, uint32_t k, int mask,
                           uint8_t* d_wire, uint64_t wire_cap, uint64_t* wire_off, void* stream);

/* ---- host-staged entry points (host buffers; PCIe in the path) ---------- */
/* XOR `len` bytes of host `src` into host `dst` with key byte (phase+i)%4 on
 * the GPU (H2D, kernel, D2H), synchronous.  src may equal dst.               */
int wsg_xor_host(wsg_ctx* ctx, const void* src, void* dst, size_t len,
                 uint32_t key, uint32_t phase);
/* Batch decode of a host wire buffer, synchronous, same results as
 * wsg_decode_batch with host pointers (payload_off are wire offsets).  The
 * batch is cut into ~32 MiB segments of whole frames ($WSG_STAGE_MB) that
 * flow through three stream slots, so H2D of one segment, decode of the next
 * and D2H of a third overlap.  Pinned buffers (wsg_host_alloc, or registered)
 * are DMA'd directly; pageable ones are staged through pinned memory.        */
int wsg_decode_batch_host(wsg_ctx* ctx, const uint8_t* wire, uint64_t wire_len,
                          const uint64_t* frame_start, uint32_t n,
                          uint8_t* out, wsg_recv_info* info);

/* Batch encode of host buffers, synchronous, the bytes wsg_encode_batch
 * produces: frames back to back in wire[0..wire_off[n]) (host pointers;
 * wire_off[0..n] is filled).  Segments of ~32 MiB of frames flow through the
 * same three stream slots; each segment's payloads are DMA'd as one range
 * (or gathered through pinned staging when its descriptors are scattered).  */
int wsg_encode_batch_host(wsg_ctx* ctx, const uint8_t* payload, uint64_t payload_len,
                          const wsg_send_desc* desc, uint32_t n,
                          uint8_t* wire, uint64_t wire_cap, uint64_t* wire_off);

/* Page-locked host memory for receive/send buffers (DMA without staging). */
int wsg_host_alloc(size_t bytes, void** out);
int wsg_host_free(void* p);

/* ---- single-frame header helpers (host; same code the kernels run) ------ */
/* Total frame size PrepareSendFrame produces (ws.cpp:215-252).               */
uint64_t wsg_frame_size(uint8_t opcode, int mask, uint64_t len, int32_t status);
/* Write the header (ws.cpp:222-248) into out[0..14); returns its length.     */
int wsg_header_pack(uint8_t opcode, int mask, uint64_t len, int32_t status,
                    uint32_t key, uint8_t* out);
/* Parse a complete header at buf[0..avail) (ws.cpp:320-386).  Returns WSG_OK,
 * or WSG_ETRUNC when avail is too short for the header.                       */
int wsg_header_unpack(const uint8_t* buf, uint64_t avail, wsg_recv_info* info);

/* ---- upgrade handshake (host; reference ws.cpp:26-210) ------------------ */
/* Sec-WebSocket-Accept for a Sec-WebSocket-Key: Base64(SHA-1(key + RFC 6455
 * GUID)), NUL-terminated in out[0..29).                                       */
int wsg_ws_accept(const char* key, size_t key_len, char* out, size_t out_cap);

/* ---- per-connection session (the WebSocket mix-in, ws.h:29) ------------- */
/* A session is the reference's per-connection codec state; its payload
 * mask/unmask runs on the GPU through the owning ctx.                         */
typedef struct wsg_session wsg_session;
/* Receive callback: kind is WSG_CB_* ; status is the close status.           */
#define WSG_CB_RECEIVED 1   /* onWSReceived (ws.cpp:445-450) */
#define WSG_CB_CLOSE    2   /* onWSClose    (ws.cpp:429-443) */
#define WSG_CB_PING     3   /* onWSPing     (ws.cpp:417-421) */
#define WSG_CB_PONG     4   /* onWSPong     (ws.cpp:423-427) */
typedef void (*wsg_receive_cb)(void* user, int kind, const uint8_t* data,
                               size_t size, int status);
int wsg_session_create(wsg_ctx* ctx, wsg_session** out);
int wsg_session_destroy(wsg_session* s);
/* _ws_send_mask as little-endian uint32 (ws.cpp:97 client / :206 server).   */
int wsg_session_set_send_key(wsg_session* s, uint32_t key);
/* PrepareSendFrame (ws.cpp:212): frame copied to out[0..*out_len).           */
int wsg_session_prepare_send(wsg_session* s, uint8_t opcode, int mask,
                             const void* buf, size_t size, int32_t status,
                             uint8_t* out, size_t out_cap, size_t* out_len);
/* PrepareReceiveFrame (ws.cpp:273): callbacks fire synchronously.            */
int wsg_session_prepare_receive(wsg_session* s, const void* buf, size_t size,
                                wsg_receive_cb cb, void* user);
/* RequiredReceiveFrameSize (ws.cpp:458).                                      */
size_t wsg_session_required(wsg_session* s);
/* ClearWSBuffers (ws.cpp:484).                                                */
int wsg_session_clear(wsg_session* s);

/* ---- batched receive over many sessions ---------- */
/* The host framer + session batcher: wsg_rx_feed runs a session's framing
 * state machine (PrepareReceiveFrame's header half, ws.cpp:292-397, the
 * split-header behaviour of SURVEY Q7 included) and appends each completed
 * frame to one page-locked batch; wsg_rx_flush unmasks the batch in one GPU
 * pass (wsg_decode_batch_host) and delivers the frames in arrival order
 * through each session's message logic (ws.cpp:399-452).  Every session sees
 * the callbacks wsg_session_prepare_receive would have fired, in the same
 * order.  Callback data stays valid until the next flush.  One thread.      */
typedef struct wsg_rx wsg_rx;
typedef void (*wsg_rx_cb)(void* user, wsg_session* s, int kind,
                          const uint8_t* data, size_t size, int status);
int wsg_rx_create(wsg_ctx* ctx, wsg_rx** out);
int wsg_rx_destroy(wsg_rx* rx);
int wsg_rx_feed(wsg_rx* rx, wsg_session* s, const void* buf, size_t size);
/* ClearWSBuffers (ws.cpp:484) for a batched session, in delivery order.       */
int wsg_rx_clear(wsg_rx* rx, wsg_session* s);
/* Drop a session's queued frames (before wsg_session_destroy).                */
int wsg_rx_forget(wsg_rx* rx, wsg_session* s);
/* Spread every flush's GPU pass over these devices' PCIe links (one context
 * per device, owned by rx; wsg_decode_batch_host_multi); n = 0: rx's own ctx.
 * Not from inside a flush (WSG_EINVAL).                                       */
int wsg_rx_set_devices(wsg_rx* rx, const int* devices, int n);
/* Complete frames and wire bytes queued for the next flush.                   */
int wsg_rx_pending(wsg_rx* rx, uint32_t* frames, uint64_t* bytes);
int wsg_rx_flush(wsg_rx* rx, wsg_rx_cb cb, void* user, uint32_t* delivered);

/* ---- batched send over many sessions ------------- */
/* wsg_tx_queue records PrepareSendFrame(opcode, mask, buf, size, status) for
 * session s with its current send key (read under its send lock) and copies
 * the payload; wsg_tx_flush encodes every queued frame in one pipelined GPU
 * pass (wsg_encode_batch_host) and hands each frame to `sink` in queue order.
 * The bytes are those wsg_session_prepare_send would produce.  One thread.  */
typedef struct wsg_tx wsg_tx;
typedef void (*wsg_tx_sink)(void* user, wsg_session* s, const uint8_t* frame,
                            size_t size);
int wsg_tx_create(wsg_ctx* ctx, wsg_tx** out);
int wsg_tx_destroy(wsg_tx* tx);
int wsg_tx_queue(wsg_tx* tx, wsg_session* s, uint8_t opcode, int mask,
                 const void* buf, size_t size, int32_t status);
/* Drop a session's queued frames (before wsg_session_destroy).                */
int wsg_tx_forget(wsg_tx* tx, wsg_session* s);
/* The same for the send batch (wsg_encode_batch_host_multi).                 */
int wsg_tx_set_devices(wsg_tx* tx, const int* devices, int n);
int wsg_tx_pending(wsg_tx* tx, uint32_t* frames, uint64_t* payload_bytes);
int wsg_tx_flush(wsg_tx* tx, wsg_tx_sink sink, void* user, uint32_t* sent);

/* ---- multi-GPU: shard, encode, gather to one rank */
/* BASELINE config C5 (1 Mi x 16 KiB frames on the 8 GPUs of a node): the
 * reference has no GPU and no collective; a C++ server that owns a node calls
 * this instead of encoding every frame on its IO threads.  Chunks of `chunk`
 * consecutive frames are dealt round-robin, chunk c to rank c % world; a
 * rank's local batch is its chunks in order (wsg_mgpu_shard_count frames).
 * The gather runs over RCCL (xGMI), loaded at run time.                      */
typedef struct wsg_mgpu wsg_mgpu;
#define WSG_MGPU_ID_BYTES 128
/* One process driving `ndev` GPUs (one ctx and stream per device). */
int wsg_mgpu_create(const int* devices, int ndev, wsg_mgpu** out);
/* One rank of a multi-process group (one process per GPU): rank 0 makes the
 * id with wsg_mgpu_unique_id and the caller hands it to every rank.        */
int wsg_mgpu_unique_id(uint8_t* id);
int wsg_mgpu_create_rank(int device, const uint8_t* id, int rank, int world, wsg_mgpu** out);
int wsg_mgpu_destroy(wsg_mgpu* g);
/* world size, ranks driven by this process, the first of them */
int wsg_mgpu_info(wsg_mgpu* g, int* world, int* nlocal, int* first_rank);
/* codec context of local rank i (its device; wsg_stream gives its stream) */
wsg_ctx* wsg_mgpu_ctx(wsg_mgpu* g, int i);
/* frames of an n_total-frame job that `rank` owns */
uint64_t wsg_mgpu_shard_count(uint64_t n_total, uint32_t chunk, int world, int rank);
/* Encode every local rank's shard and gather the job's frames, in global
 * frame order, to rank `root`.  Arrays of nlocal entries, one per local rank
 * (device buffers on that rank's GPU): d_payload / d_desc / n_local its
 * shard (as wsg_encode_batch), d_wire / wire_cap / d_wire_off its encoded
 * shard (n_local + 1 offsets).  On the root: d_out (capacity out_cap) gets
 * the whole job's wire, d_out_off (n_total + 1, or NULL) its frame offsets.
 * Synchronous; every rank of the group calls it with the same n_total,
 * chunk and root.  times (or NULL): {encode ms, gather ms}, max over the
 * local ranks.                                                              */
int wsg_mgpu_encode_gather(wsg_mgpu* g, uint64_t n_total, uint32_t chunk, const uint8_t* const* d_payload,
                           const wsg_send_desc* const* d_desc, const uint32_t* n_local, uint8_t* const* d_wire,
                           const uint64_t* wire_cap, uint64_t* const* d_wire_off, int root, uint8_t* d_out,
                           uint64_t out_cap, uint64_t* d_out_off, double* times);

/* ---- host batches over several GPUs (one process, no collective) -------- */
/* The host-staged path is PCIe-bound (one x16 link per GPU): a server whose
 * receive/send buffers live in host memory (asio socket buffers) spreads one
 * batch over its GPUs' links.  The frames are cut into contiguous runs
 * of about equal wire bytes; run i goes through ctxs[i]'s host pipeline
 * (wsg_decode_batch_host / wsg_encode_batch_host) on a thread of its own,
 * all runs at once.  Results and status are those of the one-context call
 * on the whole batch (a frame table that is not strictly increasing takes
 * that call on ctxs[0]).  Each context is used by this call alone meanwhile.
 * Only the first context of each device takes a run: two pipelines on one
 * GPU share its link and copy engines and run slower than one
 * ($WSG_HOST_MULTI_SHARE=1 splits over every context given).               */
int wsg_decode_batch_host_multi(wsg_ctx* const* ctxs, int nctx, const uint8_t* wire, uint64_t wire_len,
                                const uint64_t* frame_start, uint32_t n, uint8_t* out, wsg_recv_info* info);
int wsg_encode_batch_host_multi(wsg_ctx* const* ctxs, int nctx, const uint8_t* payload, uint64_t payload_len,
                                const wsg_send_desc* desc, uint32_t n, uint8_t* wire, uint64_t wire_cap,
                                uint64_t* wire_off);
/* The same over the GPUs a wsg_mgpu group drives in this process (its local
 * ranks' contexts).                                                          */
int wsg_mgpu_decode_batch_host(wsg_mgpu* g, const uint8_t* wire, uint64_t wire_len, const uint64_t* frame_start,
                               uint32_t n, uint8_t* out, wsg_recv_info* info);
int wsg_mgpu_encode_batch_host(wsg_mgpu* g, const uint8_t* payload, uint64_t payload_len, const wsg_send_desc* desc,
                               uint32_t n, uint8_t* wire, uint64_t wire_cap, uint64_t* wire_off);

/* ---- kernel timing (measurement hook used by bench.py) ------------------ */
/* on = k > 0: the ctx records HIP events around the dominant payload kernel of
 * every k-th batch call, on the stream it is launched on (k > 1 keeps the
 * event packets' own cost out of most steps); on = 0 disables.               */
int wsg_timing_enable(wsg_ctx* ctx, int on);
/* Sum of the dominant-kernel durations (ms) and launch count since the last
 * reset; synchronizes outstanding events.                                     */
int wsg_timing_read(wsg_ctx* ctx, double* total_ms, uint64_t* launches, int reset);
/* Shortest and longest of those durations (ms) since the last reset (0, 0
 * when none); synchronizes outstanding events, resets nothing.              */
int wsg_timing_minmax(wsg_ctx* ctx, double* min_ms, double* max_ms);

/* ---- the host lane (measurement / test hook) ----------------------------- */
/* Page-locked host batches of at most $WSG_LANE_MAX wire bytes (default 512
 * KiB) whose frame table is strictly increasing, and wsg_xor_host calls of at
 * most that many bytes (and 64 KiB), go to the device's resident lane instead
 * of a launch and a synchronize per call (the C1 echo's reads; the per-call
 * path).  One lane per device serves every context of the process:
 * $WSG_LANE_WGS workgroups (default 8) on a high-priority stream, a mailbox
 * each in host memory; a request is cut into frame groups of about equal
 * bytes (one per idle workgroup, at most $WSG_LANE_GROUPS), each a run of at
 * most 1024 whole frames; a decode with a frame larger than a group's 64 KiB
 * stage, or a request needing more than 32 groups, takes the launch path.
 * A launch ends after $WSG_LANE_IDLE_US (default 2000)
 * without a task and after $WSG_LANE_YIELD_US (default 2000) of running (a
 * running kernel holds up calls that wait for the device to drain); the next
 * call launches it again.  A request unanswered for $WSG_LANE_TIMEOUT_MS
 * (default 5000) gives the lane up: the caller waits up to
 * $WSG_LANE_DRAIN_MS (default 2000) for it to leave and then takes the
 * launch path, or, if it does not leave, returns WSG_EHIP without touching
 * the buffers (the lane may still write them) and the context returns
 * WSG_EHIP from then on (a device free in another context, e.g. its
 * wsg_destroy, waits for that lane to leave).  A lane given up comes back on
 * a later call once it has left, no request is in flight and a hold-off has
 * passed (50 ms, doubling with each give-up in a row up to 4 s); tasks the
 * old lane never took are skipped, not run.  The lane's settings are read
 * when a process first uses a device's lane.
 * Requests this context put on the lane, the launches of the device's lane,
 * and whether it runs now (1), has left (0) or is given up (-1: the launch
 * paths until it comes back).                                               */
int wsg_lane_stats(wsg_ctx* ctx, uint64_t* requests, uint64_t* launches, int* running);
/* How often the device's lane was given up (a request unanswered for
 * $WSG_LANE_TIMEOUT_MS, or a launch that failed) and brought back since the
 * process first used it.                                                    */
int wsg_lane_events(wsg_ctx* ctx, uint64_t* give_ups, uint64_t* rearms);

#ifdef __cplusplus
}
#endif

#endif /* WSG_CAPI_H */
