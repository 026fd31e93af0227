// wsg_lane_device.hip — the host lane's device side on gfx950 (CDNA4): k_lane,
// one resident kernel per device that serves small host batches from
// mailboxes in page-locked host memory (wsg_internal.h has the mailbox
// structs and the protocol, wsg_lane.cpp the host side), and launch_lane.
// Its ops work on host buffers in place, staged through LDS: lane_decode
// (k_decode's rules: frame_parse_b, wsg_device.h), lane_encode (the bytes
// k_encode_small writes: the chunk builder of wsg_small_frame.h) and lane_xor.
#include "wsg_small_frame.h"

namespace wsg {

namespace {

// 16 bytes of host memory in one request past the GPU's caches (the system
// scope of the relaxed atomic loads, sc0 sc1): one snapshot of the 16 bytes.
__device__ __forceinline__ v4u ld16_sys(const void* p)
{
    v4u r;
    asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1\n\ts_waitcnt vmcnt(0)" : "=v"(r) : "v"(p) : "memory");
    return r;
}

// The lane reads its host inputs in whole, coalesced 16-byte blocks into
// LDS, every load of a step issued before any is waited for: one workgroup
// has few requests in flight, and each PCIe round trip costs microseconds
// (a lane-per-frame read of 32-byte descriptors or headers scattered over
// lines took several; one block per lane per round trip, three for an
// echo's read, $WSG_LANE_PROFILE).  `U` blocks per lane at most.
template <int U>
struct LaneLoads {
    v4u v[U];
    __device__ __forceinline__ void load(const uint8_t* __restrict__ src, uint64_t blocks, bool on)
    {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t k = threadIdx.x + uint64_t(u) * LANE_THREADS;
            if (on && k < blocks)
                v[u] = ld16(src + k * CHUNK);
        }
    }
    __device__ __forceinline__ void store(v4u* dst, uint64_t blocks, bool on) const
    {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t k = threadIdx.x + uint64_t(u) * LANE_THREADS;
            if (on && k < blocks)
                dst[k] = v[u];
        }
    }
};

// Encode of one frame group on the lane (frames [f_lo, f_lo + cnt)): its
// offsets and descriptors — and its frames' payload span [plo, phi) when that
// span's 16-B blocks fit LANE_PSTAGE — staged in one round trip, a lane per
// frame builds its head (small_head), then the group's chunks (small_chunks,
// payload windows from LDS): the bytes k_encode_small writes, at the host's
// offsets.  The range's first and last chunk, shared with the neighbouring
// groups (other workgroups), get byte stores.
__device__ __forceinline__ void lane_encode(const uint8_t* __restrict__ payload, uint64_t plo, uint64_t phi,
                                            const wsg_send_desc* __restrict__ desc, uint32_t f_lo, uint32_t cnt,
                                            const uint64_t* __restrict__ wire_off, uint8_t* __restrict__ wire,
                                            uint8_t* lds)
{
    uint64_t* s_off = reinterpret_cast<uint64_t*>(lds);                             // LANE_THREADS + 1 (+1 pad)
    v4u* s_head = reinterpret_cast<v4u*>(lds + 8 * (LANE_THREADS + 2));
    SmallFrame* s_fr = reinterpret_cast<SmallFrame*>(s_head + LANE_THREADS);
    v4u* s_desc = reinterpret_cast<v4u*>(s_fr + LANE_THREADS);                       // 2 blocks per descriptor
    v4u* s_pay = s_desc + 2 * LANE_THREADS;                                          // LANE_PSTAGE
    static_assert(sizeof(wsg_send_desc) == 32 && sizeof(SmallFrame) == 16, "lane LDS layout");
    static_assert(8 * (LANE_THREADS + 2) + 64 * LANE_THREADS + LANE_PSTAGE <= LANE_LDS, "lane LDS layout");
    const uint32_t t = threadIdx.x;
    // the span's aligned blocks (payload + plo rounded down)
    const uint8_t* p0 = payload + plo;
    p0 -= reinterpret_cast<uintptr_t>(p0) & (CHUNK - 1);
    const uint64_t pblocks = phi > plo ? (uint64_t(payload + phi - p0) + CHUNK - 1) / CHUNK : 0;
    const bool staged = pblocks <= LANE_PSTAGE / CHUNK;
    uint64_t off = 0, off_end = 0;
    if (t < cnt)
        off = wire_off[f_lo + t];
    if (t + 1 == cnt)
        off_end = wire_off[f_lo + cnt];
    LaneLoads<2> dl;
    dl.load(reinterpret_cast<const uint8_t*>(desc + f_lo), 2 * uint64_t(cnt), true);
    LaneLoads<LANE_PSTAGE / CHUNK / LANE_THREADS> pl;
    pl.load(p0, pblocks, staged);
    if (t < cnt)
        s_off[t] = off;
    if (t + 1 == cnt)
        s_off[cnt] = off_end;
    dl.store(s_desc, 2 * uint64_t(cnt), true);
    pl.store(s_pay, pblocks, staged);
    __syncthreads();
    if (t < cnt) {
        const Desc d = load_desc(reinterpret_cast<const wsg_send_desc*>(s_desc) + t);
        (void)small_head(d, s_head[t], s_fr[t]);
    }
    __syncthreads();
    if (staged)
        small_chunks(payload, s_off, s_head, s_fr, cnt, wire, t, LANE_THREADS, StagedBlocks{s_pay, p0});
    else
        small_chunks(payload, s_off, s_head, s_fr, cnt, wire, t, LANE_THREADS);
}

// Decode of one frame group on the lane (frame table strictly increasing,
// the group's range at most LANE_STAGE - 64 bytes): the group's frame starts and its
// wire range [lo, hi) — from its first frame's start (0 for the first group)
// to the next group's (wire_len for the last) — plus the 32 bytes a header
// read may look past hi, staged in one round trip; a lane per frame parses
// it (frame_parse_b: k_decode's rules) into LDS, the group's wsg_recv_info go
// out in whole blocks; then the range chunk by chunk: the wire bytes, the
// valid frames' payload bytes XORed with their keys.  Out-of-range and error
// frames' bytes are copied, as k_decode does.  (In place, a header that runs
// past hi — a table breaking the no-overlap contract — may read bytes the
// next group's workgroup has already unmasked, as k_decode's blocks may.)
__device__ __forceinline__ void lane_decode(const uint8_t* __restrict__ wire, uint64_t wire_len, uint64_t lo,
                                            uint64_t hi, const uint64_t* __restrict__ fs, uint32_t n, uint32_t f_lo,
                                            uint32_t cnt, uint8_t* out, wsg_recv_info* __restrict__ info,
                                            uint8_t* lds, uint32_t* s_err)
{
    v4u* s_wire = reinterpret_cast<v4u*>(lds);
    v4u* s_info = reinterpret_cast<v4u*>(lds + LANE_STAGE);                          // 2 blocks per record
    uint64_t* s_pl = reinterpret_cast<uint64_t*>(s_info + 2 * LANE_THREADS);
    uint64_t* s_pe = s_pl + LANE_THREADS;
    uint32_t* s_key = reinterpret_cast<uint32_t*>(s_pe + LANE_THREADS);
    uint64_t* s_fs = reinterpret_cast<uint64_t*>(s_key + LANE_THREADS);               // the group's starts + next
    static_assert(sizeof(wsg_recv_info) == 32, "lane LDS layout");
    static_assert(LANE_STAGE + 60 * LANE_THREADS + 8 <= LANE_LDS, "lane LDS layout");
    const uint32_t t = threadIdx.x;
    const uint64_t sb = lo & ~uint64_t(CHUNK - 1);
    const uint64_t se = min(hi + 32, wire_len);
    const uint64_t wblocks = se > sb ? (se - sb + CHUNK - 1) / CHUNK : 0;   // <= LANE_STAGE / CHUNK (host's groups)
    const auto block = [s_wire, sb](uint64_t a) { return s_wire[(a - sb) / CHUNK]; };
    uint64_t st = 0, nx = wire_len;
    if (t < cnt)
        st = fs[f_lo + t];
    if (t + 1 == cnt && f_lo + cnt < n)
        nx = fs[f_lo + cnt];
    LaneLoads<LANE_STAGE / CHUNK / LANE_THREADS> wl;
    wl.load(wire + sb, wblocks, true);
    if (t < cnt)
        s_fs[t] = st;
    if (t + 1 == cnt)
        s_fs[cnt] = nx;
    wl.store(s_wire, wblocks, true);
    __syncthreads();
    if (t < cnt) {
        const uint64_t st = s_fs[t];
        const uint64_t limit = s_fs[t + 1];   // the next frame's start, wire_len after the last
        wsg_recv_info r;
        const int e = frame_parse_b(block, wire_len, st, limit, r);
        store_info(reinterpret_cast<wsg_recv_info*>(s_info) + t, r);
        const uint64_t pl = e ? st : r.payload_off;
        s_pl[t] = pl;
        s_pe[t] = e ? st : pl + r.len;
        s_key[t] = (e == 0 && r.masked) ? r.key : 0u;
        if (e)
            atomicAdd(s_err, 1u);   // (the host skips its status pass over the records when no frame erred)
    }
    __syncthreads();
    {
        v4u* dst = reinterpret_cast<v4u*>(info + f_lo);
        for (uint32_t k = t; k < 2 * cnt; k += LANE_THREADS)
            dst[k] = s_info[k];
    }
    for (uint64_t p = sb + uint64_t(t) * CHUNK; p < hi; p += uint64_t(LANE_THREADS) * CHUNK) {
        const v4u wv = s_wire[(p - sb) / CHUNK];
        // last frame whose payload starts at or before p (frame 0 if none)
        uint32_t a = 0, b = cnt - 1;
        while (a < b) {
            const uint32_t m = (a + b + 1) >> 1;
            if (s_pl[m] <= p)
                a = m;
            else
                b = m - 1;
        }
        v4u m = {0, 0, 0, 0};
        for (uint32_t j = a; j < cnt; ++j) {
            const uint64_t pl = s_pl[j], pe = s_pe[j];
            if (pl >= p + CHUNK)
                break;
            const uint32_t key = s_key[j];
            if (key == 0 || pe <= p)
                continue;
            if (pl <= p && pe >= p + CHUNK) {   // the chunk lies in this payload
                const uint32_t kw = key_rot(key, uint32_t(p - pl));
                m ^= v4u{kw, kw, kw, kw};
            } else {   // the payload's bytes of the chunk: [max(pl, p), min(pe, p + 16))
                const uint32_t kw = key_rot(key, uint32_t(p - pl));   // (mod 4 also when p < pl)
                const uint64_t b0 = pl > p ? pl - p : 0, b1 = pe - p < CHUNK ? pe - p : CHUNK;
                m ^= v4u{kw, kw, kw, kw} & (low_bytes(b1) & ~low_bytes(b0));
            }
        }
        const v4u w = wv ^ m;
        if (p >= lo && p + CHUNK <= hi) {
            st16nt(out + p, w);
        } else {
            const uint32_t j0 = p < lo ? uint32_t(lo - p) : 0;
            const uint32_t j1 = hi - p < CHUNK ? uint32_t(hi - p) : CHUNK;
            for (uint32_t j = j0; j < j1; ++j)
                out[p + j] = uint8_t(lane_byte(w, j));
        }
    }
}

// Per-call XOR on the lane: the page-locked buffer [buf, buf + len) XORed in
// place, byte i with key byte (phase + i) % 4 (len <= LANE_PSTAGE, buf 16-B
// aligned: the context's stage); every load issued before any is waited for.
__device__ __forceinline__ void lane_xor(uint8_t* buf, uint64_t len, uint32_t key, uint32_t phase)
{
    const uint32_t t = threadIdx.x;
    const uint64_t chunks = len / CHUNK, tail = len & (CHUNK - 1);
    LaneLoads<LANE_PSTAGE / CHUNK / LANE_THREADS> v;
    v.load(buf, chunks, true);
    const uint64_t q = chunks * CHUNK + t;
    const uint32_t tb = t < tail ? uint32_t(buf[q]) : 0u;
    const uint32_t kw = key_rot(key, phase);
#pragma unroll
    for (int u = 0; u < int(LANE_PSTAGE / CHUNK / LANE_THREADS); ++u) {
        const uint64_t k = t + uint64_t(u) * LANE_THREADS;
        if (k < chunks)
            *reinterpret_cast<v4u*>(buf + k * CHUNK) = v.v[u] ^ kw;
    }
    if (t < tail)
        buf[q] = uint8_t(tb ^ key_byte(key, uint32_t(phase + q)));
}

// The lane: W = gridDim.x workgroups, workgroup g serving its mailbox
// (bell->box[g]: the tickets g, g + W, g + 2W, ... in order).  Wave 0 polls
// the next slot's units and the control word, all in one round trip; a
// `stop` there means no task is taken (a request the host gave up on: it
// waits for the lane to leave before it uses the buffers itself).  The workgroups
// never wait on each other: each stages, works and answers alone, so one
// request's PCIe reads and writes spread over as many CUs as it has groups
// (one CU has few requests in flight: one workgroup took ~5 us to stage a 38
// KB read and ~7 us to write it back, round 4).
// The lane's workgroups on the XCDs nearest the PCIe root: block b runs on
// XCC b mod 8 (round-robin dispatch), and a poller on XCCs 0-3 reaches
// page-locked host memory ~0.2 us sooner per round trip than one on 4-7
// (tools/xcd_probe.hip).  Blocks on the other XCCs leave at once; workgroup g
// of the lane is block (g / LANE_NEAR_XCCS) * 8 + g % LANE_NEAR_XCCS.
constexpr uint32_t LANE_XCCS = 8, LANE_NEAR_XCCS = 4;

} // namespace

__global__ __launch_bounds__(LANE_THREADS) void k_lane(LaneBell* __restrict__ bell, uint32_t W, uint64_t idle_ticks,
                                                       uint64_t yield_ticks, uint32_t gen, uint64_t delay_ticks)
{
    __shared__ uint64_t s_w[LANE_WORDS];
    __shared__ int s_go;         // 1: a task in s_w; 0: leave
    __shared__ uint32_t s_err;   // the task's frames with an error (decode)
    __shared__ v4u s_mem[LANE_LDS / 16];   // the op's staging (lane_decode / lane_encode layouts)
    const uint32_t t = threadIdx.x;
    const uint32_t x = blockIdx.x % LANE_XCCS, g = blockIdx.x / LANE_XCCS * LANE_NEAR_XCCS + x;
    if (x >= LANE_NEAR_XCCS || g >= W)
        return;   // (a block-uniform exit before any barrier or memory access)
    uint64_t j = 0;     // (wave 0) this workgroup's mailbox position: ticket g + j W
    uint32_t why = 0;   // (wave 0) why it leaves: 1 idle or yield (announced in `closing`), 2 stop, 3 closing seen
    const LaneTask* box = bell->box[g];
    const uint64_t t_start = wall_clock64();
    if (t < 64) {
        if (delay_ticks) {   // test hook: a lane that starts late (bounded: ~2^20 sleeps)
            for (uint32_t i = 0; i < (1u << 20) && wall_clock64() - t_start < delay_ticks; ++i)
                __builtin_amdgcn_s_sleep(64);
        }
        j = uni(__hip_atomic_load(&bell->next_j[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM));
    }
    for (;;) {
        if (t < 64) {
            const uint64_t want = uint64_t(g) + j * W + 1;
            const LaneTask* task = &box[j % LANE_RING];
            int go = 0;
            if (wall_clock64() - t_start > yield_ticks)
                why = 1;   // running long enough: step aside (calls that wait for the device to drain)
            const uint64_t t0 = wall_clock64();
            // every poll reads all of the slot's units and the control word in
            // one round trip (lanes 0..LANE_WORDS): a task is taken the moment
            // its first unit shows, with no second read.  (A unit still
            // holding the slot's previous task — the reads may be served in
            // any order — is read again; the control word read with a task's
            // first unit: a `stop` set after it is covered by the host, which
            // waits for the lane to leave before it touches the buffers.)
            const void* src = t < LANE_WORDS ? static_cast<const void*>(&task->w[t])
                                             : t == LANE_WORDS ? static_cast<const void*>(&bell->ctl) : nullptr;
            uint64_t val = 0;
            // at most ~2^22 polls of >= 1 us each: ends even if the clock stalls
            for (uint32_t it = 0; !why && it < (1u << 22); ++it) {
                const v4u u = src ? ld16_sys(src) : v4u{0, 0, 0, 0};
                val = uint64_t(u.x) | (uint64_t(u.y) << 32);
                const uint64_t tag = uint64_t(u.z) | (uint64_t(u.w) << 32);
                const uint32_t stop = __builtin_amdgcn_readlane(u.x, LANE_WORDS);
                const uint32_t closing = __builtin_amdgcn_readlane(u.y, LANE_WORDS);
                if (stop) {
                    why = 2;   // given up on by the host (or teardown): no task taken
                    break;
                }
                if (closing == gen) {
                    why = 3;   // another workgroup of this launch left: follow
                    break;
                }
                // (through uint32_t: readlane returns int, and a tag whose low
                // word is 2^31 or more must not sign-extend — every ticket from
                // 2^31 - 1 on would never be taken)
                const uint64_t tag0 = uint64_t(uint32_t(__builtin_amdgcn_readlane(u.z, 0))) |
                                      (uint64_t(uint32_t(__builtin_amdgcn_readlane(u.w, 0))) << 32);
                if (tag0 == want) {
                    if (__ballot(t < LANE_WORDS && tag != want) == 0) {
                        go = 1;
                        break;
                    }
                    continue;   // (part of the slot still the old task: again, at once)
                }
                if ((it & 15) == 15) {
                    const uint64_t now = wall_clock64();
                    if (now - t0 > idle_ticks || now - t_start > yield_ticks)
                        why = 1;
                }
                if (it < 1024)
                    __builtin_amdgcn_s_sleep(1);
                else
                    __builtin_amdgcn_s_sleep(8);   // idle for a while: poll host memory less often
            }
            if (!go && !why)
                why = 1;
            if (go) {
                __atomic_thread_fence(__ATOMIC_ACQUIRE);   // (system scope: the task's host buffers)
                if (t < LANE_WORDS)
                    s_w[t] = val;
            }
            if (t == 0) {
                s_go = go;
                s_err = 0;
            }
        }
        __syncthreads();
        if (!s_go)
            break;
        const uint32_t op = uint32_t(s_w[0]);
        const uint32_t n = uint32_t(s_w[0] >> 32);
        const uint32_t f_lo = uint32_t(s_w[6]), cnt = uint32_t(s_w[6] >> 32);
        uint8_t* lds = reinterpret_cast<uint8_t*>(s_mem);
        if (op == LANE_DECODE && cnt >= 1 && cnt <= LANE_THREADS)
            lane_decode(reinterpret_cast<const uint8_t*>(s_w[1]), s_w[2], s_w[7], s_w[8],
                        reinterpret_cast<const uint64_t*>(s_w[3]), n, f_lo, cnt, reinterpret_cast<uint8_t*>(s_w[4]),
                        reinterpret_cast<wsg_recv_info*>(s_w[5]), lds, &s_err);
        else if (op == LANE_ENCODE && cnt >= 1 && cnt <= LANE_THREADS)
            lane_encode(reinterpret_cast<const uint8_t*>(s_w[1]), s_w[7], s_w[8],
                        reinterpret_cast<const wsg_send_desc*>(s_w[2]), f_lo, cnt,
                        reinterpret_cast<const uint64_t*>(s_w[3]), reinterpret_cast<uint8_t*>(s_w[4]), lds);
        else if (op == LANE_XOR && s_w[2] <= LANE_PSTAGE)
            lane_xor(reinterpret_cast<uint8_t*>(s_w[1]), s_w[2], uint32_t(s_w[3]), uint32_t(s_w[3] >> 32));
        else if (op == LANE_XOR_INLINE) {
            // the payload came with the task (w[4..8]) and the answer goes
            // back as self-tagged units (LaneXres): one dword per lane, one
            // 8-byte store each, no read of host memory and no fence
            if (s_w[2] <= LANE_INLINE && t < (s_w[2] + 3) / 4) {
                const uint32_t d = uint32_t(s_w[4 + t / 2] >> (32 * (t & 1)));
                const uint32_t tag = uint32_t(uint64_t(g) + j * W + 1);
                const uint64_t unit = uint64_t(d ^ key_rot(uint32_t(s_w[3]), uint32_t(s_w[3] >> 32))) |
                                      (uint64_t(tag) << 32);
                __hip_atomic_store(&bell->xres[g][j % LANE_RING].u[t], unit, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_SYSTEM);
            }
            ++j;
            __syncthreads();   // (every wave has read this task's words before wave 0 polls the next)
            continue;          // (every thread: op is block-uniform)
        }
        __syncthreads();
        if (t == 0) {
            __threadfence_system();   // the task's stores are visible to the host before its answer
            LaneResp* r = &bell->resp[g][j % LANE_RING];
            __hip_atomic_store(&r->errs, uint64_t(s_err), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(&r->done, uint64_t(g) + j * W + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        ++j;
    }
    if (t == 0) {
        // where the next launch resumes; then, leaving on its own, the launch
        // announces it ends (the others follow; a waiting caller launches the
        // next generation behind it on the lane's stream)
        __hip_atomic_store(&bell->next_j[g], j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (why == 1)
            __hip_atomic_store(&bell->ctl.closing, gen, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

hipError_t launch_lane(hipStream_t s, LaneBell* bell, uint32_t workgroups, uint64_t idle_ticks,
                       uint64_t yield_ticks, uint32_t gen, uint64_t delay_ticks)
{
    if (workgroups < 1 || workgroups > LANE_WGS_MAX || gen == 0)
        return hipErrorInvalidValue;
    const uint32_t blocks = (workgroups + LANE_NEAR_XCCS - 1) / LANE_NEAR_XCCS * LANE_XCCS;
    k_lane<<<blocks, LANE_THREADS, 0, s>>>(bell, workgroups, idle_ticks, yield_ticks, gen, delay_ticks);
    return hipGetLastError();
}

} // namespace wsg
