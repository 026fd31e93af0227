// wsg_capi_host.cpp — the host-staged entry points of include/wsg_capi.h: the
// registry of page-locked blocks (wsg_host_alloc), the per-call XOR, and the
// batch decode / encode of host buffers: in place where they are page-locked
// and small (the lane, or one launch), else through the three-stream staged
// pipeline and its slots.
#include "wsg_ctx.h"
#include "wsg_env.h"
#include "wsg_trace.h"

#include <atomic>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <map>
#include <mutex>
#include <thread>

namespace {

// Page-locked host memory the kernels read and write in place (the session
// batches' buffers, the direct paths' tables): the runtime's default
// (mapped at the same address on the device).  The lane's system-scope
// acquire / release fences keep its reads and writes of it coherent.
unsigned host_alloc_flags() { return unsigned(hipHostMallocDefault); }

// The blocks wsg_host_alloc made (page-locked, mapped at the same address on
// the device): a host batch in one of them (the session batches' buffers
// always are) is recognised without a runtime query, whose few us per
// pointer were a visible share of a small batch's call (tools/lane_ab.py).
// A block leaves the table before it is freed.
std::mutex& host_blocks_lock()
{
    static std::mutex* m = new std::mutex;   // leaked: used from static destructors
    return *m;
}
std::map<uintptr_t, uint64_t>& host_blocks()
{
    static auto* b = new std::map<uintptr_t, uint64_t>;
    return *b;
}
void host_blocks_add(const void* p, uint64_t bytes)
{
    std::lock_guard<std::mutex> g(host_blocks_lock());
    host_blocks()[reinterpret_cast<uintptr_t>(p)] = bytes;
}
// Bumped by every removal: a thread's cached blocks (in_host_block) are
// trusted only while it is unchanged.
std::atomic<uint64_t> g_blocks_gen{0};
void host_blocks_remove(const void* p)
{
    std::lock_guard<std::mutex> g(host_blocks_lock());
    host_blocks().erase(reinterpret_cast<uintptr_t>(p));
    g_blocks_gen.fetch_add(1, std::memory_order_release);
}
// Each host call checks several pointers (wire, output, table, records):
// under one process-wide lock, eight IO threads queued on it; a thread
// remembers the last blocks it found, valid until a block is removed.
struct BlockHit {
    uintptr_t base = 0;
    uint64_t size = 0;
    uint64_t gen = ~uint64_t(0);
};
thread_local BlockHit t_hits[4] __attribute__((tls_model("initial-exec")));
thread_local uint32_t t_hit_next __attribute__((tls_model("initial-exec"))) = 0;
} // namespace

bool in_host_block(const void* p, uint64_t bytes)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    const uint64_t gen = g_blocks_gen.load(std::memory_order_acquire);
    for (const BlockHit& h : t_hits)
        if (h.gen == gen && a - h.base < h.size && bytes <= h.size - (a - h.base))
            return true;
    std::lock_guard<std::mutex> g(host_blocks_lock());
    auto& m = host_blocks();
    auto it = m.upper_bound(a);
    if (it == m.begin())
        return false;
    --it;
    if (!(a - it->first < it->second && bytes <= it->second - (a - it->first)))
        return false;
    t_hits[t_hit_next++ & 3] = BlockHit{it->first, it->second, gen};
    return true;
}

// The per-call XOR's stage: a device buffer and its page-locked twin.
static int ensure_stage(wsg_ctx* c, uint64_t bytes)
{
    bytes = std::max<uint64_t>((bytes + 15) & ~uint64_t(15), 16);
    if (int rc = ensure_array(c->d_stage, c->d_stage_cap, bytes))
        return rc;
    return ensure_pinned(c->h_stage, c->h_stage_cap, bytes, hipHostMallocDefault);
}

int wsg_host_alloc(size_t bytes, void** out)
{
    if (!out)
        return WSG_EINVAL;
    *out = nullptr;
    wsg::hip_init_once();
    if (hipHostMalloc(out, bytes ? bytes : 1, host_alloc_flags()) != hipSuccess)
        return WSG_ENOMEM;
    host_blocks_add(*out, bytes ? bytes : 1);
    return WSG_OK;
}

int wsg_host_free(void* p)
{
    if (!p)
        return WSG_OK;
    host_blocks_remove(p);
    if (hipHostFree(p) != hipSuccess)
        return WSG_EHIP;
    return WSG_OK;
}

int wsg_xor_host(wsg_ctx* c, const void* src, void* dst, size_t len, uint32_t key, uint32_t phase)
{
    const wsg::TraceRange trace_range("wsg.xor_host");
    if (!c || (len && (!src || !dst)))
        return WSG_EINVAL;
    if (c->dead)
        return WSG_EHIP;
    if (len == 0)
        return WSG_OK;
    if (int rc = ensure_stage(c, len))
        return rc;
    if (len <= std::min<uint64_t>(c->lane_max, wsg::LANE_PSTAGE)) {
        if (LaneServer* ls = lane_for(c)) {
            // a message of the per-call path (PrepareSendFrame /
            // PrepareReceiveFrame outside a batch scope): one lane task on the
            // page-locked stage, no launch and no synchronize; a payload of
            // up to LANE_INLINE bytes (an echo's 32) travels in the task
            const bool inl = len <= wsg::LANE_INLINE;
            uint64_t w[1][wsg::LANE_WORDS];
            lane_task_xor(w[0], c->h_stage, len, key, phase, inl ? src : nullptr);
            if (!inl)
                std::memcpy(c->h_stage, src, len);
            uint64_t errs = 0;
            uint32_t answered = 0;
            uint32_t res[wsg::LANE_INLINE / 4];
            const LaneResult r = inl ? lane_run(c, ls, w, 1, &errs, &answered, uint32_t((len + 3) / 4), res)
                                     : lane_run(c, ls, w, 1, &errs, &answered);
            if (r == LANE_DONE) {
                std::memcpy(dst, inl ? static_cast<const void*>(res) : c->h_stage, len);
                return WSG_OK;
            }
            if (r == LANE_LOST)
                return WSG_EHIP;
            // (the lane has left: the launch path below, from the input)
        }
    }
    std::memcpy(c->h_stage, src, len);
    hipStream_t s = c->stream;
    const uint64_t chunks = ceil_div(len, wsg::CHUNK);
    if (len <= c->xor_direct_max) {
        // small payloads: the kernel reads and writes the page-locked stage
        // itself over PCIe, one launch and one sync instead of H2D + kernel + D2H
        WSG_HIP(wsg::launch_xor(s, grid_for(c, ceil_div(chunks, wsg::BLOCK)), c->h_stage, c->h_stage, len, key, phase));
    } else {
        WSG_HIP(hipMemcpyAsync(c->d_stage, c->h_stage, len, hipMemcpyHostToDevice, s));
        WSG_HIP(wsg::launch_xor(s, grid_for(c, ceil_div(chunks, wsg::BLOCK)), c->d_stage, c->d_stage, len, key, phase));
        WSG_HIP(hipMemcpyAsync(c->h_stage, c->d_stage, len, hipMemcpyDeviceToHost, s));
    }
    WSG_HIP(hipStreamSynchronize(s));   // (polling hipStreamQuery instead: same at 1 thread, -9 % at 4)
    std::memcpy(dst, c->h_stage, len);
    return WSG_OK;
}

#ifndef WSG_COPY_WORKERS
#define WSG_COPY_WORKERS 5   // worker threads of the staged pipelines' host copies (A/B: tools/pcie_pageable.py)
#endif

namespace {

// Large host copies of the staged pipelines (a pageable caller buffer to or
// from the page-locked staging): one core copies ~27 GB/s, and a decode from
// pageable memory makes two such copies per byte (in and out), so one thread
// held the pipeline to 12.9 GiB/s of payload against 40 for page-locked
// buffers (round 4's bench line).  Copies of at least two parts' worth are
// cut into parts done by the calling thread and a few workers (made on first
// use; they park on the queue and are left to the process's end).
class CopyPool
{
public:
    static CopyPool& get()
    {
        static CopyPool* p = new CopyPool;   // leaked: its workers stay parked until the process ends
        return *p;
    }
    void copy(void* dst, const void* src, size_t len)
    {
        const size_t parts = std::min<size_t>(kWorkers + 1, len / kPartMin);
        if (parts <= 1) {
            std::memcpy(dst, src, len);
            return;
        }
        start_workers();
        const size_t per = ((len + parts - 1) / parts + 63) & ~size_t(63);
        std::atomic<size_t> left{0};
        size_t n = 0;
        {
            std::lock_guard<std::mutex> g(m_);
            for (size_t at = per; at < len; at += per, ++n)
                q_.push_back(Job{static_cast<uint8_t*>(dst) + at, static_cast<const uint8_t*>(src) + at,
                                 std::min(per, len - at), &left});
            left.store(n, std::memory_order_relaxed);
        }
        cv_.notify_all();
        std::memcpy(dst, src, std::min(per, len));
        // then help with whatever is queued (this call's parts or another's)
        // and wait for this call's parts
        for (;;) {
            Job j{};
            {
                std::lock_guard<std::mutex> g(m_);
                if (q_.empty())
                    break;
                j = q_.back();
                q_.pop_back();
            }
            run(j);
        }
        while (left.load(std::memory_order_acquire) != 0)
            std::this_thread::yield();
    }

private:
    static constexpr size_t kWorkers = WSG_COPY_WORKERS;
    static constexpr size_t kPartMin = size_t(2) << 20;
    struct Job {
        uint8_t* dst;
        const uint8_t* src;
        size_t len;
        std::atomic<size_t>* left;
    };
    static void run(const Job& j)
    {
        std::memcpy(j.dst, j.src, j.len);
        j.left->fetch_sub(1, std::memory_order_acq_rel);
    }
    void start_workers()
    {
        std::call_once(once_, [this] {
            for (size_t i = 0; i < kWorkers; ++i)
                std::thread([this] {
                    for (;;) {
                        Job j;
                        {
                            std::unique_lock<std::mutex> g(m_);
                            cv_.wait(g, [this] { return !q_.empty(); });
                            j = q_.front();
                            q_.pop_front();
                        }
                        run(j);
                    }
                }).detach();
        });
    }
    std::once_flag once_;
    std::mutex m_;
    std::condition_variable cv_;
    std::deque<Job> q_;
};

void host_copy(void* dst, const void* src, size_t len) { CopyPool::get().copy(dst, src, len); }

} // namespace

// p is page-locked (a wsg_host_alloc block, or so the runtime says);
// direct: and mapped at the same address on the device
static bool host_locked(const void* p, bool direct)
{
    if (in_host_block(p))
        return true;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeHost && (!direct || a.devicePointer == p);
}

bool host_pinned(const void* p) { return host_locked(p, false); }
bool host_direct(const void* p) { return host_locked(p, true); }

namespace {

int slot_init(wsg_ctx::Slot& sl)
{
    if (sl.stream)
        return WSG_OK;
    WSG_HIP(hipStreamCreateWithFlags(&sl.stream, hipStreamNonBlocking));
    WSG_HIP(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
    WSG_HIP(hipEventCreateWithFlags(&sl.h2d_done, hipEventDisableTiming));
    WSG_HIP(hipEventCreateWithFlags(&sl.k_done, hipEventDisableTiming));
    return WSG_OK;
}

// The three role streams a segment's work goes to (made on first use), and
// the hand-offs between them: H2D copies, then kernels, then D2H copies.
int pipe_init(wsg_ctx* c)
{
    for (hipStream_t* r : {&c->s_h2d, &c->s_kern, &c->s_d2h})
        if (!*r)
            WSG_HIP(hipStreamCreateWithFlags(r, hipStreamNonBlocking));
    return WSG_OK;
}

// inputs copied -> kernels may start; kernels done -> copies back may start
int pipe_to_kern(wsg_ctx* c, wsg_ctx::Slot& sl)
{
    WSG_HIP(hipEventRecord(sl.h2d_done, c->s_h2d));
    WSG_HIP(hipStreamWaitEvent(c->s_kern, sl.h2d_done, 0));
    return WSG_OK;
}
int pipe_to_d2h(wsg_ctx* c, wsg_ctx::Slot& sl)
{
    WSG_HIP(hipEventRecord(sl.k_done, c->s_kern));
    WSG_HIP(hipStreamWaitEvent(c->s_d2h, sl.k_done, 0));
    return WSG_OK;
}

// h_in / h_out: a pageable caller's bytes on their way in and out
int slot_reserve_staging(wsg_ctx::Slot& sl, uint64_t bytes)
{
    if (int rc = ensure_pinned(sl.h_in, sl.h_in_cap, bytes, hipHostMallocDefault))
        return rc;
    return ensure_pinned(sl.h_out, sl.h_out_cap, bytes, hipHostMallocDefault);
}

int slot_reserve(wsg_ctx::Slot& sl, uint64_t bytes, uint64_t frames, bool need_host)
{
    if (int rc = slot_init(sl))
        return rc;
    if (int rc = ensure_array(sl.d_wire, sl.wire_cap, bytes + 32))
        return rc;
    if (int rc = ensure_array(sl.d_fs, sl.d_fs_cap, frames))
        return rc;
    if (int rc = ensure_array(sl.d_info, sl.d_info_cap, frames))
        return rc;
    if (int rc = ensure_pinned(sl.h_fs, sl.h_fs_cap, frames, host_alloc_flags()))
        return rc;
    if (int rc = ensure_pinned(sl.h_info, sl.h_info_cap, frames, host_alloc_flags()))
        return rc;
    return need_host ? slot_reserve_staging(sl, bytes + 32) : WSG_OK;
}

int slot_reserve_enc(wsg_ctx::Slot& sl, uint64_t payload_bytes, uint64_t wire_bytes, uint32_t frames,
                     bool need_host)
{
    if (int rc = slot_init(sl))
        return rc;
    if (int rc = ensure_array(sl.d_payload, sl.payload_cap, payload_bytes + 32))
        return rc;
    if (int rc = ensure_array(sl.d_wire, sl.wire_cap, wire_bytes + 32))
        return rc;
    if (int rc = ensure_array(sl.d_desc, sl.desc_cap, frames))
        return rc;
    if (int rc = ensure_array(sl.d_woff, sl.woff_cap, uint64_t(frames) + 1))
        return rc;
    if (int rc = ensure_enc(nullptr, sl.enc, frames, wire_bytes))   // both paths: segments differ
        return rc;
    if (int rc = ensure_pinned(sl.h_desc, sl.h_desc_cap, frames, host_alloc_flags()))
        return rc;
    return need_host ? slot_reserve_staging(sl, std::max(payload_bytes, wire_bytes) + 32) : WSG_OK;
}

} // namespace

void slot_free(wsg_ctx::Slot& sl)
{
    for (void* d : std::initializer_list<void*>{sl.d_wire, sl.d_fs, sl.d_info, sl.d_payload, sl.d_desc, sl.d_woff})
        (void)hipFree(d);
    free_enc(sl.enc);
    for (void* h : std::initializer_list<void*>{sl.h_in, sl.h_out, sl.h_fs, sl.h_info, sl.h_desc})
        if (h)
            (void)hipHostFree(h);
    for (hipEvent_t ev : {sl.done, sl.h2d_done, sl.k_done})
        if (ev)
            (void)hipEventDestroy(ev);
    if (sl.stream)
        (void)hipStreamDestroy(sl.stream);
    sl = wsg_ctx::Slot{};
}

namespace {

// Wait for a slot's previous segment and finish its host-side copies.
int slot_drain(wsg_ctx::Slot& sl)
{
    if (!sl.busy)
        return WSG_OK;
    WSG_HIP(hipEventSynchronize(sl.done));
    if (sl.out_dst && sl.out_len)
        host_copy(sl.out_dst, sl.h_out, sl.out_len);
    for (uint32_t k = 0; k < sl.info_n; ++k) {
        wsg_recv_info r = sl.h_info[k];
        r.payload_off += sl.base;   // segment-relative -> wire offset
        sl.info_dst[k] = r;
    }
    sl.busy = false;
    return WSG_OK;
}

// A segment's bytes on their way back: by DMA into a page-locked destination,
// else into h_out, which slot_drain copies on.
int slot_copy_back(wsg_ctx::Slot& sl, hipStream_t d2h, bool out_pinned, uint8_t* dst, const uint8_t* d_src,
                   uint64_t len)
{
    WSG_HIP(hipMemcpyAsync(out_pinned ? dst : sl.h_out, d_src, len, hipMemcpyDeviceToHost, d2h));
    sl.out_dst = out_pinned ? nullptr : dst;
    sl.out_len = len;
    return WSG_OK;
}

// The batch's frame errors as the one-context call states them: a frame that
// runs into the next one overlaps it (EINVAL) when its whole length lies
// inside the wire; the status is the lowest-indexed bad frame's.
int host_batch_status(wsg_ctx* c, const uint8_t* wire, uint64_t wire_len, const uint64_t* frame_start, uint32_t n,
                      wsg_recv_info* info)
{
    int first = WSG_OK;
    for (uint32_t i = 0; i < n; ++i) {
        wsg_recv_info& r = info[i];
        if (r.error == WSG_ETRUNC && i + 1 < n && frame_start[i] < wire_len) {
            wsg_recv_info h;
            if (wsg_header_unpack(wire + frame_start[i], wire_len - frame_start[i], &h) == WSG_OK &&
                h.len <= wire_len - frame_start[i] - h.hdr_len)
                r.error = int8_t(WSG_EINVAL);
        }
        if (r.error && !first)
            first = r.error;
    }
    if (first) {   // re-arm the host paths' latch, landed before the next call's kernels
        // (a plain hipMemset goes to the null stream, which the context's
        // non-blocking streams do not wait for, and may return before it lands)
        WSG_HIP(hipMemsetAsync(c->d_err_host, 0xFF, sizeof(unsigned long long), c->stream));
        WSG_HIP(hipStreamSynchronize(c->stream));
    }
    return first;
}

// A small host batch in page-locked buffers (a read's frames, echo size):
// k_decode reads the wire and writes the output where they are, over PCIe,
// on the context's stream — one launch and one synchronize instead of the
// pipeline's H2D + kernel + D2H on three streams with event hand-offs.
bool strictly_increasing(const uint64_t* v, uint32_t n)
{
    for (uint32_t i = 1; i < n; ++i)
        if (v[i] <= v[i - 1])
            return false;
    return true;
}

// In-place decodes of at least this many frames on the launch path read the
// error latch back instead of scanning every record for the status.
constexpr uint32_t kLatchFrames = 4096;

int decode_host_direct(wsg_ctx* c, const uint8_t* wire, uint64_t wire_len, const uint64_t* frame_start, uint32_t n,
                       uint8_t* out, wsg_recv_info* info)
{
    wsg_ctx::Slot& sl = c->slots[0];
    if (int rc = slot_reserve(sl, 0, n, false))
        return rc;
    // a table and records in wsg_host_alloc blocks (the batch classes') are
    // used where they are; others through the slot's page-locked copies
    const uint64_t* fs_dev = frame_start;
    if (!in_host_block(frame_start, uint64_t(n) * sizeof(uint64_t))) {
        std::memcpy(sl.h_fs, frame_start, size_t(n) * sizeof(uint64_t));
        fs_dev = sl.h_fs;
    }
    wsg_recv_info* info_dev =
        in_host_block(info, uint64_t(n) * sizeof(wsg_recv_info)) ? info : sl.h_info;
    LaneServer* ls = nullptr;
    LaneGroup grp[wsg::LANE_GROUPS_MAX];
    uint32_t groups = 0;
    if (wire_len <= c->lane_max && n > 0 && n <= kLaneMaxFrames && strictly_increasing(frame_start, n) &&
        (ls = lane_for(c)) &&
        (groups = lane_plan(n, lane_want(c, ls), wsg::LANE_STAGE - 64, true, [&](uint32_t i) -> uint64_t {
             return i == 0 ? 0 : i < n ? std::min(frame_start[i], wire_len) : wire_len;
         }, grp))) {
        // an echo's read, up to a few MiB: the device's resident lane, no
        // launch; group k's wire range from its first start (0 for the first)
        // to the next group's (wire_len after the last), staged whole in LDS
        uint64_t w[wsg::LANE_GROUPS_MAX][wsg::LANE_WORDS];
        for (uint32_t k = 0; k < groups; ++k)
            lane_task_decode(w[k], n, wire, wire_len, fs_dev, out, info_dev, grp[k]);
        uint64_t errs = 0;
        uint32_t answered = 0;
        const LaneResult r = lane_run(c, ls, w, groups, &errs, &answered);
        if (r == LANE_DONE) {
            if (info_dev != info)
                std::memcpy(info, info_dev, size_t(n) * sizeof(wsg_recv_info));
            // no frame erred (the lane's count): nothing for the status pass to
            // find, and the records the GPU just wrote stay out of this core's
            // caches unless the caller reads them
            return errs ? host_batch_status(c, wire, wire_len, frame_start, n, info) : WSG_OK;
        }
        // given up on the lane: its answered groups have unmasked their bytes
        // (in place: a second pass would mask them again), and a lane that did
        // not leave may still write the buffers
        if (r == LANE_LOST || (answered && out == wire))
            return WSG_EHIP;
    }
    hipStream_t s = c->stream;
    if (int rc = decode_launch(c, wire, wire_len, fs_dev, n, out, info_dev, s, c->d_err_host))
        return rc;
    // many frames: the latch read back beside the kernel (an 8-byte copy on
    // the same stream) says whether any frame erred; none did, and the status
    // pass over n records the GPU just wrote to host memory (~2 ns a frame,
    // 0.2 ms at 100 K frames) is skipped, as the lane's error count skips it
    const bool latch = n >= kLatchFrames;
    if (latch)
        WSG_HIP(hipMemcpyAsync(c->h_err_copy, c->d_err_host, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    WSG_HIP(hipStreamSynchronize(s));
    if (info_dev != info)
        std::memcpy(info, info_dev, size_t(n) * sizeof(wsg_recv_info));
    if (latch && *c->h_err_copy == ~0ull)
        return WSG_OK;
    return host_batch_status(c, wire, wire_len, frame_start, n, info);
}

} // namespace

int wsg_decode_batch_host(wsg_ctx* c, const uint8_t* wire, uint64_t wire_len, const uint64_t* frame_start,
                          uint32_t n, uint8_t* out, wsg_recv_info* info)
{
    const wsg::TraceRange trace_range("wsg.decode_batch_host");
    try {   // no C++ exception leaves the ABI (host vectors: WSG_ENOMEM)
        if (!c || (wire_len && (!wire || !out)) || (n && (!frame_start || !info)))
            return WSG_EINVAL;
        if (c->dead)
            return WSG_EHIP;
        if (n == 0) {
            if (wire_len && out != wire)
                std::memmove(out, wire, wire_len);
            return WSG_OK;
        }
        const uint64_t seg_bytes = c->seg_bytes;
        const bool in_pinned = host_pinned(wire), out_pinned = host_pinned(out);
        if (in_pinned && out_pinned && wire_len <= c->host_direct_max && aligned16(wire) && aligned16(out) &&
            host_direct(wire) && host_direct(out))
            return decode_host_direct(c, wire, wire_len, frame_start, n, out, info);

        // segments: runs of whole frames of about seg_bytes; segment k covers wire
        // bytes [start of its first frame, start of the next segment's first frame)
        std::vector<uint32_t> cut{0};
        {
            uint64_t from = 0;
            for (uint32_t i = 1; i < n; ++i) {
                if (frame_start[i] >= wire_len)
                    break;   // frames past the wire: error frames, kept with the last segment
                if (frame_start[i] > from && frame_start[i] - from >= seg_bytes) {
                    cut.push_back(i);
                    from = frame_start[i];
                }
            }
            cut.push_back(n);
        }
        const size_t nseg = cut.size() - 1;
        uint64_t max_bytes = 0, max_frames = 0;
        auto seg_lo = [&](size_t k) { return k == 0 ? uint64_t(0) : std::min(frame_start[cut[k]], wire_len); };
        auto seg_hi = [&](size_t k) { return k + 1 == nseg ? wire_len : std::min(frame_start[cut[k + 1]], wire_len); };
        for (size_t k = 0; k < nseg; ++k) {
            const uint64_t base = seg_lo(k) & ~uint64_t(15);
            max_bytes = std::max(max_bytes, std::max(seg_hi(k), seg_lo(k)) - base);
            max_frames = std::max<uint64_t>(max_frames, cut[k + 1] - cut[k]);
        }
        for (auto& sl : c->slots)
            if (int rc = slot_reserve(sl, max_bytes, max_frames, !in_pinned || !out_pinned))
                return rc;
        if (int rc = pipe_init(c))
            return rc;

        for (size_t k = 0; k < nseg; ++k) {
            wsg_ctx::Slot& sl = c->slots[k % wsg_ctx::kSlots];
            if (int rc = slot_drain(sl))
                return rc;
            const uint32_t i0 = cut[k], i1 = cut[k + 1], m = i1 - i0;
            const uint64_t lo = seg_lo(k), hi = std::max(seg_hi(k), lo);
            const uint64_t base = lo & ~uint64_t(15);   // 16-B aligned device copy of [base, hi)
            const uint64_t len = hi - base;
            for (uint32_t j = 0; j < m; ++j)
                sl.h_fs[j] = frame_start[i0 + j] >= base ? frame_start[i0 + j] - base : ~uint64_t(0);
            const uint8_t* src = wire + base;
            if (!in_pinned) {
                host_copy(sl.h_in, wire + base, len);
                src = sl.h_in;
            }
            WSG_HIP(hipMemcpyAsync(sl.d_wire, src, len, hipMemcpyHostToDevice, c->s_h2d));
            WSG_HIP(hipMemcpyAsync(sl.d_fs, sl.h_fs, m * sizeof(uint64_t), hipMemcpyHostToDevice, c->s_h2d));
            if (int rc = pipe_to_kern(c, sl))
                return rc;
            if (int rc = decode_launch(c, sl.d_wire, len, sl.d_fs, m, sl.d_wire, sl.d_info, c->s_kern, c->d_err_host))
                return rc;
            if (int rc = pipe_to_d2h(c, sl))
                return rc;
            // copy back [lo, hi): bytes before lo belong to the previous segment
            if (int rc = slot_copy_back(sl, c->s_d2h, out_pinned, out + lo, sl.d_wire + (lo - base), hi - lo))
                return rc;
            WSG_HIP(hipMemcpyAsync(sl.h_info, sl.d_info, m * sizeof(wsg_recv_info), hipMemcpyDeviceToHost, c->s_d2h));
            sl.info_dst = info + i0;
            sl.info_n = m;
            sl.base = base;
            WSG_HIP(hipEventRecord(sl.done, c->s_d2h));
            sl.busy = true;
        }
        for (auto& sl : c->slots)
            if (int rc = slot_drain(sl))
                return rc;
        // the pipeline's kernels latched into d_err_host (segment-relative frame
        // indices, meaningless to the caller); the status comes from the
        // per-frame errors below, and the caller's own latch is left alone.
        // Many frames: the latch (every kernel has finished: the slots have
        // drained) read back first, and an untouched one skips the pass
        if (n >= kLatchFrames) {
            WSG_HIP(hipMemcpyAsync(c->h_err_copy, c->d_err_host, sizeof(unsigned long long), hipMemcpyDeviceToHost,
                                   c->stream));
            WSG_HIP(hipStreamSynchronize(c->stream));
            if (*c->h_err_copy == ~0ull)
                return WSG_OK;
        }

        // batch semantics: a frame that runs into the next segment's first frame
        // overlaps it (EINVAL), it is not truncated; and the status is the error
        // of the lowest-indexed bad frame (every slot has drained)
        return host_batch_status(c, wire, wire_len, frame_start, n, info);
    } catch (...) {
        return WSG_ENOMEM;
    }
}

namespace {

// A small batch in page-locked buffers (the frames a tick sends), its offsets
// computed: the kernels read the payloads and write the frames where they
// are, one launch sequence and one synchronize (decode_host_direct's twin).
int encode_host_direct(wsg_ctx* c, const uint8_t* payload, const wsg_send_desc* desc, uint32_t n, uint8_t* wire,
                       uint64_t* wire_off)
{
    wsg_ctx::Slot& sl = c->slots[0];
    if (int rc = slot_reserve_enc(sl, 0, wire_off[n], n, false))
        return rc;
    // descriptors and offsets in wsg_host_alloc blocks (the batch classes')
    // are read where they are; others through copies
    const wsg_send_desc* desc_dev = desc;
    if (!in_host_block(desc, uint64_t(n) * sizeof(wsg_send_desc))) {
        std::memcpy(sl.h_desc, desc, size_t(n) * sizeof(wsg_send_desc));
        desc_dev = sl.h_desc;
    }
    LaneServer* ls = nullptr;
    LaneGroup grp[wsg::LANE_GROUPS_MAX];
    uint32_t groups = 0;
    if (wire_off[n] <= c->lane_max && n <= kLaneMaxFrames && (ls = lane_for(c)) &&
        (groups = lane_plan(n, lane_want(c, ls), wsg::LANE_PSTAGE - 64, false,
                            [&](uint32_t i) -> uint64_t { return wire_off[i]; }, grp))) {
        // the replies of an echo's read, up to a few MiB: the device's
        // resident lane at the offsets computed above, no launch; groups of
        // about equal wire bytes, each group's payload span for its staging
        const uint64_t* off_dev = wire_off;
        if (!in_host_block(wire_off, (uint64_t(n) + 1) * sizeof(uint64_t))) {
            if (int rc = slot_reserve(sl, 0, uint64_t(n) + 1, false))
                return rc;
            std::memcpy(sl.h_fs, wire_off, (size_t(n) + 1) * sizeof(uint64_t));
            off_dev = sl.h_fs;
        }
        uint64_t w[wsg::LANE_GROUPS_MAX][wsg::LANE_WORDS];
        for (uint32_t k = 0; k < groups; ++k) {
            const uint32_t f = grp[k].f, cnt = grp[k].cnt;
            uint64_t lo = UINT64_MAX, hi = 0;
            for (uint32_t i = f; i < f + cnt; ++i)
                if (desc[i].len) {
                    lo = std::min(lo, desc[i].src_off);
                    hi = std::max(hi, desc[i].src_off + desc[i].len);
                }
            lane_task_encode(w[k], n, payload, desc_dev, off_dev, wire, grp[k], hi ? lo : 0, hi);
        }
        uint64_t errs = 0;
        uint32_t answered = 0;
        const LaneResult r = lane_run(c, ls, w, groups, &errs, &answered);
        if (r == LANE_DONE)
            return WSG_OK;
        if (r == LANE_LOST)
            return WSG_EHIP;   // (the lane may still write the frames)
        // given up on the lane, which has left: the launch path writes every frame again
    }
    hipStream_t s = c->stream;
    if (int rc = encode_launch(c, s, payload, desc_dev, n, wire, wire_off[n], sl.d_woff, sl.enc, c->d_err_host + 1))
        return rc;
    WSG_HIP(hipStreamSynchronize(s));
    return WSG_OK;   // capacity was checked on the host: nothing for the latch to report
}

} // namespace

int wsg_encode_batch_host(wsg_ctx* c, const uint8_t* payload, uint64_t payload_len, const wsg_send_desc* desc,
                          uint32_t n, uint8_t* wire, uint64_t wire_cap, uint64_t* wire_off)
{
    const wsg::TraceRange trace_range("wsg.encode_batch_host");
    try {   // no C++ exception leaves the ABI (host vectors: WSG_ENOMEM)
        if (!c || !wire_off || (n && (!desc || !wire)) || (payload_len && !payload))
            return WSG_EINVAL;
        if (c->dead)
            return WSG_EHIP;
        // frame offsets on the host (the same arithmetic as k_encode_scan_*), so
        // that segments can be cut and copied back without a device round trip
        wire_off[0] = 0;
        for (uint32_t i = 0; i < n; ++i) {
            const wsg_send_desc& d = desc[i];
            if (d.len > payload_len || d.src_off > payload_len - d.len)
                return WSG_EINVAL;
            const wsg::SendGeom g = wsg::send_geom(d.opcode, d.mask != 0, d.len, d.status);   // = wsg_frame_size
            wire_off[i + 1] = wire_off[i] + g.hdr + g.body;
        }
        if (wire_off[n] > wire_cap)
            return WSG_ENOMEM;
        if (n == 0)
            return WSG_OK;
        const uint64_t seg_bytes = c->seg_bytes;
        const bool in_pinned = host_pinned(payload), out_pinned = host_pinned(wire);
        if (in_pinned && out_pinned && wire_off[n] <= c->host_direct_max && aligned16(wire) && n <= (1u << 20) &&
            host_direct(wire) && (payload_len == 0 || host_direct(payload)))
            return encode_host_direct(c, payload, desc, n, wire, wire_off);

        // segments of whole frames, ~seg_bytes of wire each
        struct Seg {
            uint32_t i0, i1;
            uint64_t lo, hi;   // payload source range [lo, hi) (16-B aligned lo)
            uint64_t sum;      // payload bytes of its frames
            bool gather;       // frames' payloads not one tight range: copy them together
        };
        std::vector<Seg> segs;
        for (uint32_t i0 = 0; i0 < n;) {
            Seg g{i0, i0, ~uint64_t(0), 0, 0, false};
            do {
                const wsg_send_desc& d = desc[g.i1];
                if (d.len) {
                    g.lo = std::min(g.lo, d.src_off);
                    g.hi = std::max(g.hi, d.src_off + d.len);
                }
                g.sum += d.len;
                ++g.i1;
            } while (g.i1 < n && wire_off[g.i1] - wire_off[i0] < seg_bytes);
            if (g.lo > g.hi)
                g.lo = g.hi = 0;
            g.lo &= ~uint64_t(15);
            g.gather = g.hi - g.lo > g.sum + 16 * uint64_t(g.i1 - g.i0) + 4096;
            segs.push_back(g);
            i0 = g.i1;
        }
        uint64_t max_payload = 0, max_wire = 0;
        uint32_t max_frames = 0;
        bool need_host = !out_pinned;
        for (const Seg& g : segs) {
            max_payload = std::max(max_payload, g.gather ? g.sum : g.hi - g.lo);
            max_wire = std::max(max_wire, wire_off[g.i1] - wire_off[g.i0]);
            max_frames = std::max(max_frames, g.i1 - g.i0);
            need_host = need_host || g.gather || !in_pinned;
        }
        for (auto& sl : c->slots)
            if (int rc = slot_reserve_enc(sl, max_payload, max_wire, max_frames, need_host))
                return rc;
        if (int rc = pipe_init(c))
            return rc;

        for (size_t k = 0; k < segs.size(); ++k) {
            const Seg& g = segs[k];
            wsg_ctx::Slot& sl = c->slots[k % wsg_ctx::kSlots];
            if (int rc = slot_drain(sl))
                return rc;
            const uint32_t m = g.i1 - g.i0;
            const uint8_t* src = payload + g.lo;
            uint64_t plen = g.hi - g.lo;
            if (g.gather) {
                uint64_t at = 0;
                for (uint32_t j = 0; j < m; ++j) {
                    wsg_send_desc d = desc[g.i0 + j];
                    if (d.len)
                        std::memcpy(sl.h_in + at, payload + d.src_off, d.len);
                    d.src_off = at;
                    sl.h_desc[j] = d;
                    at += d.len;
                }
                src = sl.h_in;
                plen = at;
            } else {
                for (uint32_t j = 0; j < m; ++j) {
                    wsg_send_desc d = desc[g.i0 + j];
                    d.src_off = d.len ? d.src_off - g.lo : 0;
                    sl.h_desc[j] = d;
                }
                if (!in_pinned && plen) {
                    host_copy(sl.h_in, src, plen);
                    src = sl.h_in;
                }
            }
            if (plen)
                WSG_HIP(hipMemcpyAsync(sl.d_payload, src, plen, hipMemcpyHostToDevice, c->s_h2d));
            WSG_HIP(hipMemcpyAsync(sl.d_desc, sl.h_desc, m * sizeof(wsg_send_desc), hipMemcpyHostToDevice, c->s_h2d));
            if (int rc = pipe_to_kern(c, sl))
                return rc;
            const uint64_t wlen = wire_off[g.i1] - wire_off[g.i0];
            if (int rc = encode_launch(c, c->s_kern, sl.d_payload, sl.d_desc, m, sl.d_wire, wlen, sl.d_woff, sl.enc,
                                       c->d_err_host + 1))
                return rc;
            if (int rc = pipe_to_d2h(c, sl))
                return rc;
            if (int rc = slot_copy_back(sl, c->s_d2h, out_pinned, wire + wire_off[g.i0], sl.d_wire, wlen))
                return rc;
            sl.info_n = 0;
            WSG_HIP(hipEventRecord(sl.done, c->s_d2h));
            sl.busy = true;
        }
        for (auto& sl : c->slots)
            if (int rc = slot_drain(sl))
                return rc;
        // the encode kernels latch only capacity errors, and capacity was checked
        // on the host above: nothing for the pipeline's latch to report
        return WSG_OK;
    } catch (...) {
        return WSG_ENOMEM;
    }
}
