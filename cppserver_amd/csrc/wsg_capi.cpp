// wsg_capi.cpp — the core of the C-ABI in include/wsg_capi.h: the context and
// its knobs, wsg_sync, the timing hooks, the header helpers, and the helpers
// the other host sources share (wsg_ctx.h).  The device-resident entry points
// are in wsg_capi_device.cpp, the host-staged ones in wsg_capi_host.cpp, the
// lane in wsg_lane.cpp.  Nothing in them computes payload bytes on the CPU:
// every payload byte of every entry point is produced by a gfx950 kernel.
#include "wsg_ctx.h"
#include "wsg_env.h"
#include "wsg_utf8.h"

#include <cstdlib>
#include <mutex>
#include <new>

void free_enc(wsg_enc_scratch& e)
{
    (void)hipFree(e.d_scan);
    (void)hipFree(e.d_piece_start);
    (void)hipFree(e.d_piece_frame);
    e = wsg_enc_scratch{};
}

int scratch_enter(wsg_scratch_order& o, hipStream_t s, bool* ordered)
{
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    WSG_HIP(hipStreamIsCapturing(s, &cap));
    *ordered = cap == hipStreamCaptureStatusNone;
    if (!*ordered)
        return WSG_OK;
    if (!o.done)
        WSG_HIP(hipEventCreateWithFlags(&o.done, hipEventDisableTiming));
    if (o.recorded && o.last != s)
        WSG_HIP(hipStreamWaitEvent(s, o.done, 0));
    return WSG_OK;
}

int scratch_leave(wsg_scratch_order& o, hipStream_t s, bool ordered)
{
    if (!ordered)
        return WSG_OK;
    WSG_HIP(hipEventRecord(o.done, s));
    o.last = s;
    o.recorded = true;
    return WSG_OK;
}

static int drain_timing(wsg_ctx* c)
{
    for (auto& ev : c->pending) {
        WSG_HIP(hipEventSynchronize(ev.b));
        float ms = 0.f;
        WSG_HIP(hipEventElapsedTime(&ms, ev.a, ev.b));
        c->acc_ms += ms;
        c->min_ms = c->launches ? std::min(c->min_ms, double(ms)) : double(ms);
        c->max_ms = c->launches ? std::max(c->max_ms, double(ms)) : double(ms);
        c->launches += 1;
        c->pool.push_back(ev);
    }
    c->pending.clear();
    return WSG_OK;
}

bool in_alloc(const void* p, uint64_t bytes)
{
    if (bytes == 0)
        return true;
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void*>(p)) != hipSuccess)
        return false;
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(base);
    return a >= b && a - b <= size && bytes <= size - (a - b);
}

// The runtime's first initialization under the environment lock (wsg_env.h):
// every entry point that can be a process's first HIP call goes through here
// before touching HIP or reading a knob.
void wsg::hip_init_once()
{
    static std::once_flag once;
    std::call_once(once, [] {
        std::lock_guard<std::recursive_mutex> g(wsg::env_mutex());
        (void)hipInit(0);
    });
}

int wsg_abi_version(void) { return WSG_ABI_VERSION; }

const char* wsg_strerror(int code)
{
    switch (code) {
    case WSG_OK:
        return "ok";
    case WSG_EINVAL:
        return "invalid argument or overlapping frames";
    case WSG_ETRUNC:
        return "frame runs past the end of the wire";
    case WSG_ENOMEM:
        return "out of memory or output capacity too small";
    case WSG_EHIP:
        return "HIP runtime error";
    default:
        return "unknown error";
    }
}


namespace {

// The context's knobs from the environment, over the defaults wsg_ctx states:
// read once per context in wsg_create (no environment read on any data path);
// a value outside a knob's range leaves its default.
void read_knobs(wsg_ctx* c)
{
    std::lock_guard<std::recursive_mutex> g(wsg::env_mutex());
    const auto ranged = [](const char* e, long lo, long hi, long now) {
        const long v = std::atol(e);
        return v >= lo && v <= hi ? v : now;
    };
    if (const char* e = wsg::envp("WSG_CHECK"))
        c->check = *e == '1';
    if (const char* e = wsg::envp("WSG_LANE_MAX"))
        c->lane_max = std::strtoull(e, nullptr, 10);
    if (const char* e = wsg::envp("WSG_LANE_GROUPS"))
        c->lane_groups = uint32_t(ranged(e, 1, long(wsg::LANE_GROUPS_MAX), c->lane_groups));
    if (const char* e = wsg::envp("WSG_HOST_DIRECT_MAX"))
        c->host_direct_max = std::strtoull(e, nullptr, 10);
    if (const char* e = wsg::envp("WSG_STAGE_MB"))
        c->seg_bytes = std::max<uint64_t>(1, std::strtoull(e, nullptr, 10)) << 20;
    if (const char* e = wsg::envp("WSG_ENC_BLOCKS_PER_CU"))
        c->enc_blocks_per_cu = int(ranged(e, 1, 32768, c->enc_blocks_per_cu));
    if (const char* e = wsg::envp("WSG_ENC_LAUNCH_PIECES"))
        c->enc_launch_pieces = std::strtoull(e, nullptr, 10);
    if (const char* e = wsg::envp("WSG_DEC_BLOCKS_PER_CU"))
        c->dec_blocks_per_cu = int(ranged(e, 1, 4096, c->dec_blocks_per_cu));
    if (const char* e = wsg::envp("WSG_UTF8_BLOCKS_PER_CU"))
        c->utf8_blocks_per_cu = int(ranged(e, 1, 4096, c->utf8_blocks_per_cu));
    if (const char* e = wsg::envp("WSG_UTF8_WIRE_BLOCKS_PER_CU"))
        c->utf8_wire_blocks_per_cu = int(ranged(e, 1, 4096, c->utf8_wire_blocks_per_cu));
    if (const char* e = wsg::envp("WSG_HOST_MULTI_SHARE"))
        c->multi_share = *e == '1';
}

} // namespace

int wsg_create(int device, wsg_ctx** out)
{
    if (!out)
        return WSG_EINVAL;
    *out = nullptr;
    wsg::hip_init_once();
    wsg_ctx* c = nullptr;
    hipDeviceProp_t prop;
    {
        // a device's first use edits the environment as the runtime's
        // initialization does (wsg_env.h): these calls under the environment
        // lock; the synchronize below, which waits for this stream only, not
        std::lock_guard<std::recursive_mutex> env_guard(wsg::env_mutex());
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count)
            return WSG_EHIP;
        c = new (std::nothrow) wsg_ctx();
        if (!c)
            return WSG_ENOMEM;
        c->device = device;
        read_knobs(c);
        if (hipSetDevice(device) != hipSuccess || hipGetDeviceProperties(&prop, device) != hipSuccess ||
            hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
            hipMalloc(&c->d_err, sizeof(unsigned long long)) != hipSuccess ||
            hipMalloc(&c->d_err_host, 2 * sizeof(unsigned long long)) != hipSuccess ||
            hipHostMalloc(&c->h_err_copy, sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess) {
            wsg_destroy(c);
            return WSG_EHIP;
        }
    }
    if (hipMemsetAsync(c->d_err, 0xFF, sizeof(unsigned long long), c->stream) != hipSuccess ||
        hipMemsetAsync(c->d_err_host, 0xFF, 2 * sizeof(unsigned long long), c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) {
        wsg_destroy(c);
        return WSG_EHIP;
    }
    c->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    *out = c;
    return WSG_OK;
}

int wsg_destroy(wsg_ctx* c)
{
    if (!c)
        return WSG_EINVAL;
    if (c->dead) {
        // a lane request of this context neither answered nor drained: the
        // lane may still write its page-locked buffers, and freeing device or
        // page-locked memory waits for a device that may never drain; its
        // memory is left to the process's end
        delete c;
        return WSG_OK;
    }
    (void)hipSetDevice(c->device);
    if (c->stream)
        (void)hipStreamSynchronize(c->stream);
    for (auto& ev : c->pending) {
        (void)hipEventDestroy(ev.a);
        (void)hipEventDestroy(ev.b);
    }
    for (auto& ev : c->pool) {
        (void)hipEventDestroy(ev.a);
        (void)hipEventDestroy(ev.b);
    }
    (void)hipFree(c->d_err);
    (void)hipFree(c->d_err_host);
    if (c->h_err_copy)
        (void)hipHostFree(c->h_err_copy);
    free_enc(c->enc);
    for (hipEvent_t ev : {c->enc_order.done, c->msg_order.done, c->frame_order.done, c->proto_order.done})
        if (ev)
            (void)hipEventDestroy(ev);
    (void)hipFree(c->d_proto_plan);
    (void)hipFree(c->d_frame_plan);
    (void)hipFree(c->d_msg_plan);
    (void)hipFree(c->d_msg_pieces);
    (void)hipFree(c->d_relay_plan);
    (void)hipFree(c->d_relay_pieces);
    (void)hipFree(c->d_stage);
    if (c->h_stage)
        (void)hipHostFree(c->h_stage);
    for (hipStream_t r : {c->s_h2d, c->s_kern, c->s_d2h})
        if (r) {
            (void)hipStreamSynchronize(r);
            (void)hipStreamDestroy(r);
        }
    for (auto& sl : c->slots)
        slot_free(sl);
    if (c->stream)
        (void)hipStreamDestroy(c->stream);
    delete c;
    return WSG_OK;
}

int wsg_set_assembly(wsg_ctx* c, int mode)
{
    if (!c || (mode != WSG_ASSEMBLY_REFERENCE && mode != WSG_ASSEMBLY_RFC))
        return WSG_EINVAL;
    c->assembly = mode;
    return WSG_OK;
}

int wsg_get_assembly(wsg_ctx* c) { return c ? c->assembly : WSG_EINVAL; }

void* wsg_stream(wsg_ctx* c) { return c ? static_cast<void*>(c->stream) : nullptr; }

int wsg_sync(wsg_ctx* c, void* stream)
{
    if (!c)
        return WSG_EINVAL;
    hipStream_t s = as_stream(stream);
    unsigned long long e = kNoError;
    WSG_HIP(hipMemcpyAsync(&e, c->d_err, sizeof(e), hipMemcpyDeviceToHost, s));
    WSG_HIP(hipStreamSynchronize(s));
    if (e == kNoError)
        return WSG_OK;
    WSG_HIP(hipMemsetAsync(c->d_err, 0xFF, sizeof(unsigned long long), s));
    WSG_HIP(hipStreamSynchronize(s));
    return -int(e & 0xFFu);
}

uint64_t wsg_frame_size(uint8_t opcode, int mask, uint64_t len, int32_t status)
{
    const wsg::SendGeom g = wsg::send_geom(opcode, mask != 0, len, status);
    return g.hdr + g.body;
}

uint64_t wsg_utf8_valid_up_to(const uint8_t* buf, uint64_t len)
{
    return buf ? wsg::utf8_valid_up_to(buf, len) : 0;
}

int wsg_header_pack(uint8_t opcode, int mask, uint64_t len, int32_t status, uint32_t key, uint8_t* out)
{
    if (!out)
        return WSG_EINVAL;
    const wsg::SendGeom g = wsg::send_geom(opcode, mask != 0, len, status);
    for (uint32_t r = 0; r < g.hdr; ++r)
        out[r] = wsg::header_byte(opcode, mask != 0, g.body, key, r);
    return int(g.hdr);
}

int wsg_header_unpack(const uint8_t* buf, uint64_t avail, wsg_recv_info* info)
{
    if (!info || (avail && !buf))
        return WSG_EINVAL;
    wsg_recv_info r = {};
    const int e = wsg::parse_header([&](uint32_t k) { return buf[k]; }, avail, r);
    if (e)
        return e;
    r.payload_off = r.hdr_len;
    *info = r;
    return WSG_OK;
}

int wsg_timing_enable(wsg_ctx* c, int on)
{
    if (!c)
        return WSG_EINVAL;
    c->timing = on > 0 ? on : 0;
    c->timing_seq = 0;
    return WSG_OK;
}

int wsg_timing_read(wsg_ctx* c, double* total_ms, uint64_t* launches, int reset)
{
    if (!c)
        return WSG_EINVAL;
    if (int rc = drain_timing(c))
        return rc;
    if (total_ms)
        *total_ms = c->acc_ms;
    if (launches)
        *launches = c->launches;
    if (reset) {
        c->acc_ms = 0.0;
        c->launches = 0;
        c->min_ms = c->max_ms = 0.0;
    }
    return WSG_OK;
}

int wsg_timing_minmax(wsg_ctx* c, double* min_ms, double* max_ms)
{
    if (!c)
        return WSG_EINVAL;
    if (int rc = drain_timing(c))
        return rc;
    if (min_ms)
        *min_ms = c->min_ms;
    if (max_ms)
        *max_ms = c->max_ms;
    return WSG_OK;
}
