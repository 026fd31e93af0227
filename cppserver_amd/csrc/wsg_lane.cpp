// wsg_lane.cpp — the host side of the device's resident lane (wsg_internal.h):
// its server, mailboxes, give-up and re-arm.  Only this file sees inside
// LaneServer; the entry points use the interface in wsg_ctx.h.
#include "wsg_ctx.h"
#include "wsg_env.h"

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <thread>

// One lane per device, shared by every context of the process on it
// (wsg_internal.h): its mailboxes, its stream and the launches of its
// resident kernel.  Servers are made on first use and live as long as the
// process (the at-exit handler stops their kernels).
struct LaneServer {
    int device = 0;
    wsg::LaneBell* bell = nullptr;   // page-locked, coherent, mapped
    hipStream_t stream = nullptr;
    uint32_t W = 8;                  // workgroups ($WSG_LANE_WGS)
    uint64_t idle_ticks = 0, yield_ticks = 0, delay_ticks = 0;
    int timeout_ms = 5000;           // a request unanswered this long: the lane is given up ($WSG_LANE_TIMEOUT_MS)
    int drain_ms = 2000;             // ... and waited for this long to leave ($WSG_LANE_DRAIN_MS)
    uint32_t delay_gens = ~0u;       // test hook: generations up to this one start late ($WSG_TEST_LANE_DELAY_GENS)
    std::mutex launch_lock;
    std::atomic<uint32_t> gen{0};        // the last launch's generation (0: none yet)
    std::atomic<bool> broken{false};     // given up: no launches until re-armed, every caller takes the launch paths
    // a lane given up is re-armed (lane_rearm) once its stream has drained and
    // this hold-off has passed: it doubles with every give-up in a row (from
    // kRearmFirstMs up to kRearmMaxMs) and resets once a re-armed lane answers
    std::atomic<int64_t> retry_at_ns{0};
    uint32_t backoff_ms = 0;             // (under launch_lock)
    std::atomic<bool> rearmed{false};    // re-armed and not yet answered a request since
    std::atomic<uint64_t> give_ups{0}, rearms{0};   // (wsg_lane_events)
    uint32_t delay_every = 0;            // test hook: every launch whose generation it divides starts late too ($WSG_TEST_LANE_DELAY_EVERY)
    std::atomic<uint64_t> tickets{0};    // next ticket
    std::atomic<int> inflight{0};        // requests posted and not yet answered
    std::atomic<uint64_t> launches{0};
    // per mailbox slot: the last ticket + 1 whose caller has read its answer
    // (a slot is reused only after that: its previous task done and read)
    std::atomic<uint64_t> released[wsg::LANE_WGS_MAX * wsg::LANE_RING];
};

namespace {

std::mutex& lane_servers_lock()
{
    static std::mutex* m = new std::mutex;   // leaked: used at exit
    return *m;
}
std::map<int, LaneServer*>& lane_servers()
{
    static auto* v = new std::map<int, LaneServer*>;
    return *v;
}

// Wait (at most ms) until every launch on the lane's stream has ended.
bool lane_drained(LaneServer* s, int ms)
{
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t q = hipStreamQuery(s->stream);
        if (q == hipSuccess)
            return true;
        if (q != hipErrorNotReady) {
            (void)hipGetLastError();
            return false;
        }
        if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(ms))
            return false;
        std::this_thread::sleep_for(std::chrono::microseconds(100));
    }
}

// Start the lane's mailboxes at ticket `base` (a multiple of W), with no
// launch running or queued and no request in flight: every workgroup resumes
// at its first ticket from `base` on, and every slot counts as answered and
// read, so the first W * LANE_RING tickets from `base` post without waiting.
// (Slots keep their old units: every tag in them is below base + 1, and
// every ticket from base on has a tag above that.)
void lane_set_frontier(LaneServer* s, uint64_t base)
{
    const uint64_t W = s->W, R = wsg::LANE_RING;
    for (uint32_t g = 0; g < s->W; ++g)
        __atomic_store_n(&s->bell->next_j[g], base / W, __ATOMIC_RELAXED);
    for (uint64_t t = base; t < base + W * R; ++t)
        s->released[(t % W) * R + (t / W) % R].store(t >= W * R ? t - W * R + 1 : 0, std::memory_order_relaxed);
    s->tickets.store(base);
}

int64_t steady_ns()
{
    return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch())
        .count();
}

// Every lane told to leave at process exit (a lane also leaves on its own
// after its idle limit); a lane already given up is not waited for again.
void lanes_at_exit()
{
    std::lock_guard<std::mutex> g(lane_servers_lock());
    for (auto& kv : lane_servers()) {
        LaneServer* s = kv.second;
        if (s->broken.load() || s->gen.load() == 0)
            continue;
        __atomic_store_n(&s->bell->ctl.stop, 1u, __ATOMIC_RELEASE);
        (void)lane_drained(s, 1000);
    }
}

// The device's lane, made on first use (nullptr: it cannot be made).
LaneServer* lane_server(int device)
{
    std::lock_guard<std::mutex> g(lane_servers_lock());
    auto& m = lane_servers();
    auto it = m.find(device);
    if (it != m.end())
        return it->second;
    auto* s = new (std::nothrow) LaneServer;
    if (!s)
        return nullptr;
    s->device = device;
    for (auto& r : s->released)
        r.store(0, std::memory_order_relaxed);
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) != hipSuccess || khz <= 0)
        khz = 100000;   // 100 MHz, the gfx9 constant clock
    long idle_us = 2000, yield_us = 2000, delay_us = 0;
    uint64_t ticket_base = 0;
    bool stale_xres = false;
    {
        std::lock_guard<std::recursive_mutex> eg(wsg::env_mutex());
        if (const char* e = wsg::envp("WSG_LANE_WGS")) {
            const long v = std::atol(e);
            if (v >= 1 && v <= long(wsg::LANE_WGS_MAX))
                s->W = uint32_t(v);
        }
        if (const char* e = wsg::envp("WSG_LANE_IDLE_US"))
            idle_us = std::max(1l, std::min(1000000l, std::atol(e)));
        if (const char* e = wsg::envp("WSG_LANE_YIELD_US"))
            yield_us = std::max(1l, std::min(1000000l, std::atol(e)));
        if (const char* e = wsg::envp("WSG_LANE_TIMEOUT_MS"))
            s->timeout_ms = int(std::max(1l, std::min(600000l, std::atol(e))));
        if (const char* e = wsg::envp("WSG_LANE_DRAIN_MS"))
            s->drain_ms = int(std::max(1l, std::min(600000l, std::atol(e))));
        if (const char* e = wsg::envp("WSG_TEST_LANE_DELAY_US"))   // test hook: the kernel starts late
            delay_us = std::max(0l, std::min(10000000l, std::atol(e)));
        if (const char* e = wsg::envp("WSG_TEST_LANE_DELAY_GENS"))   // ... only its first launches
            s->delay_gens = uint32_t(std::max(0l, std::min(1000000l, std::atol(e))));
        if (const char* e = wsg::envp("WSG_TEST_LANE_DELAY_EVERY")) {   // ... or every n-th (then only those
            s->delay_every = uint32_t(std::max(0l, std::min(1000000l, std::atol(e))));   //  and the first GENS)
            if (!wsg::envp("WSG_TEST_LANE_DELAY_GENS"))
                s->delay_gens = 0;
        }
        if (const char* e = wsg::envp("WSG_TEST_LANE_TICKET_BASE"))  // test hook: the ticket counter starts here
            ticket_base = std::strtoull(e, nullptr, 10);
        if (const char* e = wsg::envp("WSG_TEST_LANE_STALE_XRES"))   // ... with every inline answer unit stale
            stale_xres = *e == '1';
    }
    s->idle_ticks = uint64_t(idle_us) * uint64_t(khz) / 1000u;
    s->yield_ticks = uint64_t(yield_us) * uint64_t(khz) / 1000u;
    s->delay_ticks = uint64_t(delay_us) * uint64_t(khz) / 1000u;
    void* p = nullptr;
    int dev0 = 0;
    (void)hipGetDevice(&dev0);
    // A running lane holds the hardware queue its stream is on: every packet
    // queued behind it waits until the launch ends.  The runtime keeps streams
    // of each priority on their own queues, so the lane goes on a
    // high-priority stream (ahead of nothing but itself) and the contexts'
    // ordinary streams never queue behind it.
    int lo = 0, hi = 0;
    const bool ok = hipSetDevice(device) == hipSuccess &&
                    hipHostMalloc(&p, sizeof(wsg::LaneBell), hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess &&
                    hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess &&
                    hipStreamCreateWithPriority(&s->stream, hipStreamNonBlocking, hi) == hipSuccess;
    (void)hipSetDevice(dev0);
    if (!ok) {
        if (p)
            (void)hipHostFree(p);
        delete s;
        return nullptr;
    }
    std::memset(p, 0, sizeof(wsg::LaneBell));
    s->bell = static_cast<wsg::LaneBell*>(p);
    if (ticket_base) {
        lane_set_frontier(s, ticket_base / s->W * s->W);
        if (stale_xres) {
            // every slot's inline answer units as a task 2^32 tickets before
            // its next one would have left them: the low 32 bits of the tag
            // are the next ticket's, the dword not its answer
            const uint64_t b = s->tickets.load();
            for (uint64_t t = b; t < b + uint64_t(s->W) * wsg::LANE_RING; ++t)
                for (uint64_t& u : s->bell->xres[t % s->W][(t / s->W) % wsg::LANE_RING].u)
                    u = (uint64_t(uint32_t(t + 1)) << 32) | 0xA5A5A5A5u;
        }
    }
    static std::once_flag once;
    std::call_once(once, [] { std::atexit(lanes_at_exit); });
    m[device] = s;
    return s;
}

constexpr uint32_t kRearmFirstMs = 50, kRearmMaxMs = 4000;

// (under launch_lock) No launch until re-armed, and every workgroup leaves at
// its next check without taking another task; the hold-off before a re-arm
// doubles with every give-up in a row.
void lane_break_locked(LaneServer* s)
{
    if (s->broken.load())
        return;
    s->backoff_ms = s->backoff_ms ? std::min(kRearmMaxMs, s->backoff_ms * 2) : kRearmFirstMs;
    s->retry_at_ns.store(steady_ns() + int64_t(s->backoff_ms) * 1000000);
    s->rearmed.store(false);
    s->give_ups.fetch_add(1);
    s->broken.store(true);
    __atomic_store_n(&s->bell->ctl.stop, 1u, __ATOMIC_RELEASE);
}

// Give the lane up (a request went unanswered).
void lane_give_up(LaneServer* s)
{
    std::lock_guard<std::mutex> g(s->launch_lock);
#ifdef WSG_DIAG_LANE   // (diagnostic build: where the mailboxes stand at a give-up)
    std::fprintf(stderr, "lane give-up: tickets %llu gen %u closing %u stop %u\n",
                 (unsigned long long)s->tickets.load(), s->gen.load(), s->bell->ctl.closing, s->bell->ctl.stop);
    for (uint32_t q = 0; q < s->W; ++q)
        std::fprintf(stderr, "  wg %u next_j %llu slot %llu tag0 %llu\n", q, (unsigned long long)s->bell->next_j[q],
                     (unsigned long long)(s->bell->next_j[q] % wsg::LANE_RING),
                     (unsigned long long)s->bell->box[q][s->bell->next_j[q] % wsg::LANE_RING].w[0].tag);
#endif
    lane_break_locked(s);
}

// Bring a given-up lane back: once its hold-off has passed, no request is in
// flight (every caller of the give-up has taken its fallback and released its
// slots) and its stream has drained (no workgroup left to write a request's
// buffers), the mailboxes restart past every ticket handed out so far —
// tasks posted to the old lane and never taken are skipped, not run — and
// the next request launches a new generation.  False: still given up.
bool lane_rearm(LaneServer* s)
{
    if (steady_ns() < s->retry_at_ns.load(std::memory_order_relaxed))
        return false;
    std::unique_lock<std::mutex> g(s->launch_lock, std::try_to_lock);
    if (!g.owns_lock())
        return false;
    if (!s->broken.load())
        return true;
    if (s->inflight.load() != 0)
        return false;
    const hipError_t q = hipStreamQuery(s->stream);
    if (q != hipSuccess) {
        if (q != hipErrorNotReady)
            (void)hipGetLastError();
        s->retry_at_ns.store(steady_ns() + int64_t(s->backoff_ms) * 1000000);
        return false;
    }
    const uint64_t W = s->W;
    lane_set_frontier(s, (s->tickets.load() + W - 1) / W * W);
    __atomic_store_n(&s->bell->ctl.stop, 0u, __ATOMIC_RELAXED);
    // the last generation counts as ended: the next request launches
    __atomic_store_n(&s->bell->ctl.closing, s->gen.load(), __ATOMIC_RELEASE);
    s->rearmed.store(true);
    s->rearms.fetch_add(1);
    s->broken.store(false);
    return true;
}

// Launch the next generation if generation `seen` is the last one (none yet,
// or it announced its end): queued behind it on the lane's stream, it starts
// once every workgroup of the old one has left, each mailbox where it was.
void lane_relaunch(LaneServer* s, uint32_t seen)
{
    std::lock_guard<std::mutex> g(s->launch_lock);
    if (s->broken.load() || s->gen.load() != seen)
        return;
    uint32_t next = seen + 1;
    if (next == 0)
        next = 1;
    if (wsg::launch_lane(s->stream, s->bell, s->W, s->idle_ticks, s->yield_ticks, next,
                         next <= s->delay_gens || (s->delay_every && next % s->delay_every == 0) ? s->delay_ticks
                                                                                                 : 0) != hipSuccess) {
        (void)hipGetLastError();
        lane_break_locked(s);
        return;
    }
    s->launches.fetch_add(1);
    s->gen.store(next);
}

// A launch running (or queued) that has not announced its end; else launch.
void lane_ensure_running(LaneServer* s)
{
    const uint32_t g = s->gen.load(std::memory_order_acquire);
    if (g == 0 || __atomic_load_n(&s->bell->ctl.closing, __ATOMIC_ACQUIRE) == g)
        lane_relaunch(s, g);
}
} // namespace

LaneServer* lane_for(wsg_ctx* c)
{
    if (!c->lane_max)
        return nullptr;
    if (!c->lane) {
        c->lane = lane_server(c->device);
        if (!c->lane) {
            c->lane_max = 0;
            return nullptr;
        }
    }
    if (c->lane->broken.load(std::memory_order_relaxed) && !lane_rearm(c->lane))
        return nullptr;
    return c->lane;
}

uint32_t lane_want(const wsg_ctx* c, const LaneServer* s)
{
    const uint32_t busy = uint32_t(std::max(0, s->inflight.load(std::memory_order_relaxed))) + 1;
    return std::max<uint32_t>(1, std::min(s->W / busy, c->lane_groups));
}

// A task's words, as the comment on wsg::LaneTask (wsg_internal.h) lays them
// out and k_lane reads them.
void lane_task_decode(uint64_t* w, uint32_t n, const uint8_t* wire, uint64_t wire_len, const uint64_t* frame_start,
                      uint8_t* out, wsg_recv_info* info, const LaneGroup& g)
{
    w[0] = wsg::LANE_DECODE | (uint64_t(n) << 32);
    w[1] = reinterpret_cast<uint64_t>(wire);
    w[2] = wire_len;
    w[3] = reinterpret_cast<uint64_t>(frame_start);
    w[4] = reinterpret_cast<uint64_t>(out);
    w[5] = reinterpret_cast<uint64_t>(info);
    w[6] = uint64_t(g.f) | (uint64_t(g.cnt) << 32);
    w[7] = g.lo;
    w[8] = g.hi;
}

void lane_task_encode(uint64_t* w, uint32_t n, const uint8_t* payload, const wsg_send_desc* desc,
                      const uint64_t* wire_off, uint8_t* wire, const LaneGroup& g, uint64_t lo, uint64_t hi)
{
    w[0] = wsg::LANE_ENCODE | (uint64_t(n) << 32);
    w[1] = reinterpret_cast<uint64_t>(payload);
    w[2] = reinterpret_cast<uint64_t>(desc);
    w[3] = reinterpret_cast<uint64_t>(wire_off);
    w[4] = reinterpret_cast<uint64_t>(wire);
    w[5] = 0;
    w[6] = uint64_t(g.f) | (uint64_t(g.cnt) << 32);
    w[7] = lo;
    w[8] = hi;
}

void lane_task_xor(uint64_t* w, uint8_t* stage, uint64_t len, uint32_t key, uint32_t phase, const void* inline_src)
{
    w[0] = (inline_src ? wsg::LANE_XOR_INLINE : wsg::LANE_XOR) | (uint64_t(1) << 32);
    w[1] = reinterpret_cast<uint64_t>(stage);
    w[2] = len;
    w[3] = uint64_t(key) | (uint64_t(phase & 3u) << 32);
    std::memset(&w[4], 0, (wsg::LANE_WORDS - 4) * sizeof(uint64_t));
    if (inline_src)   // (the answer comes back in the slot's self-tagged units, no buffer)
        std::memcpy(&w[4], inline_src, len);
}

LaneResult lane_run(wsg_ctx* c, LaneServer* s, const uint64_t (*words)[wsg::LANE_WORDS], uint32_t groups,
                    uint64_t* errs, uint32_t* answered, uint32_t xwords, uint32_t* xout)
{
    *errs = 0;
    *answered = 0;
    // in flight before the check: a re-arm (which needs none in flight while
    // the lane is given up) never runs under a request that saw it working
    s->inflight.fetch_add(1);
    if (s->broken.load()) {
        s->inflight.fetch_sub(1);
        return LANE_FALLBACK;
    }
    const uint32_t W = s->W, R = wsg::LANE_RING;
    const uint64_t x = s->tickets.fetch_add(groups);
    ++c->lane_requests;
    const auto t0 = std::chrono::steady_clock::now();
    auto late = [&] { return std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(s->timeout_ms); };
    // post: every group's slot (its previous task answered and read first),
    // each unit's value then its tag, the first unit last
    for (uint32_t k = 0; k < groups; ++k) {
        const uint64_t tk = x + k;
        const uint32_t wg = uint32_t(tk % W), slot = uint32_t((tk / W) % R);
        if (tk >= uint64_t(W) * R) {
            const uint64_t prev = tk - uint64_t(W) * R + 1;
            for (uint64_t i = 1; s->released[wg * R + slot].load(std::memory_order_acquire) != prev; ++i) {
                if ((i & 1023) == 0 && late()) {   // (posted anyway: the lane is stopped)
                    lane_give_up(s);
                    break;
                }
                __builtin_ia32_pause();
            }
        }
#ifndef WSG_DIAG_NO_XRES_POISON   // (diagnostic build only: shows test_lane_inline_answers_across_the_tag_wrap failing)
        if (xwords) {
            // an inline answer's units carry only the low 32 bits of the
            // ticket, which recur in this slot every 2^32 tickets (W * R
            // divides 2^32), and the slot's last inline task may have been
            // that long ago: units that tag no ticket of this lap before the
            // task goes out (its answer has been read: `released`, above)
            for (uint32_t q = 0; q < xwords; ++q)
                __atomic_store_n(&s->bell->xres[wg][slot].u[q], uint64_t(~uint32_t(tk + 1)) << 32, __ATOMIC_RELAXED);
        }
#endif
        wsg::LaneTask* T = &s->bell->box[wg][slot];
        for (uint32_t u = wsg::LANE_WORDS; u-- > 0;) {
            T->w[u].v = words[k][u];
            __atomic_store_n(&T->w[u].tag, tk + 1, __ATOMIC_RELEASE);
        }
    }
    lane_ensure_running(s);
    // wait for the answers, group by group
    uint32_t k = 0;
    bool gave_up = false;
    for (uint64_t i = 1; k < groups; ++i) {
        while (k < groups) {
            const uint64_t tk = x + k;
            const uint32_t wg = uint32_t(tk % W), slot = uint32_t((tk / W) % R);
            if (xwords) {   // (one group) every unit shows the tag: the answer is complete
                const wsg::LaneXres& xr = s->bell->xres[wg][slot];
                uint32_t q = 0;
                for (; q < xwords; ++q) {
                    const uint64_t u = __atomic_load_n(&xr.u[q], __ATOMIC_ACQUIRE);
                    if (uint32_t(u >> 32) != uint32_t(tk + 1))
                        break;
                    xout[q] = uint32_t(u);
                }
                if (q < xwords)
                    break;
            } else {
                wsg::LaneResp& r = s->bell->resp[wg][slot];
                if (__atomic_load_n(&r.done, __ATOMIC_ACQUIRE) != tk + 1)
                    break;
                *errs += __atomic_load_n(&r.errs, __ATOMIC_RELAXED);
            }
            s->released[wg * R + slot].store(tk + 1, std::memory_order_release);
            ++k;
        }
        if (k == groups)
            break;
        if ((i & 255) == 0) {
            if (s->broken.load()) {
                gave_up = true;
                break;
            }
            lane_ensure_running(s);   // the launch announced its end before these tasks: the next one
            if (late()) {
                lane_give_up(s);
                gave_up = true;
                break;
            }
        }
        __builtin_ia32_pause();
    }
    if (!gave_up) {
        s->inflight.fetch_sub(1);
        if (s->rearmed.load(std::memory_order_relaxed)) {   // the re-armed lane works: the next give-up's hold-off starts over
            std::lock_guard<std::mutex> g(s->launch_lock);
            if (s->rearmed.exchange(false) && !s->broken.load())
                s->backoff_ms = 0;
        }
        return LANE_DONE;
    }
    // Given up: nothing of the request may be touched until the lane has
    // left (a workgroup that took a task before `stop` finishes it).
    const bool drained = lane_drained(s, s->drain_ms);
    for (uint32_t q = 0; q < groups; ++q) {
        const uint64_t tk = x + q;
        const uint32_t wg = uint32_t(tk % W), slot = uint32_t((tk / W) % R);
        if (xwords ? uint32_t(__atomic_load_n(&s->bell->xres[wg][slot].u[0], __ATOMIC_ACQUIRE) >> 32) == uint32_t(tk + 1)
                   : __atomic_load_n(&s->bell->resp[wg][slot].done, __ATOMIC_ACQUIRE) == tk + 1)
            ++*answered;
        s->released[wg * R + slot].store(tk + 1, std::memory_order_release);
    }
    s->inflight.fetch_sub(1);
    if (!drained) {
        c->dead = true;
        return LANE_LOST;
    }
    return LANE_FALLBACK;
}

int wsg_lane_stats(wsg_ctx* c, uint64_t* requests, uint64_t* launches, int* running)
{
    if (!c)
        return WSG_EINVAL;
    LaneServer* s = c->lane;
    if (requests)
        *requests = c->lane_requests;
    if (launches)
        *launches = s ? s->launches.load() : 0;
    if (running) {
        const uint32_t g = s ? s->gen.load() : 0;
        *running = !s ? 0 : s->broken.load() ? -1 : (g && __atomic_load_n(&s->bell->ctl.closing, __ATOMIC_ACQUIRE) != g) ? 1 : 0;
    }
    return WSG_OK;
}

int wsg_lane_events(wsg_ctx* c, uint64_t* give_ups, uint64_t* rearms)
{
    if (!c)
        return WSG_EINVAL;
    LaneServer* s = c->lane;
    if (give_ups)
        *give_ups = s ? s->give_ups.load() : 0;
    if (rearms)
        *rearms = s ? s->rearms.load() : 0;
    return WSG_OK;
}
