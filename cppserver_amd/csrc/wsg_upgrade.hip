// wsg_upgrade.hip — the WebSocket upgrade handshake on the device
// (wsg_upgrade_streams): the rule of wsg_upgrade.h over a batch of streams.
#include "wsg_device.h"
#include "wsg_upgrade.h"

namespace wsg {

// A connection's first bytes are independent of every other connection's and a
// few hundred bytes long: one wave takes one stream (grid-stride over streams),
// as in the framer.
//   k_upgrade_parse       the wave reads its stream in aligned 16-byte blocks,
//                         a 1 KiB tile per step, bytes outside the span read
//                         as 0, the last three bytes carried from lane to
//                         lane and tile to tile.  Ballots find the header end
//                         and the line starts; the lane that owns a line's
//                         first byte judges the line (up_line, byte loads of
//                         lines the tile load has just brought in) and folds
//                         its own lines in order; ballots and readlanes fold
//                         the lanes into the wave's running facts.  The walk
//                         ends with the tile that holds the header end.  Lane
//                         0 writes the record and the span.
//   k_upgrade_scan_local  one lane per stream: block scan of the response
//   k_upgrade_scan_blocks bytes, block sums of the three counts; one block
//                         over the partials: d_count, the capacity latch
//   k_upgrade_accept      one lane per stream: d_resp_off, and for an accepted
//                         stream SHA-1 over the key bytes on the wire and the
//                         GUID, then Base64, the 28 bytes to the plan
//   k_upgrade_respond     one wave per stream: the outcome's template from
//                         constant memory, the accept bytes in their place
// Limits: a lane walks its line byte by byte, so one very long header line is
// serial on one lane; the accept kernel's lanes diverge where accepted and
// other streams share a wave.

namespace {

constexpr uint32_t UP_TILE = 64 * CHUNK;   // 1 KiB: a 16-B block per lane

__constant__ char c_up_tpl[UP_TEMPLATES][WSG_UPGRADE_RESP_MAX + 1] = {
    "",   // WSG_UP_INCOMPLETE
    WSG_UP_T_ACCEPTED,
    WSG_UP_T_BAD_HTTP,
    WSG_UP_T_BAD_CONNECTION,
    WSG_UP_T_BAD_UPGRADE,
    WSG_UP_T_EMPTY_KEY,
    WSG_UP_T_BAD_VERSION,
    WSG_UP_T_MISSING,
};
static_assert(WSG_UP_ACCEPTED == 1 && WSG_UP_BAD_HTTP == 2 && WSG_UP_BAD_CONNECTION == 3 && WSG_UP_BAD_UPGRADE == 4 &&
                  WSG_UP_EMPTY_KEY == 5 && WSG_UP_BAD_VERSION == 6 && WSG_UP_MISSING == 7,
              "c_up_tpl is indexed by the outcome code");
static_assert(sizeof(wsg_upgrade) == 32 && offsetof(wsg_upgrade, key_len) == 16 && offsetof(wsg_upgrade, resp_len) == 24 &&
                  offsetof(wsg_upgrade, status) == 28 && offsetof(wsg_upgrade, code) == 30,
              "wsg_upgrade layout (up_record)");

// The request at wire[off, off + len): every argument and the result are
// wave-uniform.
__device__ __forceinline__ UpOutcome upgrade_walk(const uint8_t* __restrict__ wire, uint64_t off, uint64_t len,
                                                  uint64_t max_request, uint32_t lane)
{
    const uint64_t end = off + len;
    const auto src = [wire, off](uint64_t r) -> uint32_t { return wire[off + r]; };
    UpFold W{};
    bool found = false, have_first = false;
    uint64_t p = 0, first = 0;   // absolute: the header end's first byte, the first line start
    uint32_t carry = 0;          // the three bytes in front of the tile
    // (W's 64-bit members and `first` are the same in every lane but kept in vector registers, through
    // __shfl: as scalars they took the kernel over its SGPRs)
    for (uint64_t t0 = off & ~uint64_t(15); t0 < end && !found; t0 += UP_TILE) {
        const uint64_t a = t0 + uint64_t(lane) * CHUNK;
        const v4u v = a < end ? ld16(wire + a) : v4u{0, 0, 0, 0};
        // the block's bytes inside [off, end), 0 outside
        const int64_t lo = off > a ? int64_t(off - a) : 0;
        const int64_t hi = end > a ? int64_t(min(end - a, uint64_t(16))) : 0;
        const uint64_t q0 = (uint64_t(v.x) | (uint64_t(v.y) << 32)) & bytes_below(hi) & ~bytes_below(lo);
        const uint64_t q1 = (uint64_t(v.z) | (uint64_t(v.w) << 32)) & bytes_below(hi - 8) & ~bytes_below(lo - 8);
        const uint32_t tail = (uint32_t(q1 >> 40) & 0xFFu) << 16 | (uint32_t(q1 >> 48) & 0xFFu) << 8 | uint32_t(q1 >> 56);
        const uint32_t before = __shfl_up(tail, 1, 64);
        uint32_t hist = lane ? before : carry;
        carry = lane_bcast32(tail, 63);
        // ls: a line starts at byte k ("\r\n" in front of it); hm: a header end's last byte is k
        uint32_t ls = 0, hm = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const uint32_t b = uint32_t(k < 8 ? q0 >> (8 * k) : q1 >> (8 * (k - 8))) & 0xFFu;
            if ((hist & 0xFFFFu) == 0x0D0Au)
                ls |= 1u << k;
            hist = (hist << 8) | b;
            if (hist == 0x0D0A0D0Au)
                hm |= 1u << k;
        }
        ls &= (1u << hi) - 1u;   // a line start is a byte of the span
        const uint64_t fm = __ballot(hm != 0);
        if (fm) {
            found = true;
            p = lane_bcast(a + uint32_t(__builtin_ctz(hm | 0x10000u)) - 3, int(uni(uint32_t(__builtin_ctzll(fm)))));
            const uint64_t keep = p > a ? min(p - a, uint64_t(16)) : 0;   // lines start in front of the header end
            ls &= (1u << keep) - 1u;
        }
        const uint64_t lm = __ballot(ls != 0);
        if (!have_first && lm) {
            have_first = true;
            first = __shfl(a + uint32_t(__builtin_ctz(ls | 0x10000u)), __builtin_ctzll(lm), 64);
        }
        if (!lm)
            continue;
        // this lane's lines, in order
        UpFold A{};
        while (ls) {
            const uint32_t k = uint32_t(__builtin_ctz(ls));
            ls &= ls - 1u;
            const UpLine ln = up_line(src, a + k - off, len);
            if (!ln.open)
                up_fold(A, ln);
        }
        // the lanes, in order, behind the tiles in front
        W.malformed = W.malformed || __ballot(A.malformed) != 0;
        const uint64_t cm = __ballot(A.has_clen);
        if (cm) {
            W.has_clen = true;
            W.clen = __shfl(A.clen, 63 - __builtin_clzll(cm), 64);
        }
        if (!W.fail) {
            const uint64_t xm = __ballot(A.fail != 0);
            const uint32_t F = xm ? uint32_t(__builtin_ctzll(xm)) : 63u;
            const uint64_t upto = F == 63u ? ~0ull : (2ull << F) - 1ull;   // the lanes up to the first failing one
#pragma unroll
            for (uint32_t bit = 1; bit <= UP_VERSION; bit <<= 1)
                if (__ballot((A.seen & bit) != 0) & upto)
                    W.seen |= bit;
            const uint64_t km = __ballot((A.seen & UP_KEY) != 0) & upto;
            if (km) {
                const int L = 63 - __builtin_clzll(km);
                W.key_off = __shfl(A.key_off, L, 64);
                W.key_len = __shfl(A.key_len, L, 64);
            }
            if (xm)
                W.fail = lane_bcast32(A.fail, F);
        }
    }
    if (!found)
        return up_outcome(false, 0, UpStart{}, W, off, len, max_request);
    const uint64_t eol = (have_first ? first - 2 : p) - off;
    return up_outcome(true, p + 4 - off, up_start(src, eol), W, off, len, max_request);
}

} // namespace

__global__ __launch_bounds__(BLOCK) void k_upgrade_parse(const uint8_t* __restrict__ wire, uint64_t wire_len,
                                                         wsg_stream_span* span, uint32_t ns, uint64_t max_request,
                                                         wsg_upgrade* __restrict__ up, unsigned long long* err)
{
    const uint64_t waves = uint64_t(gridDim.x) * (BLOCK / 64);
    const uint32_t lane = threadIdx.x & 63, wid = wave_id();
    for (uint64_t j64 = uint64_t(blockIdx.x) * (BLOCK / 64) + wid; j64 < ns; j64 += waves) {
        const uint32_t j = uint32_t(j64);
        const SpanIn s = span_in(span, j, wire_len);
        UpOutcome o{};   // a span that may not be walked: incomplete, nothing consumed, no response
        if (s.ok)
            o = upgrade_walk(wire, s.off, s.len, max_request, lane);
        if (lane == 0) {
            if (!s.ok)
                latch(err, j, WSG_EINVAL);
            uint64_t w[4];
            up_record(o, w);
            uint64_t* r = reinterpret_cast<uint64_t*>(up + j);
            r[0] = w[0];
            r[1] = w[1];
            r[2] = w[2];
            r[3] = w[3];
            uint64_t* sp = reinterpret_cast<uint64_t*>(span + j);
            sp[2] = o.consumed;
            sp[3] = o.need;
        }
    }
}

__global__ __launch_bounds__(BLOCK) void k_upgrade_scan_local(const wsg_upgrade* __restrict__ up, uint32_t ns,
                                                              UpgradePlan P)
{
    const uint64_t j64 = uint64_t(blockIdx.x) * BLOCK + threadIdx.x;
    uint64_t bytes = 0, acc = 0, rej = 0, inc = 0;
    if (j64 < ns) {
        const uint64_t w3 = reinterpret_cast<const uint64_t*>(up + j64)[3];
        const uint32_t code = uint32_t(w3 >> 48) & 0xFFu;
        bytes = uint32_t(w3);
        acc = code == WSG_UP_ACCEPTED;
        rej = (uint32_t(w3 >> 32) & 0xFFFFu) == 400u;
        inc = code == WSG_UP_INCOMPLETE;
    }
    uint64_t tb, ta, tr, ti;
    const uint64_t ex = block_scan_ex(bytes, OpAdd{}, &tb);
    (void)block_scan_ex(acc, OpAdd{}, &ta);
    (void)block_scan_ex(rej, OpAdd{}, &tr);
    (void)block_scan_ex(inc, OpAdd{}, &ti);
    if (j64 < ns)
        P.ex[j64] = ex;
    if (threadIdx.x == 0) {
        const uint64_t nb = gridDim.x;
        P.bsum[blockIdx.x] = tb;
        P.bsum[nb + blockIdx.x] = ta;
        P.bsum[2 * nb + blockIdx.x] = tr;
        P.bsum[3 * nb + blockIdx.x] = ti;
    }
}

__global__ __launch_bounds__(BLOCK) void k_upgrade_scan_blocks(UpgradePlan P, uint32_t nb, uint32_t ns,
                                                               uint64_t resp_cap, uint64_t* __restrict__ count,
                                                               unsigned long long* err)
{
    const uint64_t tb = scan_partials(P.bsum, P.bpre, nb, OpAdd{});
    const uint64_t ta = scan_partials<uint64_t>(P.bsum + nb, nullptr, nb, OpAdd{});
    const uint64_t tr = scan_partials<uint64_t>(P.bsum + 2 * uint64_t(nb), nullptr, nb, OpAdd{});
    const uint64_t ti = scan_partials<uint64_t>(P.bsum + 3 * uint64_t(nb), nullptr, nb, OpAdd{});
    if (threadIdx.x == 0) {
        P.tot[0] = tb;
        count[0] = ta;
        count[1] = tr;
        count[2] = ti;
        count[3] = tb;
        if (tb > resp_cap)   // behind every span error: the latch keeps the smallest
            latch(err, ns, WSG_ENOMEM);
    }
}

__global__ __launch_bounds__(BLOCK) void k_upgrade_accept(const uint8_t* __restrict__ wire,
                                                          const wsg_upgrade* __restrict__ up, uint32_t ns,
                                                          UpgradePlan P, uint64_t* __restrict__ resp_off)
{
    const uint64_t j64 = uint64_t(blockIdx.x) * BLOCK + threadIdx.x;
    if (j64 >= ns)
        return;
    resp_off[j64] = P.ex[j64] + P.bpre[j64 / BLOCK];
    if (j64 + 1 == ns)
        resp_off[ns] = P.tot[0];
    const uint64_t* w = reinterpret_cast<const uint64_t*>(up + j64);
    if ((uint32_t(w[3] >> 48) & 0xFFu) != WSG_UP_ACCEPTED)
        return;
    const uint8_t* key = wire + w[0];
    uint32_t out[7];
    up_accept([key](uint64_t t) -> uint32_t { return key[t]; }, uint32_t(w[2]), out);
    v4u* dst = reinterpret_cast<v4u*>(P.accept + 8 * j64);
    dst[0] = v4u{out[0], out[1], out[2], out[3]};
    dst[1] = v4u{out[4], out[5], out[6], 0};
}

__global__ __launch_bounds__(BLOCK) void k_upgrade_respond(const wsg_upgrade* __restrict__ up, uint32_t ns,
                                                           UpgradePlan P, const uint64_t* __restrict__ resp_off,
                                                           uint8_t* __restrict__ resp, uint64_t resp_cap)
{
    if (uni(P.tot[0]) > resp_cap)   // WSG_ENOMEM latched by k_upgrade_scan_blocks: no byte of resp
        return;
    const uint64_t waves = uint64_t(gridDim.x) * (BLOCK / 64);
    const uint32_t lane = threadIdx.x & 63, wid = wave_id();
    for (uint64_t j64 = uint64_t(blockIdx.x) * (BLOCK / 64) + wid; j64 < ns; j64 += waves) {
        const uint64_t w3 = uni(reinterpret_cast<const uint64_t*>(up + j64)[3]);
        const uint32_t len = uint32_t(w3), code = uint32_t(w3 >> 48) & 0xFFu;
        if (!len || code >= UP_TEMPLATES || len > WSG_UPGRADE_RESP_MAX)
            continue;
        uint8_t* dst = resp + uni(resp_off[j64]);
        const uint8_t* acc = reinterpret_cast<const uint8_t*>(P.accept + 8 * j64);
        for (uint32_t k = lane; k < len; k += 64) {
            uint32_t b = uint8_t(c_up_tpl[code][k]);
            if (code == WSG_UP_ACCEPTED && k - UP_ACCEPT_AT < UP_ACCEPT_LEN)
                b = acc[k - UP_ACCEPT_AT];
            dst[k] = uint8_t(b);
        }
    }
}

uint64_t upgrade_plan_layout(uint64_t* base, uint32_t ns, UpgradePlan* plan)
{
    const uint64_t nb = (uint64_t(ns) + BLOCK - 1) / BLOCK;
    Carve c{reinterpret_cast<uint8_t*>(base), 16};
    UpgradePlan P;
    P.accept = c.take<uint32_t>(8 * uint64_t(ns));
    P.ex = c.take<uint64_t>(ns);
    P.bsum = c.take<uint64_t>(4 * nb);
    P.bpre = c.take<uint64_t>(nb);
    P.tot = c.take<uint64_t>(2);
    if (plan)
        *plan = P;
    return c.at / sizeof(uint64_t);
}

hipError_t launch_upgrade_streams(hipStream_t s, int grid, const uint8_t* wire, uint64_t wire_len,
                                  wsg_stream_span* span, uint32_t ns, uint64_t max_request, wsg_upgrade* up,
                                  uint8_t* resp, uint64_t resp_cap, uint64_t* resp_off, uint64_t* count,
                                  const UpgradePlan& plan, unsigned long long* err)
{
    if (ns == 0) {   // no stream: no response
        if (hipError_t e = hipMemsetAsync(count, 0, 4 * sizeof(uint64_t), s); e != hipSuccess)
            return e;
        return hipMemsetAsync(resp_off, 0, sizeof(uint64_t), s);
    }
    const uint32_t nb = uint32_t((uint64_t(ns) + BLOCK - 1) / BLOCK);
    k_upgrade_parse<<<grid, BLOCK, 0, s>>>(wire, wire_len, span, ns, max_request, up, err);
    k_upgrade_scan_local<<<nb, BLOCK, 0, s>>>(up, ns, plan);
    k_upgrade_scan_blocks<<<1, BLOCK, 0, s>>>(plan, nb, ns, resp_cap, count, err);
    k_upgrade_accept<<<nb, BLOCK, 0, s>>>(wire, up, ns, plan, resp_off);
    k_upgrade_respond<<<grid, BLOCK, 0, s>>>(up, ns, plan, resp_off, resp, resp_cap);
    return hipGetLastError();
}

} // namespace wsg
