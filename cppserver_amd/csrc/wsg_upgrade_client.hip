// wsg_upgrade_client.hip — the client's half of the upgrade handshake on the
// device (wsg_upgrade_client_streams, wsg_upgrade_requests): the rule of
// wsg_upgrade_client.h over a batch of streams.
#include "wsg_device.h"
#include "wsg_upgrade_client.h"

namespace wsg {

//   k_upclient_expect       one lane per stream: Base64 of the nonce, SHA-1
//                           over it and the GUID (two blocks, every index a
//                           constant), the 20 digest bytes to the plan
//   k_upclient_parse        k_upgrade_parse's walk (one wave per stream, 1 KiB
//                           tiles, the line's first byte's lane judges the
//                           line) with the client's fold: any malformed line,
//                           the last Content-Length, the first failing line,
//                           the names in front of it, the last accept value
//                           judged.  An accept line is judged against the
//                           stream's 20 bytes of the plan.  Lane 0 writes the
//                           record and the span.
//   k_upclient_count_local  one lane per stream: block sums of the three
//   k_upclient_count_blocks counts; one block over the partials: d_count
//   k_upgrade_requests      one lane per 16-byte block of d_req, grid-stride:
//                           the template through aligned 16-byte loads (a
//                           block holds bytes of two requests at most), the
//                           key's characters from the nonce in their place.
//                           The last block, when it is not whole, goes out by
//                           the byte.
// Limits: as k_upgrade_parse, a lane walks its line byte by byte.

namespace {

constexpr uint32_t UC_TILE = 64 * CHUNK;   // 1 KiB: a 16-B block per lane

static_assert(sizeof(wsg_upgrade_reply) == 32 && offsetof(wsg_upgrade_reply, accept_len) == 16 &&
                  offsetof(wsg_upgrade_reply, _zero) == 24 && offsetof(wsg_upgrade_reply, status) == 28 &&
                  offsetof(wsg_upgrade_reply, code) == 30,
              "wsg_upgrade_reply layout (uc_record)");

// A wave-uniform value held in vector registers from here on.
__device__ __forceinline__ uint32_t vec(uint32_t x)
{
    asm volatile("" : "+v"(x));
    return x;
}
__device__ __forceinline__ uint64_t vec(uint64_t x)
{
    return uint64_t(vec(uint32_t(x))) | (uint64_t(vec(uint32_t(x >> 32))) << 32);
}

// The response at wire[off, off + len) against the digest at dig[0, 20): every
// argument and the result are wave-uniform.
__device__ __forceinline__ UcOutcome upclient_walk(const uint8_t* __restrict__ wire, uint64_t off, uint64_t len,
                                                   const uint8_t* __restrict__ dig, uint64_t max_response,
                                                   uint32_t lane)
{
    const uint64_t end = off + len;
    // (the byte loads' base in vector registers: with it in scalar ones the lines' judges, up_line's and the
    // accept value's, take the kernel 12 over its scalar registers)
    const uint64_t voff = vec(off);
    const auto src = [wire, voff](uint64_t r) -> uint32_t { return wire[voff + r]; };
    const auto expect = [dig](uint32_t i) -> uint32_t { return dig[i]; };
    UcFold W{};
    bool found = false, have_first = false;
    uint64_t p = 0, first = 0;   // absolute: the header end's first byte, the first line start
    uint32_t carry = 0;          // the three bytes in front of the tile
    // (W's 64-bit members and `first` are the same in every lane but kept in vector registers, as in
    // k_upgrade_parse)
    for (uint64_t t0 = off & ~uint64_t(15); t0 < end && !found; t0 += UC_TILE) {
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
        UcFold A{};
        while (ls) {
            const uint32_t k = uint32_t(__builtin_ctz(ls));
            ls &= ls - 1u;
            const UcLine ln = uc_line(src, a + k - off, len, expect);
            if (!ln.open)
                uc_fold(A, ln);
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
            for (uint32_t bit = 1; bit <= UC_ACCEPT; bit <<= 1)
                if (__ballot((A.seen & bit) != 0) & upto)
                    W.seen |= bit;
            const uint64_t jm = __ballot(A.judged) & upto;   // (a failing lane's own accept line included)
            if (jm) {
                const int L = 63 - __builtin_clzll(jm);
                W.judged = true;
                W.acc_off = __shfl(A.acc_off, L, 64);
                W.acc_len = __shfl(A.acc_len, L, 64);
            }
            if (xm)
                W.fail = lane_bcast32(A.fail, F);
        }
    }
    if (!found)
        return uc_outcome(false, 0, UcStatus{}, W, off, len, max_response);
    const uint64_t eol = (have_first ? first - 2 : p) - off;
    return uc_outcome(true, p + 4 - off, uc_status(src, eol), W, off, len, max_response);
}

} // namespace

__global__ __launch_bounds__(BLOCK) void k_upclient_expect(const uint8_t* __restrict__ nonce, uint32_t ns,
                                                           uint32_t* __restrict__ digest)
{
    const uint64_t j64 = uint64_t(blockIdx.x) * BLOCK + threadIdx.x;
    if (j64 >= ns)
        return;
    const v4u nv = ld16(nonce + 16 * j64);
    const uint32_t n[4] = {nv.x, nv.y, nv.z, nv.w};
    uint32_t h[5];
    uc_expect(n, h);
    // the digest's bytes in memory order
    v4u* dst = reinterpret_cast<v4u*>(digest + 8 * j64);
    dst[0] = v4u{__builtin_bswap32(h[0]), __builtin_bswap32(h[1]), __builtin_bswap32(h[2]), __builtin_bswap32(h[3])};
    dst[1] = v4u{__builtin_bswap32(h[4]), 0, 0, 0};
}

__global__ __launch_bounds__(BLOCK) void k_upclient_parse(const uint8_t* __restrict__ wire, uint64_t wire_len,
                                                          wsg_stream_span* span, uint32_t ns,
                                                          const uint32_t* __restrict__ digest, uint64_t max_response,
                                                          wsg_upgrade_reply* __restrict__ up, unsigned long long* err)
{
    const uint64_t waves = uint64_t(gridDim.x) * (BLOCK / 64);
    const uint32_t lane = threadIdx.x & 63, wid = wave_id();
    for (uint64_t j64 = uint64_t(blockIdx.x) * (BLOCK / 64) + wid; j64 < ns; j64 += waves) {
        const uint32_t j = uint32_t(j64);
        const SpanIn s = span_in(span, j, wire_len);
        UcOutcome o{};   // a span that may not be walked: incomplete, nothing consumed, a zero record
        if (s.ok)
            o = upclient_walk(wire, s.off, s.len, reinterpret_cast<const uint8_t*>(digest + 8 * j64), max_response, lane);
        if (lane == 0) {
            if (!s.ok)
                latch(err, j, WSG_EINVAL);
            uint64_t w[4];
            uc_record(o, w);
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

__global__ __launch_bounds__(BLOCK) void k_upclient_count_local(const wsg_upgrade_reply* __restrict__ up, uint32_t ns,
                                                                UpClientPlan P)
{
    const uint64_t j64 = uint64_t(blockIdx.x) * BLOCK + threadIdx.x;
    uint64_t acc = 0, rej = 0, inc = 0;
    if (j64 < ns) {
        const uint32_t code = uint32_t(reinterpret_cast<const uint64_t*>(up + j64)[3] >> 48) & 0xFFu;
        acc = code == WSG_UC_ACCEPTED;
        rej = code >= WSG_UC_BAD_HTTP && code <= WSG_UC_NOT_101;
        inc = code == WSG_UC_INCOMPLETE;
    }
    uint64_t ta, tr, ti;
    (void)block_scan_ex(acc, OpAdd{}, &ta);
    (void)block_scan_ex(rej, OpAdd{}, &tr);
    (void)block_scan_ex(inc, OpAdd{}, &ti);
    if (threadIdx.x == 0) {
        const uint64_t nb = gridDim.x;
        P.bsum[blockIdx.x] = ta;
        P.bsum[nb + blockIdx.x] = tr;
        P.bsum[2 * nb + blockIdx.x] = ti;
    }
}

__global__ __launch_bounds__(BLOCK) void k_upclient_count_blocks(UpClientPlan P, uint32_t nb,
                                                                 uint64_t* __restrict__ count)
{
    const uint64_t ta = scan_partials<uint64_t>(P.bsum, nullptr, nb, OpAdd{});
    const uint64_t tr = scan_partials<uint64_t>(P.bsum + nb, nullptr, nb, OpAdd{});
    const uint64_t ti = scan_partials<uint64_t>(P.bsum + 2 * uint64_t(nb), nullptr, nb, OpAdd{});
    if (threadIdx.x == 0) {
        count[0] = ta;
        count[1] = tr;
        count[2] = ti;
    }
}

// blocks: ceil(total / 16), total = n * tpl_len > 0.
__global__ __launch_bounds__(BLOCK) void k_upgrade_requests(const uint8_t* __restrict__ tpl, uint32_t tpl_len,
                                                            uint32_t key_at, const uint8_t* __restrict__ nonce,
                                                            uint8_t* __restrict__ req, uint64_t total, uint64_t blocks)
{
    const uint64_t step = uint64_t(gridDim.x) * BLOCK;
    for (uint64_t q = uint64_t(blockIdx.x) * BLOCK + threadIdx.x; q < blocks; q += step) {
        const uint64_t b0 = q * CHUNK;
        const uint64_t j0 = b0 / tpl_len;
        const int64_t r0 = int64_t(b0 - j0 * tpl_len);   // the block's first byte in request j0
        // the template's bytes of request j0 and, behind its end, of request j0 + 1
        // (fan_window leaves what the last aligned block holds behind the template's end: masked here)
        v4u out = fan_window(tpl, tpl_len, r0);
        const bool two = r0 + CHUNK > int64_t(tpl_len);
        if (two) {
            const v4u own = low_bytes(uint64_t(int64_t(tpl_len) - r0));
            const v4u next = fan_window(tpl, tpl_len, r0 - int64_t(tpl_len));
            out = v4u{(out.x & own.x) | (next.x & ~own.x), (out.y & own.y) | (next.y & ~own.y),
                      (out.z & own.z) | (next.z & ~own.z), (out.w & own.w) | (next.w & ~own.w)};
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (r && !two)
                break;
            // the hole of request j0 + r, in the block's bytes: [hs, hs + 24)
            const int64_t hs = int64_t(key_at) - r0 + (r ? int64_t(tpl_len) : 0);
            if (hs >= CHUNK || hs + 24 <= 0 || (j0 + r) * uint64_t(tpl_len) >= total)
                continue;
            const v4u nv = ld16(nonce + 16 * (j0 + r));
            const auto nb = [nv](uint32_t i) -> uint32_t { return lane_byte(nv, i); };
            const uint32_t from = uint32_t(hs > 0 ? hs : 0), to = uint32_t(hs + 24 < CHUNK ? hs + 24 : CHUNK);
            const v4u lo = low_bytes(uint64_t(from)), hi = low_bytes(uint64_t(to));
            out = v4u{out.x & ~(hi.x & ~lo.x), out.y & ~(hi.y & ~lo.y), out.z & ~(hi.z & ~lo.z), out.w & ~(hi.w & ~lo.w)};
            for (uint32_t k = from; k < to; ++k)
                put_byte(out, k, uc_key_char(nb, uint32_t(int64_t(k) - hs)));
        }
        if (b0 + CHUNK <= total) {
            st16nt(req + b0, out);
        } else {   // the last block: no byte at or behind `total`
            const uint32_t rest = uint32_t(total - b0);
            for (uint32_t k = 0; k < rest; ++k)
                req[b0 + k] = uint8_t(lane_byte(out, k));
        }
    }
}

uint64_t upclient_plan_layout(uint64_t* base, uint32_t ns, UpClientPlan* plan)
{
    const uint64_t nb = (uint64_t(ns) + BLOCK - 1) / BLOCK;
    Carve c{reinterpret_cast<uint8_t*>(base), 16};
    UpClientPlan P;
    P.digest = c.take<uint32_t>(8 * uint64_t(ns));
    P.bsum = c.take<uint64_t>(3 * nb);
    if (plan)
        *plan = P;
    return c.at / sizeof(uint64_t);
}

hipError_t launch_upgrade_client_streams(hipStream_t s, int grid, const uint8_t* wire, uint64_t wire_len,
                                         wsg_stream_span* span, uint32_t ns, const uint8_t* nonce,
                                         uint64_t max_response, wsg_upgrade_reply* up, uint64_t* count,
                                         const UpClientPlan& plan, unsigned long long* err)
{
    if (ns == 0)   // no stream: no count
        return hipMemsetAsync(count, 0, 3 * sizeof(uint64_t), s);
    const uint32_t nb = uint32_t((uint64_t(ns) + BLOCK - 1) / BLOCK);
    k_upclient_expect<<<nb, BLOCK, 0, s>>>(nonce, ns, plan.digest);
    k_upclient_parse<<<grid, BLOCK, 0, s>>>(wire, wire_len, span, ns, plan.digest, max_response, up, err);
    k_upclient_count_local<<<nb, BLOCK, 0, s>>>(up, ns, plan);
    k_upclient_count_blocks<<<1, BLOCK, 0, s>>>(plan, nb, count);
    return hipGetLastError();
}

hipError_t launch_upgrade_requests(hipStream_t s, int grid, const uint8_t* tpl, uint32_t tpl_len, uint32_t key_at,
                                   const uint8_t* nonce, uint8_t* req, uint64_t total)
{
    k_upgrade_requests<<<grid, BLOCK, 0, s>>>(tpl, tpl_len, key_at, nonce, req, total, (total + CHUNK - 1) / CHUNK);
    return hipGetLastError();
}

} // namespace wsg
