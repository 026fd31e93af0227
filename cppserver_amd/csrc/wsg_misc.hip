// wsg_misc.hip — the small kernels outside the batch paths, each with its
// launcher: k_xor (the per-frame host path's single-buffer XOR),
// k_rebase_offsets (the multi-GPU gather root's wire offsets, wsg_mgpu.cpp)
// and k_test_spin (a test hook of that gather).
#include "wsg_device.h"

namespace wsg {

// Single-buffer XOR used by the per-frame host path: dst[i] = src[i] ^
// key[(phase + i) % 4].  src/dst 16-byte aligned device staging buffers.
__global__ __launch_bounds__(BLOCK) void k_xor(const uint8_t* src, uint8_t* dst, uint64_t len, uint32_t key,
                                               uint32_t phase)
{
    const uint32_t k = key_rot(key, phase);
    const uint64_t chunks = len / CHUNK;
    for (uint64_t c = uint64_t(blockIdx.x) * BLOCK + threadIdx.x; c < chunks; c += uint64_t(gridDim.x) * BLOCK)
        *reinterpret_cast<v4u*>(dst + c * CHUNK) = ld16(src + c * CHUNK) ^ k;
    if (blockIdx.x == 0 && threadIdx.x < (len & (CHUNK - 1))) {
        const uint64_t q = chunks * CHUNK + threadIdx.x;
        dst[q] = src[q] ^ key_byte(key, phase + q);
    }
}

hipError_t launch_xor(hipStream_t s, int grid, const uint8_t* src, uint8_t* dst, uint64_t len, uint32_t key,
                      uint32_t phase)
{
    k_xor<<<grid, BLOCK, 0, s>>>(src, dst, len, key, phase);
    return hipGetLastError();
}

// The job's wire offsets on the gather root: every chunk's frame offsets
// arrive relative to its sender's local wire.
// Multi-GPU gather root: the job's wire offsets from every rank's local
// frame offsets.  stage holds rank r's n_local(r) local offsets at
// [rank_base[r], rank_base[r + 1]) (one transfer per rank); global frame g
// is in chunk c = g / chunk, owned by rank c % world as its local chunk
// q = c / world, which the gather placed at goff[c] in the job's wire.
__global__ __launch_bounds__(BLOCK) void k_rebase_offsets(const uint64_t* __restrict__ stage,
                                                          const uint64_t* __restrict__ goff,
                                                          const uint64_t* __restrict__ rank_base, uint64_t n_total,
                                                          uint32_t chunk, uint32_t world, uint64_t* __restrict__ out_off,
                                                          uint64_t total)
{
    const uint64_t stride = uint64_t(gridDim.x) * BLOCK;
    for (uint64_t g = uint64_t(blockIdx.x) * BLOCK + threadIdx.x; g < n_total; g += stride) {
        const uint64_t c = g / chunk;
        const uint64_t r = c % world, q = c / world;
        const uint64_t* loc = stage + rank_base[r] + q * chunk;
        out_off[g] = loc[g - c * chunk] - loc[0] + goff[c];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        out_off[n_total] = total;
}

hipError_t launch_rebase_offsets(hipStream_t s, const uint64_t* stage, const uint64_t* goff, const uint64_t* rank_base,
                                 uint64_t n_total, uint32_t chunk, uint32_t world, uint64_t* out_off, uint64_t total)
{
    const uint64_t blocks = std::min<uint64_t>(std::max<uint64_t>((n_total + BLOCK - 1) / BLOCK, 1), 8192);
    k_rebase_offsets<<<uint32_t(blocks), BLOCK, 0, s>>>(stage, goff, rank_base, n_total, chunk, world, out_off, total);
    return hipGetLastError();
}

// Test hook of the multi-GPU gather ($WSG_TEST_NULL_SPIN_US, wsg_mgpu.cpp):
// one wave that waits `ticks` of the constant-rate wall clock on the stream
// it is launched on.  The iteration cap ends it whatever the clock does
// (about 2 s at the most).
__global__ __launch_bounds__(64) void k_test_spin(uint64_t ticks)
{
    const uint64_t t0 = wall_clock64();
    for (uint32_t i = 0; i < (1u << 20); ++i) {
        if (wall_clock64() - t0 >= ticks)
            break;
        __builtin_amdgcn_s_sleep(64);
    }
}

hipError_t launch_test_spin(hipStream_t s, uint32_t us)
{
    int dev = 0, khz = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0)
        khz = 100000;   // 100 MHz, the gfx9 constant clock
    k_test_spin<<<1, 64, 0, s>>>(uint64_t(std::min<uint32_t>(us, 200000u)) * uint64_t(khz) / 1000u);
    return hipGetLastError();
}

} // namespace wsg
