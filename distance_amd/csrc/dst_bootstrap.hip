// dst_bootstrap.hip — the replicate alignments of dst_nj_bootstrap: the column map of one replicate and
// the gather of its n x len codes from the call's device copy of the original codes, into a pitched buffer that the
// upload path packs (pack_queue) like any device upload.
//
//   boot_map_kernel        map[c] := boot_column(seed, r * len + c, len) for the replicate's len columns
//   boot_resample_kernel   row by row: out[i][c] := src[i][map[c]].  A row of at most kBootLdsBytes is first staged in
//                          LDS with 16-byte loads and gathered from there; a longer one is gathered from global memory.
//                          Each thread writes 4 columns as one 32-bit store, so a wave writes 256 contiguous bytes; the
//                          row's padding up to the next 4 bytes (inside the 128-byte pitch) is written as N.
#include "dst_device.hpp"

namespace dst {

// SplitMix64 output number k of the generator seeded with `seed`, scaled to [0, len) by the high half of z * len
// (include/distance_hip.h).  The only definition: the host export and the device map both call it.
__host__ __device__ inline uint32_t boot_column(uint64_t seed, uint64_t k, uint64_t len)
{
    uint64_t z = seed + (k + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
#ifdef __HIP_DEVICE_COMPILE__
    return (uint32_t)__umul64hi(z, len);
#else
    return (uint32_t)(((unsigned __int128)z * len) >> 64);
#endif
}

namespace {

constexpr int kBootThreads = 256;
constexpr uint64_t kBootLdsBytes = 48 * 1024;   // a 30 kbp genome's row fits; several workgroups per CU (160 KiB of LDS)
constexpr uint64_t kBootMaxBlocks = 65536;

__global__ __launch_bounds__(kBootThreads) void boot_map_kernel(uint64_t seed, uint32_t replicate, uint64_t len,
                                                                uint32_t *map)
{
    const uint64_t c = (uint64_t)blockIdx.x * kBootThreads + threadIdx.x;
    if (c < len)
        map[c] = boot_column(seed, (uint64_t)replicate * len + c, len);
}

// src and out rows are `pitch` bytes apart; pitch is a multiple of 128 and at least len, so the 16-byte staging loads
// (ceil(len / 16) of them) and the 4-byte stores (ceil(len / 4)) stay inside the row.
template <bool kLds>
__global__ __launch_bounds__(kBootThreads) void boot_resample_kernel(const uint8_t *__restrict__ src, uint64_t pitch,
                                                                     uint8_t *__restrict__ out, uint64_t n, uint64_t len,
                                                                     const uint32_t *__restrict__ map)
{
    extern __shared__ uint4 s_row[];
    const uint8_t *s_bytes = reinterpret_cast<const uint8_t *>(s_row);
    const uint64_t words = (len + 3) / 4;
    for (uint64_t i = blockIdx.x; i < n; i += gridDim.x) {
        const uint8_t *row = src + i * pitch;
        if (kLds) {
            const uint64_t vecs = (len + 15) / 16;
            for (uint64_t q = threadIdx.x; q < vecs; q += kBootThreads)
                s_row[q] = reinterpret_cast<const uint4 *>(row)[q];
            __syncthreads();
        }
        uint32_t *dst = reinterpret_cast<uint32_t *>(out + i * pitch);
        for (uint64_t w = threadIdx.x; w < words; w += kBootThreads) {
            uint32_t v = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const uint64_t c = 4 * w + b;
                const uint32_t code = c < len ? (uint32_t)(kLds ? s_bytes[map[c]] : row[map[c]]) : 240u;   // 240: N
                v |= code << (8 * b);
            }
            dst[w] = v;
        }
        if (kLds)
            __syncthreads();   // (the next row's staging overwrites s_row)
    }
}

}  // namespace

hipError_t launch_boot_resample(const uint8_t *src, uint64_t pitch, uint8_t *out, uint64_t n, uint64_t len, uint64_t seed,
                                uint32_t replicate, uint32_t *map, hipStream_t stream)
{
    if (n == 0 || len == 0)
        return hipSuccess;
    hipLaunchKernelGGL(boot_map_kernel, dim3((unsigned)((len + kBootThreads - 1) / kBootThreads)), dim3(kBootThreads), 0,
                       stream, seed, replicate, len, map);
    const dim3 grid((unsigned)std::min<uint64_t>(n, kBootMaxBlocks));
    const uint64_t staged = (len + 15) / 16 * 16;
    if (staged <= kBootLdsBytes)
        hipLaunchKernelGGL(boot_resample_kernel<true>, grid, dim3(kBootThreads), (unsigned)staged, stream, src, pitch, out,
                           n, len, map);
    else
        hipLaunchKernelGGL(boot_resample_kernel<false>, grid, dim3(kBootThreads), 0, stream, src, pitch, out, n, len, map);
    return hipGetLastError();
}

}  // namespace dst

extern "C" void dst_bootstrap_columns(uint64_t seed, uint32_t replicate, uint64_t len, uint32_t *cols)
{
    if (!cols)
        return;
    for (uint64_t c = 0; c < len; ++c)
        cols[c] = dst::boot_column(seed, (uint64_t)replicate * len + c, len);
}
