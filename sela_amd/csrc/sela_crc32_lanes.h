// sela_crc32_lanes.h -- how the digest kernels (sela_digest.hip; sela_digest_pcm.hip, 5.29) put a CRC together from
// their lanes, waves and workgroups: the shift identity of sela_crc32.h with the multipliers as literals.  Device code only.
//
// A thread takes pieces of P bytes at the workgroup's stride T (piece t, t + T, ...): its register times x^(8 P (T - 1)) before each
// further piece, each dword of the piece by (r ^ w) * x^32 -- the multiplier's 32 columns are literals.  The 64 lanes are joined on
// the DPP ladder of wave_sum_small with a multiply by x^(8 P 2^k) per rung, the waves through one word each of LDS.  Everything is
// XOR, shift and AND on 32-bit integers: no float, no atomics, no table.
#ifndef SELA_CRC32_LANES_H_
#define SELA_CRC32_LANES_H_

#include <hip/hip_runtime.h>

#include "sela_crc32.h"

namespace sela {

// a * K for a constant K: the 32 columns K * x^i are literals
template <uint32_t K>
struct CrcColumns {
    uint32_t c[32];
    constexpr CrcColumns() : c{}
    {
        uint32_t b = K;
        for (int i = 0; i < 32; i++) {
            c[i] = b;
            b = crc_times_x(b);
        }
    }
};
template <uint32_t K>
__device__ __forceinline__ uint32_t crc_mul_const(uint32_t a)
{
    constexpr CrcColumns<K> cols;
    uint32_t p = 0;
#pragma unroll
    for (int i = 0; i < 32; i++)
        p ^= (uint32_t)((int32_t)(a << i) >> 31) & cols.c[i];
    return p;
}
// the register after four more bytes (little-endian in w), after two (in the low half of v)
__device__ __forceinline__ uint32_t crc_step32(uint32_t r, uint32_t w) { return crc_mul_const<kCrcX32>(r ^ w); }
__device__ __forceinline__ uint32_t crc_step16(uint32_t r, uint32_t v) { return crc_mul_const<kCrcX16>(r ^ v); }

// The constants of one (piece, workgroup) shape: P bytes a piece, T threads.
struct DigestShape {
    uint32_t stride;  // x^(8 P (T - 1)): a thread's register before its next piece
    uint32_t lane[6]; // x^(8 P 2^k): the rungs of the lane ladder
    uint32_t wave;    // x^(8 P 64): from one wave to the next
    uint32_t finish;  // fused frames: crc = raw ^ finish (0xFFFFFFFF * x^(8 bytes) ^ 0xFFFFFFFF)
    uint32_t steps, pad; // fused frames: pieces per thread, and the empty pieces ahead of the first (steps * T - pieces)
};
constexpr DigestShape digest_shape(uint32_t piece_bytes, uint32_t threads, uint32_t pieces)
{
    DigestShape s{};
    s.stride = crc_xpow8((uint64_t)piece_bytes * (threads - 1));
    for (int k = 0; k < 6; k++)
        s.lane[k] = crc_xpow8((uint64_t)piece_bytes << k);
    s.wave = crc_xpow8((uint64_t)piece_bytes * 64);
    s.finish = crc_from_raw(0, (uint64_t)piece_bytes * pieces);
    s.steps = (pieces + threads - 1) / threads;
    s.pad = s.steps * threads - pieces;
    return s;
}

__device__ __forceinline__ uint32_t wave_xor(uint32_t v)
{
    v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111 /* row_shr:1 */, 0xf, 0xf, false);
    v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112 /* row_shr:2 */, 0xf, 0xf, false);
    v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114 /* row_shr:4 */, 0xf, 0xf, false);
    v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118 /* row_shr:8 */, 0xf, 0xf, false);
    v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142 /* row_bcast:15 */, 0xa, 0xf, false);
    v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143 /* row_bcast:31 */, 0xc, 0xf, false);
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// The wave's raw CRC from its lanes' (lane l's pieces lie one piece ahead of lane l + 1's): wave_sum_small's ladder, what comes
// from k lanes below times x^(8 P k) on its way.  A lane that receives nothing receives 0, and 0 times anything is 0.
__device__ __forceinline__ uint32_t wave_crc(uint32_t v, const DigestShape& s)
{
    v ^= crc_mul((uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111 /* row_shr:1 */, 0xf, 0xf, false), s.lane[0]);
    v ^= crc_mul((uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112 /* row_shr:2 */, 0xf, 0xf, false), s.lane[1]);
    v ^= crc_mul((uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114 /* row_shr:4 */, 0xf, 0xf, false), s.lane[2]);
    v ^= crc_mul((uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118 /* row_shr:8 */, 0xf, 0xf, false), s.lane[3]);
    // lane 15 of every row now holds its row's; lanes 31 and 63 take the row below theirs, then lane 63 the lower half
    v ^= crc_mul((uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142 /* row_bcast:15 */, 0xa, 0xf, false), s.lane[4]);
    v ^= crc_mul((uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143 /* row_bcast:31 */, 0xc, 0xf, false), s.lane[5]);
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// The workgroup's raw CRC from its waves' (one word each in `part`), by one thread.
__device__ __forceinline__ uint32_t waves_crc(const uint32_t* part, int part_stride, int n_waves, const DigestShape& s)
{
    uint32_t r = 0;
    for (int w = 0; w < n_waves; w++)
        r = crc_mul(r, s.wave) ^ part[w * part_stride];
    return r;
}

// The kernels that take bytes out of memory (global or LDS) and fold words: 256 threads, 16-byte lines.
constexpr uint32_t kDigestThreads = 256;
constexpr DigestShape kPcmShape = digest_shape(16, kDigestThreads, 0);

// XOR over the workgroup, in thread 0
__device__ __forceinline__ uint32_t block_xor(uint32_t v, uint32_t* s_part /* [kDigestThreads / 64] */)
{
    v = wave_xor(v);
    if (threadIdx.x % 64 == 0)
        s_part[threadIdx.x / 64] = v;
    __syncthreads();
    uint32_t all = 0;
    if (threadIdx.x == 0)
        for (uint32_t w = 0; w < kDigestThreads / 64; w++)
            all ^= s_part[w];
    return all;
}

} // namespace sela
#endif
