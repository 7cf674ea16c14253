// sela_crc32.h -- the arithmetic of the digest calls: CRC-32 of IEEE 802.3 (zlib.crc32) as polynomials over
// GF(2) mod P, in zlib's reflected representation -- bit 31 of a word is x^0, bit 0 is x^31, P without its x^32 term is 0xEDB88320.
//
//   raw(M)   the register after the bytes of M from a register of 0, no final XOR: linear in M, and raw(A | B) = raw(A) * x^(8 |B|) ^ raw(B)
//   crc(M)   = raw(M) ^ 0xFFFFFFFF * x^(8 |M|) ^ 0xFFFFFFFF, what everybody prints; crc(A | B) = crc(A) * x^(8 |B|) ^ crc(B), crc() = 0
//
// Plain C++17, host and device alike; no HIP needed: tests/c/crc32_combine.cpp compiles it alone.
#ifndef SELA_CRC32_H_
#define SELA_CRC32_H_

#include <cstddef>
#include <cstdint>

#include "sela_crc32_tables.h"

#if defined(__HIPCC__)
#define SELA_CRC_FN __host__ __device__ inline
#else
#define SELA_CRC_FN inline
#endif

namespace sela {

constexpr uint32_t kCrcPoly = 0xEDB88320u; // = x^32 mod P
constexpr uint32_t kCrcOne = 0x80000000u;  // x^0
constexpr uint32_t kCrcX8 = kCrcOne >> 8, kCrcX16 = kCrcOne >> 16, kCrcX32 = kCrcPoly;

// b * x mod P
SELA_CRC_FN constexpr uint32_t crc_times_x(uint32_t b) { return (b >> 1) ^ ((0u - (b & 1u)) & kCrcPoly); }

// a * b mod P: 32 steps of select-and-XOR over b * x^i
SELA_CRC_FN constexpr uint32_t crc_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 0; i < 32; i++) {
        p ^= (0u - ((a >> (31 - i)) & 1u)) & b;
        b = crc_times_x(b);
    }
    return p;
}

// x^(8 n) mod P by square-and-multiply over x^(8 * 2^k).  (x^(2^32) = x mod P, so the table repeats with period 32 behind its end.)
SELA_CRC_FN constexpr uint32_t crc_xpow8(uint64_t n)
{
    const uint32_t table[SELA_CRC32_X8POW2_ENTRIES] = { SELA_CRC32_X8POW2 };
    uint32_t p = kCrcOne;
    for (int k = 0; n; n >>= 1, k++)
        if (n & 1)
            p = crc_mul(table[k < SELA_CRC32_X8POW2_ENTRIES ? k : k - 32], p);
    return p;
}

// crc(A | B) from crc(A), crc(B) and |B|
SELA_CRC_FN constexpr uint32_t crc_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) { return crc_mul(crc_a, crc_xpow8(len_b)) ^ crc_b; }

// crc(M) from raw(M) and |M|
SELA_CRC_FN constexpr uint32_t crc_from_raw(uint32_t raw, uint64_t len) { return raw ^ crc_mul(0xFFFFFFFFu, crc_xpow8(len)) ^ 0xFFFFFFFFu; }

// raw(M | one byte) from raw(M), bit by bit (the edges of a range; the host's check of the kernels' constants)
SELA_CRC_FN constexpr uint32_t crc_raw_byte(uint32_t raw, uint32_t byte)
{
    raw ^= byte & 0xFFu;
    for (int i = 0; i < 8; i++)
        raw = crc_times_x(raw);
    return raw;
}

} // namespace sela
#endif
