// crc32_combine.cpp -- sela_amd/csrc/sela_crc32.h and host/include/sela_host/digest.hpp alone (plain C++17, no HIP), under
// -fsanitize=address,undefined: the shift identities the digest kernels are built on and the host's table-driven CRC-32, held
// against a bit-by-bit CRC-32 written out here.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "sela_crc32.h"
#include "sela_host/digest.hpp"

static uint32_t plain_crc(const uint8_t* p, size_t n, uint32_t crc = 0)
{
    crc = ~crc;
    for (size_t i = 0; i < n; i++) {
        crc ^= p[i];
        for (int k = 0; k < 8; k++)
            crc = (crc >> 1) ^ ((crc & 1u) ? 0xEDB88320u : 0u);
    }
    return ~crc;
}

static int failures = 0;
#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);      \
            failures++;                                                \
        }                                                              \
    } while (0)

int main()
{
    using namespace sela;
    CHECK(plain_crc(reinterpret_cast<const uint8_t*>("123456789"), 9) == 0xCBF43926u); // the check value of CRC-32
    std::vector<uint8_t> data(20000);
    uint32_t x = 12345;
    for (auto& b : data) {
        x = x * 1664525u + 1013904223u;
        b = (uint8_t)(x >> 24);
    }
    // the table: entry k is entry k - 1 squared, entry 0 is x^8
    const uint32_t table[SELA_CRC32_X8POW2_ENTRIES] = { SELA_CRC32_X8POW2 };
    CHECK(table[0] == kCrcX8 && table[1] == kCrcX16 && table[2] == kCrcX32);
    for (int k = 1; k < SELA_CRC32_X8POW2_ENTRIES; k++)
        CHECK(table[k] == crc_mul(table[k - 1], table[k - 1]));
    CHECK(crc_mul(kCrcOne, 0x12345678u) == 0x12345678u && crc_mul(0x12345678u, kCrcOne) == 0x12345678u);
    // crc(A | B) for second parts of 0, 1, 3, 4, 8192 bytes, at several splits
    const size_t second[] = { 0, 1, 3, 4, 8192 };
    for (size_t nb : second)
        for (size_t na : { (size_t)0, (size_t)1, (size_t)5, (size_t)4097 }) {
            const uint32_t a = plain_crc(data.data(), na), b = plain_crc(data.data() + na, nb);
            CHECK(crc_combine(a, b, nb) == plain_crc(data.data(), na + nb));
        }
    // a chain of six parts, one of them empty
    const size_t cuts[] = { 0, 7, 7, 2048, 2051, 12000, 20000 };
    uint32_t chain = 0;
    for (int i = 0; i < 6; i++)
        chain = crc_combine(chain, plain_crc(data.data() + cuts[i], cuts[i + 1] - cuts[i]), cuts[i + 1] - cuts[i]);
    CHECK(chain == plain_crc(data.data(), 20000));
    // raw and crc: crc(M) = raw(M) ^ 0xFFFFFFFF x^(8 |M|) ^ 0xFFFFFFFF
    for (size_t n : { (size_t)0, (size_t)1, (size_t)2, (size_t)3, (size_t)100 }) {
        uint32_t raw = 0;
        for (size_t i = 0; i < n; i++)
            raw = crc_raw_byte(raw, data[i]);
        CHECK(crc_from_raw(raw, n) == plain_crc(data.data(), n));
    }
    CHECK(crc_from_raw(0, 0) == 0);
    // huge distances: x^(8 (a + b)) = x^(8 a) x^(8 b), the period of the table behind its end
    const uint64_t huge[] = { ((uint64_t)1 << 32) + 5, (uint64_t)1 << 40, ((uint64_t)1 << 52) + 3, ~(uint64_t)0 };
    for (uint64_t n : huge) {
        const uint64_t half = n / 2;
        CHECK(crc_xpow8(n) == crc_mul(crc_xpow8(half), crc_xpow8(n - half)));
        CHECK(crc_combine(0xDEADBEEFu, 0x01020304u, n) == crc_combine(crc_combine(0xDEADBEEFu, 0, half), 0x01020304u, n - half));
    }
    // the host's CRC-32 of a WAV's data chunk: in one piece, in pieces (an empty one among them), of nothing
    {
        Crc32 whole, pieces, none;
        whole.update(data.data(), data.size());
        pieces.update(data.data(), 1), pieces.update(data.data() + 1, 0), pieces.update(data.data() + 1, 4096), pieces.update(data.data() + 4097, data.size() - 4097);
        CHECK(whole.value() == plain_crc(data.data(), data.size()) && pieces.value() == whole.value() && none.value() == 0);
        DigestReport r;
        r.crc32 = 0xCBF43926u, r.bytes = 9, r.frames = 1;
        CHECK(formatDigestReport(r) == "crc32=cbf43926 bytes=9 frames=1\n" && r.agree());
        r.haveWav = true, r.wavCrc32 = 0xCBF43926u, r.wavBytes = 9;
        CHECK(r.agree() && formatDigestReport(r).find("\nmatch\n") != std::string::npos);
        r.wavBytes = 8;
        CHECK(!r.agree() && formatDigestReport(r).find("MISMATCH") != std::string::npos);
    }
    static_assert(crc_xpow8(4) == kCrcX32 && crc_xpow8(0) == kCrcOne, "usable in constant expressions");
    std::printf("crc32_combine: %d failures\n", failures);
    return failures != 0;
}
