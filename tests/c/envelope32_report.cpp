// envelope32_report.cpp -- host/include/sela_host/envelope.hpp alone (no GPU, no library), the wide part: the
// frames' slots of 32-byte records compacted onto the track's grid, the wide .env file's header and bytes, the refusals -- and the
// 16-bit functions beside them still give their bytes -- under -fsanitize=address,undefined.  The expectations are computed
// here, from the definitions.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "sela_host/envelope.hpp"

static int failures = 0;
#define CHECK(x)                                                         \
    do {                                                                 \
        if (!(x)) {                                                      \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);   \
            failures++;                                                  \
        }                                                                \
    } while (0)

template <typename F>
static bool refuses(F f, const char* needle)
{
    try {
        f();
    } catch (const std::invalid_argument& e) {
        return std::strstr(e.what(), needle) != nullptr;
    }
    return false;
}

static bool same(const sela::EnvelopeRecord32& a, const sela::EnvelopeRecord32& b)
{
    return a.min == b.min && a.max == b.max && a.sum == b.sum && a.sumSquaresLo == b.sumSquaresLo && a.sumSquaresHi == b.sumSquaresHi;
}

int main()
{
    using namespace sela;
    // the record as the device lays it out
    {
        CHECK(sizeof(EnvelopeRecord32) == 32 && offsetof(EnvelopeRecord32, min) == 0 && offsetof(EnvelopeRecord32, max) == 4 && offsetof(EnvelopeRecord32, sum) == 8
            && offsetof(EnvelopeRecord32, sumSquaresLo) == 16 && offsetof(EnvelopeRecord32, sumSquaresHi) == 24);
    }
    // compaction: frames of 2048, 2048 and 2048 + 777 samples at stride 2825, bucket 1024: 3 slots a frame, 2 + 2 + 3 used
    {
        const uint32_t slots = envelopeSlots(2825, 1024), channels = 2;
        CHECK(slots == 3);
        const uint64_t so[4] = { 0, 2048, 4096, 4096 + 2825 };
        std::vector<EnvelopeRecord32> rec((size_t)3 * slots * channels);
        for (size_t i = 0; i < rec.size(); i++)
            rec[i] = { (int32_t)(INT32_MIN + (int32_t)i), (int32_t)(INT32_MAX - (int32_t)i), -((int64_t)1 << 42) + (int64_t)i, (uint64_t)i << 60, (uint64_t)512 - i };
        const std::vector<EnvelopeRecord32> got = compactEnvelope32(rec.data(), so, 3, slots, channels, 1024);
        CHECK(got.size() == (size_t)(2 + 2 + 3) * channels);
        size_t at = 0;
        for (size_t f = 0; f < 3; f++)
            for (size_t b = 0; b < (f == 2 ? 3u : 2u); b++)
                for (uint32_t c = 0; c < channels; c++, at++)
                    CHECK(at < got.size() && same(got[at], rec[(f * slots + b) * channels + c]));
        // no frames, and a frame without samples
        CHECK(compactEnvelope32(nullptr, so, 0, slots, channels, 1024).empty());
        const uint64_t none[2] = { 5, 5 };
        CHECK(compactEnvelope32(rec.data(), none, 1, slots, channels, 1024).empty());
        // a middle frame whose length is no multiple of the bucket, a frame longer than its slots, a bucket outside the set
        const uint64_t ragged[4] = { 0, 2048, 2048 + 777, 2048 + 777 + 2048 };
        CHECK(refuses([&] { compactEnvelope32(rec.data(), ragged, 3, slots, channels, 1024); }, "frame 1 holds 777 samples"));
        CHECK(compactEnvelope32(rec.data(), ragged, 2, slots, channels, 1024).size() == (size_t)(2 + 1) * channels); // (the last frame may be ragged)
        const uint64_t longer[2] = { 0, 3073 };
        CHECK(refuses([&] { compactEnvelope32(rec.data(), longer, 1, slots, channels, 1024); }, "more than its slots"));
        CHECK(refuses([&] { compactEnvelope32(rec.data(), so, 3, slots, channels, 48); }, kEnvelopeBucketSet));
    }
    // the wide file: the 16-bit file's header with the file's bits for its last word, then 32-byte records, little-endian
    {
        EnvelopeReport32 r;
        r.channels = 2, r.bucket = 256, r.sampleRate = 48000, r.bitsPerSample = 24, r.samplesPerChannel = 600;
        CHECK(r.buckets() == 3);
        r.records.assign(6, EnvelopeRecord32{ INT32_MIN, INT32_MAX, -((int64_t)1 << 42), 0, 512 });
        r.records[5] = { -2, -1, -3, 5, 0 };
        std::vector<uint8_t> bytes = envelopeFileBytes32(r);
        CHECK(bytes.size() == 32 + 6 * 32);
        const uint8_t head[32] = { 'S', 'E', 'L', 'A', 'E', 'N', 'V', '1', 2, 0, 0, 0, 0, 1, 0, 0, 0x58, 2, 0, 0, 0, 0, 0, 0, 0x80, 0xBB, 0, 0, 24, 0, 0, 0 };
        CHECK(std::memcmp(bytes.data(), head, 32) == 0);
        const uint8_t first[32] = { 0, 0, 0, 0x80, 0xFF, 0xFF, 0xFF, 0x7F, 0, 0, 0, 0, 0, 0xFC, 0xFF, 0xFF, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0 };
        const uint8_t last[32] = { 0xFE, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFD, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 5, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
        CHECK(std::memcmp(bytes.data() + 32, first, 32) == 0 && std::memcmp(bytes.data() + 32 + 5 * 32, last, 32) == 0);
        r.bitsPerSample = 32;
        bytes = envelopeFileBytes32(r);
        CHECK(bytes.size() == 32 + 6 * 32 && bytes[28] == 32 && bytes[29] == 0 && std::memcmp(bytes.data() + 32, first, 32) == 0);
        // a count beyond 32 bits, no channels: no records, whatever the length
        r.samplesPerChannel = ((uint64_t)5 << 32) + 600;
        r.records.clear();
        r.bucket = 2048, r.channels = 0;
        const std::vector<uint8_t> bare = envelopeFileBytes32(r);
        CHECK(bare.size() == 32 && bare[16] == 0x58 && bare[17] == 2 && bare[20] == 5 && bare[12] == 0 && bare[13] == 8 && bare[28] == 32);
        // a report whose records do not match its header, or whose samples are not wide, is not written
        r.channels = 2;
        CHECK(refuses([&] { envelopeFileBytes32(r); }, "its header says"));
        r.channels = 0, r.bitsPerSample = 16;
        CHECK(refuses([&] { envelopeFileBytes32(r); }, "24- or 32-bit"));
        const EnvelopeReport32 empty;
        CHECK(empty.buckets() == 0 && refuses([&] { envelopeFileBytes32(empty); }, "24- or 32-bit"));
    }
    // the 16-bit functions beside them: their bytes as before
    {
        EnvelopeReport r;
        r.channels = 2, r.bucket = 256, r.sampleRate = 44100, r.samplesPerChannel = 600;
        r.records.assign(6, EnvelopeRecord{ -32768, 32767, -(1 << 26), (uint64_t)1 << 41 });
        r.records[5] = { -2, -1, -3, 5 };
        const std::vector<uint8_t> bytes = envelopeFileBytes(r);
        CHECK(bytes.size() == 32 + 6 * 16 && kEnvelopeHeaderBytes == 32);
        const uint8_t head[32] = { 'S', 'E', 'L', 'A', 'E', 'N', 'V', '1', 2, 0, 0, 0, 0, 1, 0, 0, 0x58, 2, 0, 0, 0, 0, 0, 0, 0x44, 0xAC, 0, 0, 16, 0, 0, 0 };
        CHECK(std::memcmp(bytes.data(), head, 32) == 0);
        const uint8_t first[16] = { 0x00, 0x80, 0xFF, 0x7F, 0, 0, 0, 0xFC, 0, 0, 0, 0, 0, 2, 0, 0 };
        const uint8_t last[16] = { 0xFE, 0xFF, 0xFF, 0xFF, 0xFD, 0xFF, 0xFF, 0xFF, 5, 0, 0, 0, 0, 0, 0, 0 };
        CHECK(std::memcmp(bytes.data() + 32, first, 16) == 0 && std::memcmp(bytes.data() + 32 + 5 * 16, last, 16) == 0);
        const uint64_t so[3] = { 0, 2048, 2048 + 777 };
        std::vector<EnvelopeRecord> rec((size_t)2 * 2 * 1);
        for (size_t i = 0; i < rec.size(); i++)
            rec[i] = { (int16_t)-(int)i, (int16_t)i, (int32_t)(1000 + i), (uint64_t)i << 33 };
        const std::vector<EnvelopeRecord> got = compactEnvelope(rec.data(), so, 2, 2, 1, 1024);
        CHECK(got.size() == 3 && got[2].sum == 1002 && got[2].sumSquares == ((uint64_t)2 << 33));
        CHECK(envelopeBitsRefusal("a/b.sela", 24).find("the envelope is taken of 16-bit streams only") != std::string::npos);
    }
    std::printf("envelope32_report: %d failures\n", failures);
    return failures ? 1 : 0;
}
