// envelope_report.cpp -- host/include/sela_host/envelope.hpp alone (no GPU, no library): the frames' slots compacted onto the
// track's grid, the .env file's bytes and the refusals, under -fsanitize=address,undefined.  The expectations are computed here,
// from the definitions.
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

static bool same(const sela::EnvelopeRecord& a, const sela::EnvelopeRecord& b)
{
    return a.min == b.min && a.max == b.max && a.sum == b.sum && a.sumSquares == b.sumSquares;
}

int main()
{
    using namespace sela;
    // buckets and slots
    {
        for (uint32_t b : { 32u, 64u, 128u, 256u, 512u, 1024u, 2048u })
            CHECK(envelopeBucketOk(b));
        for (uint32_t b : { 0u, 1u, 16u, 48u, 2047u, 4096u, 0x80000000u })
            CHECK(!envelopeBucketOk(b) && envelopeSlots(2048, b) == 0);
        CHECK(envelopeSlots(1, 32) == 1 && envelopeSlots(2047, 32) == 64 && envelopeSlots(2048, 32) == 64 && envelopeSlots(2049, 32) == 65);
        CHECK(envelopeSlots(4095, 2048) == 2 && envelopeSlots(65535, 32) == 2048 && envelopeSlots(0xFFFFFFFFu, 2048) == (1u << 21));
    }
    // compaction: frames of 2048, 2048 and 2048 + 777 samples at stride 4095, bucket 1024: 4 slots a frame, 2 + 2 + 3 used
    {
        const uint32_t slots = envelopeSlots(4095, 1024), channels = 2;
        CHECK(slots == 4);
        const uint64_t so[4] = { 0, 2048, 4096, 4096 + 2825 };
        std::vector<EnvelopeRecord> rec((size_t)3 * slots * channels);
        for (size_t i = 0; i < rec.size(); i++)
            rec[i] = { (int16_t)-(int)i, (int16_t)i, (int32_t)(1000 + i), (uint64_t)i << 33 };
        const std::vector<EnvelopeRecord> got = compactEnvelope(rec.data(), so, 3, slots, channels, 1024);
        CHECK(got.size() == (size_t)(2 + 2 + 3) * channels);
        size_t at = 0;
        for (size_t f = 0; f < 3; f++)
            for (size_t b = 0; b < (f == 2 ? 3u : 2u); b++)
                for (uint32_t c = 0; c < channels; c++, at++)
                    CHECK(at < got.size() && same(got[at], rec[(f * slots + b) * channels + c]));
        // no frames, and a frame without samples
        CHECK(compactEnvelope(nullptr, so, 0, slots, channels, 1024).empty());
        const uint64_t none[2] = { 5, 5 };
        CHECK(compactEnvelope(rec.data(), none, 1, slots, channels, 1024).empty());
        // a middle frame whose length is no multiple of the bucket, a frame longer than its slots, a bucket outside the set
        const uint64_t ragged[4] = { 0, 2048, 2048 + 777, 2048 + 777 + 2048 };
        CHECK(refuses([&] { compactEnvelope(rec.data(), ragged, 3, slots, channels, 1024); }, "frame 1 holds 777 samples"));
        CHECK(compactEnvelope(rec.data(), ragged, 2, slots, channels, 1024).size() == (size_t)(2 + 1) * channels); // (the last frame may be ragged)
        const uint64_t longer[2] = { 0, 4097 };
        CHECK(refuses([&] { compactEnvelope(rec.data(), longer, 1, slots, channels, 1024); }, "more than its slots"));
        CHECK(refuses([&] { compactEnvelope(rec.data(), so, 3, slots, channels, 48); }, kEnvelopeBucketSet));
    }
    // the file: header fields at their offsets, little-endian, then the records as they lie in memory
    {
        EnvelopeReport r;
        r.channels = 2, r.bucket = 256, r.sampleRate = 44100, r.samplesPerChannel = ((uint64_t)1 << 32) + 257; // (a count beyond 32 bits)
        CHECK(r.buckets() == ((uint64_t)1 << 24) + 2);
        r.samplesPerChannel = 600;
        CHECK(r.buckets() == 3);
        r.records.assign(6, EnvelopeRecord{ -32768, 32767, -(1 << 26), (uint64_t)1 << 41 });
        r.records[5] = { -2, -1, -3, 5 };
        const std::vector<uint8_t> bytes = envelopeFileBytes(r);
        CHECK(bytes.size() == 32 + 6 * 16 && kEnvelopeHeaderBytes == 32);
        const uint8_t head[32] = { 'S', 'E', 'L', 'A', 'E', 'N', 'V', '1', 2, 0, 0, 0, 0, 1, 0, 0, 0x58, 2, 0, 0, 0, 0, 0, 0, 0x44, 0xAC, 0, 0, 16, 0, 0, 0 };
        CHECK(std::memcmp(bytes.data(), head, 32) == 0);
        const uint8_t first[16] = { 0x00, 0x80, 0xFF, 0x7F, 0, 0, 0, 0xFC, 0, 0, 0, 0, 0, 2, 0, 0 };
        const uint8_t last[16] = { 0xFE, 0xFF, 0xFF, 0xFF, 0xFD, 0xFF, 0xFF, 0xFF, 5, 0, 0, 0, 0, 0, 0, 0 };
        CHECK(std::memcmp(bytes.data() + 32, first, 16) == 0 && std::memcmp(bytes.data() + 32 + 5 * 16, last, 16) == 0);
        r.samplesPerChannel = ((uint64_t)5 << 32) + 600;
        r.records.clear();
        r.bucket = 2048, r.channels = 0; // (no channels: no records, whatever the length)
        const std::vector<uint8_t> wide = envelopeFileBytes(r);
        CHECK(wide.size() == 32 && wide[16] == 0x58 && wide[17] == 2 && wide[20] == 5 && wide[12] == 0 && wide[13] == 8);
        // a report whose records do not match its header is not written
        r.channels = 2;
        CHECK(refuses([&] { envelopeFileBytes(r); }, "its header says"));
        const EnvelopeReport empty;
        CHECK(empty.buckets() == 0 && envelopeFileBytes(empty).size() == 32);
    }
    // the refusals' texts
    {
        CHECK(envelopeBucketRefusal(48) == std::string("Envelope: --bucket 48 is not one of 32, 64, 128, 256, 512, 1024, 2048"));
        CHECK(envelopeBucketRefusal(-5).find("-5") != std::string::npos);
        const std::string bits = envelopeBitsRefusal("a/b.sela", 24);
        CHECK(bits.find("a/b.sela") != std::string::npos && bits.find("24-bit") != std::string::npos && bits.find("16-bit") != std::string::npos);
        CHECK(kEnvelopeDefaultBucket == 256);
    }
    std::printf("envelope_report: %d failures\n", failures);
    return failures ? 1 : 0;
}
