// envelope.hpp -- what a stream's envelope records (struct sela_hip_envelope, include/sela_hip.h; DESIGN.md 5.31 -- and struct
// sela_hip_envelope32 of 24- and 32-bit streams, 5.32) become on the
// host: the frames' slots compacted onto the track's grid, and the .env file sela_mi355x -w and -W write.  Pure arithmetic: no GPU, no
// file, nothing but the standard library -- tests/c/envelope_report.cpp compiles it alone.
#ifndef SELA_HOST_ENVELOPE_HPP_
#define SELA_HOST_ENVELOPE_HPP_

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

namespace sela {

// One (frame, bucket, channel) as the device writes it: the layout of struct sela_hip_envelope.
struct EnvelopeRecord {
    int16_t min, max;    // the smallest and the largest sample of the bucket
    int32_t sum;         // sum of v
    uint64_t sumSquares; // sum of v * v
};
static_assert(sizeof(EnvelopeRecord) == 16, "struct sela_hip_envelope");

constexpr uint32_t kEnvelopeDefaultBucket = 256;
constexpr const char* kEnvelopeBucketSet = "32, 64, 128, 256, 512, 1024, 2048";

inline bool envelopeBucketOk(uint32_t bucket) { return bucket >= 32 && bucket <= 2048 && (bucket & (bucket - 1)) == 0; }
// records per frame and channel: ceil(stride / bucket); 0 for a bucket outside the set
inline uint32_t envelopeSlots(uint32_t stride, uint32_t bucket) { return envelopeBucketOk(bucket) ? (uint32_t)(((uint64_t)stride + bucket - 1) / bucket) : 0u; }

// What the verb says when it refuses: a bucket outside the set (the set named), a file of wider samples (the file named).
inline std::string envelopeBucketRefusal(long long bucket)
{
    return "Envelope: --bucket " + std::to_string(bucket) + " is not one of " + kEnvelopeBucketSet;
}
inline std::string envelopeBitsRefusal(const std::string& path, uint32_t bits)
{
    return "Envelope: " + path + " holds " + std::to_string(bits) + "-bit samples: the envelope is taken of 16-bit streams only";
}

// A track's envelope: records [ceil(samples / bucket)][channels] on the track's absolute grid.
struct EnvelopeReport {
    uint32_t channels = 0, bucket = 0, sampleRate = 0;
    uint64_t samplesPerChannel = 0;
    std::vector<EnvelopeRecord> records;
    uint64_t buckets() const { return bucket ? (samplesPerChannel + bucket - 1) / bucket : 0; }
};

// records: [frames][slots][channels] as the device call leaves them, sampleOffsets: [frames + 1] -> the report's records: every
// frame's first ceil(n_f / bucket) slots back to back, the empty slots behind a frame's end dropped.  Every frame but the last
// must hold a multiple of `bucket` samples, and no frame more than its slots (std::invalid_argument): frames of 2048 samples and
// a whole-track stream's long last frame do.
inline std::vector<EnvelopeRecord> compactEnvelope(const EnvelopeRecord* records, const uint64_t* sampleOffsets, size_t frames, uint32_t slots, uint32_t channels,
    uint32_t bucket)
{
    if (!envelopeBucketOk(bucket))
        throw std::invalid_argument(envelopeBucketRefusal(bucket));
    std::vector<EnvelopeRecord> out;
    for (size_t f = 0; f < frames; f++) {
        const uint64_t n = sampleOffsets[f + 1] - sampleOffsets[f];
        if (f + 1 < frames && n % bucket)
            throw std::invalid_argument("Envelope: frame " + std::to_string(f) + " holds " + std::to_string(n) + " samples, not a multiple of the bucket");
        const uint64_t used = (n + bucket - 1) / bucket;
        if (used > slots)
            throw std::invalid_argument("Envelope: frame " + std::to_string(f) + " holds " + std::to_string(n) + " samples, more than its slots");
        const EnvelopeRecord* const first = records + f * slots * channels;
        out.insert(out.end(), first, first + used * channels);
    }
    return out;
}

// The .env file: 32 bytes of header, little-endian -- "SELAENV1", uint32 channels, uint32 bucket, uint64 samples per channel,
// uint32 sample rate, uint32 16 (the bits of the samples measured) -- then the records [bucket][channel], 16 bytes each as above.
constexpr size_t kEnvelopeHeaderBytes = 32;
inline void putEnvelopeLe(uint8_t* at, uint64_t v, int bytes)
{
    for (int i = 0; i < bytes; i++)
        at[i] = (uint8_t)(v >> (8 * i));
}
inline std::vector<uint8_t> envelopeFileBytes(const EnvelopeReport& r)
{
    if ((uint64_t)r.records.size() != r.buckets() * r.channels)
        throw std::invalid_argument("Envelope: the report holds " + std::to_string(r.records.size()) + " records, its header says "
            + std::to_string(r.buckets() * r.channels));
    std::vector<uint8_t> out(kEnvelopeHeaderBytes + r.records.size() * sizeof(EnvelopeRecord));
    std::memcpy(out.data(), "SELAENV1", 8);
    putEnvelopeLe(out.data() + 8, r.channels, 4);
    putEnvelopeLe(out.data() + 12, r.bucket, 4);
    putEnvelopeLe(out.data() + 16, r.samplesPerChannel, 8);
    putEnvelopeLe(out.data() + 24, r.sampleRate, 4);
    putEnvelopeLe(out.data() + 28, 16, 4);
    uint8_t* at = out.data() + kEnvelopeHeaderBytes;
    for (const EnvelopeRecord& e : r.records) {
        putEnvelopeLe(at, (uint16_t)e.min, 2);
        putEnvelopeLe(at + 2, (uint16_t)e.max, 2);
        putEnvelopeLe(at + 4, (uint32_t)e.sum, 4);
        putEnvelopeLe(at + 8, e.sumSquares, 8);
        at += sizeof(EnvelopeRecord);
    }
    return out;
}

// ---- 24- and 32-bit streams (struct sela_hip_envelope32) -------------------------------------------------------------
// One (frame, bucket, channel) as the device writes it: the layout of struct sela_hip_envelope32.
struct EnvelopeRecord32 {
    int32_t min, max;      // the smallest and the largest sample of the bucket
    int64_t sum;           // sum of v
    uint64_t sumSquaresLo; // sum of v * v, bits 0 .. 63
    uint64_t sumSquaresHi; // ... and bits 64 .. 127
};
static_assert(sizeof(EnvelopeRecord32) == 32, "struct sela_hip_envelope32");

// A wide track's envelope: records [ceil(samples / bucket)][channels] on the track's absolute grid; bitsPerSample 24 or 32.
struct EnvelopeReport32 {
    uint32_t channels = 0, bucket = 0, sampleRate = 0, bitsPerSample = 0;
    uint64_t samplesPerChannel = 0;
    std::vector<EnvelopeRecord32> records;
    uint64_t buckets() const { return bucket ? (samplesPerChannel + bucket - 1) / bucket : 0; }
};

// compactEnvelope for the wide record: the same grid, the same two refusals.
inline std::vector<EnvelopeRecord32> compactEnvelope32(const EnvelopeRecord32* records, const uint64_t* sampleOffsets, size_t frames, uint32_t slots, uint32_t channels,
    uint32_t bucket)
{
    if (!envelopeBucketOk(bucket))
        throw std::invalid_argument(envelopeBucketRefusal(bucket));
    std::vector<EnvelopeRecord32> out;
    for (size_t f = 0; f < frames; f++) {
        const uint64_t n = sampleOffsets[f + 1] - sampleOffsets[f];
        if (f + 1 < frames && n % bucket)
            throw std::invalid_argument("Envelope: frame " + std::to_string(f) + " holds " + std::to_string(n) + " samples, not a multiple of the bucket");
        const uint64_t used = (n + bucket - 1) / bucket;
        if (used > slots)
            throw std::invalid_argument("Envelope: frame " + std::to_string(f) + " holds " + std::to_string(n) + " samples, more than its slots");
        const EnvelopeRecord32* const first = records + f * slots * channels;
        out.insert(out.end(), first, first + used * channels);
    }
    return out;
}

// The wide .env file: the same 32 bytes of header with the file's bits (24 or 32) for its last word -- a reader tells the two
// record sizes apart by that word -- then the records [bucket][channel], 32 bytes each as above, little-endian.
inline std::vector<uint8_t> envelopeFileBytes32(const EnvelopeReport32& r)
{
    if (r.bitsPerSample != 24 && r.bitsPerSample != 32)
        throw std::invalid_argument("Envelope: a wide report holds 24- or 32-bit samples, not " + std::to_string(r.bitsPerSample) + "-bit ones");
    if ((uint64_t)r.records.size() != r.buckets() * r.channels)
        throw std::invalid_argument("Envelope: the report holds " + std::to_string(r.records.size()) + " records, its header says "
            + std::to_string(r.buckets() * r.channels));
    std::vector<uint8_t> out(kEnvelopeHeaderBytes + r.records.size() * sizeof(EnvelopeRecord32));
    std::memcpy(out.data(), "SELAENV1", 8);
    putEnvelopeLe(out.data() + 8, r.channels, 4);
    putEnvelopeLe(out.data() + 12, r.bucket, 4);
    putEnvelopeLe(out.data() + 16, r.samplesPerChannel, 8);
    putEnvelopeLe(out.data() + 24, r.sampleRate, 4);
    putEnvelopeLe(out.data() + 28, r.bitsPerSample, 4);
    uint8_t* at = out.data() + kEnvelopeHeaderBytes;
    for (const EnvelopeRecord32& e : r.records) {
        putEnvelopeLe(at, (uint32_t)e.min, 4);
        putEnvelopeLe(at + 4, (uint32_t)e.max, 4);
        putEnvelopeLe(at + 8, (uint64_t)e.sum, 8);
        putEnvelopeLe(at + 16, e.sumSquaresLo, 8);
        putEnvelopeLe(at + 24, e.sumSquaresHi, 8);
        at += sizeof(EnvelopeRecord32);
    }
    return out;
}

} // namespace sela
#endif
