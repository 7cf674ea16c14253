// digest.hpp -- the host's side of the digest (sela_hip_digest, include/sela_hip.h): a table-driven CRC-32 (IEEE
// 802.3: zlib.crc32, `crc32`, `cksum -a crc32`) for the bytes of a WAV's data chunk, and the report sela::digestFile and
// sela::digestWideFile (sela_hip_digest_pcm) return.  Pure
// arithmetic: no GPU, no file, nothing but the standard library.
#ifndef SELA_HOST_DIGEST_HPP_
#define SELA_HOST_DIGEST_HPP_

#include <array>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>

namespace sela {

// CRC-32 over bytes handed in in pieces: update() as often as there are pieces, value() at any time.
class Crc32 {
public:
    void update(const void* data, size_t bytes)
    {
        static const std::array<uint32_t, 256> table = makeTable();
        const unsigned char* p = static_cast<const unsigned char*>(data);
        uint32_t r = reg_;
        for (size_t i = 0; i < bytes; i++)
            r = (r >> 8) ^ table[(r ^ p[i]) & 0xFFu];
        reg_ = r;
    }
    uint32_t value() const { return reg_ ^ 0xFFFFFFFFu; }

private:
    static std::array<uint32_t, 256> makeTable()
    {
        std::array<uint32_t, 256> t{};
        for (uint32_t b = 0; b < 256; b++) {
            uint32_t r = b;
            for (int k = 0; k < 8; k++)
                r = (r >> 1) ^ ((r & 1u) ? 0xEDB88320u : 0u);
            t[b] = r;
        }
        return t;
    }
    uint32_t reg_ = 0xFFFFFFFFu;
};

// What digestFile found.  The stream's figures are the device's (no PCM reaches the host); the WAV's, where a WAV was named, are
// the host's over the part of its data chunk the .sela can hold: all of it for a whole-track file, its whole 2048-sample frames
// for any other.
struct DigestReport {
    uint32_t channels = 0;
    uint64_t frames = 0;
    uint32_t crc32 = 0;  // of the PCM the stream decodes to
    uint64_t bytes = 0;
    bool haveWav = false;
    uint32_t wavCrc32 = 0;
    uint64_t wavBytes = 0;      // the bytes of the data chunk the figure is taken over
    uint64_t wavTailBytes = 0;  // the bytes of the data chunk behind them
    uint32_t wideSamples = 0;   // digestWideFile of a 24-bit file: samples beyond 24 bits (their low three bytes are digested)
    bool agree() const { return !haveWav || (wavCrc32 == crc32 && wavBytes == bytes); }
};

inline std::string formatDigestReport(const DigestReport& r)
{
    char line[160];
    std::snprintf(line, sizeof(line), "crc32=%08x bytes=%llu frames=%llu\n", r.crc32, (unsigned long long)r.bytes, (unsigned long long)r.frames);
    std::string out = line;
    if (r.haveWav) {
        std::snprintf(line, sizeof(line), "wav: crc32=%08x bytes=%llu", r.wavCrc32, (unsigned long long)r.wavBytes);
        out += line;
        if (r.wavTailBytes)
            out += " (" + std::to_string(r.wavTailBytes) + " bytes behind the last whole frame left out)";
        out += r.agree() ? "\nmatch\n" : "\nMISMATCH\n";
    }
    return out;
}

} // namespace sela
#endif
