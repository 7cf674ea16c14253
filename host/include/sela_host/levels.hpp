// levels.hpp -- what a stream's level records (sela_hip_level, include/sela_hip.h) say about a whole channel:
// the fold over the frames, and the figures a person reads (dBFS peak, dBFS RMS, DC offset).  Pure arithmetic: no GPU, no file,
// nothing but the standard library -- tests/c/level_report.cpp compiles it alone.
#ifndef SELA_HOST_LEVELS_HPP_
#define SELA_HOST_LEVELS_HPP_

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <string>
#include <vector>

namespace sela {

// One (frame, channel) as the device writes it: the layout of sela_hip_level.
struct LevelRecord {
    uint32_t peak;       // max |v|: 0 .. 32768
    uint32_t samples;    // samples of the frame, per channel
    int64_t sum;         // sum of v
    uint64_t sumSquares; // sum of v * v
};
static_assert(sizeof(LevelRecord) == 24, "sela_hip_level");

// A channel over any number of frames.  sumSquares holds 2^18 full-scale frames of 65535 samples (2^46 each) -- about 108 hours
// at 44.1 kHz -- and sum far more; fold() stops at neither, the caller of a longer stream folds in pieces.
struct ChannelLevel {
    uint32_t peak = 0;
    uint64_t samples = 0;
    int64_t sum = 0;
    uint64_t sumSquares = 0;
};

constexpr double kFullScale = 32768.0; // |-32768|: 0 dBFS

inline void fold(ChannelLevel& into, const LevelRecord& r)
{
    into.peak = r.peak > into.peak ? r.peak : into.peak;
    into.samples += r.samples;
    into.sum += r.sum;
    into.sumSquares += r.sumSquares;
}
inline void fold(ChannelLevel& into, const ChannelLevel& r)
{
    into.peak = r.peak > into.peak ? r.peak : into.peak;
    into.samples += r.samples;
    into.sum += r.sum;
    into.sumSquares += r.sumSquares;
}

// records: [frames][channels] -> one ChannelLevel per channel
inline std::vector<ChannelLevel> foldChannels(const LevelRecord* records, size_t frames, uint32_t channels)
{
    std::vector<ChannelLevel> out(channels);
    for (size_t f = 0; f < frames; f++)
        for (uint32_t c = 0; c < channels; c++)
            fold(out[c], records[f * channels + c]);
    return out;
}

// 20 log10(peak / 32768); -inf for silence (and for no samples)
inline double peakDbfs(const ChannelLevel& l)
{
    return l.peak ? 20.0 * std::log10((double)l.peak / kFullScale) : -std::numeric_limits<double>::infinity();
}
// 10 log10(sumSquares / samples / 32768^2); -inf for silence (and for no samples)
inline double rmsDbfs(const ChannelLevel& l)
{
    if (!l.samples || !l.sumSquares)
        return -std::numeric_limits<double>::infinity();
    return 10.0 * std::log10((double)l.sumSquares / (double)l.samples / (kFullScale * kFullScale));
}
// the mean sample value, in sample units; 0 for no samples
inline double dcOffset(const ChannelLevel& l) { return l.samples ? (double)l.sum / (double)l.samples : 0.0; }

} // namespace sela
#endif
