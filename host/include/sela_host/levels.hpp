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
#include <type_traits>
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

// ---- 24- and 32-bit streams (sela_hip_level32) ---------------------------------------------------------------------
// One (frame, channel) as the device writes it: the layout of sela_hip_level32.
struct LevelRecord32 {
    uint32_t peak;         // max |v|: 0 .. 2^31
    uint32_t samples;      // samples of the channel in the frame
    int64_t sum;           // sum of v
    uint64_t sumSquaresLo; // sum of v * v, bits 0 .. 63
    uint64_t sumSquaresHi; // sum of v * v, bits 64 .. 127
};
static_assert(sizeof(LevelRecord32) == 32, "sela_hip_level32");

// A channel over any number of frames, the energy in 128 bits: a full-scale frame of 65535 samples is below 2^78, so 2^50 of them fit.
struct ChannelLevelWide {
    uint32_t peak = 0;
    uint64_t samples = 0;
    int64_t sum = 0;
    uint64_t sumSquaresLo = 0, sumSquaresHi = 0;
};

inline void addEnergy(ChannelLevelWide& into, uint64_t lo, uint64_t hi)
{
    into.sumSquaresLo += lo;
    into.sumSquaresHi += hi + (into.sumSquaresLo < lo ? 1u : 0u);
}
inline void fold(ChannelLevelWide& into, const LevelRecord32& r)
{
    into.peak = r.peak > into.peak ? r.peak : into.peak;
    into.samples += r.samples;
    into.sum += r.sum;
    addEnergy(into, r.sumSquaresLo, r.sumSquaresHi);
}
inline void fold(ChannelLevelWide& into, const ChannelLevelWide& r)
{
    into.peak = r.peak > into.peak ? r.peak : into.peak;
    into.samples += r.samples;
    into.sum += r.sum;
    addEnergy(into, r.sumSquaresLo, r.sumSquaresHi);
}

// records: [frames][channels] -> one ChannelLevelWide per channel.  (Deduced from the pointer's type, so that a literal nullptr
// with no frames still means the 16-bit overload above, as it always has.)
template <typename Record, typename = typename std::enable_if<std::is_same<Record, LevelRecord32>::value>::type>
inline std::vector<ChannelLevelWide> foldChannels(const Record* records, size_t frames, uint32_t channels)
{
    std::vector<ChannelLevelWide> out(channels);
    for (size_t f = 0; f < frames; f++)
        for (uint32_t c = 0; c < channels; c++)
            fold(out[c], records[f * channels + c]);
    return out;
}

// 2^(bits - 1): |the most negative sample| of a `bits`-bit stream, 0 dBFS
inline double fullScale(uint32_t bits) { return std::ldexp(1.0, (int)bits - 1); }
// the energy as a double (rounded once per word: good for a figure in dB, not for arithmetic)
inline double energyOf(const ChannelLevelWide& l) { return std::ldexp((double)l.sumSquaresHi, 64) + (double)l.sumSquaresLo; }

// The figures above against a full scale of the caller's: 20 log10(peak / fullScale), 10 log10(energy / samples / fullScale^2), the mean.
inline double peakDbfs(const ChannelLevelWide& l, double fullScale)
{
    return l.peak ? 20.0 * std::log10((double)l.peak / fullScale) : -std::numeric_limits<double>::infinity();
}
inline double rmsDbfs(const ChannelLevelWide& l, double fullScale)
{
    if (!l.samples || !(l.sumSquaresLo | l.sumSquaresHi))
        return -std::numeric_limits<double>::infinity();
    return 10.0 * std::log10(energyOf(l) / (double)l.samples / (fullScale * fullScale));
}
inline double dcOffset(const ChannelLevelWide& l) { return l.samples ? (double)l.sum / (double)l.samples : 0.0; }

// hi * 2^64 + lo in decimal, exactly: long division of four 32-bit digits by 10^9, nine decimal digits a pass
inline std::string energyDecimal(uint64_t lo, uint64_t hi)
{
    uint32_t digits[4] = { (uint32_t)(hi >> 32), (uint32_t)hi, (uint32_t)(lo >> 32), (uint32_t)lo };
    std::string out;
    for (;;) {
        uint64_t rem = 0;
        for (int i = 0; i < 4; i++) {
            const uint64_t cur = (rem << 32) | digits[i]; // (rem < 10^9 < 2^30)
            digits[i] = (uint32_t)(cur / 1000000000u);
            rem = cur % 1000000000u;
        }
        const bool last = !(digits[0] | digits[1] | digits[2] | digits[3]);
        std::string part = std::to_string(rem);
        if (!last)
            part.insert(0, 9 - part.size(), '0');
        out.insert(0, part);
        if (last)
            return out;
    }
}
inline std::string energyDecimal(const ChannelLevelWide& l) { return energyDecimal(l.sumSquaresLo, l.sumSquaresHi); }

} // namespace sela
#endif
