// level_report.cpp -- host/include/sela_host/levels.hpp alone (no GPU, no library): the fold over level records and the figures
// read from it, under -fsanitize=address,undefined.  The expectations are computed here, from the definitions.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <vector>

#include "sela_host/levels.hpp"

static int failures = 0;
#define CHECK(x)                                                         \
    do {                                                                 \
        if (!(x)) {                                                      \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);   \
            failures++;                                                  \
        }                                                                \
    } while (0)

static bool close_to(double got, double want) { return std::fabs(got - want) <= 1e-9 * std::fmax(1.0, std::fabs(want)); }

int main()
{
    using namespace sela;
    // a single sample
    {
        const LevelRecord one = { 16384, 1, -16384, (uint64_t)16384 * 16384 };
        const std::vector<ChannelLevel> l = foldChannels(&one, 1, 1);
        CHECK(l.size() == 1 && l[0].peak == 16384 && l[0].samples == 1 && l[0].sum == -16384 && l[0].sumSquares == (uint64_t)1 << 28);
        CHECK(close_to(peakDbfs(l[0]), 20.0 * std::log10(0.5)));  // -6.0206 dBFS
        CHECK(close_to(rmsDbfs(l[0]), 20.0 * std::log10(0.5)));   // one sample: its RMS is its magnitude
        CHECK(close_to(dcOffset(l[0]), -16384.0));
    }
    // silence, and no samples at all
    {
        const LevelRecord silent[2] = { { 0, 2048, 0, 0 }, { 0, 777, 0, 0 } };
        const std::vector<ChannelLevel> l = foldChannels(silent, 2, 1);
        CHECK(l[0].peak == 0 && l[0].samples == 2825 && l[0].sum == 0 && l[0].sumSquares == 0);
        CHECK(std::isinf(peakDbfs(l[0])) && peakDbfs(l[0]) < 0 && std::isinf(rmsDbfs(l[0])) && rmsDbfs(l[0]) < 0 && dcOffset(l[0]) == 0.0);
        const ChannelLevel none;
        CHECK(std::isinf(peakDbfs(none)) && std::isinf(rmsDbfs(none)) && dcOffset(none) == 0.0);
        CHECK(foldChannels(nullptr, 0, 3).size() == 3);
    }
    // full scale: peak = 32768 is 0 dBFS; a frame of 65535 samples at -32768, many of them: sumSquares near 2^46 per frame
    {
        const uint32_t frames = 1 << 17; // 2^17 frames of 2^46 - 2^30 each: below 2^63
        const LevelRecord full = { 32768, 65535, -(int64_t)65535 * 32768, (uint64_t)65535 << 30 };
        std::vector<LevelRecord> records((size_t)frames * 2);
        for (uint32_t f = 0; f < frames; f++) {
            records[(size_t)f * 2] = full;
            records[(size_t)f * 2 + 1] = { f == 5 ? 32767u : 1u, 65535, 65535, 65535 }; // channel 1: every sample 1, one frame's peak planted
        }
        const std::vector<ChannelLevel> l = foldChannels(records.data(), frames, 2);
        CHECK(l[0].peak == 32768 && l[0].samples == (uint64_t)65535 << 17 && l[0].sum == -(((int64_t)65535 * 32768) << 17));
        CHECK(l[0].sumSquares == ((uint64_t)65535 << 47) && l[0].sumSquares > ((uint64_t)1 << 62));
        CHECK(peakDbfs(l[0]) == 0.0 && close_to(rmsDbfs(l[0]), 0.0) && close_to(dcOffset(l[0]), -32768.0));
        CHECK(l[1].peak == 32767 && l[1].sum == (int64_t)65535 << 17 && l[1].sumSquares == (uint64_t)65535 << 17);
        CHECK(close_to(peakDbfs(l[1]), 20.0 * std::log10(32767.0 / 32768.0)));
        CHECK(close_to(rmsDbfs(l[1]), 10.0 * std::log10(1.0 / (32768.0 * 32768.0)))); // -90.309 dBFS
        CHECK(close_to(dcOffset(l[1]), 1.0));
        // the track: both channels into one
        ChannelLevel track;
        fold(track, l[0]);
        fold(track, l[1]);
        CHECK(track.peak == 32768 && track.samples == (uint64_t)65535 << 18 && track.sum == l[0].sum + l[1].sum && track.sumSquares == l[0].sumSquares + l[1].sumSquares);
        CHECK(close_to(rmsDbfs(track), 10.0 * std::log10((double)track.sumSquares / (double)track.samples / (32768.0 * 32768.0))));
    }
    // a square wave at +-8192 with a DC offset of 100: the figures by the definitions
    {
        LevelRecord r = { 0, 2048, 0, 0 };
        for (int i = 0; i < 2048; i++) {
            const int64_t v = (i & 1 ? -8192 : 8192) + 100;
            r.peak = (uint32_t)std::llabs(v) > r.peak ? (uint32_t)std::llabs(v) : r.peak;
            r.sum += v;
            r.sumSquares += (uint64_t)(v * v);
        }
        const ChannelLevel l = foldChannels(&r, 1, 1)[0];
        CHECK(l.peak == 8292 && l.sum == 204800 && l.sumSquares == (uint64_t)2048 * (8192 * 8192 + 100 * 100));
        CHECK(close_to(dcOffset(l), 100.0));
        CHECK(close_to(peakDbfs(l), 20.0 * std::log10(8292.0 / 32768.0)));
        CHECK(close_to(rmsDbfs(l), 10.0 * std::log10((8192.0 * 8192.0 + 100.0 * 100.0) / (32768.0 * 32768.0))));
    }
    std::printf("level_report: %d failures\n", failures);
    return failures ? 1 : 0;
}
