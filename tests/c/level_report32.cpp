// level_report32.cpp -- host/include/sela_host/levels.hpp alone (no GPU, no library): the fold over the level records of 24- and
// 32-bit streams, its 128-bit energy and the decimal printer, and the figures against a full scale of 2^23 and 2^31, under
// -fsanitize=address,undefined.  The expectations are computed here, from the definitions.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <string>
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
    // the decimal printer
    {
        CHECK(energyDecimal(0, 0) == "0");
        CHECK(energyDecimal(7, 0) == "7");
        CHECK(energyDecimal(1000000000ull, 0) == "1000000000");
        CHECK(energyDecimal(~(uint64_t)0, 0) == "18446744073709551615");               // 2^64 - 1
        CHECK(energyDecimal(0, 1) == "18446744073709551616");                          // 2^64
        CHECK(energyDecimal((uint64_t)65535 << 62, 65535 >> 2) == "302226843217638866288640"); // 65535 * 2^62 = 2^78 - 2^62
        CHECK(energyDecimal(~(uint64_t)0, ~(uint64_t)0) == "340282366920938463463374607431768211455"); // 2^128 - 1
    }
    // the fold carries past 2^64: four full-scale samples are 2^64 already
    {
        const LevelRecord32 four = { 0x80000000u, 4, -((int64_t)4 << 31), 0, 1 };
        std::vector<LevelRecord32> records(3, four);
        records[1] = { 5, 1, 5, ~(uint64_t)0, 0 };
        records[2] = { 1, 1, -1, 1, 0 };
        const std::vector<ChannelLevelWide> l = foldChannels(records.data(), 3, 1);
        CHECK(l.size() == 1 && l[0].peak == 0x80000000u && l[0].samples == 6 && l[0].sum == -((int64_t)4 << 31) + 4);
        CHECK(l[0].sumSquaresLo == 0 && l[0].sumSquaresHi == 2); // 2^64 + (2^64 - 1) + 1
        CHECK(energyDecimal(l[0]) == "36893488147419103232");
        // a full-scale frame of 65535 samples, many of them
        const LevelRecord32 full = { 0x80000000u, 65535, -((int64_t)65535 << 31), (uint64_t)65535 << 62, 65535 >> 2 };
        ChannelLevelWide track;
        for (int f = 0; f < 1024; f++)
            fold(track, full);
        CHECK(track.peak == 0x80000000u && track.samples == (uint64_t)65535 << 10 && track.sum == -((int64_t)65535 << 41));
        CHECK(track.sumSquaresLo == 0 && track.sumSquaresHi == (uint64_t)65535 << 8); // 65535 * 2^72
        CHECK(peakDbfs(track, fullScale(32)) == 0.0 && close_to(rmsDbfs(track, fullScale(32)), 0.0) && close_to(dcOffset(track), -2147483648.0));
        ChannelLevelWide both;
        fold(both, track);
        fold(both, l[0]);
        CHECK(both.samples == track.samples + 6 && both.sumSquaresHi == track.sumSquaresHi + 2 && both.sum == track.sum + l[0].sum);
        CHECK(foldChannels(static_cast<const LevelRecord32*>(nullptr), 0, 3).size() == 3);
    }
    // dBFS against the stream's own full scale: 0.00 for a full-scale peak, -inf for silence
    {
        CHECK(fullScale(24) == 8388608.0 && fullScale(32) == 2147483648.0 && fullScale(16) == 32768.0);
        ChannelLevelWide top24;
        fold(top24, LevelRecord32{ 1u << 23, 1, -(1 << 23), (uint64_t)1 << 46, 0 });
        CHECK(peakDbfs(top24, fullScale(24)) == 0.0 && close_to(rmsDbfs(top24, fullScale(24)), 0.0));
        CHECK(close_to(peakDbfs(top24, fullScale(32)), 20.0 * std::log10(1.0 / 256.0))); // the same sample in a 32-bit stream: -48.16 dBFS
        ChannelLevelWide top32;
        fold(top32, LevelRecord32{ 0x80000000u, 1, -((int64_t)1 << 31), (uint64_t)1 << 62, 0 });
        CHECK(peakDbfs(top32, fullScale(32)) == 0.0 && close_to(rmsDbfs(top32, fullScale(32)), 0.0));
        char text[64];
        std::snprintf(text, sizeof(text), "%.2f %.2f", peakDbfs(top32, fullScale(32)), peakDbfs(top24, fullScale(24)));
        CHECK(std::string(text) == "0.00 0.00");
        ChannelLevelWide silent;
        fold(silent, LevelRecord32{ 0, 2048, 0, 0, 0 });
        for (double scale : { fullScale(24), fullScale(32) })
            CHECK(std::isinf(peakDbfs(silent, scale)) && peakDbfs(silent, scale) < 0 && std::isinf(rmsDbfs(silent, scale)) && rmsDbfs(silent, scale) < 0 && dcOffset(silent) == 0.0);
        const ChannelLevelWide none;
        CHECK(std::isinf(peakDbfs(none, fullScale(24))) && std::isinf(rmsDbfs(none, fullScale(24))) && dcOffset(none) == 0.0);
        // half scale with a DC offset, by the definitions
        ChannelLevelWide half;
        LevelRecord32 r = { 0, 2048, 0, 0, 0 };
        for (int i = 0; i < 2048; i++) {
            const int64_t v = (i & 1 ? -(1 << 22) : (1 << 22)) + 100;
            r.peak = (uint32_t)std::llabs(v) > r.peak ? (uint32_t)std::llabs(v) : r.peak;
            r.sum += v;
            r.sumSquaresLo += (uint64_t)(v * v);
        }
        fold(half, r);
        CHECK(close_to(dcOffset(half), 100.0) && close_to(peakDbfs(half, fullScale(24)), 20.0 * std::log10(4194404.0 / 8388608.0)));
        CHECK(close_to(rmsDbfs(half, fullScale(24)), 10.0 * std::log10((4194304.0 * 4194304.0 + 100.0 * 100.0) / (8388608.0 * 8388608.0))));
    }
    // the 16-bit names are what they were
    {
        const LevelRecord one = { 16384, 1, -16384, (uint64_t)16384 * 16384 };
        const ChannelLevel l = foldChannels(&one, 1, 1)[0];
        CHECK(close_to(peakDbfs(l), 20.0 * std::log10(0.5)) && close_to(rmsDbfs(l), 20.0 * std::log10(0.5)) && close_to(dcOffset(l), -16384.0));
    }
    std::printf("level_report32: %d failures\n", failures);
    return failures ? 1 : 0;
}
