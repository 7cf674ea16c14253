// window_compact.cpp -- the plan of sela_hip_decode_windows (sela_amd/csrc/sela_window_plan.h) on the CPU, for the sanitizers:
// which frames a batch of windows touches, where they lie when staged back to back, every descriptor on the compacted table.
// The plan is held against a model that needs no plan: a table whose frame f "decodes" to the samples (f, 0), (f, 1), ... of a
// stream is cut by the caller's windows and by the remapped windows on the compacted table; both cuts must name the same
// (original frame, sample) at every output position, or zero.  Seeded random batches and the edges (starts at and beyond every
// boundary, 2^64 - 1, streams past the table, empty tables).  Prints "<cases> cases, <n> failures".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sela_window_plan.h"

namespace {

uint64_t g_seed = 0x9E3779B97F4A7C15ull;
uint64_t rnd()
{
    g_seed ^= g_seed << 13, g_seed ^= g_seed >> 7, g_seed ^= g_seed << 17;
    return g_seed;
}

constexpr uint64_t kNone = ~0ull;

// what output sample i of window w names: table frame * 2048 + sample, or kNone (zero)
uint64_t cut(const sela_hip_window& w, uint32_t n_frames_total, uint32_t i)
{
    const uint64_t in_stream = w.first_frame < n_frames_total ? (w.n_frames < n_frames_total - w.first_frame ? w.n_frames : n_frames_total - w.first_frame) : 0;
    const uint64_t q = w.start / 2048, r = w.start % 2048;
    if (q >= in_stream)
        return kNone;
    const uint64_t frame = q + (r + i) / 2048;
    if (frame >= in_stream)
        return kNone;
    return (w.first_frame + frame) * 2048 + (r + i) % 2048;
}

int check(const std::vector<uint64_t>& offsets, const std::vector<sela_hip_window>& windows, uint32_t window_samples)
{
    const uint32_t n_frames_total = (uint32_t)offsets.size() - 1;
    sela::WindowPlan plan;
    sela::plan_windows(offsets.data(), n_frames_total, windows.data(), (uint32_t)windows.size(), window_samples, &plan);
    int failures = 0;
    if (plan.offsets.size() != plan.frames.size() + 1 || plan.windows.size() != windows.size())
        return 1;
    uint64_t bytes = 0;
    for (size_t k = 0; k < plan.frames.size(); k++) {
        const uint32_t f = plan.frames[k];
        failures += f >= n_frames_total || (k && f <= plan.frames[k - 1]); // ascending, distinct, in the table
        if (f >= n_frames_total)
            return failures;
        failures += plan.offsets[k] != bytes || plan.offsets[k + 1] - plan.offsets[k] != offsets[f + 1] - offsets[f];
        bytes += offsets[f + 1] - offsets[f];
    }
    failures += plan.staged_bytes() != bytes;
    std::vector<uint8_t> used(plan.frames.size(), 0);
    for (size_t w = 0; w < windows.size(); w++) {
        // every sample at the ends and around every frame boundary of the window, and a few in between
        std::vector<uint32_t> at = { 0, window_samples - 1, window_samples / 2 };
        for (uint32_t b = 0; b <= (window_samples + 2047) / 2048; b++)
            for (int d = -1; d <= 1; d++) {
                const int64_t i = (int64_t)b * 2048 - (int64_t)(windows[w].start % 2048) + d;
                if (i >= 0 && i < (int64_t)window_samples)
                    at.push_back((uint32_t)i);
            }
        for (uint32_t i : at) {
            const uint64_t want = cut(windows[w], n_frames_total, i);
            uint64_t got = cut(plan.windows[w], (uint32_t)plan.frames.size(), i);
            if (got != kNone) {
                used[got / 2048] = 1;
                got = (uint64_t)plan.frames[got / 2048] * 2048 + got % 2048; // the compacted frame is that frame of the table
            }
            failures += got != want;
        }
    }
    for (size_t k = 0; k < used.size(); k++)
        failures += !used[k]; // nothing is staged that no window touches (the boundary samples above visit every covering frame)
    return failures;
}

} // namespace

int main()
{
    int cases = 0, failures = 0;
    const uint32_t lengths[] = { 1, 2, 777, 2047, 2048, 2049, 2050, 3 * 2048, 16000, 1u << 24 };
    for (uint32_t n_frames_total : { 0u, 1u, 5u, 40u, 300u }) {
        std::vector<uint64_t> offsets(n_frames_total + 1, 0);
        for (uint32_t f = 0; f < n_frames_total; f++)
            offsets[f + 1] = offsets[f] + 4 * (rnd() % 1500); // (sizes of 0 among them)
        for (uint32_t window_samples : lengths) {
            std::vector<sela_hip_window> edges;
            for (uint64_t start : { 0ull, 1ull, 2047ull, 2048ull, 2049ull, 5 * 2048ull - 1, 5 * 2048ull, 40 * 2048ull - 1, ~0ull, ~0ull - 2047, 1ull << 43 })
                for (uint32_t first : { 0u, 2u, n_frames_total, 0xFFFFFFFFu })
                    for (uint32_t n : { 0u, 1u, 2u, 3u, n_frames_total, 0xFFFFFFFFu })
                        edges.push_back({ start, first, n });
            failures += check(offsets, edges, window_samples), cases++;
            for (int round = 0; round < 20; round++) {
                std::vector<sela_hip_window> batch(1 + rnd() % 64);
                for (sela_hip_window& w : batch) {
                    w.first_frame = (uint32_t)(rnd() % (n_frames_total + 2));
                    w.n_frames = (uint32_t)(rnd() % (n_frames_total + 3));
                    w.start = rnd() % (2048ull * (w.n_frames + 1) + 1);
                }
                if (round % 4 == 0)
                    batch.push_back(batch[0]); // a duplicate
                failures += check(offsets, batch, window_samples), cases++;
            }
        }
    }
    std::printf("%d cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
