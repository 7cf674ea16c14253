// tail32_store_plan.cpp -- the packed 3-byte store of k_tail32_store (sela_amd/csrc/sela_window32_whole.hip) replayed
// on the CPU from the arithmetic it is compiled from: the window's share of the long last frame (window_tail_share,
// sela_window_tail.h) and the bytes each round of 256 samples owns (pcm24_span, sela_pcm24_edges.h).  The output buffer of a batch
// of windows is exact-size (AddressSanitizer sees a byte beyond it); every round's head bytes, aligned dwords and tail bytes are
// counted.  For every shape: every byte of a window's share of L is written exactly once, no byte outside it, every dword is
// aligned, and bytes go out singly only at a share's two ends.  The descriptors come through the host plan for tailed tables
// (plan_windows_whole, sela_window_plan.h), as sela_hip_decode_windows_i32_whole stages them: the share is found on the staged
// table the way k_tailwin_plan finds it, and must be the caller's.  Built with -fsanitize=address,undefined by
// tests/test_whole_pcm_cpu.py.  Prints "<cases> cases, <n> failures".
#include <cstdint>
#include <cstdio>
#include <vector>

#include "sela_pcm24_edges.h"
#include "sela_window_plan.h"

using namespace sela;

namespace {

constexpr uint32_t kRound = 256; // kTail32Threads

int failures = 0, cases = 0;

struct Table {
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> offsets;
};

// every frame a sync word and one subframe header that says a length
Table make_table(const std::vector<uint32_t>& lengths)
{
    Table t;
    t.offsets.push_back(0);
    for (uint32_t n : lengths) {
        const uint8_t f[16] = { 0x00, 0xFF, 0x55, 0xAA, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, (uint8_t)(n & 0xFF), (uint8_t)(n >> 8) };
        t.bytes.insert(t.bytes.end(), f, f + 16);
        t.offsets.push_back(t.bytes.size());
    }
    return t;
}

// k_tailwin_plan on one descriptor
WindowTail plan_tail(const Table& t, uint32_t n_frames_total, const sela_hip_window& d, uint32_t window_samples)
{
    WindowTail tl = {};
    const uint32_t n = window_stream_frames(d, n_frames_total);
    if (n != 0) {
        const uint32_t last = d.first_frame + n - 1, n_last = frame_says_samples(t.bytes.data(), t.offsets.data(), last);
        if (tail_length(n_last)) {
            tl = window_tail_share(d.start, window_samples, n, n_last);
            tl.frame = last;
        }
    }
    return tl;
}

// the store's rounds for window w: counts every byte it writes
void store_share(uint32_t w, const WindowTail& tl, uint32_t window_samples, uint32_t channels, std::vector<uint8_t>& written, bool& ok)
{
    if (tl.lo >= tl.hi)
        return;
    const uint32_t n_share = tl.hi - tl.lo;
    uint32_t singles = 0;
    for (uint32_t base = 0; base < n_share; base += kRound) {
        const uint32_t here = n_share - base < kRound ? n_share - base : kRound, m = here * channels;
        const uint64_t v0 = ((uint64_t)w * window_samples + tl.lo + base) * channels, b0 = 3 * v0, lead_at = b0 - 3;
        const bool first = base == 0, last = base + kRound >= n_share;
        const Pcm24Span sp = pcm24_span(b0, b0 + 3ull * m, first, last);
        ok = ok && sp.head <= 3 && sp.tail <= 3 && sp.mid_at % 4 == 0 && (sp.head == 0 || first) && (sp.tail == 0 || last);
        singles += sp.head + sp.tail;
        auto slot_ok = [&](uint64_t at, uint32_t bytes) { // the table holds the lead (later rounds only) and the round's m values
            const uint32_t lo = pcm24_slot_of((uint32_t)(at - lead_at)), hi = pcm24_slot_of((uint32_t)(at + bytes - 1 - lead_at));
            return hi <= m && (lo >= 1 || !first);
        };
        for (uint32_t k = 0; k < sp.head; k++)
            ok = ok && slot_ok(sp.head_at + k, 1), written.at(sp.head_at + k)++;
        for (uint64_t e = 0; e < sp.dwords; e++)
            for (uint32_t k = 0; k < 4; k++)
                ok = ok && slot_ok(sp.mid_at + 4 * e, 4), written.at(sp.mid_at + 4 * e + k)++;
        for (uint32_t k = 0; k < sp.tail; k++)
            ok = ok && slot_ok(sp.tail_at + k, 1), written.at(sp.tail_at + k)++;
    }
    ok = ok && singles <= 6;
}

// A batch on the caller's table, through the plan: the staged descriptors' shares are the caller's, and the stores cover them.
void check(const Table& t, const std::vector<sela_hip_window>& windows, uint32_t window_samples, uint32_t channels)
{
    cases++;
    const uint32_t total = (uint32_t)t.offsets.size() - 1, n_windows = (uint32_t)windows.size();
    WindowPlan plan;
    plan_windows_whole(t.bytes.data(), t.offsets.data(), total, windows.data(), n_windows, window_samples, &plan);
    Table staged;
    staged.offsets = plan.offsets;
    for (uint32_t f : plan.frames)
        staged.bytes.insert(staged.bytes.end(), t.bytes.begin() + (size_t)t.offsets[f], t.bytes.begin() + (size_t)t.offsets[f + 1]);
    staged.bytes.resize(staged.bytes.size() + 8); // (the staging buffer's slack: nothing reads it)
    bool ok = plan.windows.size() == windows.size();
    std::vector<uint8_t> written((size_t)n_windows * window_samples * channels * 3, 0); // exact size
    std::vector<uint8_t> want(written.size(), 0);
    for (uint32_t w = 0; ok && w < n_windows; w++) {
        const WindowTail mine = plan_tail(t, total, windows[w], window_samples);
        const WindowTail theirs = plan_tail(staged, (uint32_t)plan.frames.size(), plan.windows[w], window_samples);
        const bool share = mine.lo < mine.hi;
        ok = share == (theirs.lo < theirs.hi) && (!share || (mine.lo == theirs.lo && mine.hi == theirs.hi && mine.s0 == theirs.s0 && mine.n == theirs.n
                                                                && plan.frames[theirs.frame] == mine.frame));
        ok = ok && (!share || (mine.hi <= window_samples && mine.s0 + (mine.hi - mine.lo) <= mine.n && mine.n <= kTailMaxSamples));
        if (!ok)
            break;
        store_share(w, theirs, window_samples, channels, written, ok);
        if (share)
            for (uint64_t at = ((uint64_t)w * window_samples + mine.lo) * channels * 3; at < ((uint64_t)w * window_samples + mine.hi) * channels * 3; at++)
                want[at] = 1;
    }
    ok = ok && written == want; // every byte of a share once, no byte outside
    if (!ok) {
        failures++;
        std::printf("FAIL: %u frames, %u windows of %u samples, %u channels (first: start %llu, frames %u + %u)\n", total, n_windows, window_samples, channels,
            windows.empty() ? 0ull : (unsigned long long)windows[0].start, windows.empty() ? 0u : windows[0].first_frame, windows.empty() ? 0u : windows[0].n_frames);
    }
}

} // namespace

int main()
{
    const uint32_t tails[] = { 1, 2, 3, 255, 256, 257, 300, 2047, 2049, 2048 + 255, 2048 + 256, 2048 + 257, 4095 };
    const uint32_t sizes[] = { 1, 2, 3, 5, 255, 256, 257, 777, 4097 };
    for (uint32_t channels = 1; channels <= 8; channels++)
        for (uint32_t n_last : tails) {
            const Table t = make_table({ 2048, n_last, n_last, 2048, 4096, n_last }); // a tailed stream (0, 1), a tail alone (2), a plain stream (3, 4), a table cut (5)
            for (uint32_t ws : sizes) {
                std::vector<sela_hip_window> windows;
                // every byte phase of the share's start and end: consecutive windows of an odd length shift by three bytes a channel
                for (uint64_t back : std::vector<uint64_t>{ 0, 1, 2, 3, 5, (uint64_t)ws - 1, ws, (uint64_t)ws + 1 })
                    windows.push_back({ 2048 >= back ? 2048 - back : 0, 0, 2 });
                for (uint64_t in : std::vector<uint64_t>{ 0, 1, 2, 3, 254, 255, 256, 257 })
                    windows.push_back({ 2048 + (in < n_last ? in : n_last - 1), 0, 2 });
                for (uint64_t left : std::vector<uint64_t>{ 1, 2, 3, 4, 5 })
                    windows.push_back({ 2048 + n_last - (left < n_last ? left : n_last), 0, 2 });
                windows.push_back({ 2048ull + n_last, 0, 2 });
                windows.push_back({ ~0ull, 0, 2 });
                windows.push_back({ 0, 2, 1 });
                windows.push_back({ n_last - 1, 2, 1 });
                windows.push_back({ 5, 3, 2 });
                windows.push_back({ 2048 + 7, 4, 100 });
                windows.push_back({ 3, 5, 0xFFFFFFFFu });
                windows.push_back({ 0, 6, 1 });
                check(t, windows, ws, channels);
            }
        }
    std::printf("%d cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
