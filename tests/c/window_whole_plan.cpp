// window_whole_plan.cpp -- the plan of sela_hip_decode_windows_whole (plan_windows_whole, sela_amd/csrc/sela_window_plan.h) on the
// CPU, for the sanitizers.  The table is real bytes: every frame a sync word and one subframe header that says a length (or
// eight bytes, too short to hold one).  The model needs no plan: output sample i of a window names (table frame, sample, decoded
// as a long last frame or as one of 2048) by the call's contract -- the stream's last frame inside the table is a long one when it
// says 1 .. 4095 and not 2048 -- or nothing.  The caller's windows on the caller's table and the planned windows on the staged
// table must name the same thing at every position; and the staged frames of hand-made batches are listed outright.
// Prints "<cases> cases, <n> failures".
#include <cstdint>
#include <cstdio>
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
constexpr uint32_t kHeaderless = 0xFFFFFFFFu; // a frame of eight bytes

struct Table {
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> offsets;
    std::vector<uint32_t> says;
};

Table make_table(const std::vector<uint32_t>& lengths)
{
    Table t;
    t.offsets.push_back(0);
    for (uint32_t n : lengths) {
        const uint8_t sync[4] = { 0x00, 0xFF, 0x55, 0xAA };
        t.bytes.insert(t.bytes.end(), sync, sync + 4);
        if (n == kHeaderless) {
            const uint8_t four[4] = { 0, 0, 0, 0 };
            t.bytes.insert(t.bytes.end(), four, four + 4);
            t.says.push_back(0);
        } else { // channel, type, parent, ck, cw = 0 (u16), order | rk, rw = 0 (u16), n (u16)
            const uint8_t h[12] = { 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, (uint8_t)(n & 0xFF), (uint8_t)(n >> 8) };
            t.bytes.insert(t.bytes.end(), h, h + 12);
            t.says.push_back(n);
        }
        t.offsets.push_back(t.bytes.size());
    }
    return t;
}

bool tail(uint32_t n) { return n >= 1 && n <= 4095 && n != 2048; }

// what output sample i of window w names on a table whose frames say `says`: (frame * 8192 + sample) * 2 + as_tail, or kNone
uint64_t cut(const sela_hip_window& w, const std::vector<uint32_t>& says, uint32_t i)
{
    const uint32_t total = (uint32_t)says.size();
    const uint64_t n = w.first_frame < total ? (w.n_frames < total - w.first_frame ? w.n_frames : total - w.first_frame) : 0;
    if (n == 0)
        return kNone;
    const uint64_t last = w.first_frame + n - 1;
    const bool tailed = tail(says[last]);
    const uint64_t end = tailed ? 2048 * (n - 1) + says[last] : 2048 * n;
    if (w.start >= end || i >= end - w.start)
        return kNone;
    const uint64_t pos = w.start + i;
    const uint64_t frame = tailed && pos / 2048 >= n - 1 ? n - 1 : pos / 2048;
    return ((w.first_frame + frame) * 8192 + (pos - 2048 * frame)) * 2 + (tailed && frame == n - 1 ? 1 : 0);
}

int failures = 0, cases = 0;

void check(const Table& t, const std::vector<sela_hip_window>& windows, uint32_t window_samples, const std::vector<uint32_t>* staged = nullptr)
{
    cases++;
    const uint32_t total = (uint32_t)t.says.size();
    sela::WindowPlan plan;
    sela::plan_windows_whole(t.bytes.data(), t.offsets.data(), total, windows.data(), (uint32_t)windows.size(), window_samples, &plan);
    bool ok = plan.windows.size() == windows.size() && plan.offsets.size() == plan.frames.size() + 1;
    // the staged table: the frames in ascending order, their sizes the caller's
    std::vector<uint32_t> staged_says;
    for (size_t k = 0; ok && k < plan.frames.size(); k++) {
        ok = plan.frames[k] < total && (k == 0 || plan.frames[k] > plan.frames[k - 1])
            && plan.offsets[k + 1] - plan.offsets[k] == t.offsets[plan.frames[k] + 1] - t.offsets[plan.frames[k]];
        if (ok)
            staged_says.push_back(t.says[plan.frames[k]]);
    }
    if (ok && staged && *staged != plan.frames)
        ok = false;
    for (size_t w = 0; ok && w < windows.size(); w++)
        for (uint32_t i = 0; ok && i < window_samples; i++) {
            const uint64_t want = cut(windows[w], t.says, i);
            uint64_t got = cut(plan.windows[w], staged_says, i);
            if (got != kNone) { // back to the caller's frame numbers
                const uint64_t k = got / 2 / 8192;
                got = ((uint64_t)plan.frames[k] * 8192 + got / 2 % 8192) * 2 + got % 2;
            }
            ok = want == got;
        }
    if (!ok) {
        failures++;
        std::printf("FAIL: %zu frames, %zu windows of %u samples (first: start %llu, frames %u + %u)\n", t.says.size(), windows.size(), window_samples,
            windows.empty() ? 0ull : (unsigned long long)windows[0].start, windows.empty() ? 0u : windows[0].first_frame, windows.empty() ? 0u : windows[0].n_frames);
    }
}

} // namespace

int main()
{
    const uint64_t B = 2048;
    // ---- which frames are staged ------------------------------------------------------------------------------------------
    {
        const Table t = make_table({ 2048, 2048, 2125, 2048, 2048, 2048, 2053 }); // a tailed stream (0 .. 2), a plain one (3 .. 5), a long frame alone (6)
        const std::vector<uint32_t> f2 = { 2 }, f12 = { 1, 2 }, f0 = { 0 }, f4 = { 4 }, f6 = { 6 }, none = {}, f23 = { 2, 3 }, f56 = { 5, 6 };
        check(t, { { 2 * B + 2100, 0, 3 } }, 300, &f2);        // entirely inside the tail, behind 2048 n
        check(t, { { 2 * B + 2125, 0, 3 } }, 300, &f2);        // at S: zeros, the frame is covered all the same
        check(t, { { ~0ull, 0, 3 } }, 300, &f2);               // start / 2048 >= n - 1 for any start
        check(t, { { 2 * B - 5, 0, 3 } }, 300, &f12);
        check(t, { { 5, 0, 3 } }, 300, &f0);
        check(t, { { B + 5, 3, 3 } }, 300, &f4);
        check(t, { { 3 * B, 3, 3 } }, 300, &none);             // behind a plain stream: nothing
        check(t, { { 0, 6, 1 }, { 2052, 6, 9 }, { 2053, 6, 1 } }, 300, &f6);
        check(t, { { 3 * B - 5, 3, 4 } }, 300, &f56);          // a stream cut at the table's end whose last frame is the long one
        check(t, { { 5, 2, 5 } }, 300, &f23);                  // a long frame in front of the last (a malformed stream) is staged with the frame behind it
        check(t, { { 0, 7, 1 }, { 0, 0, 0 }, { 0, 0xFFFFFFFFu, 0xFFFFFFFFu } }, 300, &none);
    }
    {
        const Table t = make_table({ 2048, kHeaderless }); // the table's last frame is too short to hold a header: it says nothing
        const std::vector<uint32_t> f1 = { 1 }, f01 = { 0, 1 }, none = {};
        check(t, { { B + 5, 0, 2 } }, 300, &f1);
        check(t, { { B - 5, 0, 2 } }, 300, &f01);
        check(t, { { 2 * B, 0, 2 }, { ~0ull, 0, 2 } }, 300, &none);
    }
    {
        const Table t = make_table({ 700 }); // one short frame alone
        const std::vector<uint32_t> f0 = { 0 };
        check(t, { { 0, 0, 1 }, { 699, 0, 1 }, { 700, 0, 1 }, { 1ull << 63, 0, 5 }, { ~0ull - 100, 0, 1 } }, 777, &f0);
    }
    check(make_table({}), { { 0, 0, 1 }, { ~0ull, 0, 0xFFFFFFFFu } }, 5);
    // ---- seeded batches: every position names the same thing through the plan ----------------------------------------------
    const uint32_t lengths[] = { 2048, 2048, 2048, 2048, 2048, 1, 77, 700, 2047, 2049, 2125, 4095, 4096, 0, 65535, kHeaderless };
    const uint32_t sizes[4] = { 1, 300, 2049, 5000 };
    for (int round = 0; round < 400; round++) {
        std::vector<uint32_t> ls(rnd() % 9);
        for (uint32_t& l : ls)
            l = lengths[rnd() % (sizeof lengths / sizeof lengths[0])];
        const Table t = make_table(ls);
        const uint32_t ws = sizes[rnd() % 4];
        std::vector<sela_hip_window> windows(1 + rnd() % 6);
        for (sela_hip_window& w : windows) {
            w.first_frame = (uint32_t)(rnd() % (ls.size() + 2));
            w.n_frames = rnd() % 5 == 0 ? 0xFFFFFFFFu : (uint32_t)(rnd() % (ls.size() + 2));
            const uint64_t span = 2048 * (uint64_t)(ls.size() + 3);
            switch (rnd() % 6) {
            case 0: w.start = ~0ull - rnd() % 5000; break;
            case 1: w.start = (1ull << 32) + rnd() % span; break;
            default: w.start = rnd() % span; break;
            }
        }
        check(t, windows, ws);
    }
    std::printf("%d cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
