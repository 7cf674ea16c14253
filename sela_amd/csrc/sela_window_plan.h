// sela_window_plan.h -- what sela_hip_decode_windows copies to the device: only the frames its windows touch.
//
// Plain C++ on the caller's table and descriptors, no device and no library state, so that tests/c/window_compact.cpp drives it
// on the CPU under the sanitizers.  The plan: mark the distinct covering frames; lay their bytes back to back (new offsets; the
// sizes stay what the table says, so a frame the device refuses for its size is refused as before); put every descriptor on the
// compacted table.  A window's covering frames [a, b) are consecutive in the caller's table and all of them are marked, so they
// are consecutive in the compacted one:  first_frame' = map[a],  n_frames' = b - a,  start' = start - 2048 * (a - first_frame).
// Behind b - a frames the device stores zeros, which is what the window holds there: b is the stream's end, the table's end, or
// behind the window's last sample.  The offsets must not decrease (the caller has checked).
#ifndef SELA_WINDOW_PLAN_H_
#define SELA_WINDOW_PLAN_H_

#include <stdint.h>

#include <vector>

#include "sela_hip.h"
#include "sela_window_tail.h"

namespace sela {

struct WindowPlan {
    std::vector<uint32_t> frames;         // the distinct covering frames, ascending (indices into the caller's table)
    std::vector<uint64_t> offsets;        // [frames.size() + 1]: where their bytes lie when staged back to back
    std::vector<sela_hip_window> windows; // the descriptors on the compacted table
    uint64_t staged_bytes() const { return offsets.empty() ? 0 : offsets.back(); }
};

// The covering frames of one window, [*a, *b) in the caller's table; false: it touches none (its output is all zeros).
inline bool window_covering_frames(const sela_hip_window& w, uint32_t n_frames_total, uint32_t window_samples, uint32_t* a, uint32_t* b)
{
    const uint32_t in_stream = w.first_frame < n_frames_total ? (w.n_frames < n_frames_total - w.first_frame ? w.n_frames : n_frames_total - w.first_frame) : 0u;
    const uint64_t q = w.start / SELA_HIP_SAMPLES_PER_FRAME; // (compared before anything is added to it: any uint64 start)
    if (window_samples == 0 || q >= in_stream)
        return false;
    const uint64_t r = w.start % SELA_HIP_SAMPLES_PER_FRAME;
    const uint64_t touched = (r + window_samples - 1) / SELA_HIP_SAMPLES_PER_FRAME + 1; // frames from q on, were the stream long enough
    const uint64_t left = in_stream - q;
    *a = w.first_frame + (uint32_t)q;
    *b = *a + (uint32_t)(touched < left ? touched : left);
    return true;
}

// The plan for a rule that says which frames a window covers and where it starts among them:
// cover(window, &a, &b, &start) -> false for a window that touches nothing.
template <typename Cover>
inline void plan_windows_by(const uint64_t* frame_offsets, uint32_t n_frames_total, const sela_hip_window* windows, uint32_t n_windows, WindowPlan* plan, Cover cover)
{
    std::vector<uint32_t> map((size_t)n_frames_total + 1, 0); // first a mark per frame, then the frame's place in the compacted table
    for (uint32_t i = 0; i < n_windows; i++) {
        uint32_t a, b;
        uint64_t start;
        if (cover(windows[i], &a, &b, &start))
            for (uint32_t f = a; f < b; f++)
                map[f] = 1;
    }
    plan->frames.clear();
    plan->offsets.assign(1, 0);
    for (uint32_t f = 0; f < n_frames_total; f++) {
        const bool marked = map[f] != 0;
        map[f] = (uint32_t)plan->frames.size();
        if (marked) {
            plan->frames.push_back(f);
            plan->offsets.push_back(plan->offsets.back() + (frame_offsets[f + 1] - frame_offsets[f]));
        }
    }
    plan->windows.resize(n_windows);
    for (uint32_t i = 0; i < n_windows; i++) {
        uint32_t a, b;
        uint64_t start;
        sela_hip_window& out = plan->windows[i];
        if (cover(windows[i], &a, &b, &start)) {
            out.start = start;
            out.first_frame = map[a];
            out.n_frames = b - a;
        } else {
            out.start = 0, out.first_frame = 0, out.n_frames = 0; // an empty stream: zeros
        }
    }
}

inline void plan_windows(const uint64_t* frame_offsets, uint32_t n_frames_total, const sela_hip_window* windows, uint32_t n_windows, uint32_t window_samples,
    WindowPlan* plan)
{
    plan_windows_by(frame_offsets, n_frames_total, windows, n_windows, plan, [&](const sela_hip_window& w, uint32_t* a, uint32_t* b, uint64_t* start) {
        *start = w.start % SELA_HIP_SAMPLES_PER_FRAME; // = start - 2048 * (a - first_frame)
        return window_covering_frames(w, n_frames_total, window_samples, a, b);
    });
}

// ---- whole-track streams: sela_hip_decode_windows_whole --------------------------------------------------------
// The device call takes the LAST frame of a descriptor's stream for the long one when it says 1 .. 4095 samples and not 2048
// (frame_says_samples on the host's bytes here, on the staged ones there).  So, for a stream of n frames inside the table whose
// last frame L says such a length:
//   * a window with start / 2048 >= n - 1 covers L and nothing else -- not nothing, as it would among 2048-sample frames;
//     start' = start - 2048 (n - 1), any uint64;
//   * every other window covers what it covered, L included where it reaches it.
// A compacted stream that ends in front of L ends on one of the 2048-sample run, which the device must not take for a long last
// frame: where such a frame says 1 .. 4095 and not 2048 (a malformed stream), the frame behind it is staged too and the compacted
// stream ends on that one, outside the window.
inline bool window_covering_frames_whole(const uint8_t* frames, const uint64_t* frame_offsets, const sela_hip_window& w, uint32_t n_frames_total,
    uint32_t window_samples, uint32_t* a, uint32_t* b, uint64_t* start)
{
    const uint32_t n = window_stream_frames(w, n_frames_total);
    if (window_samples == 0 || n == 0)
        return false;
    const uint32_t last = w.first_frame + n - 1;
    if (w.start / SELA_HIP_SAMPLES_PER_FRAME >= n - 1 && tail_length(frame_says_samples(frames, frame_offsets, last))) {
        *a = last, *b = last + 1;
        *start = w.start - (uint64_t)SELA_HIP_SAMPLES_PER_FRAME * (n - 1);
        return true;
    }
    if (!window_covering_frames(w, n_frames_total, window_samples, a, b))
        return false;
    *start = w.start % SELA_HIP_SAMPLES_PER_FRAME;
    if (*b <= last && tail_length(frame_says_samples(frames, frame_offsets, *b - 1)))
        (*b)++;
    return true;
}

inline void plan_windows_whole(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames_total, const sela_hip_window* windows, uint32_t n_windows,
    uint32_t window_samples, WindowPlan* plan)
{
    plan_windows_by(frame_offsets, n_frames_total, windows, n_windows, plan, [&](const sela_hip_window& w, uint32_t* a, uint32_t* b, uint64_t* start) {
        return window_covering_frames_whole(frames, frame_offsets, w, n_frames_total, window_samples, a, b, start);
    });
}

} // namespace sela
#endif // SELA_WINDOW_PLAN_H_
