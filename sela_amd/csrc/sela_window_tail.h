// sela_window_tail.h -- the long last frame of a whole-track stream, as a window sees it.
//
// Plain arithmetic, compiled for the device (k_tailwin_plan, sela_window_whole.hip) and for the host (plan_windows_whole,
// sela_window_plan.h) from this one text.  A stream of n frames inside the table whose last frame L says n_L samples, 1 .. 4095
// and not 2048, holds S = 2048 (n - 1) + n_L samples per channel: frame f still starts at sample 2048 f, only L is odd.
#ifndef SELA_WINDOW_TAIL_H_
#define SELA_WINDOW_TAIL_H_

#include <stdint.h>

#include "sela_format.h"
#include "sela_hip.h"

namespace sela {

constexpr uint32_t kTailMaxSamples = 4095;  // the longest last frame sela_hip_encode_whole writes (2048 + 2047)
constexpr uint32_t kTailStride = 4096;      // int32 per decoded subframe of a tail in the workspace

// One per window, written by k_tailwin_plan: the window's share [lo, hi) of its stream's last frame, in window samples; sample lo
// of the window is sample s0 of the frame.  lo >= hi: the window has no share (no such frame, or it does not reach it).
struct WindowTail {
    uint32_t frame, n, lo, hi, s0, pad[3];
};
static_assert(sizeof(WindowTail) == 32, "two 16-byte words");

SELA_HOST_DEVICE inline bool tail_length(uint32_t n_last) { return n_last >= 1 && n_last <= kTailMaxSamples && n_last != SELA_HIP_SAMPLES_PER_FRAME; }

// The frames of a window's stream that lie inside the table.
SELA_HOST_DEVICE inline uint32_t window_stream_frames(const sela_hip_window& w, uint32_t n_frames_total)
{
    return w.first_frame < n_frames_total ? (w.n_frames < n_frames_total - w.first_frame ? w.n_frames : n_frames_total - w.first_frame) : 0u;
}

// What a frame says its length is, by sela_hip_index_samples' rule: its first subframe's samplesPerChannel, read at any alignment;
// 0 where the frame is too short to hold that header (or the offsets decrease).
SELA_HOST_DEVICE inline uint32_t frame_says_samples(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t f)
{
    const uint64_t o0 = frame_offsets[f], o1 = frame_offsets[f + 1];
    SelaSubframeHeader h = {};
    (void)sela_subframe_read_bytes(frames + o0, o1 >= o0 ? o1 - o0 : 0, 4, &h); // (n is read even when only the residue words run past the frame)
    return h.n;
}

// The share of a last frame of n_last samples (tail_length) in a window of a stream of in_stream >= 1 frames.  Any uint64 start:
// nothing is added to it before it is known to be small.
SELA_HOST_DEVICE inline WindowTail window_tail_share(uint64_t start, uint32_t window_samples, uint32_t in_stream, uint32_t n_last)
{
    WindowTail t = {};
    t.n = n_last;
    const uint64_t base = (uint64_t)SELA_HIP_SAMPLES_PER_FRAME * (in_stream - 1); // the frame's first sample in the stream (< 2^43)
    if (start >= base + n_last)
        return t;
    if (start >= base) {
        t.s0 = (uint32_t)(start - base);
        t.lo = 0;
        t.hi = n_last - t.s0 < window_samples ? n_last - t.s0 : window_samples;
    } else {
        const uint64_t d = base - start;
        if (d >= window_samples)
            return t;
        t.lo = (uint32_t)d;
        t.hi = d + n_last < window_samples ? (uint32_t)d + n_last : window_samples;
    }
    return t;
}

} // namespace sela
#endif // SELA_WINDOW_TAIL_H_
