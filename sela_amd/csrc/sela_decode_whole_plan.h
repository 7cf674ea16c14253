// sela_decode_whole_plan.h -- how a full decode reads a whole-track stream.
//
// Plain arithmetic on the stream's bytes, compiled for the device (k_whole_plan, sela_window_whole.hip), for the host call
// (sela_hip_decode_whole, sela_capi.hip) and for tests/c/decode_whole_plan.cpp from this one text.  It is the reading 5.20 gives a
// window's stream: the last frame L of n says n_L samples (frame_says_samples); 1 .. 4095 and not 2048 makes it the long last frame
// of S = 2048 (n - 1) + n_L samples, decoded by the any-length kernel beside frames 0 .. n - 2 on the 2048-sample decoder; any other
// n_L leaves all n frames to that decoder, S = 2048 n.  A stream that does not fit the caller's room is not decoded at all.
#ifndef SELA_DECODE_WHOLE_PLAN_H_
#define SELA_DECODE_WHOLE_PLAN_H_

#include <stdint.h>

#include "sela_window_tail.h"

namespace sela {

constexpr uint32_t kWholeRouteNone = 0, kWholeRouteFast = 1, kWholeRouteTail = 3; // status[3] of sela_hip_decode_whole_device

struct DecodeWholePlan {
    uint64_t samples;     // S, per channel, whatever the capacity
    uint32_t fast_frames; // frames 0 .. fast_frames - 1 go to the 2048-sample decoder
    uint32_t route;       // kWholeRoute*: None for an empty stream and for one the capacity refuses
    uint32_t flags;       // SELA_HIP_FLAG_STRIDE where S > pcm_capacity, else 0
    WindowTail tail;      // the long last frame with its share [0, n_L) (lo < hi), or empty
};

SELA_HOST_DEVICE inline DecodeWholePlan plan_decode_whole(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint64_t pcm_capacity)
{
    DecodeWholePlan p = {};
    if (n_frames == 0)
        return p;
    const uint32_t last = n_frames - 1;
    const uint32_t n_last = frame_says_samples(frames, frame_offsets, last);
    const bool tailed = tail_length(n_last);
    p.samples = tailed ? (uint64_t)SELA_HIP_SAMPLES_PER_FRAME * last + n_last : (uint64_t)SELA_HIP_SAMPLES_PER_FRAME * n_frames;
    if (p.samples > pcm_capacity) {
        p.flags = SELA_HIP_FLAG_STRIDE;
        return p;
    }
    p.fast_frames = tailed ? last : n_frames;
    p.route = tailed ? kWholeRouteTail : kWholeRouteFast;
    if (tailed) {
        p.tail.frame = last;
        p.tail.n = n_last;
        p.tail.lo = 0, p.tail.hi = n_last, p.tail.s0 = 0;
    }
    return p;
}

} // namespace sela
#endif // SELA_DECODE_WHOLE_PLAN_H_
