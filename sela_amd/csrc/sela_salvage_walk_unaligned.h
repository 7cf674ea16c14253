// sela_salvage_walk_unaligned.h -- the salvage walk at ANY BYTE on the host: the DEFINITION of sela_hip_salvage_frames_unaligned
// (include/sela_hip.h), which the device (sela_salvage_unaligned.hip) reproduces byte for byte.  DESIGN.md 5.33.
//
// sela_salvage_walk.h's rule with "word" replaced by "byte": a frame may start at any byte offset of the payload (its length
// stays a multiple of 4), so damage that inserts or deletes any number of bytes no longer loses what lies behind it.
//
// Plain C++, no HIP: sela_capi.hip wraps it, and tests/c/salvage_walk_unaligned.cpp compiles it alone under ASan + UBSan.  Every
// read goes through sela_format.h's byte reader with the payload's length as its bound, or is a 4-byte memcpy at an offset
// checked against that length, so the payload may lie at any alignment and end at any byte.
#ifndef SELA_SALVAGE_WALK_UNALIGNED_H_
#define SELA_SALVAGE_WALK_UNALIGNED_H_

#include <cstddef>
#include <cstdint>
#include <cstring>

#include "sela_format.h"
#include "sela_hip.h"

namespace sela {

// The frame that would start at byte `off` (any byte): where it ends, or 0 when `off` is no candidate -- no sync word there,
// or one of its `channels` subframe headers does not fit `bytes`.
inline uint64_t salvage_unaligned_frame_end(const uint8_t* payload, uint64_t bytes, uint64_t off, uint32_t channels)
{
    if (off + 4 > bytes)
        return 0;
    uint32_t sync;
    std::memcpy(&sync, payload + off, 4);
    if (sync != SELA_SYNC_WORD)
        return 0;
    uint64_t p = off + 4;
    for (uint32_t c = 0; c < channels && p; c++) {
        SelaSubframeHeader h;
        p = sela_subframe_read_bytes(payload, bytes, p, &h);
    }
    return p;
}

// A candidate behind whose end fewer than 4 bytes are left, or whose end is where another candidate starts.
inline bool salvage_unaligned_confirmed(const uint8_t* payload, uint64_t bytes, uint64_t off, uint32_t channels)
{
    const uint64_t end = salvage_unaligned_frame_end(payload, bytes, off, channels);
    return end && (bytes - end < 4 || salvage_unaligned_frame_end(payload, bytes, end, channels));
}

// The walk.  records (or null): [max_frames], entries [0 .. the count) are written; totals (or null): [4].
inline uint32_t salvage_walk_unaligned(const uint8_t* payload, uint64_t bytes, uint32_t max_frames, uint32_t channels, sela_hip_salvaged* records,
    uint64_t* totals)
{
    uint64_t p = 0, gaps = 0, kept = 0, last_end = 0;
    uint32_t n = 0;
    if (channels == 0 || channels > 255)
        max_frames = 0;
    while (n < max_frames) {
        uint64_t at = p, end = salvage_unaligned_frame_end(payload, bytes, p, channels); // a trusted position: offset 0, or where a taken frame ended
        if (!end) {
            for (; at + 4 <= bytes; at++)
                if (salvage_unaligned_confirmed(payload, bytes, at, channels))
                    break;
            if (at + 4 > bytes)
                break;
            end = salvage_unaligned_frame_end(payload, bytes, at, channels);
        }
        if (records) {
            records[n].offset = at;
            records[n].skipped_before = at - p;
            records[n].bytes = (uint32_t)(end - at);
            records[n].reserved = 0;
        }
        gaps += at != p;
        kept += end - at;
        last_end = p = end;
        n++;
    }
    if (totals)
        totals[0] = n, totals[1] = gaps, totals[2] = kept, totals[3] = last_end;
    return n;
}

} // namespace sela
#endif
