// sela_verify32_rule.h -- what the compare kernels of sela_verify32.hip (against int32 samples) and of
// sela_verify_pcm.hip (against packed PCM; 5.24) share: which frames a compare takes straight from the subframes as decoded
// (the DIRECT layouts), and how a workgroup leaves its two words.  Device code only.
#ifndef SELA_VERIFY32_RULE_H_
#define SELA_VERIFY32_RULE_H_

#include "sela_device.h"
#include "sela_generic.h"

namespace sela {
namespace {

constexpr uint32_t kNoDiff = 0xFFFFFFFFu;
constexpr uint32_t kV32Threads = 256, kV32Waves = kV32Threads / 64;
constexpr uint32_t kV32NoParent = 0xFFFFu;

// Minimum of one unsigned 32-bit value per lane (wave_max_u32 on the complements; the result is wave-uniform).
__device__ __forceinline__ uint32_t wave_min32(uint32_t v) { return ~wave_max_u32(~v); }

__device__ __forceinline__ uint32_t frames_in_call(const uint32_t* __restrict__ n_frames_found, uint32_t max_frames)
{
    return n_frames_found ? min(*n_frames_found, max_frames) : max_frames;
}

// Is the frame's layout DIRECT: every channel 0 .. channels-1 named by exactly one subframe that is ok and of type 0 or 1, every
// type-1 subframe's parent named by a type-0 subframe at least as long.  The whole workgroup (kV32Threads threads, t its
// threadIdx.x) calls it; it leaves, by channel, the subframe's position and length and its parent's position (kV32NoParent:
// independent), and s_other non-zero for any other layout.
__device__ __forceinline__ void verify32_judge_layout(const GenericSubInfo* inf, uint32_t channels, uint32_t t, uint32_t* s_named, uint32_t* s_n,
    uint16_t* s_pos, uint16_t* s_ppos, uint32_t& s_other)
{
    s_named[t] = 0, s_pos[t] = 0;
    if (t == 0)
        s_other = 0;
    __syncthreads();
    GenericSubInfo si;
    si.channel = si.type = si.parent = si.ok = 0, si.n = 0;
    bool good = false;
    if (t < channels) {
        si = inf[t];
        good = si.ok && si.type <= 1 && si.channel < channels;
        if (good) {
            atomicAdd(&s_named[si.channel], 1u);
            s_pos[si.channel] = (uint16_t)t, s_n[si.channel] = si.n; // (a channel named twice: either one, the frame is not direct)
        }
    }
    __syncthreads();
    if (t < channels) {
        bool ok = good && s_named[t] == 1;
        uint32_t ppos = kV32NoParent;
        if (ok && si.type == 1) {
            ok = si.parent < channels && s_named[si.parent] == 1;
            if (ok) {
                ppos = s_pos[si.parent];
                const GenericSubInfo ps = inf[ppos];
                ok = ps.type == 0 && ps.n >= si.n;
            }
        }
        if (good)
            s_ppos[si.channel] = (uint16_t)ppos;
        if (!ok)
            s_other = 1;
    }
    __syncthreads();
}

// The workgroup's count and smallest index: DPP rows inside a wave, LDS across the waves; thread 0 leaves the slice's two words
// (parts: the counts of every (frame, slice), then the smallest indices: n_slots of each).
__device__ __forceinline__ void leave_slice_words(uint32_t n_diff, uint32_t first, uint32_t* s_count, uint32_t* s_first, uint32_t* __restrict__ parts,
    size_t slot, size_t n_slots)
{
    n_diff = wave_sum_small(n_diff);
    first = wave_min32(first);
    if (threadIdx.x % 64 == 0)
        s_count[threadIdx.x / 64] = n_diff, s_first[threadIdx.x / 64] = first;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0, least = kNoDiff;
        for (uint32_t w = 0; w < kV32Waves; w++) {
            total += s_count[w];
            least = min(least, s_first[w]);
        }
        parts[slot] = total;
        parts[n_slots + slot] = least;
    }
}

} // namespace
} // namespace sela
#endif
