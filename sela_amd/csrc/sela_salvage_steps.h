// sela_salvage_steps.h -- what the two salvages share (sela_salvage.hip: frames at word positions, DESIGN.md 5.30;
// sela_salvage_unaligned.hip: frames at any byte): the workspace, the backward min-scan of a workgroup, the
// search of a rank by its place in the compacted payload, and the launches of the middle of the chain.  None of these asks
// what UNIT a position is counted in -- words in the first file, bytes in the second -- as long as pos[], next[], the gaps and
// the limit of one call agree.
#ifndef SELA_SALVAGE_STEPS_H_
#define SELA_SALVAGE_STEPS_H_

#include <algorithm>

#include "sela_host.h"

namespace sela {

constexpr int kSalvageThreads = 256;
constexpr int kSalvagePerThread = 16;
constexpr uint32_t kSalvageChunk = (uint32_t)kSalvageThreads * kSalvagePerThread; // candidates one links workgroup covers; words one copy workgroup writes
constexpr int kSalvageBlocks = 1024; // grid of the succ / round / scatter / records launches (grid-stride)

struct SalvageWs {
    IndexWs ix;             // the index's own, at the workspace's start as launch_index has it
    uint64_t* scan_offsets; // [1] what k_index_scan initialises: nobody's output here
    uint32_t* scan_count;   // [1]
    uint32_t* nconf;        // [n_cand] the first confirmed candidate at or behind i within i's 4096, or none
    uint32_t* gap_a;        // [n_cand] the gap, in words, of jump array A's links ...
    uint32_t* gap_b;        // [n_cand] ... and of B's
    uint32_t* bsuf;         // [blocks + 1] the first confirmed candidate in workgroup b's 4096 or behind
    uint32_t* r_pos;        // [frames] by rank: the frame's word index,
    uint32_t* r_end;        // [frames] its end,
    uint32_t* r_dst;        // [frames] and its word index in the compacted payload
    uint32_t* head;         // [1] the first frame taken, or none
    uint32_t* copy_words;   // [1] the words of the compacted payload that fit out_cap in whole frames
};
// The workspace, for a payload of `words` 32-bit words: the index's, three more arrays of one uint32 per word, a word per 4096
// candidates, three per frame (no more frames than words), and four single words.  (The chain's skip[] lives in ix.map, which
// nothing reads after k_salvage_links.)
inline SalvageWs carve_salvage(Carve& c, uint64_t words, uint32_t max_frames)
{
    const uint64_t blocks = (words + kSalvageChunk - 1) / kSalvageChunk, frames = std::min<uint64_t>(max_frames, words);
    SalvageWs ws;
    ws.ix = carve_index(c, words);
    ws.scan_offsets = c.take<uint64_t>(1);
    ws.scan_count = c.take<uint32_t>(1);
    ws.nconf = c.take<uint32_t>(words);
    ws.gap_a = c.take<uint32_t>(words);
    ws.gap_b = c.take<uint32_t>(words);
    ws.bsuf = c.take<uint32_t>(blocks + 1);
    ws.r_pos = c.take<uint32_t>(frames);
    ws.r_end = c.take<uint32_t>(frames);
    ws.r_dst = c.take<uint32_t>(frames);
    ws.head = c.take<uint32_t>(1);
    ws.copy_words = c.take<uint32_t>(1);
    return ws;
}

#if defined(__HIPCC__)
// Per thread: the minimum of v over the threads BEHIND it in the workgroup (kIndexNone, the largest value, where there is
// none), and `total`, the minimum over all.  sh: a word per wave.
__device__ __forceinline__ uint32_t block_suffix_min(uint32_t v, uint32_t* sh, uint32_t& total)
{
    const int lane = threadIdx.x % 64, wave = threadIdx.x / 64, n_waves = blockDim.x / 64;
    uint32_t incl = v;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_down(incl, d); // (its own value where lane + d runs off the wave)
        incl = min(incl, o);
    }
    uint32_t after = __shfl_down(incl, 1);
    if (lane == 63)
        after = kIndexNone;
    if (lane == 0)
        sh[wave] = incl;
    __syncthreads();
    total = kIndexNone;
    for (int w = 0; w < n_waves; w++) {
        const uint32_t t = sh[w];
        total = min(total, t);
        if (w > wave)
            after = min(after, t);
    }
    __syncthreads();
    return after;
}

// The rank whose frame holds position d of the compacted payload, between two ranks known to bracket it (r_dst[] increases).
__device__ __forceinline__ uint32_t salvage_frame_of(const uint32_t* __restrict__ r_dst, uint32_t lo, uint32_t hi, uint32_t d)
{
    while (lo < hi) { // the last rank in [lo, hi] with r_dst <= d
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (r_dst[mid] <= d)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}
#endif

// sela_salvage.hip's launches that both salvages run as they are.  launch_salvage_clear: the outputs' initial state alone (a
// payload that can hold no candidate, or a call that asks for no frame).  launch_salvage_chain: what lies between the links
// and the records -- the block suffix with the head and the outputs' initial state, succ, the doubling rounds and the scatter
// -- on pos[], next[], stage_pos[] (the direct successors), nconf[] and bsuf[] as the caller's links kernel left them;
// `limit` is the payload's length in the caller's unit, `grid_items` what the grid-stride launches are sized by.
hipError_t launch_salvage_clear(uint64_t* d_totals, uint64_t* d_frame_offsets, hipStream_t stream);
hipError_t launch_salvage_chain(const SalvageWs& ws, uint32_t blocks, uint32_t limit, uint32_t grid_items, uint32_t max_frames, uint64_t* d_totals,
    uint64_t* d_frame_offsets, hipStream_t stream);

} // namespace sela
#endif
