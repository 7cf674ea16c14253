// sela_salvage.hip -- the frames of a DAMAGED .sela payload found on the device, and copied back to back
// (sela_hip_salvage_frames_device, sela_hip_salvage_payload_device).  DESIGN.md 5.30.
//
// The rule is the host walk's (sela_salvage_walk.h): from a trusted position -- offset 0, or the end of a taken frame -- a
// candidate is taken as it is; anywhere else only a CONFIRMED candidate is, one whose end is the payload's or another candidate.
// The index (sela_index.inc) already lists the candidates in position order and ranks a chain by pointer doubling; its first
// three kernels run here unchanged (launch_index_candidates), and what follows gives the chain a successor that does not give up:
//
//   k_salvage_links         per candidate i: direct[i] = the candidate at next[i] (as index_link finds it), and whether i is
//                           confirmed (direct[i] exists, or next[i] is the payload's last whole word's end).  nconf[i] = the first
//                           confirmed candidate at or behind i INSIDE i's workgroup's 4096 candidates (a backward min-scan:
//                           thread, wave, workgroup), and the workgroup's first confirmed candidate;
//   k_salvage_block_suffix  one workgroup: the backward min-scan of those per-workgroup firsts, so that "the first confirmed
//                           candidate at or behind i" is nconf[i] or, where that is none, bsuf[i / 4096 + 1]; the head of the
//                           chain by the rule from p = 0 (candidate 0 if it lies at offset 0, else the first confirmed one);
//                           the outputs' initial state;
//   succ                    the resynchronising successor: direct[i], else the first confirmed candidate at or behind the lower
//                           bound of next[i] in pos[] (sorted: a binary search), and the GAP of that link in words;
//   rounds                  index_round's doubling, with the gaps carried along: a node marked with rank r + 2^j also gets
//                           skip = the marking node's skip + the gaps of the 2^j links between them.  Chains still merge and
//                           positions still increase, so ranking from the head keeps false chains out, and a node reached by
//                           several chains gets the gaps of the ranked one only;
//   scatter                 by rank: the frame's position, its end, and its place in the compacted payload (position - skip:
//                           the exclusive sum of the lengths before it), all in words;
//   records                 per rank: the record (skipped_before from the rank before), the compacted offset, the totals, and
//                           how far the copy may write (the last frame end inside out_cap);
//   k_salvage_copy          one workgroup per 4096 words of the COMPACTED payload (so a frame of any length is many workgroups'
//                           job and each destination word is written once).  The shift between source and destination is the
//                           sum of the gaps so far, which never decreases along the ranks: a workgroup whose first and last word
//                           have the same shift copies straight (16 bytes per lane where source and destination agree modulo 16, else
//                           coalesced dwords); only a workgroup that holds a gap looks its frame up per word.
//
// succ, rounds, scatter and records are 3 + ceil(log2(max_frames)) launches over the whole device, for every max_frames: the
// one-workgroup form the index has for a track (links, rounds and scatter on LDS) was built and measured here too, and on the
// bench track it was no faster -- 0.0744 ms against 0.0745 ms intact, 0.0845 ms against 0.0782 ms with 64 damaged headers
//  -- so it was dropped, and with it a limit on max_frames and one on the candidates.
//
// The workspace, the workgroup's backward min-scan and the rank search live in sela_salvage_steps.h, and the block suffix, succ,
// the rounds and the scatter are launched through launch_salvage_chain: sela_salvage_unaligned.hip runs them
// as they are, on byte positions.
#include "sela_salvage_steps.h"

namespace sela {

__global__ __launch_bounds__(kSalvageThreads) void k_salvage_links(SalvageWs ws, uint32_t words)
{
    __shared__ uint32_t sh[kSalvageThreads / 64];
    const uint32_t n = *ws.ix.n_cand;
    const uint32_t first = blockIdx.x * kSalvageChunk + threadIdx.x * kSalvagePerThread; // (below 2^32: no more workgroups than words / 4096, rounded up)
    uint32_t conf[kSalvagePerThread];
#pragma unroll
    for (int k = 0; k < kSalvagePerThread; k++) {
        const uint32_t i = first + k;
        conf[k] = kIndexNone;
        if (i < n) {
            const uint32_t w = ws.ix.next[i];
            const uint32_t j = w < words ? ws.ix.map[w] : kIndexNone; // (map[] is read only where pos[] confirms it)
            const uint32_t direct = j < n && ws.ix.pos[j] == w ? j : kIndexNone;
            ws.ix.stage_pos[i] = direct;
            if (direct != kIndexNone || w == words)
                conf[k] = i;
        }
    }
    uint32_t run = kIndexNone;
#pragma unroll
    for (int k = kSalvagePerThread - 1; k >= 0; k--) {
        run = min(run, conf[k]);
        conf[k] = run;
    }
    uint32_t total;
    const uint32_t after = block_suffix_min(run, sh, total);
#pragma unroll
    for (int k = 0; k < kSalvagePerThread; k++)
        if (first + k < n)
            ws.nconf[first + k] = min(conf[k], after);
    if (threadIdx.x == 0)
        ws.bsuf[blockIdx.x] = total;
}

// One workgroup: bsuf[0 .. blocks) -> their backward min-scan, bsuf[blocks] = none; the head; nothing taken yet.
__global__ __launch_bounds__(1024) void k_salvage_block_suffix(SalvageWs ws, uint32_t blocks, uint64_t* __restrict__ totals, uint64_t* __restrict__ frame_offsets)
{
    __shared__ uint32_t sh[16];
    constexpr uint32_t kPer = 8, kTile = 1024 * kPer;
    uint32_t carry = kIndexNone;
    for (uint32_t tile = (blocks + kTile - 1) / kTile; tile-- > 0;) {
        const uint32_t first = tile * kTile + threadIdx.x * kPer;
        uint32_t v[kPer], run = kIndexNone;
#pragma unroll
        for (int k = kPer - 1; k >= 0; k--) {
            run = min(run, first + k < blocks ? ws.bsuf[first + k] : kIndexNone);
            v[k] = run;
        }
        uint32_t total;
        const uint32_t after = min(carry, block_suffix_min(run, sh, total));
#pragma unroll
        for (uint32_t k = 0; k < kPer; k++)
            if (first + k < blocks)
                ws.bsuf[first + k] = min(v[k], after);
        carry = min(carry, total);
    }
    if (threadIdx.x == 0) {
        ws.bsuf[blocks] = kIndexNone;
        *ws.head = *ws.ix.n_cand && ws.ix.pos[0] == 0 ? 0u : carry; // offset 0 is trusted; else the first confirmed candidate
        *ws.copy_words = 0;
        totals[0] = totals[1] = totals[2] = totals[3] = 0;
        if (frame_offsets)
            frame_offsets[0] = 0;
    }
}

// A payload without a word, or a call that asks for no frame: the outputs' initial state alone.
__global__ void k_salvage_clear(uint64_t* __restrict__ totals, uint64_t* __restrict__ frame_offsets)
{
    if (threadIdx.x == 0) {
        totals[0] = totals[1] = totals[2] = totals[3] = 0;
        if (frame_offsets)
            frame_offsets[0] = 0;
    }
}

// ---- the per-node steps -----------------------------------------------------------------------------------------------
struct SalvageChain {
    uint32_t *cur, *nxt;   // the jump arrays, ping-ponged
    uint32_t *gcur, *gnxt; // the words skipped along each jump
    uint32_t* rank;        // the frame index of a reached candidate, kIndexNone otherwise
    uint32_t* skip;        // of a reached candidate: the words skipped up to it, its own gap included
};
__device__ __forceinline__ SalvageChain salvage_chain_in_workspace(const SalvageWs& ws)
{
    return { ws.ix.stage_pos, ws.ix.stage_next, ws.gap_a, ws.gap_b, ws.ix.rank, ws.ix.map };
}

__device__ __forceinline__ uint32_t salvage_next_confirmed(const SalvageWs& ws, uint32_t i, uint32_t n)
{
    if (i >= n)
        return kIndexNone;
    const uint32_t v = ws.nconf[i];
    return v != kIndexNone ? v : ws.bsuf[i / kSalvageChunk + 1];
}

__device__ __forceinline__ void salvage_succ(const SalvageWs& ws, uint32_t i, uint32_t n, uint32_t words, uint32_t head, const SalvageChain& c)
{
    const uint32_t end = ws.ix.next[i];
    uint32_t t = ws.ix.stage_pos[i]; // the direct successor: a trusted position, taken as it is
    if (t == kIndexNone && end < words) {
        uint32_t lo = i + 1, hi = n; // the first candidate at or behind `end` (pos[] increases, and end > pos[i])
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (ws.ix.pos[mid] < end)
                lo = mid + 1;
            else
                hi = mid;
        }
        t = salvage_next_confirmed(ws, lo, n);
    }
    c.cur[i] = t;
    c.gcur[i] = t != kIndexNone ? ws.ix.pos[t] - end : 0u;
    c.rank[i] = i == head ? 0u : kIndexNone;
    c.skip[i] = i == head ? ws.ix.pos[i] : 0u;
}

// index_round with the gaps: ranks below 2^round are final, and so are their skips; a node marked in this round had no rank
// before it, so nobody reads its skip in the same round.
__device__ __forceinline__ void salvage_round(uint32_t i, uint32_t round, uint32_t max_frames, const SalvageChain& c, bool compose)
{
    const uint32_t t = c.cur[i], r = c.rank[i], step = 1u << round;
    if (t != kIndexNone && r < step && (uint64_t)r + step < max_frames) {
        c.rank[t] = r + step;
        c.skip[t] = c.skip[i] + c.gcur[i];
    }
    if (compose) {
        c.nxt[i] = t == kIndexNone ? kIndexNone : c.cur[t];
        c.gnxt[i] = t == kIndexNone ? 0u : c.gcur[i] + c.gcur[t];
    }
}

__device__ __forceinline__ bool salvage_scatter(const SalvageWs& ws, uint32_t i, uint32_t max_frames, const SalvageChain& c)
{
    const uint32_t r = c.rank[i];
    if (r >= max_frames)
        return false;
    const uint32_t p = ws.ix.pos[i];
    ws.r_pos[r] = p;
    ws.r_end[r] = ws.ix.next[i];
    ws.r_dst[r] = p - c.skip[i];
    return true;
}

// The record of rank r < count; true where a gap lies in front of it.  The last rank also writes what is known only there.
__device__ __forceinline__ bool salvage_record(const SalvageWs& ws, uint32_t r, uint32_t count, uint32_t cap_words, sela_hip_salvaged* __restrict__ records,
    uint64_t* __restrict__ totals, uint64_t* __restrict__ frame_offsets)
{
    const uint32_t p = ws.r_pos[r], e = ws.r_end[r], d = ws.r_dst[r], before = r ? ws.r_end[r - 1] : 0u;
    const uint32_t d_end = d + (e - p);
    if (records) {
        sela_hip_salvaged rec;
        rec.offset = (uint64_t)p * 4;
        rec.skipped_before = (uint64_t)(p - before) * 4;
        rec.bytes = (e - p) * 4; // (a frame is below 2^28 bytes: 255 subframes of 12 bytes and two times 65535 words)
        rec.reserved = 0;
        records[r] = rec;
    }
    if (frame_offsets)
        frame_offsets[r] = (uint64_t)d * 4;
    if (r + 1 == count) {
        if (frame_offsets)
            frame_offsets[count] = (uint64_t)d_end * 4;
        totals[2] = (uint64_t)d_end * 4;
        totals[3] = (uint64_t)e * 4;
    }
    // the copy writes whole frames, up to the last one that ends inside the room: one rank is that one
    if (d_end <= cap_words && (r + 1 == count || ws.r_dst[r + 1] + (ws.r_end[r + 1] - ws.r_pos[r + 1]) > cap_words))
        *ws.copy_words = d_end;
    return p != before;
}

__global__ __launch_bounds__(kSalvageThreads) void k_salvage_succ(SalvageWs ws, uint32_t words)
{
    const uint32_t n = *ws.ix.n_cand, head = *ws.head;
    const SalvageChain c = salvage_chain_in_workspace(ws);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        salvage_succ(ws, i, n, words, head, c);
}

__global__ __launch_bounds__(kSalvageThreads) void k_salvage_round(SalvageWs ws, uint32_t round, uint32_t max_frames, uint32_t swapped, uint32_t compose)
{
    const uint32_t n = *ws.ix.n_cand;
    SalvageChain c = salvage_chain_in_workspace(ws);
    if (swapped)
        c = SalvageChain{ c.nxt, c.cur, c.gnxt, c.gcur, c.rank, c.skip };
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        salvage_round(i, round, max_frames, c, compose != 0);
}

__global__ __launch_bounds__(kSalvageThreads) void k_salvage_scatter(SalvageWs ws, uint32_t max_frames, uint64_t* __restrict__ totals)
{
    const uint32_t n = *ws.ix.n_cand;
    const SalvageChain c = salvage_chain_in_workspace(ws);
    uint32_t mine = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        mine += salvage_scatter(ws, i, max_frames, c) ? 1u : 0u;
    mine = wave_sum_small(mine);
    if (threadIdx.x % 64 == 0 && mine)
        atomicAdd(reinterpret_cast<unsigned long long*>(totals), (unsigned long long)mine);
}

__global__ __launch_bounds__(kSalvageThreads) void k_salvage_records(SalvageWs ws, uint32_t cap_words, sela_hip_salvaged* __restrict__ records,
    uint64_t* __restrict__ totals, uint64_t* __restrict__ frame_offsets)
{
    const uint32_t count = (uint32_t)totals[0]; // k_salvage_scatter's
    uint32_t mine = 0;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < count; r += gridDim.x * blockDim.x)
        mine += salvage_record(ws, r, count, cap_words, records, totals, frame_offsets) ? 1u : 0u;
    mine = wave_sum_small(mine);
    if (threadIdx.x % 64 == 0 && mine)
        atomicAdd(reinterpret_cast<unsigned long long*>(totals + 1), (unsigned long long)mine);
}

__global__ __launch_bounds__(kSalvageThreads) void k_salvage_copy(const uint32_t* __restrict__ payload, uint32_t* __restrict__ out, SalvageWs ws,
    const uint64_t* __restrict__ totals)
{
    __shared__ uint32_t ends[2];
    const uint32_t limit = *ws.copy_words; // whole frames inside out_cap, and never more than the payload's words
    const uint32_t d0 = blockIdx.x * kSalvageChunk;
    if (d0 >= limit)
        return;
    const uint32_t len = min(limit - d0, kSalvageChunk), count = (uint32_t)totals[0];
    if (threadIdx.x == 0)
        ends[0] = salvage_frame_of(ws.r_dst, 0, count - 1, d0);
    if (threadIdx.x == 64)
        ends[1] = salvage_frame_of(ws.r_dst, 0, count - 1, d0 + len - 1);
    __syncthreads();
    const uint32_t r0 = ends[0], r1 = ends[1];
    const uint32_t shift = ws.r_pos[r0] - ws.r_dst[r0];
    uint32_t* const dst = out + d0;
    if (shift == ws.r_pos[r1] - ws.r_dst[r1]) { // the shift never decreases along the ranks: the same at both ends, the same between
        const uint32_t* const src = payload + d0 + shift;
        uint32_t done = 0;
        if ((((uintptr_t)src ^ (uintptr_t)dst) & 15) == 0) { // they agree modulo 16: dwords up to the next 16-byte line, then lines
            const uint32_t lead = min(len, (uint32_t)(0 - ((uintptr_t)dst >> 2)) & 3u), quads = (len - lead) / 4;
            if (threadIdx.x < lead)
                dst[threadIdx.x] = src[threadIdx.x];
            for (uint32_t k = threadIdx.x; k < quads; k += kSalvageThreads)
                reinterpret_cast<uint4*>(dst + lead)[k] = reinterpret_cast<const uint4*>(src + lead)[k];
            done = lead + quads * 4;
        }
        for (uint32_t k = done + threadIdx.x; k < len; k += kSalvageThreads)
            dst[k] = src[k];
        return;
    }
    for (uint32_t k = threadIdx.x; k < len; k += kSalvageThreads) { // a gap inside: each word from its own frame
        const uint32_t d = d0 + k, r = salvage_frame_of(ws.r_dst, r0, r1, d);
        dst[k] = payload[ws.r_pos[r] + (d - ws.r_dst[r])];
    }
}

size_t salvage_workspace_bytes(uint64_t payload_bytes, uint32_t max_frames, Carve* at)
{
    return measured(at, [&](Carve& c) { carve_salvage(c, payload_bytes / 4, max_frames); });
}

hipError_t launch_salvage_clear(uint64_t* d_totals, uint64_t* d_frame_offsets, hipStream_t stream)
{
    hipLaunchKernelGGL(k_salvage_clear, dim3(1), dim3(64), 0, stream, d_totals, d_frame_offsets);
    return hipGetLastError();
}

hipError_t launch_salvage_chain(const SalvageWs& ws, uint32_t blocks, uint32_t limit, uint32_t grid_items, uint32_t max_frames, uint64_t* d_totals,
    uint64_t* d_frame_offsets, hipStream_t stream)
{
    hipLaunchKernelGGL(k_salvage_block_suffix, dim3(1), dim3(1024), 0, stream, ws, blocks, d_totals, d_frame_offsets);
    uint32_t rounds = 0;
    while (rounds < 32 && (1ull << rounds) < max_frames)
        rounds++;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(kSalvageBlocks, ((uint64_t)grid_items + kSalvageThreads - 1) / kSalvageThreads);
    hipLaunchKernelGGL(k_salvage_succ, dim3(grid), dim3(kSalvageThreads), 0, stream, ws, limit);
    for (uint32_t r = 0; r < rounds; r++)
        hipLaunchKernelGGL(k_salvage_round, dim3(grid), dim3(kSalvageThreads), 0, stream, ws, r, max_frames, r & 1u, r + 1 < rounds ? 1u : 0u);
    hipLaunchKernelGGL(k_salvage_scatter, dim3(grid), dim3(kSalvageThreads), 0, stream, ws, max_frames, d_totals);
    return hipGetLastError();
}

// Everything on `stream`, nothing waited for.  The caller has checked the arguments (payload and out 4-byte aligned and apart,
// payload below 16 GiB, channels 1..255, workspace of salvage_workspace_bytes()).
hipError_t launch_salvage(const uint8_t* d_payload, uint64_t payload_bytes, uint32_t max_frames, uint32_t channels, sela_hip_salvaged* d_records,
    uint64_t* d_totals, uint8_t* d_out, uint64_t out_cap, uint64_t* d_frame_offsets, void* d_workspace, hipStream_t stream)
{
    const uint32_t words = (uint32_t)(payload_bytes / 4), blocks = (uint32_t)(((uint64_t)words + kSalvageChunk - 1) / kSalvageChunk);
    Carve carve(d_workspace);
    const SalvageWs ws = carve_salvage(carve, words, max_frames);
    if (blocks == 0 || max_frames == 0)
        return launch_salvage_clear(d_totals, d_frame_offsets, stream);
    hipError_t e = launch_index_candidates(d_payload, payload_bytes, channels, ws.ix, ws.scan_offsets, ws.scan_count, stream);
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_salvage_links, dim3(blocks), dim3(kSalvageThreads), 0, stream, ws, words);
    e = launch_salvage_chain(ws, blocks, words, words, max_frames, d_totals, d_frame_offsets, stream);
    if (e != hipSuccess)
        return e;
    const uint32_t cap_words = d_out ? (uint32_t)std::min<uint64_t>(out_cap / 4, words) : 0u; // (the taken frames are no more than the payload)
    const uint32_t grid = (uint32_t)std::min<uint64_t>(kSalvageBlocks, ((uint64_t)words + kSalvageThreads - 1) / kSalvageThreads);
    hipLaunchKernelGGL(k_salvage_records, dim3(grid), dim3(kSalvageThreads), 0, stream, ws, cap_words, d_records, d_totals, d_frame_offsets);
    if (cap_words)
        hipLaunchKernelGGL(k_salvage_copy, dim3((uint32_t)(((uint64_t)cap_words + kSalvageChunk - 1) / kSalvageChunk)), dim3(kSalvageThreads), 0, stream,
            reinterpret_cast<const uint32_t*>(d_payload), reinterpret_cast<uint32_t*>(d_out), ws, d_totals);
    return hipGetLastError();
}

} // namespace sela
