// sela_salvage_unaligned.hip -- the frames of a DAMAGED .sela payload found at ANY BYTE on the device, and copied back to back
// (sela_hip_salvage_frames_unaligned_device, sela_hip_salvage_payload_unaligned_device).  DESIGN.md 5.33.
//
// The rule is the host walk's (sela_salvage_walk_unaligned.h): sela_salvage.hip's with "word" replaced by "byte".  A frame is a
// multiple of 4 bytes long but may START at any byte once bytes were inserted or deleted in front of it.  The sync word
// (00 FF 55 AA) cannot overlap itself, so at most ONE candidate starts inside any aligned word of the payload, and a candidate
// needs 16 bytes at the least: the workspace stays sela_salvage.hip's, one entry per WORD, with pos[], next[], the gaps and
// r_pos[], r_end[], r_dst[] counted in BYTES and map[] indexed by pos >> 2 (and confirmed by pos[] == the byte, as before).
//
//   k_salvage_ua_candidates the index's candidates kernel with four phases per word: word w and its successor (a second
//                           coalesced load, which the caches serve) give the four dwords that start inside w through one
//                           v_alignbyte_b32 each; a hit walks its headers with the BYTE reader (hits are rare).  A sync word that
//                           straddles two threads', two waves' or two workgroups' words belongs to the word it starts in and is
//                           seen there alone.  The payload's last partial word is put together from its bytes: no dword is
//                           read that reaches past the payload;
//   k_index_scan            the index's own (launch_index_scan);
//   k_salvage_ua_compact    k_index_compact with map[pos >> 2];
//   k_salvage_ua_links      k_salvage_links with map[end >> 2], and "confirmed" where fewer than 4 bytes lie behind the end;
//   block suffix, succ, rounds, scatter
//                           sela_salvage.hip's kernels as they are (launch_salvage_chain): they never ask what a position counts;
//   k_salvage_ua_records    k_salvage_records on bytes;
//   k_salvage_ua_copy       cut by 4096 DESTINATION words as k_salvage_copy is (frames are multiples of 4 bytes, so the compacted
//                           payload is made of whole words); the shift between source and destination is a byte count.  A
//                           workgroup whose run has one shift copies straight: as k_salvage_copy where the shift is a multiple
//                           of 4 (16-byte lines where source and destination agree modulo 16), else two aligned dword loads and
//                           a funnel shift per word; a workgroup with a gap inside looks each word up.
#include "sela_salvage_steps.h"

namespace sela {

// Word w of the payload: an aligned dword where the payload holds all of it, the bytes it has (zeros above them) where it is
// the last, partial one, and 0 behind that.  Zeros never complete a sync word: its three upper bytes are not 0.
__device__ __forceinline__ uint32_t ua_word(const uint8_t* __restrict__ payload, uint32_t bytes, uint32_t w)
{
    const uint32_t whole = bytes >> 2;
    if (w < whole)
        return reinterpret_cast<const uint32_t*>(payload)[w];
    uint32_t v = 0;
    if (w == whole)
        for (uint32_t t = 0; t < (bytes & 3u); t++)
            v |= (uint32_t)payload[(uint64_t)whole * 4 + t] << (8 * t);
    return v;
}

// The host walk's test of one byte position that holds the sync word: the frame's end in bytes, or 0.
__device__ __forceinline__ uint32_t ua_frame_end(const uint8_t* __restrict__ payload, uint32_t bytes, uint32_t off, uint32_t channels)
{
    uint64_t p = (uint64_t)off + 4;
    for (uint32_t c = 0; c < channels && p; c++) {
        SelaSubframeHeader h;
        p = sela_subframe_read_bytes(payload, bytes, p, &h);
    }
    return (uint32_t)p; // (at most `bytes`, which is below 2^32)
}

__global__ __launch_bounds__(kIndexThreads) void k_salvage_ua_candidates(const uint8_t* __restrict__ payload, uint32_t bytes, uint32_t words,
    uint32_t channels, IndexWs ws)
{
    __shared__ uint32_t wave_counts[kIndexWordsPerThread * (kIndexThreads / 64)];
    const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    const uint32_t base = blockIdx.x * kIndexChunkWords;
    // Word base + k * 256 + threadIdx.x, and the one behind it: in position order (k, wave, lane), every load one coalesced KiB
    // per wave.  (A candidate needs 16 bytes, so none starts in a word at or behind `words` = bytes / 4.)
    uint32_t cur[kIndexWordsPerThread], nxt[kIndexWordsPerThread];
#pragma unroll
    for (int k = 0; k < kIndexWordsPerThread; k++) {
        const uint32_t w = base + (uint32_t)k * kIndexThreads + threadIdx.x;
        cur[k] = w < words ? ua_word(payload, bytes, w) : 0u;
        nxt[k] = w < words ? ua_word(payload, bytes, w + 1) : 0u;
    }
    uint32_t pos[kIndexWordsPerThread], end[kIndexWordsPerThread];
    uint64_t hit[kIndexWordsPerThread];
#pragma unroll
    for (int k = 0; k < kIndexWordsPerThread; k++) {
        const uint32_t w = base + (uint32_t)k * kIndexThreads + threadIdx.x;
        uint32_t phase = 4; // at most one of the four matches
        phase = cur[k] == SELA_SYNC_WORD ? 0u : phase;
        phase = __builtin_amdgcn_alignbyte(nxt[k], cur[k], 1) == SELA_SYNC_WORD ? 1u : phase;
        phase = __builtin_amdgcn_alignbyte(nxt[k], cur[k], 2) == SELA_SYNC_WORD ? 2u : phase;
        phase = __builtin_amdgcn_alignbyte(nxt[k], cur[k], 3) == SELA_SYNC_WORD ? 3u : phase;
        pos[k] = w * 4 + phase;
        end[k] = phase < 4 ? ua_frame_end(payload, bytes, pos[k], channels) : 0u;
        hit[k] = __ballot(end[k] != 0);
        if (lane == 0)
            wave_counts[k * (kIndexThreads / 64) + wave] = (uint32_t)__popcll(hit[k]);
    }
    __syncthreads();
    if (wave == 0) { // the 64 (k, wave) counts in position order: one per lane
        const uint32_t c = wave_counts[lane];
        const uint32_t ex = wave_exclusive_scan(c, lane);
        wave_counts[lane] = ex;
        if (lane == 63)
            ws.counts[blockIdx.x] = ex + c;
    }
    __syncthreads();
    const uint64_t below = (1ull << lane) - 1;
#pragma unroll
    for (int k = 0; k < kIndexWordsPerThread; k++)
        if (end[k] != 0) {
            const uint32_t at = base + wave_counts[k * (kIndexThreads / 64) + wave] + (uint32_t)__popcll(hit[k] & below);
            ws.stage_pos[at] = pos[k];
            ws.stage_next[at] = end[k];
        }
}

__global__ __launch_bounds__(kIndexThreads) void k_salvage_ua_compact(IndexWs ws)
{
    const uint32_t first = ws.counts[blockIdx.x], n = ws.counts[blockIdx.x + 1] - first, base = blockIdx.x * kIndexChunkWords;
    for (uint32_t k = threadIdx.x; k < n; k += kIndexThreads) {
        const uint32_t b = ws.stage_pos[base + k];
        ws.pos[first + k] = b;
        ws.next[first + k] = ws.stage_next[base + k];
        ws.map[b >> 2] = first + k;
    }
}

__global__ __launch_bounds__(kSalvageThreads) void k_salvage_ua_links(SalvageWs ws, uint32_t bytes)
{
    __shared__ uint32_t sh[kSalvageThreads / 64];
    const uint32_t n = *ws.ix.n_cand, words = bytes >> 2;
    const uint32_t first = blockIdx.x * kSalvageChunk + threadIdx.x * kSalvagePerThread; // (below 2^32: no more workgroups than words / 4096, rounded up)
    uint32_t conf[kSalvagePerThread];
#pragma unroll
    for (int k = 0; k < kSalvagePerThread; k++) {
        const uint32_t i = first + k;
        conf[k] = kIndexNone;
        if (i < n) {
            const uint32_t e = ws.ix.next[i];
            const uint32_t j = (e >> 2) < words ? ws.ix.map[e >> 2] : kIndexNone; // (map[] is read only where pos[] confirms it)
            const uint32_t direct = j < n && ws.ix.pos[j] == e ? j : kIndexNone;
            ws.ix.stage_pos[i] = direct;
            if (direct != kIndexNone || bytes - e < 4)
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

// The record of rank r < count; true where a gap lies in front of it.  The last rank also writes what is known only there.
__device__ __forceinline__ bool ua_record(const SalvageWs& ws, uint32_t r, uint32_t count, uint32_t cap_words, sela_hip_salvaged* __restrict__ records,
    uint64_t* __restrict__ totals, uint64_t* __restrict__ frame_offsets)
{
    const uint32_t p = ws.r_pos[r], e = ws.r_end[r], d = ws.r_dst[r], before = r ? ws.r_end[r - 1] : 0u;
    const uint32_t d_end = d + (e - p); // (d and e - p are multiples of 4)
    if (records) {
        sela_hip_salvaged rec;
        rec.offset = p;
        rec.skipped_before = p - before;
        rec.bytes = e - p;
        rec.reserved = 0;
        records[r] = rec;
    }
    if (frame_offsets)
        frame_offsets[r] = d;
    if (r + 1 == count) {
        if (frame_offsets)
            frame_offsets[count] = d_end;
        totals[2] = d_end;
        totals[3] = e;
    }
    // the copy writes whole frames, up to the last one that ends inside the room: one rank is that one
    if (d_end / 4 <= cap_words && (r + 1 == count || (ws.r_dst[r + 1] + (ws.r_end[r + 1] - ws.r_pos[r + 1])) / 4 > cap_words))
        *ws.copy_words = d_end / 4;
    return p != before;
}

__global__ __launch_bounds__(kSalvageThreads) void k_salvage_ua_records(SalvageWs ws, uint32_t cap_words, sela_hip_salvaged* __restrict__ records,
    uint64_t* __restrict__ totals, uint64_t* __restrict__ frame_offsets)
{
    const uint32_t count = (uint32_t)totals[0]; // k_salvage_scatter's
    uint32_t mine = 0;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < count; r += gridDim.x * blockDim.x)
        mine += ua_record(ws, r, count, cap_words, records, totals, frame_offsets) ? 1u : 0u;
    mine = wave_sum_small(mine);
    if (threadIdx.x % 64 == 0 && mine)
        atomicAdd(reinterpret_cast<unsigned long long*>(totals + 1), (unsigned long long)mine);
}

// The four bytes at byte `at` of the payload, all of them inside it: the word they start in is whole, the one behind it may
// be the last, partial one.
__device__ __forceinline__ uint32_t ua_dword_at(const uint8_t* __restrict__ payload, uint32_t bytes, uint32_t at)
{
    const uint32_t w = at >> 2, s = at & 3u, lo = reinterpret_cast<const uint32_t*>(payload)[w];
    return s ? __builtin_amdgcn_alignbyte(ua_word(payload, bytes, w + 1), lo, s) : lo;
}

__global__ __launch_bounds__(kSalvageThreads) void k_salvage_ua_copy(const uint8_t* __restrict__ payload, uint32_t bytes, uint32_t* __restrict__ out,
    SalvageWs ws, const uint64_t* __restrict__ totals)
{
    __shared__ uint32_t ends[2];
    const uint32_t limit = *ws.copy_words; // whole frames inside out_cap, and never more than the payload's words
    const uint32_t d0 = blockIdx.x * kSalvageChunk;
    if (d0 >= limit)
        return;
    const uint32_t len = min(limit - d0, kSalvageChunk), count = (uint32_t)totals[0];
    if (threadIdx.x == 0)
        ends[0] = salvage_frame_of(ws.r_dst, 0, count - 1, d0 * 4);
    if (threadIdx.x == 64)
        ends[1] = salvage_frame_of(ws.r_dst, 0, count - 1, (d0 + len - 1) * 4);
    __syncthreads();
    const uint32_t r0 = ends[0], r1 = ends[1];
    const uint32_t shift = ws.r_pos[r0] - ws.r_dst[r0]; // in bytes
    uint32_t* const dst = out + d0;
    if (shift == ws.r_pos[r1] - ws.r_dst[r1]) { // the shift never decreases along the ranks: the same at both ends, the same between
        const uint32_t* const src = reinterpret_cast<const uint32_t*>(payload) + d0 + shift / 4;
        const uint32_t phase = shift & 3u;
        if (phase) { // word k of the run lies across src[k] and src[k + 1]; the last src[k + 1] may be the payload's partial word
            const uint32_t w0 = d0 + shift / 4;
            for (uint32_t k = threadIdx.x; k < len; k += kSalvageThreads)
                dst[k] = __builtin_amdgcn_alignbyte(ua_word(payload, bytes, w0 + k + 1), src[k], phase);
            return;
        }
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
        const uint32_t d = (d0 + k) * 4, r = salvage_frame_of(ws.r_dst, r0, r1, d);
        dst[k] = ua_dword_at(payload, bytes, ws.r_pos[r] + (d - ws.r_dst[r]));
    }
}

// sela_salvage.hip's workspace as it is: a candidate needs 16 bytes and no two start in one aligned word, so payload_bytes / 4
// entries hold them at any phase.
size_t salvage_unaligned_workspace_bytes(uint64_t payload_bytes, uint32_t max_frames, Carve* at)
{
    return measured(at, [&](Carve& c) { carve_salvage(c, payload_bytes / 4, max_frames); });
}

// Everything on `stream`, nothing waited for.  The caller has checked the arguments (payload and out 4-byte aligned and apart,
// payload below 4 GiB, channels 1..255, workspace of salvage_unaligned_workspace_bytes()).
hipError_t launch_salvage_unaligned(const uint8_t* d_payload, uint64_t payload_bytes, uint32_t max_frames, uint32_t channels, sela_hip_salvaged* d_records,
    uint64_t* d_totals, uint8_t* d_out, uint64_t out_cap, uint64_t* d_frame_offsets, void* d_workspace, hipStream_t stream)
{
    const uint32_t bytes = (uint32_t)payload_bytes, words = bytes / 4, blocks = (uint32_t)(((uint64_t)words + kSalvageChunk - 1) / kSalvageChunk);
    static_assert(kSalvageChunk == kIndexChunkWords, "one workgroup count for the candidates, the compaction and the links");
    Carve carve(d_workspace);
    const SalvageWs ws = carve_salvage(carve, words, max_frames);
    if (blocks == 0 || max_frames == 0)
        return launch_salvage_clear(d_totals, d_frame_offsets, stream);
    hipLaunchKernelGGL(k_salvage_ua_candidates, dim3(blocks), dim3(kIndexThreads), 0, stream, d_payload, bytes, words, channels, ws.ix);
    hipError_t e = launch_index_scan(ws.ix, blocks, ws.scan_offsets, ws.scan_count, stream);
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_salvage_ua_compact, dim3(blocks), dim3(kIndexThreads), 0, stream, ws.ix);
    hipLaunchKernelGGL(k_salvage_ua_links, dim3(blocks), dim3(kSalvageThreads), 0, stream, ws, bytes);
    e = launch_salvage_chain(ws, blocks, bytes, words, max_frames, d_totals, d_frame_offsets, stream);
    if (e != hipSuccess)
        return e;
    const uint32_t cap_words = d_out ? (uint32_t)std::min<uint64_t>(out_cap / 4, words) : 0u; // (the taken frames are no more than the payload)
    const uint32_t grid = (uint32_t)std::min<uint64_t>(kSalvageBlocks, ((uint64_t)words + kSalvageThreads - 1) / kSalvageThreads);
    hipLaunchKernelGGL(k_salvage_ua_records, dim3(grid), dim3(kSalvageThreads), 0, stream, ws, cap_words, d_records, d_totals, d_frame_offsets);
    if (cap_words)
        hipLaunchKernelGGL(k_salvage_ua_copy, dim3((uint32_t)(((uint64_t)cap_words + kSalvageChunk - 1) / kSalvageChunk)), dim3(kSalvageThreads), 0, stream,
            d_payload, bytes, reinterpret_cast<uint32_t*>(d_out), ws, d_totals);
    return hipGetLastError();
}

} // namespace sela
