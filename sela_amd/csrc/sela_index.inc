// sela_index.inc -- the frames of a .sela payload found on the device (sela_hip_index_frames_device; included by
// sela_decode.hip inside namespace sela).  DESIGN.md 5.10.
//
// The host walk (sela_hip_index_frames) follows the chain offset 0 -> end of frame 0 -> end of frame 1 -> ...; a frame's size
// is known only from its `channels` subframe headers, so the chain is sequential.  Here it is taken apart:
//
//   k_index_candidates  every payload word that holds the sync word and whose header walk succeeds (the host walk's
//                       reader and bounds, sela_format.h) is a CANDIDATE; its `next` is the end of the frame it would be.
//                       Frames are 4-byte aligned relative to the payload (4 + 12 per subframe + 4 per word), so only
//                       words are looked at.
//                       Each workgroup lists its candidates in position order in its own stretch of the workspace and
//                       counts them;
//   k_index_scan        one workgroup: exclusive scan of the counts (and the outputs' initial state: no frame found);
//   k_index_compact     the lists, packed in position order: pos[i], next[i], and map[pos[i]] = i;
//   links               succ[i] = the candidate at next[i], or none (map[] is read only where pos[] confirms it, so the rest
//                       of map[] is never initialised);
//   rounds              reach from offset 0 by doubling: in round j every node reached with rank r < 2^j marks
//                       jump_j(node) with rank r + 2^j, and jump_{j+1} = jump_j o jump_j (ping-ponged).  Positions strictly
//                       increase along a chain, so each frame is reached once and its rank is its index.  A false candidate
//                       (a sync word inside Rice data) is never reached from offset 0 even when its `next` lands on a true
//                       frame: ranking from the head, not from the tails, keeps merging chains apart;
//   scatter             frame_offsets[r + 1] = byte position of next[node] for every reached node of rank r < max_frames,
//                       *n_frames = how many there are; frame_offsets[0] = 0 from the scan.  That is what the host walk
//                       leaves: [found] is the end of the last frame found (where it stopped, or where the cap stopped it).
//
// links + rounds + scatter run in ONE workgroup, on LDS, when max_frames <= kIndexOneGroupFrames (a track; four launches in
// all), and as 2 + ceil(log2(max_frames)) launches over the whole device otherwise.
// (kIndexNone, the candidates kernel's shape, IndexWs and carve_index: sela_host.h, for sela_salvage.hip's sake)
constexpr int kIndexScanThreads = 1024;
constexpr uint32_t kIndexOneGroupFrames = 4096;  // max_frames up to this: links, rounds and scatter in one workgroup
constexpr uint32_t kIndexOneGroupNodes = 5120;   // ... on LDS while the candidates fit (12 bytes each: 60 KiB); beyond, in the workspace
constexpr int kIndexLinkBlocks = 1024;           // grid of the device-wide link / round / scatter launches (grid-stride)

// The host walk's test of one position (sela_hip_index_frames): the frame's end in words, or kIndexNone.  `off` is a word
// boundary that holds the sync word, so every subframe of the frame is one too: the word form of the header reader, whose
// bounds are the host walk's (only the word counts are used: the other loads fold away).
__device__ __forceinline__ uint32_t index_frame_end(const uint8_t* __restrict__ payload, uint64_t bytes, uint64_t off, uint32_t channels)
{
    uint64_t p = off + 4;
    for (uint32_t c = 0; c < channels && p; c++) {
        SelaSubframeHeader h;
        p = sela_subframe_read_words(payload, bytes, p, &h);
    }
    return p ? (uint32_t)(p >> 2) : kIndexNone;
}

// Exclusive scan of one value per thread over the workgroup (totals fit 32 bits).  sh: 17 words of LDS.
__device__ __forceinline__ uint32_t index_block_scan(uint32_t v, uint32_t* sh, uint32_t& total)
{
    const int lane = threadIdx.x % 64, wave = threadIdx.x / 64, n_waves = blockDim.x / 64;
    const uint32_t ex = wave_exclusive_scan(v, lane);
    if (lane == 63)
        sh[wave] = ex + v;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (int w = 0; w < n_waves; w++) {
            const uint32_t t = sh[w];
            sh[w] = run;
            run += t;
        }
        sh[16] = run;
    }
    __syncthreads();
    const uint32_t out = ex + sh[wave];
    total = sh[16];
    __syncthreads();
    return out;
}

__global__ __launch_bounds__(kIndexThreads) void k_index_candidates(const uint8_t* __restrict__ payload, uint64_t bytes, uint32_t words,
    uint32_t channels, IndexWs ws)
{
    __shared__ uint32_t wave_counts[kIndexWordsPerThread * (kIndexThreads / 64)];
    const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    const uint32_t base = blockIdx.x * kIndexChunkWords;
    const uint32_t* const pw = reinterpret_cast<const uint32_t*>(payload);
    // Word base + k * 256 + threadIdx.x: in position order (k, wave, lane), every load one coalesced KiB per wave.
    uint32_t sync[kIndexWordsPerThread];
#pragma unroll
    for (int k = 0; k < kIndexWordsPerThread; k++) {
        const uint32_t w = base + (uint32_t)k * kIndexThreads + threadIdx.x;
        sync[k] = w < words ? pw[w] : 0u;
    }
    uint32_t next[kIndexWordsPerThread];
    uint64_t hit[kIndexWordsPerThread];
#pragma unroll
    for (int k = 0; k < kIndexWordsPerThread; k++) {
        const uint32_t w = base + (uint32_t)k * kIndexThreads + threadIdx.x;
        next[k] = sync[k] == SELA_SYNC_WORD ? index_frame_end(payload, bytes, (uint64_t)w * 4, channels) : kIndexNone;
        hit[k] = __ballot(next[k] != kIndexNone);
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
        if (next[k] != kIndexNone) {
            const uint32_t at = base + wave_counts[k * (kIndexThreads / 64) + wave] + (uint32_t)__popcll(hit[k] & below);
            ws.stage_pos[at] = base + (uint32_t)k * kIndexThreads + threadIdx.x;
            ws.stage_next[at] = next[k];
        }
}

// One workgroup: counts[0 .. blocks) -> their exclusive scan, counts[blocks] = *n_cand = the total; no frame found yet.
__global__ __launch_bounds__(kIndexScanThreads) void k_index_scan(IndexWs ws, uint32_t blocks, uint64_t* __restrict__ frame_offsets,
    uint32_t* __restrict__ n_frames)
{
    __shared__ uint32_t sh[17];
    constexpr uint32_t kPer = 8;
    uint32_t carry = 0;
    for (uint32_t tile = 0; tile < blocks; tile += kIndexScanThreads * kPer) {
        const uint32_t first = tile + threadIdx.x * kPer;
        uint32_t v[kPer], sum = 0;
#pragma unroll
        for (uint32_t k = 0; k < kPer; k++) {
            v[k] = first + k < blocks ? ws.counts[first + k] : 0u;
            sum += v[k];
        }
        uint32_t total;
        uint32_t run = carry + index_block_scan(sum, sh, total);
#pragma unroll
        for (uint32_t k = 0; k < kPer; k++)
            if (first + k < blocks) {
                ws.counts[first + k] = run;
                run += v[k];
            }
        carry += total;
    }
    if (threadIdx.x == 0) {
        ws.counts[blocks] = carry;
        *ws.n_cand = carry;
        frame_offsets[0] = 0;
        *n_frames = 0;
    }
}

__global__ __launch_bounds__(kIndexThreads) void k_index_compact(IndexWs ws)
{
    const uint32_t first = ws.counts[blockIdx.x], n = ws.counts[blockIdx.x + 1] - first, base = blockIdx.x * kIndexChunkWords;
    for (uint32_t k = threadIdx.x; k < n; k += kIndexThreads) {
        const uint32_t w = ws.stage_pos[base + k];
        ws.pos[first + k] = w;
        ws.next[first + k] = ws.stage_next[base + k];
        ws.map[w] = first + k;
    }
}

// ---- the per-node steps, shared by the one-workgroup kernel and the device-wide launches --------------------------------
__device__ __forceinline__ void index_link(const IndexWs& ws, uint32_t i, uint32_t n_cand, uint32_t words, uint32_t* jump, uint32_t* rank)
{
    const uint32_t w = ws.next[i];
    const uint32_t j = w < words ? ws.map[w] : kIndexNone;
    jump[i] = j < n_cand && ws.pos[j] == w ? j : kIndexNone;
    rank[i] = i == 0 && ws.pos[0] == 0 ? 0u : kIndexNone; // the head: a frame at offset 0
}

// Round `round`: ranks below 2^round are final; mark those 2^round further on (only below max_frames: nothing else is
// asked for, and so no rank reaches kIndexNone), and compose the jump unless it is the last round.
__device__ __forceinline__ void index_round(uint32_t i, uint32_t round, uint32_t max_frames, const uint32_t* cur, uint32_t* nxt, uint32_t* rank,
    bool compose)
{
    const uint32_t t = cur[i], r = rank[i], step = 1u << round;
    if (t != kIndexNone && r < step && (uint64_t)r + step < max_frames)
        rank[t] = r + step;
    if (compose)
        nxt[i] = t == kIndexNone ? kIndexNone : cur[t];
}

__device__ __forceinline__ bool index_scatter(const IndexWs& ws, uint32_t i, uint32_t max_frames, const uint32_t* rank, uint64_t* frame_offsets)
{
    const uint32_t r = rank[i];
    if (r >= max_frames)
        return false;
    frame_offsets[(size_t)r + 1] = (uint64_t)ws.next[i] * 4;
    return true;
}

__global__ __launch_bounds__(1024) void k_index_chain_one_group(IndexWs ws, uint32_t words, uint32_t max_frames, uint32_t rounds,
    uint64_t* __restrict__ frame_offsets, uint32_t* __restrict__ n_frames)
{
    __shared__ uint32_t lds[3 * kIndexOneGroupNodes];
    __shared__ uint32_t found;
    const uint32_t n = *ws.n_cand;
    const bool on_chip = n <= kIndexOneGroupNodes;
    uint32_t* cur = on_chip ? lds : ws.stage_pos;
    uint32_t* nxt = on_chip ? lds + kIndexOneGroupNodes : ws.stage_next;
    uint32_t* const rank = on_chip ? lds + 2 * kIndexOneGroupNodes : ws.rank;
    if (threadIdx.x == 0)
        found = 0;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x)
        index_link(ws, i, n, words, cur, rank);
    __syncthreads();
    for (uint32_t r = 0; r < rounds; r++) {
        for (uint32_t i = threadIdx.x; i < n; i += blockDim.x)
            index_round(i, r, max_frames, cur, nxt, rank, r + 1 < rounds);
        __syncthreads();
        uint32_t* const t = cur;
        cur = nxt, nxt = t;
    }
    uint32_t mine = 0;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x)
        mine += index_scatter(ws, i, max_frames, rank, frame_offsets) ? 1u : 0u;
    if (mine)
        atomicAdd(&found, mine);
    __syncthreads();
    if (threadIdx.x == 0)
        *n_frames = found;
}

__global__ __launch_bounds__(kIndexThreads) void k_index_links(IndexWs ws, uint32_t words)
{
    const uint32_t n = *ws.n_cand;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        index_link(ws, i, n, words, ws.stage_pos, ws.rank);
}

__global__ __launch_bounds__(kIndexThreads) void k_index_round(IndexWs ws, uint32_t round, uint32_t max_frames, const uint32_t* cur, uint32_t* nxt,
    uint32_t compose)
{
    const uint32_t n = *ws.n_cand;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        index_round(i, round, max_frames, cur, nxt, ws.rank, compose != 0);
}

__global__ __launch_bounds__(kIndexThreads) void k_index_scatter(IndexWs ws, uint32_t max_frames, uint64_t* __restrict__ frame_offsets,
    uint32_t* __restrict__ n_frames)
{
    const uint32_t n = *ws.n_cand;
    uint32_t mine = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        mine += index_scatter(ws, i, max_frames, ws.rank, frame_offsets) ? 1u : 0u;
    mine = wave_sum_small(mine);
    if (threadIdx.x % 64 == 0 && mine)
        atomicAdd(n_frames, mine);
}

size_t index_workspace_bytes(uint64_t payload_bytes, Carve* at)
{
    return measured(at, [&](Carve& c) { carve_index(c, payload_bytes / 4); });
}

// Everything on `stream`, nothing waited for.  The caller has checked the arguments (payload 4-byte aligned and below 16 GiB,
// channels 1..255, workspace of index_workspace_bytes()).
hipError_t launch_index(const uint8_t* d_payload, uint64_t payload_bytes, uint32_t max_frames, uint32_t channels, uint64_t* d_frame_offsets,
    uint32_t* d_n_frames, void* d_workspace, hipStream_t stream)
{
    const uint32_t words = (uint32_t)(payload_bytes / 4), blocks = (uint32_t)(((uint64_t)words + kIndexChunkWords - 1) / kIndexChunkWords);
    Carve carve(d_workspace);
    const IndexWs ws = carve_index(carve, words);
    uint32_t rounds = 0;
    while (rounds < 32 && (1ull << rounds) < max_frames)
        rounds++;
    if (blocks)
        hipLaunchKernelGGL(k_index_candidates, dim3(blocks), dim3(kIndexThreads), 0, stream, d_payload, payload_bytes, words, channels, ws);
    hipLaunchKernelGGL(k_index_scan, dim3(1), dim3(kIndexScanThreads), 0, stream, ws, blocks, d_frame_offsets, d_n_frames);
    if (blocks == 0 || max_frames == 0)
        return hipGetLastError();
    hipLaunchKernelGGL(k_index_compact, dim3(blocks), dim3(kIndexThreads), 0, stream, ws);
    if (max_frames <= kIndexOneGroupFrames) {
        hipLaunchKernelGGL(k_index_chain_one_group, dim3(1), dim3(1024), 0, stream, ws, words, max_frames, rounds, d_frame_offsets, d_n_frames);
        return hipGetLastError();
    }
    const uint32_t grid = (uint32_t)std::min<uint64_t>(kIndexLinkBlocks, ((uint64_t)words + kIndexThreads - 1) / kIndexThreads);
    hipLaunchKernelGGL(k_index_links, dim3(grid), dim3(kIndexThreads), 0, stream, ws, words);
    uint32_t* cur = ws.stage_pos;
    uint32_t* nxt = ws.stage_next;
    for (uint32_t r = 0; r < rounds; r++) {
        hipLaunchKernelGGL(k_index_round, dim3(grid), dim3(kIndexThreads), 0, stream, ws, r, max_frames, cur, nxt, r + 1 < rounds ? 1u : 0u);
        std::swap(cur, nxt);
    }
    hipLaunchKernelGGL(k_index_scatter, dim3(grid), dim3(kIndexThreads), 0, stream, ws, max_frames, d_frame_offsets, d_n_frames);
    return hipGetLastError();
}

// The first three launches alone, for sela_salvage.hip (sela_host.h): the candidates of a payload of words > 0 words, packed.
hipError_t launch_index_candidates(const uint8_t* d_payload, uint64_t payload_bytes, uint32_t channels, const IndexWs& ws, uint64_t* d_frame_offsets,
    uint32_t* d_n_frames, hipStream_t stream)
{
    const uint32_t words = (uint32_t)(payload_bytes / 4), blocks = (uint32_t)(((uint64_t)words + kIndexChunkWords - 1) / kIndexChunkWords);
    hipLaunchKernelGGL(k_index_candidates, dim3(blocks), dim3(kIndexThreads), 0, stream, d_payload, payload_bytes, words, channels, ws);
    hipLaunchKernelGGL(k_index_scan, dim3(1), dim3(kIndexScanThreads), 0, stream, ws, blocks, d_frame_offsets, d_n_frames);
    hipLaunchKernelGGL(k_index_compact, dim3(blocks), dim3(kIndexThreads), 0, stream, ws);
    return hipGetLastError();
}

// k_index_scan alone, for sela_salvage_unaligned.hip (sela_host.h): the exclusive scan of counts[0 .. blocks), and *n_cand.
hipError_t launch_index_scan(const IndexWs& ws, uint32_t blocks, uint64_t* d_frame_offsets, uint32_t* d_n_frames, hipStream_t stream)
{
    hipLaunchKernelGGL(k_index_scan, dim3(1), dim3(kIndexScanThreads), 0, stream, ws, blocks, d_frame_offsets, d_n_frames);
    return hipGetLastError();
}
