// sela_digest.hip -- the CRC-32 (IEEE 802.3, zlib.crc32) of the PCM a .sela stream decodes to, on the device: per frame the CRC of
// the bytes sela_hip_decode_n_device would write, and the track's from those (gfx950).  The launches are the int16
// family's sequence (launch_n_sequence, sela_generic.hip); launch_digest_n_device plugs in
//
//   k_digest_frames   the fused kernel: k_level_frames (sela_levels.hip) with the CRC where the reduction is.  One workgroup per
//                     frame, one wave per subframe: frame_prologue and decode_subframe of sela_decode_core.inc, the barrier, then
//                     the shared second pass -- and where the decoder stores a frame's interleaved int16 samples, this kernel runs
//                     them through the CRC in registers.  No decoded sample reaches global memory; the LDS plan is the decoder's.
//   k_digest_pcm      the raw CRC of a contiguous byte range in global memory, one workgroup per (frame, slice): the routes that are
//                     not fused (frames of any other length, frames of more than eight channels), and sela_hip_crc32_device.
//   k_digest_slices   a frame's slices folded into its record (or sela_hip_crc32_device's two words).
//   k_digest_fold, k_digest_track   the track: the XOR over f of crc_f * x^(8 * bytes behind frame f).
//
// A CRC is ordered, so the lanes, waves and slices are put together by the shift identity of sela_crc32.h: a piece's raw CRC
// times x^(8 * bytes behind it), XORed -- the lanes' and waves' side of it is sela_crc32_lanes.h, which the digest of the 24- and
// 32-bit family (sela_digest_pcm.hip, 5.29) shares; that call also runs the three folds here, with its own bytes per value.
#include "sela_host.h"

#include "sela_crc32_lanes.h"
#include "sela_synth.h"

namespace sela {

#include "sela_decode_core.inc"

static_assert(kVerifyFusedChannels == (uint32_t)kDecMaxWaves, "the fused route takes what k_decode_frames takes");
static_assert(sizeof(struct sela_hip_digest) == 8 && alignof(struct sela_hip_digest) == 4, "the record of include/sela_hip.h");
static_assert(offsetof(struct sela_hip_digest, crc32) == 0 && offsetof(struct sela_hip_digest, samples) == 4, "a record leaves as one 8-byte word");

// The fused kernel's shapes by channels: mono takes four samples a piece, stereo stereo_words' four of both channels, more
// channels one sample of every channel.
constexpr uint32_t fused_piece_samples(uint32_t channels) { return channels <= 2 ? 4u : 1u; }
constexpr DigestShape fused_shape(uint32_t channels)
{
    const uint32_t g = fused_piece_samples(channels);
    return digest_shape(2 * channels * g, 64 * (channels < (uint32_t)kDecMaxWaves ? channels : (uint32_t)kDecMaxWaves), (uint32_t)kBlock / g);
}
constexpr DigestShape kFusedShapes[kDecMaxWaves + 1] = { DigestShape{}, fused_shape(1), fused_shape(2), fused_shape(3), fused_shape(4), fused_shape(5), fused_shape(6),
    fused_shape(7), fused_shape(8) };
static_assert(kFusedShapes[2].pad == 0 && kFusedShapes[2].steps == 4 && kFusedShapes[3].pad == 11 * 192 - 2048, "pieces and threads");

__global__ __launch_bounds__(kDecMaxWaves * 64) __attribute__((amdgpu_waves_per_eu(7, 8))) void k_digest_frames(const uint8_t* __restrict__ frames,
    const uint64_t* __restrict__ frame_offsets, uint32_t n_frames, uint32_t channels, struct sela_hip_digest* __restrict__ digests /* [n_frames] */,
    uint32_t* __restrict__ status, int32_t* __restrict__ ws_residues, uint32_t vec_shift_from /* as in k_decode_frames */,
    uint32_t synth_priorities /* as in k_decode_frames */, const uint32_t* __restrict__ n_frames_found /* or null: frames from *n_frames_found on are left alone */,
    const DigestShape shape)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    const int n_waves = blockDim.x / 64;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / 64)), lane = threadIdx.x % 64;
    const DecFrameLds l = carve_frame_lds(dyn, channels, n_waves);

    const uint32_t f = blockIdx.x;
    if (f >= n_frames || (n_frames_found && f >= *n_frames_found))
        return;
    const bool vec_shift = f >= vec_shift_from;
    const uint8_t* const fb = frames + frame_offsets[f];
    const uint64_t fbytes = frame_offsets[f + 1] - frame_offsets[f];
    uint32_t flags = 0;
    SubHeader hd;
    bool ok;
    const bool fast = frame_prologue(l, fb, fbytes, channels, n_waves, wave, lane, hd, ok);

    for (uint32_t c = wave; c < channels; c += n_waves) {
        if (c != (uint32_t)wave) {
            hd = walk_headers(fb, fbytes, c);
            ok = block_header_ok(hd, channels);
        }
        if (!ok) {
            flags |= SELA_HIP_FLAG_BAD_FRAME;
            continue;
        }
        decode_subframe<false>(fb, fbytes, hd, fast, l.sub + c, l.scratch0 + wave, ws_residues, (size_t)f * channels + c, vec_shift, synth_priorities, lane, flags, nullptr);
        if (lane == 0)
            l.sub_info[hd.channel] = sub_info_word(hd.type, hd.parent, c);
    }
    __syncthreads();

    // ---- the second pass, digested instead of stored ------------------------------------------------------------------
    // What k_decode_frames would write at pcm_out[(f * 2048 + i) * channels + c], in that order, is cut into pieces; thread t
    // takes pieces t - pad, t - pad + T, ... (the pieces below 0 are empty: a register of 0 stays 0).
    uint32_t r = 0;
    if (channels == 2) {
        const StereoPass sp = stereo_pass(l.sub, l.sub_info);
        for (uint32_t i4 = threadIdx.x, j = 0; i4 < (uint32_t)kBlock / 4; i4 += blockDim.x, j++) {
            const uint4 w = stereo_words(sp, i4);
            if (j)
                r = crc_mul(r, shape.stride);
            r = crc_step32(crc_step32(crc_step32(crc_step32(r, w.x), w.y), w.z), w.w);
        }
    } else if (channels == 1) {
        for (uint32_t i4 = threadIdx.x, j = 0; i4 < (uint32_t)kBlock / 4; i4 += blockDim.x, j++) {
            uint32_t v[4];
#pragma unroll
            for (uint32_t k = 0; k < 4; k++)
                v[k] = channel_value16(l.sub, l.sub_info, 0, 4 * i4 + k);
            if (j)
                r = crc_mul(r, shape.stride);
            r = crc_step32(crc_step32(r, v[0] | (v[1] << 16)), v[2] | (v[3] << 16));
        }
    } else {
        for (uint32_t j = 0; j < shape.steps; j++) {
            const int32_t i = (int32_t)(threadIdx.x + j * blockDim.x) - (int32_t)shape.pad;
            if (j)
                r = crc_mul(r, shape.stride);
            if (i < 0)
                continue;
            uint32_t c = 0;
            for (; c + 1 < channels; c += 2)
                r = crc_step32(r, channel_value16(l.sub, l.sub_info, c, (uint32_t)i) | (channel_value16(l.sub, l.sub_info, c + 1, (uint32_t)i) << 16));
            if (c < channels)
                r = crc_step16(r, channel_value16(l.sub, l.sub_info, c, (uint32_t)i));
        }
    }
    r = wave_crc(r, shape);
    // the waves' words go into their synthesis tables, dead behind the barrier above
    if (lane == 0)
        *reinterpret_cast<uint32_t*>(&l.scratch0[wave].t) = r;
    if (threadIdx.x == 0)
        flags |= layout_flags(l.sub_info, channels);
    flags = wave_or(flags);
    if (lane == 0 && flags) {
        atomicOr(&status[0], flags);
        if (wave == 0 && (flags & SELA_HIP_FLAG_BAD_FRAME))
            atomicAdd(&status[1], 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t raw = 0;
        for (int w = 0; w < n_waves; w++)
            raw = crc_mul(raw, shape.wave) ^ *reinterpret_cast<const uint32_t*>(&l.scratch0[w].t);
        reinterpret_cast<uint64_t*>(digests)[f] = ((uint64_t)(uint32_t)kBlock << 32) | (raw ^ shape.finish);
    }
}

// ---- bytes in global memory -----------------------------------------------------------------------------------------------------
// One workgroup per (range, slice of slice_bytes): a frame's range is what another kernel decoded into the workspace, at
// sample_offsets[f] * channels * value_bytes (2: int16; sela_digest_pcm.hip's tiles: 3 or 4).  Frames from *n_a + *n_b on are left
// alone: the device's count of the route that ran, the other route's being 0 (n_a null: every frame of the call); without sample
// offsets there is one range, [0, raw_bytes).  The slice's whole 16-byte lines are read as
// such, 256 threads at their stride; what lies ahead of the first line and behind the last (up to 15 bytes each) is taken byte by
// byte by thread 0, which puts the three together.  parts[range * slices + slice]: the slice's raw CRC.

struct DigestRange {
    uint64_t start, bytes; // in `bytes`; bytes: what the decoder wrote
    uint32_t samples;      // the frame's samples per channel
    bool there;
};
__device__ __forceinline__ DigestRange digest_range(uint32_t f, const uint64_t* __restrict__ sample_offsets, uint32_t max_frames, uint32_t channels, uint32_t stride,
    const uint32_t* __restrict__ n_a /* or null */, const uint32_t* __restrict__ n_b /* or null */, uint64_t raw_bytes, uint32_t value_bytes)
{
    DigestRange g = { 0, raw_bytes, 0, true };
    if (!sample_offsets)
        return g;
    const uint32_t n = n_a ? *n_a + (n_b ? *n_b : 0u) : max_frames;
    g.there = f < min(n, max_frames);
    if (g.there) {
        const uint64_t so = sample_offsets[f], in_frame = sample_offsets[f + 1] - so;
        g.start = so * channels * value_bytes;
        g.bytes = min(in_frame, (uint64_t)stride) * channels * value_bytes; // (never more than the decoder wrote)
        g.samples = (uint32_t)in_frame;
    }
    return g;
}

__global__ __launch_bounds__(kDigestThreads) void k_digest_pcm(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ sample_offsets /* or null */,
    uint32_t max_frames, uint32_t channels, uint32_t stride, const uint32_t* __restrict__ n_a, const uint32_t* __restrict__ n_b /* or null */, uint64_t raw_bytes,
    uint64_t slice_bytes, uint32_t slices, uint32_t* __restrict__ parts, const DigestShape shape)
{
    __shared__ uint32_t s_part[kDigestThreads / 64];
    const uint32_t f = blockIdx.x, s = blockIdx.y;
    const DigestRange g = digest_range(f, sample_offsets, max_frames, channels, stride, n_a, n_b, raw_bytes, 2);
    const uint64_t lo = (uint64_t)s * slice_bytes;
    if (!g.there || lo >= g.bytes)
        return;
    const uint64_t n = min(slice_bytes, g.bytes - lo);
    const uint8_t* const p = bytes + g.start + lo;
    const uint64_t head = min(n, (uint64_t)((16 - ((uintptr_t)p & 15)) & 15));
    const uint64_t lines = (n - head) / 16, tail = n - head - 16 * lines;
    const uint4* const body = reinterpret_cast<const uint4*>(p + head);
    const uint64_t steps = (lines + kDigestThreads - 1) / kDigestThreads, pad = steps * kDigestThreads - lines;
    uint32_t r = 0;
    for (uint64_t j = 0; j < steps; j++) {
        const uint64_t q = threadIdx.x + j * kDigestThreads;
        if (j)
            r = crc_mul(r, shape.stride);
        if (q < pad)
            continue;
        const uint4 w = body[q - pad];
        r = crc_step32(crc_step32(crc_step32(crc_step32(r, w.x), w.y), w.z), w.w);
    }
    r = wave_crc(r, shape);
    if (threadIdx.x % 64 == 0)
        s_part[threadIdx.x / 64] = r;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t raw_head = 0, raw_tail = 0;
        for (uint64_t i = 0; i < head; i++)
            raw_head = crc_raw_byte(raw_head, p[i]);
        for (uint64_t i = n - tail; i < n; i++)
            raw_tail = crc_raw_byte(raw_tail, p[i]);
        const uint32_t raw_body = waves_crc(s_part, 1, kDigestThreads / 64, shape);
        const uint32_t behind_body = crc_xpow8(tail);
        parts[(size_t)f * slices + s] = crc_mul(raw_head, crc_mul(crc_xpow8(16 * lines), behind_body)) ^ crc_mul(raw_body, behind_body) ^ raw_tail;
    }
}

// One workgroup per range: a thread takes a run of consecutive slices, moves its run's raw CRC over the bytes behind the run, and
// the XOR of those is the range's; thread 0 turns it into the CRC and writes the record (a frame) or the two words (raw bytes).
__global__ __launch_bounds__(kDigestThreads) void k_digest_slices(const uint32_t* __restrict__ parts, const uint64_t* __restrict__ sample_offsets /* or null */,
    uint32_t max_frames, uint32_t channels, uint32_t stride, const uint32_t* __restrict__ n_a, const uint32_t* __restrict__ n_b /* or null */, uint64_t raw_bytes,
    uint64_t slice_bytes, uint32_t slices, uint32_t value_bytes, struct sela_hip_digest* __restrict__ digests /* frames */,
    uint64_t* __restrict__ out /* raw bytes: [2] */)
{
    __shared__ uint32_t s_part[kDigestThreads / 64];
    const uint32_t f = blockIdx.x;
    const DigestRange g = digest_range(f, sample_offsets, max_frames, channels, stride, n_a, n_b, raw_bytes, value_bytes);
    if (!g.there)
        return;
    const uint64_t used = (g.bytes + slice_bytes - 1) / slice_bytes; // (<= slices)
    const uint64_t run = (used + kDigestThreads - 1) / kDigestThreads;
    const uint64_t s0 = min(used, threadIdx.x * run), s1 = min(used, s0 + run);
    // (a run of one slice has nothing in front of it to move, and the last run nothing behind it: a frame of one slice -- every frame
    // of a 2048-sample stream in sela_digest_pcm.hip's tiles -- costs no multiplier at all, and the threads without a run none either)
    const uint32_t whole = run > 1 ? crc_xpow8(slice_bytes) : 0u;
    uint32_t r = 0;
    for (uint64_t s = s0; s < s1; s++) {
        const uint64_t in_slice = min(slice_bytes, g.bytes - s * slice_bytes);
        if (r)
            r = crc_mul(r, in_slice == slice_bytes ? whole : crc_xpow8(in_slice));
        r ^= parts[(size_t)f * slices + s];
    }
    const uint64_t behind = g.bytes - min(g.bytes, s1 * slice_bytes);
    if (s1 > s0 && behind)
        r = crc_mul(r, crc_xpow8(behind));
    const uint32_t raw = block_xor(r, s_part);
    if (threadIdx.x == 0) {
        const uint32_t crc = crc_from_raw(raw, g.bytes);
        if (sample_offsets)
            reinterpret_cast<uint64_t*>(digests)[f] = ((uint64_t)g.samples << 32) | crc;
        else
            out[0] = crc, out[1] = g.bytes;
    }
}

// ---- the track --------------------------------------------------------------------------------------------------------------------
// crc(frame 0 | frame 1 | ...) = XOR over f of crc_f * x^(8 * bytes behind frame f), the distance from the sample offsets.  XOR
// commutes, so the grid's shape does not show: k_digest_fold leaves one word per workgroup, k_digest_track joins them and writes
// track[0] = the CRC, track[1] = the bytes.
constexpr uint32_t kDigestFoldBlocks = 256;

__device__ __forceinline__ uint32_t digest_frames_found(uint32_t max_frames, const uint32_t* __restrict__ n_frames_found)
{
    return n_frames_found ? min(*n_frames_found, max_frames) : max_frames;
}

__global__ __launch_bounds__(kDigestThreads) void k_digest_fold(const struct sela_hip_digest* __restrict__ digests, const uint64_t* __restrict__ sample_offsets,
    uint32_t max_frames, const uint32_t* __restrict__ n_frames_found /* or null */, uint32_t channels, uint32_t value_bytes,
    uint32_t* __restrict__ fold /* [gridDim.x] */)
{
    __shared__ uint32_t s_part[kDigestThreads / 64];
    const uint32_t n = digest_frames_found(max_frames, n_frames_found);
    const uint64_t end = n ? sample_offsets[n] : 0;
    uint32_t r = 0;
    for (uint64_t f = (uint64_t)blockIdx.x * kDigestThreads + threadIdx.x; f < n; f += (uint64_t)gridDim.x * kDigestThreads)
        r ^= crc_mul(digests[f].crc32, crc_xpow8((end - sample_offsets[f + 1]) * channels * value_bytes));
    r = block_xor(r, s_part);
    if (threadIdx.x == 0)
        fold[blockIdx.x] = r;
}

__global__ __launch_bounds__(kDigestThreads) void k_digest_track(const uint32_t* __restrict__ fold, uint32_t fold_blocks, const uint64_t* __restrict__ sample_offsets,
    uint32_t max_frames, const uint32_t* __restrict__ n_frames_found /* or null */, uint32_t channels, uint32_t value_bytes, uint64_t* __restrict__ track /* [2] */)
{
    __shared__ uint32_t s_part[kDigestThreads / 64];
    uint32_t r = 0;
    for (uint32_t b = threadIdx.x; b < fold_blocks; b += kDigestThreads)
        r ^= fold[b];
    r = block_xor(r, s_part);
    if (threadIdx.x == 0) {
        const uint32_t n = digest_frames_found(max_frames, n_frames_found);
        track[0] = r;
        track[1] = n ? sample_offsets[n] * channels * value_bytes : 0;
    }
}

// ---- launches ---------------------------------------------------------------------------------------------------------------------
// the dynamic LDS launch_digest_frames asks for (sela_hip_debug_digest_lds_bytes: tests hold it against the decoder's)
size_t digest_lds_bytes(uint32_t channels) { return decode_lds_bytes_for(channels, decode_waves(channels)); }

uint32_t digest_slices(uint32_t channels, uint32_t stride)
{
    const uint64_t bytes = (uint64_t)channels * stride * 2;
    return (uint32_t)std::max<uint64_t>((bytes + kDigestSliceBytes - 1) / kDigestSliceBytes, 1);
}
uint32_t digest_fold_blocks(uint32_t max_frames)
{
    return std::max(1u, std::min(kDigestFoldBlocks, (uint32_t)(((uint64_t)max_frames + kDigestThreads - 1) / kDigestThreads)));
}

hipError_t launch_digest_frames(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames, uint32_t channels, struct sela_hip_digest* d_digests,
    uint32_t* d_status, void* d_workspace, hipStream_t stream, int recurrence_form, uint32_t synth_priorities, const uint32_t* d_n_found)
{
    if (n_frames == 0)
        return hipSuccess;
    if (channels == 0 || channels > (uint32_t)kDecMaxWaves)
        return hipErrorInvalidValue;
    const int n_waves = decode_waves(channels);
    Carve carve(d_workspace); // (launch_decode's workspace: the route's kernel with the CRC for its stores)
    int32_t* const ws = carve_decode(carve, n_frames, channels);
    const size_t lds = digest_lds_bytes(channels);
    if (lds > 64 * 1024) { // above the default dynamic-LDS limit (more than four channels); per device, so every time
        const hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(k_digest_frames), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (err != hipSuccess)
            return err;
    }
    const uint32_t from = recurrence_form >= 0
        ? (recurrence_form ? 0u : n_frames)
        : vec_shift_from_for(n_frames, n_waves, resident_frames(reinterpret_cast<const void*>(k_digest_frames), n_waves, lds, kResidencyDigest));
    hipLaunchKernelGGL(k_digest_frames, dim3(n_frames), dim3(n_waves * 64), lds, stream, d_frames, d_frame_offsets, n_frames, channels, d_digests, d_status, ws, from,
        synth_priorities, d_n_found, kFusedShapes[channels]);
    return hipGetLastError();
}

hipError_t launch_digest_pcm(const int16_t* d_decoded, const uint64_t* d_sample_offsets, uint32_t max_frames, uint32_t channels, uint32_t stride, const uint32_t* d_n_a,
    const uint32_t* d_n_b, uint32_t* d_parts, struct sela_hip_digest* d_digests, hipStream_t stream)
{
    if (max_frames == 0)
        return hipSuccess;
    const uint32_t slices = digest_slices(channels, stride);
    hipLaunchKernelGGL(k_digest_pcm, dim3(max_frames, slices), dim3(kDigestThreads), 0, stream, reinterpret_cast<const uint8_t*>(d_decoded), d_sample_offsets, max_frames,
        channels, stride, d_n_a, d_n_b, (uint64_t)0, (uint64_t)kDigestSliceBytes, slices, d_parts, kPcmShape);
    return launch_digest_slices(d_parts, d_sample_offsets, max_frames, channels, stride, d_n_a, d_n_b, kDigestSliceBytes, slices, 2, d_digests, stream);
}

// the records from the raw CRCs of a frame's slices -- k_digest_pcm's, or the tiles of sela_digest_pcm.hip (value_bytes 3 or 4)
hipError_t launch_digest_slices(const uint32_t* d_parts, const uint64_t* d_sample_offsets, uint32_t max_frames, uint32_t channels, uint32_t stride,
    const uint32_t* d_n_a, const uint32_t* d_n_b, uint64_t slice_bytes, uint32_t slices, uint32_t value_bytes, struct sela_hip_digest* d_digests, hipStream_t stream)
{
    if (max_frames == 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_digest_slices, dim3(max_frames), dim3(kDigestThreads), 0, stream, d_parts, d_sample_offsets, max_frames, channels, stride, d_n_a, d_n_b,
        (uint64_t)0, slice_bytes, slices, value_bytes, d_digests, static_cast<uint64_t*>(nullptr));
    return hipGetLastError();
}

hipError_t launch_digest_fold(const struct sela_hip_digest* d_digests, const uint64_t* d_sample_offsets, uint32_t max_frames, const uint32_t* d_n_found,
    uint32_t channels, uint32_t value_bytes, uint32_t* d_fold, uint64_t* d_track, hipStream_t stream)
{
    const uint32_t blocks = digest_fold_blocks(max_frames);
    hipLaunchKernelGGL(k_digest_fold, dim3(blocks), dim3(kDigestThreads), 0, stream, d_digests, d_sample_offsets, max_frames, d_n_found, channels, value_bytes, d_fold);
    hipLaunchKernelGGL(k_digest_track, dim3(1), dim3(kDigestThreads), 0, stream, d_fold, blocks, d_sample_offsets, max_frames, d_n_found, channels, value_bytes,
        d_track);
    return hipGetLastError();
}

// sela_hip_crc32_device: slices of 32 KiB, or of whatever keeps a range at kCrc32MaxSlices of them (a multiple of 16 bytes)
constexpr uint64_t kCrc32MaxSlices = 4096;
static uint64_t crc32_slice_bytes(uint64_t n_bytes)
{
    const uint64_t even = ((n_bytes + kCrc32MaxSlices - 1) / kCrc32MaxSlices + 15) & ~(uint64_t)15;
    return std::max<uint64_t>(kDigestSliceBytes, even);
}
static uint32_t crc32_slices(uint64_t n_bytes)
{
    const uint64_t slice = crc32_slice_bytes(n_bytes);
    return (uint32_t)std::max<uint64_t>((n_bytes + slice - 1) / slice, 1);
}
size_t crc32_workspace_bytes(uint64_t n_bytes, Carve* at)
{
    return measured(at, [&](Carve& c) { c.take<uint32_t>(crc32_slices(n_bytes)); });
}
hipError_t launch_crc32_device(const void* d_bytes, uint64_t n_bytes, uint64_t* d_out, void* d_workspace, hipStream_t stream)
{
    Carve c(d_workspace);
    const uint32_t slices = crc32_slices(n_bytes);
    uint32_t* const parts = c.take<uint32_t>(slices);
    const uint64_t slice = crc32_slice_bytes(n_bytes);
    if (n_bytes)
        hipLaunchKernelGGL(k_digest_pcm, dim3(1, slices), dim3(kDigestThreads), 0, stream, static_cast<const uint8_t*>(d_bytes), static_cast<const uint64_t*>(nullptr), 1u,
            1u, 1u, static_cast<const uint32_t*>(nullptr), static_cast<const uint32_t*>(nullptr), n_bytes, slice, slices, parts, kPcmShape);
    hipLaunchKernelGGL(k_digest_slices, dim3(1), dim3(kDigestThreads), 0, stream, parts, static_cast<const uint64_t*>(nullptr), 1u, 1u, 1u,
        static_cast<const uint32_t*>(nullptr), static_cast<const uint32_t*>(nullptr), n_bytes, slice, slices, 1u, static_cast<struct sela_hip_digest*>(nullptr), d_out);
    return hipGetLastError();
}

} // namespace sela

extern "C" size_t sela_hip_debug_digest_lds_bytes(uint32_t channels)
{
    return channels == 0 || channels > sela::kVerifyFusedChannels ? 0 : sela::digest_lds_bytes(channels);
}
