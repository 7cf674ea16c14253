// sela_verify.hip -- a .sela stream checked against its PCM on the device, frame by frame (gfx950).
//
// The codec is not lossless on every frame (the reference's encoder rounds a prediction half-up, its decoder
// half-down; on a tie the sample comes back off by one and the error runs on through the predictor), and reproducing the
// reference bit for bit means reproducing that.  Which frames of a caller's audio are affected is answered here:
//
//   k_verify_frames    the decoder with a compare for a store.  One workgroup per frame, one wave per subframe: frame_prologue and
//                      decode_subframe of sela_decode_core.inc, which k_decode_frames calls too (the lane-parallel parse, step-up and
//                      tuned synthesis, the serial parse for subframes outside the LDS plan), then the shared second pass (parent -
//                      difference, mod 2^16) -- and where the decoder stores a frame's interleaved int16 samples, this kernel loads
//                      the original's, counts the values that differ and keeps the smallest differing index.  No decoded sample
//                      reaches global memory; the LDS plan is the decoder's (decode_lds_bytes_for: the reduction's words lie in
//                      the waves' synthesis tables, dead behind the barrier), so the occupancy is the decoder's too.  What is
//                      written in this file is the compare, its reduction and the launches.
//   k_verify_compare   the same counts for PCM that another kernel decoded into the workspace: the routes that are not fused
//                      (frames of any other length, frames of more than eight channels).  One workgroup per (frame, slice);
//                      k_verify_combine adds a frame's slices up.
//
// Per frame: diff_count[f], first_diff[f] (0xFFFFFFFF: nothing differs); status[2] counts the frames with a difference.
#include "sela_host.h"

#include "sela_synth.h"

namespace sela {

#include "sela_decode_core.inc"

static_assert(kVerifyFusedChannels == (uint32_t)kDecMaxWaves, "the fused route takes what k_decode_frames takes");

constexpr uint32_t kNoDiff = 0xFFFFFFFFu;

// Minimum of one unsigned 32-bit value per lane (wave_max_u32 on the complements; the result is wave-uniform).
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) { return ~wave_max_u32(~v); }

__global__ __launch_bounds__(kDecMaxWaves * 64) __attribute__((amdgpu_waves_per_eu(7, 8))) void k_verify_frames(const uint8_t* __restrict__ frames,
    const uint64_t* __restrict__ frame_offsets, uint32_t n_frames, uint32_t channels, const int16_t* __restrict__ pcm /* the original: frame f at f * 2048 * channels */,
    uint32_t* __restrict__ diff_count, uint32_t* __restrict__ first_diff, uint32_t* __restrict__ status, int32_t* __restrict__ ws_residues,
    uint32_t vec_shift_from /* as in k_decode_frames */, uint32_t synth_priorities /* as in k_decode_frames */,
    const uint32_t* __restrict__ n_frames_found /* or null: frames from *n_frames_found on are left alone */)
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

    // ---- the second pass, compared instead of stored ------------------------------------------------------------------
    // What k_decode_frames would write at pcm_out[(f * 2048 + i) * channels + c] is held against pcm at the same place: the
    // values that differ are counted, the smallest differing i * channels + c is kept (a thread meets its indices in
    // ascending order: the first it finds is its smallest).
    uint32_t n_diff = 0, first = kNoDiff;
    const int16_t* const orig = pcm + (size_t)f * kBlock * channels;
    if (channels == 2 && ((uintptr_t)orig & 15) == 0) {
        // stereo: four samples of both channels per thread, one 16-byte load
        const StereoPass sp = stereo_pass(l.sub, l.sub_info);
        const uint4* in = reinterpret_cast<const uint4*>(orig);
        for (uint32_t i4 = threadIdx.x; i4 < (uint32_t)kBlock / 4; i4 += blockDim.x) {
            const uint4 o = in[i4], w = stereo_words(sp, i4);
            const uint32_t x[4] = { w.x ^ o.x, w.y ^ o.y, w.z ^ o.z, w.w ^ o.w };
            if (x[0] | x[1] | x[2] | x[3]) { // (rare: a handful of frames in thousands)
#pragma unroll
                for (int k = 3; k >= 0; k--) { // (downwards: the smallest index is assigned last)
                    const uint32_t lo = x[k] & 0xFFFFu, hi = x[k] >> 16;
                    n_diff += (lo ? 1u : 0u) + (hi ? 1u : 0u);
                    if (x[k])
                        first = min(first, i4 * 8 + 2 * k + (lo ? 0u : 1u));
                }
            }
        }
    } else {
        for (uint32_t i = threadIdx.x; i < (uint32_t)kBlock; i += blockDim.x)
            for (uint32_t c = 0; c < channels; c++)
                if (channel_value16(l.sub, l.sub_info, c, i) != (uint16_t)orig[(size_t)i * channels + c]) {
                    n_diff++;
                    first = min(first, i * channels + c);
                }
    }
    if (threadIdx.x == 0)
        flags |= layout_flags(l.sub_info, channels);
    flags = wave_or(flags);
    if (lane == 0 && flags) {
        atomicOr(&status[0], flags);
        if (wave == 0 && (flags & SELA_HIP_FLAG_BAD_FRAME))
            atomicAdd(&status[1], 1u);
    }
    // within the wave, then across the waves through two words of each wave's synthesis table (dead behind the barrier above)
    n_diff = wave_sum_small(n_diff); // (at most 2048 * 8)
    first = wave_min_u32(first);
    uint32_t* const part = reinterpret_cast<uint32_t*>(&l.scratch0[wave].t);
    if (lane == 0)
        part[0] = n_diff, part[1] = first;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0, least = kNoDiff;
        for (int w = 0; w < n_waves; w++) {
            const uint32_t* const p = reinterpret_cast<const uint32_t*>(&l.scratch0[w].t);
            total += p[0];
            least = min(least, p[1]);
        }
        diff_count[f] = total;
        first_diff[f] = least;
        if (total)
            atomicAdd(&status[2], 1u);
    }
}

// ---- PCM another kernel decoded, against the original ---------------------------------------------------------------------
// One workgroup per (frame, slice of kVerifySliceValues interleaved values): frame f's values lie at sample_offsets[f] *
// channels in both buffers.  A slice leaves its count and its smallest differing index (relative to the frame) in the
// workspace; k_verify_combine, a thread per frame, adds the slices up, writes the frame's two words and counts the frame in
// status[2].  Frames from *n_a + *n_b on are left alone (the device's count of the route that ran: the other route's is 0).
constexpr uint32_t kVerifyThreads = 256;

__device__ __forceinline__ uint32_t verify_frames_on_route(const uint32_t* __restrict__ n_a, const uint32_t* __restrict__ n_b, uint32_t max_frames)
{
    const uint32_t n = *n_a + (n_b ? *n_b : 0u);
    return min(n, max_frames);
}

__global__ __launch_bounds__(kVerifyThreads) void k_verify_compare(const int16_t* __restrict__ decoded, const int16_t* __restrict__ pcm,
    const uint64_t* __restrict__ sample_offsets, uint32_t max_frames, uint32_t channels, uint32_t stride, const uint32_t* __restrict__ n_a,
    const uint32_t* __restrict__ n_b /* or null */, uint2* __restrict__ parts /* [max_frames][gridDim.y] */)
{
    __shared__ uint32_t s_count[kVerifyThreads / 64], s_first[kVerifyThreads / 64];
    const uint32_t f = blockIdx.x;
    if (f >= verify_frames_on_route(n_a, n_b, max_frames))
        return;
    const uint64_t so = sample_offsets[f];
    const uint64_t in_frame = min(sample_offsets[f + 1] - so, (uint64_t)stride) * channels; // (never more than the decoder wrote)
    const uint64_t lo = (uint64_t)blockIdx.y * kVerifySliceValues, hi = min(in_frame, lo + kVerifySliceValues);
    const int16_t* const d = decoded + so * channels;
    const int16_t* const o = pcm + so * channels;
    uint32_t n_diff = 0, first = kNoDiff;
    for (uint64_t j = lo + threadIdx.x; j < hi; j += kVerifyThreads)
        if (d[j] != o[j]) {
            n_diff++;
            first = min(first, (uint32_t)j);
        }
    n_diff = wave_sum_small(n_diff);
    first = wave_min_u32(first);
    if (threadIdx.x % 64 == 0)
        s_count[threadIdx.x / 64] = n_diff, s_first[threadIdx.x / 64] = first;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0, least = kNoDiff;
        for (uint32_t w = 0; w < kVerifyThreads / 64; w++) {
            total += s_count[w];
            least = min(least, s_first[w]);
        }
        parts[(size_t)f * gridDim.y + blockIdx.y] = make_uint2(total, least);
    }
}

__global__ __launch_bounds__(kVerifyThreads) void k_verify_combine(const uint2* __restrict__ parts, uint32_t n_slices, uint32_t max_frames,
    const uint32_t* __restrict__ n_a, const uint32_t* __restrict__ n_b, uint32_t* __restrict__ diff_count, uint32_t* __restrict__ first_diff,
    uint32_t* __restrict__ status)
{
    const uint32_t f = blockIdx.x * kVerifyThreads + threadIdx.x;
    uint32_t lossy = 0;
    if (f < verify_frames_on_route(n_a, n_b, max_frames)) {
        uint32_t total = 0, least = kNoDiff;
        for (uint32_t s = 0; s < n_slices; s++) {
            const uint2 p = parts[(size_t)f * n_slices + s];
            total += p.x;
            least = min(least, p.y);
        }
        diff_count[f] = total;
        first_diff[f] = least;
        lossy = total ? 1u : 0u;
    }
    lossy = wave_sum_small(lossy);
    if (threadIdx.x % 64 == 0 && lossy)
        atomicAdd(&status[2], lossy);
}

uint32_t verify_slices(uint32_t channels, uint32_t stride)
{
    return (uint32_t)(((uint64_t)channels * stride + kVerifySliceValues - 1) / kVerifySliceValues);
}

// the dynamic LDS launch_verify_frames asks for (sela_hip_debug_verify_lds_bytes: tests hold it against the decoder's)
size_t verify_lds_bytes(uint32_t channels) { return decode_lds_bytes_for(channels, decode_waves(channels)); }

hipError_t launch_verify_frames(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames, uint32_t channels, const int16_t* d_pcm,
    uint32_t* d_diff_counts, uint32_t* d_first_diff, uint32_t* d_status, void* d_workspace, hipStream_t stream, int recurrence_form, uint32_t synth_priorities,
    const uint32_t* d_n_found)
{
    if (n_frames == 0)
        return hipSuccess;
    if (channels == 0 || channels > (uint32_t)kDecMaxWaves)
        return hipErrorInvalidValue;
    const int n_waves = decode_waves(channels);
    Carve carve(d_workspace); // (launch_decode's workspace: the route's kernel with a compare for its stores)
    int32_t* const ws = carve_decode(carve, n_frames, channels);
    const size_t lds = verify_lds_bytes(channels);
    if (lds > 64 * 1024) { // above the default dynamic-LDS limit (more than four channels); per device, so every time
        const hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(k_verify_frames), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (err != hipSuccess)
            return err;
    }
    const uint32_t from = recurrence_form >= 0
        ? (recurrence_form ? 0u : n_frames)
        : vec_shift_from_for(n_frames, n_waves, resident_frames(reinterpret_cast<const void*>(k_verify_frames), n_waves, lds, kResidencyVerify));
    hipLaunchKernelGGL(k_verify_frames, dim3(n_frames), dim3(n_waves * 64), lds, stream, d_frames, d_frame_offsets, n_frames, channels, d_pcm, d_diff_counts,
        d_first_diff, d_status, ws, from, synth_priorities, d_n_found);
    return hipGetLastError();
}

hipError_t launch_verify_compare(const int16_t* d_decoded, const int16_t* d_pcm, const uint64_t* d_sample_offsets, uint32_t max_frames, uint32_t channels,
    uint32_t stride, const uint32_t* d_n_a, const uint32_t* d_n_b, void* d_parts, uint32_t* d_diff_counts, uint32_t* d_first_diff, uint32_t* d_status,
    hipStream_t stream)
{
    if (max_frames == 0)
        return hipSuccess;
    const uint32_t n_slices = verify_slices(channels, stride);
    uint2* const parts = static_cast<uint2*>(d_parts);
    hipLaunchKernelGGL(k_verify_compare, dim3(max_frames, n_slices), dim3(kVerifyThreads), 0, stream, d_decoded, d_pcm, d_sample_offsets, max_frames, channels,
        stride, d_n_a, d_n_b, parts);
    hipLaunchKernelGGL(k_verify_combine, dim3((max_frames + kVerifyThreads - 1) / kVerifyThreads), dim3(kVerifyThreads), 0, stream, parts, n_slices, max_frames,
        d_n_a, d_n_b, d_diff_counts, d_first_diff, d_status);
    return hipGetLastError();
}

} // namespace sela

extern "C" size_t sela_hip_debug_verify_lds_bytes(uint32_t channels)
{
    return channels == 0 || channels > sela::kVerifyFusedChannels ? 0 : sela::verify_lds_bytes(channels);
}
