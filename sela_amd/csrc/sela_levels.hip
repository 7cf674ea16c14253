// sela_levels.hip -- how loud a .sela stream is, measured on the device: per frame and channel the peak, the sum and the sum of
// squares of the int16 samples sela_hip_decode_n_device would write (gfx950).  The launches are the int16 family's
// sequence (launch_n_sequence, sela_generic.hip: the sample index, k_route_n, k_verify_begin, a fused kernel for the 2048-sample
// route of up to eight channels, every other route decoded into the workspace, a consumer of that PCM); launch_levels_n_device
// plugs in
//
//   k_level_frames     the fused kernel: the decoder with a reduction for a store: k_verify_frames (sela_verify.hip) with the compare taken out.  One
//                      workgroup per frame, one wave per subframe: frame_prologue and decode_subframe of sela_decode_core.inc, the
//                      barrier, then the shared second pass (parent - difference, mod 2^16) -- and where the decoder stores a
//                      frame's interleaved int16 samples, this kernel folds them into max |v|, sum v and sum v * v per channel.
//                      No decoded sample reaches global memory; the LDS plan is the decoder's (the waves' partial results lie in
//                      their synthesis tables, dead behind the barrier), so the occupancy is the decoder's too.
//   k_level_channels   the same record from PCM that another kernel decoded into the workspace: the routes that are not fused
//                      (frames of any other length, frames of more than eight channels).  One workgroup per (frame, channel).
//   k_level_count      status[2] for those routes: a thread per frame looks at its channels' peaks.
//
// Every figure is an integer, so it is exact and does not depend on the order of the additions: |sum| <= 65535 * 32768 < 2^31,
// sum_squares <= 65535 * 2^30 < 2^46.
#include "sela_host.h"

#include "sela_synth.h"

namespace sela {

#include "sela_decode_core.inc"

static_assert(kVerifyFusedChannels == (uint32_t)kDecMaxWaves, "the fused route takes what k_decode_frames takes");
static_assert(sizeof(sela_hip_level) == 24 && alignof(sela_hip_level) == 8, "the record of include/sela_hip.h");
static_assert((size_t)kDecMaxWaves * 16 <= sizeof(SynthTables), "a wave's partial results fit its synthesis table");

// What a thread, then a wave, has seen of one channel.
struct LevelAcc {
    uint32_t peak = 0;
    int32_t sum = 0;       // (a frame's whole channel stays below 2^31)
    uint64_t squares = 0;
    __device__ __forceinline__ void take(int32_t v)
    {
        peak = max(peak, (uint32_t)(v < 0 ? -v : v));
        sum += v;
        squares += (uint32_t)(v * v); // (32768^2 = 2^30)
    }
};

// A wave's view of one channel: peak, sum, squares (low, high) in four words of LDS (lane 63 holds the DPP ladders' totals:
// wave_max_u32, wave_sum_small and wave_sum_64 return them wave-uniform).
__device__ __forceinline__ void deposit_wave(const LevelAcc& a, uint32_t* part, int lane)
{
    const uint32_t peak = wave_max_u32(a.peak);
    const uint32_t sum = wave_sum_small((uint32_t)a.sum);
    const uint64_t squares = wave_sum_64(a.squares);
    if (lane == 0) {
        part[0] = peak, part[1] = sum;
        part[2] = (uint32_t)squares, part[3] = (uint32_t)(squares >> 32);
    }
}

// A record leaves as three 8-byte words, one lane each (little-endian: peak | samples << 32, sum, sum_squares): word k of it.
static_assert(offsetof(sela_hip_level, peak) == 0 && offsetof(sela_hip_level, samples) == 4 && offsetof(sela_hip_level, sum) == 8
        && offsetof(sela_hip_level, sum_squares) == 16,
    "the words of a record");
__device__ __forceinline__ uint64_t level_word(uint32_t k, uint32_t peak, uint32_t samples, int32_t sum, uint64_t squares)
{
    return k == 0 ? ((uint64_t)samples << 32) | peak : (k == 1 ? (uint64_t)(int64_t)sum : squares);
}

__global__ __launch_bounds__(kDecMaxWaves * 64) __attribute__((amdgpu_waves_per_eu(7, 8))) void k_level_frames(const uint8_t* __restrict__ frames,
    const uint64_t* __restrict__ frame_offsets, uint32_t n_frames, uint32_t channels, sela_hip_level* __restrict__ levels /* [n_frames][channels] */,
    uint32_t* __restrict__ status, int32_t* __restrict__ ws_residues, uint32_t vec_shift_from /* as in k_decode_frames */,
    uint32_t synth_priorities /* as in k_decode_frames */, const uint32_t* __restrict__ n_frames_found /* or null: frames from *n_frames_found on are left alone */)
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

    // ---- the second pass, folded instead of stored --------------------------------------------------------------------
    // What k_decode_frames would write at pcm_out[(f * 2048 + i) * channels + c] goes into channel c's three figures: within the
    // thread, within the wave, then across the waves through four words per channel of each wave's synthesis table (dead behind
    // the barrier above).
    uint32_t* const part = reinterpret_cast<uint32_t*>(&l.scratch0[wave].t);
    if (channels == 2) {
        // stereo: four samples of both channels per thread
        const StereoPass sp = stereo_pass(l.sub, l.sub_info);
        LevelAcc a0, a1;
        for (uint32_t i4 = threadIdx.x; i4 < (uint32_t)kBlock / 4; i4 += blockDim.x) {
            const uint4 w = stereo_words(sp, i4);
            const uint32_t x[4] = { w.x, w.y, w.z, w.w };
#pragma unroll
            for (int k = 0; k < 4; k++) {
                a0.take((int32_t)(int16_t)(x[k] & 0xFFFFu));
                a1.take((int32_t)x[k] >> 16);
            }
        }
        deposit_wave(a0, part, lane);
        deposit_wave(a1, part + 4, lane);
    } else {
        for (uint32_t c = 0; c < channels; c++) {
            LevelAcc a;
            for (uint32_t i = threadIdx.x; i < (uint32_t)kBlock; i += blockDim.x)
                a.take((int32_t)(int16_t)channel_value16(l.sub, l.sub_info, c, i));
            deposit_wave(a, part + 4 * c, lane);
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
    __syncthreads();
    if (wave == 0) {
        // three lanes per channel add the waves up and write one word of the record each; the frame counts in status[2] if any
        // channel is not silent
        const uint32_t c = (uint32_t)lane / 3, k = (uint32_t)lane % 3;
        uint32_t peak = 0;
        if (c < channels) {
            int32_t sum = 0;
            uint64_t squares = 0;
            for (int w = 0; w < n_waves; w++) {
                const uint32_t* const p = reinterpret_cast<const uint32_t*>(&l.scratch0[w].t) + 4 * c;
                peak = max(peak, p[0]);
                sum += (int32_t)p[1];
                squares += ((uint64_t)p[3] << 32) | p[2];
            }
            reinterpret_cast<uint64_t*>(levels + (size_t)f * channels)[lane] = level_word(k, peak, (uint32_t)kBlock, sum, squares);
        }
        peak = wave_or(peak);
        if (lane == 0 && peak)
            atomicAdd(&status[2], 1u);
    }
}

// ---- PCM another kernel decoded ---------------------------------------------------------------------------------------------
// One workgroup per (frame, channel): frame f's values lie at sample_offsets[f] * channels, interleaved (a strided 2-byte read:
// this is the cold route).  Frames from *n_a + *n_b on are left alone (the device's count of the route that ran: the other
// route's is 0).
constexpr uint32_t kLevelThreads = 256;

__device__ __forceinline__ uint32_t level_frames_on_route(const uint32_t* __restrict__ n_a, const uint32_t* __restrict__ n_b, uint32_t max_frames)
{
    const uint32_t n = *n_a + (n_b ? *n_b : 0u);
    return min(n, max_frames);
}

__global__ __launch_bounds__(kLevelThreads) void k_level_channels(const int16_t* __restrict__ decoded, const uint64_t* __restrict__ sample_offsets,
    uint32_t max_frames, uint32_t channels, uint32_t stride, const uint32_t* __restrict__ n_a, const uint32_t* __restrict__ n_b /* or null */,
    sela_hip_level* __restrict__ levels /* [max_frames][channels] */)
{
    __shared__ uint32_t s_part[kLevelThreads / 64][4];
    const uint32_t f = blockIdx.x, c = blockIdx.y;
    if (f >= level_frames_on_route(n_a, n_b, max_frames))
        return;
    const uint64_t so = sample_offsets[f], in_frame = sample_offsets[f + 1] - so;
    const uint32_t n = (uint32_t)min(in_frame, (uint64_t)stride); // (never more than the decoder wrote)
    const int16_t* const d = decoded + so * channels + c;
    LevelAcc a;
    for (uint32_t i = threadIdx.x; i < n; i += kLevelThreads)
        a.take((int32_t)d[(size_t)i * channels]);
    deposit_wave(a, s_part[threadIdx.x / 64], threadIdx.x % 64);
    __syncthreads();
    if (threadIdx.x < 3) { // (a thread per word of the record)
        uint32_t peak = 0;
        int32_t sum = 0;
        uint64_t squares = 0;
        for (uint32_t w = 0; w < kLevelThreads / 64; w++) {
            peak = max(peak, s_part[w][0]);
            sum += (int32_t)s_part[w][1];
            squares += ((uint64_t)s_part[w][3] << 32) | s_part[w][2];
        }
        reinterpret_cast<uint64_t*>(levels + (size_t)f * channels + c)[threadIdx.x] = level_word(threadIdx.x, peak, (uint32_t)in_frame, sum, squares);
    }
}

__global__ __launch_bounds__(kLevelThreads) void k_level_count(const sela_hip_level* __restrict__ levels, uint32_t max_frames, uint32_t channels,
    const uint32_t* __restrict__ n_a, const uint32_t* __restrict__ n_b, uint32_t* __restrict__ status)
{
    const uint32_t f = blockIdx.x * kLevelThreads + threadIdx.x;
    uint32_t loud = 0;
    if (f < level_frames_on_route(n_a, n_b, max_frames))
        for (uint32_t c = 0; c < channels; c++)
            loud |= levels[(size_t)f * channels + c].peak ? 1u : 0u;
    loud = wave_sum_small(loud);
    if (threadIdx.x % 64 == 0 && loud)
        atomicAdd(&status[2], loud);
}

// the dynamic LDS launch_level_frames asks for (sela_hip_debug_levels_lds_bytes: tests hold it against the decoder's)
size_t levels_lds_bytes(uint32_t channels) { return decode_lds_bytes_for(channels, decode_waves(channels)); }

hipError_t launch_level_frames(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames, uint32_t channels, sela_hip_level* d_levels,
    uint32_t* d_status, void* d_workspace, hipStream_t stream, int recurrence_form, uint32_t synth_priorities, const uint32_t* d_n_found)
{
    if (n_frames == 0)
        return hipSuccess;
    if (channels == 0 || channels > (uint32_t)kDecMaxWaves)
        return hipErrorInvalidValue;
    const int n_waves = decode_waves(channels);
    Carve carve(d_workspace); // (launch_decode's workspace: the route's kernel with a reduction for its stores)
    int32_t* const ws = carve_decode(carve, n_frames, channels);
    const size_t lds = levels_lds_bytes(channels);
    if (lds > 64 * 1024) { // above the default dynamic-LDS limit (more than four channels); per device, so every time
        const hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(k_level_frames), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (err != hipSuccess)
            return err;
    }
    const uint32_t from = recurrence_form >= 0
        ? (recurrence_form ? 0u : n_frames)
        : vec_shift_from_for(n_frames, n_waves, resident_frames(reinterpret_cast<const void*>(k_level_frames), n_waves, lds, kResidencyLevels));
    hipLaunchKernelGGL(k_level_frames, dim3(n_frames), dim3(n_waves * 64), lds, stream, d_frames, d_frame_offsets, n_frames, channels, d_levels, d_status, ws, from,
        synth_priorities, d_n_found);
    return hipGetLastError();
}

hipError_t launch_level_channels(const int16_t* d_decoded, const uint64_t* d_sample_offsets, uint32_t max_frames, uint32_t channels, uint32_t stride,
    const uint32_t* d_n_a, const uint32_t* d_n_b, sela_hip_level* d_levels, uint32_t* d_status, hipStream_t stream)
{
    if (max_frames == 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_level_channels, dim3(max_frames, channels), dim3(kLevelThreads), 0, stream, d_decoded, d_sample_offsets, max_frames, channels, stride, d_n_a,
        d_n_b, d_levels);
    hipLaunchKernelGGL(k_level_count, dim3((max_frames + kLevelThreads - 1) / kLevelThreads), dim3(kLevelThreads), 0, stream, d_levels, max_frames, channels, d_n_a,
        d_n_b, d_status);
    return hipGetLastError();
}

} // namespace sela

extern "C" size_t sela_hip_debug_levels_lds_bytes(uint32_t channels)
{
    return channels == 0 || channels > sela::kVerifyFusedChannels ? 0 : sela::levels_lds_bytes(channels);
}
