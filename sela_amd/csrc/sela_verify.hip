// sela_verify.hip -- a .sela stream checked against its PCM on the device, frame by frame (gfx950).
//
// The codec is not lossless on every frame (the reference's encoder rounds a prediction half-up, its decoder
// half-down; on a tie the sample comes back off by one and the error runs on through the predictor), and reproducing the
// reference bit for bit means reproducing that.  Which frames of a caller's audio are affected is answered here:
//
//   k_verify_frames    k_decode_frames<false> (sela_decode.hip) up to the workgroup barrier behind the synthesis -- one workgroup
//                      per frame, one wave per subframe, the lane-parallel parse, step-up and tuned synthesis of
//                      sela_decode_core.inc, the serial parse for subframes outside the LDS plan -- and then the second pass
//                      (parent - difference, mod 2^16) run as a COMPARE: where the decoder stores a frame's interleaved int16
//                      samples, this kernel loads the original's, counts the values that differ and keeps the smallest
//                      differing index.  No decoded sample reaches global memory; the LDS plan is the decoder's, byte for byte
//                      (the reduction's words lie in the waves' synthesis tables, dead behind the barrier), so the occupancy
//                      is the decoder's too.
//   k_verify_compare   the same counts for PCM that another kernel decoded into the workspace: the routes that are not fused
//                      (frames of any other length, frames of more than eight channels).  One workgroup per (frame, slice);
//                      k_verify_combine adds a frame's slices up.
//
// Per frame: diff_count[f], first_diff[f] (0xFFFFFFFF: nothing differs); status[2] counts the frames with a difference.
#include "sela_device.h"
#include "sela_generic.h"

namespace sela {

#include "sela_decode_core.inc"

static_assert(kVerifyFusedChannels == (uint32_t)kDecMaxWaves, "the fused route takes what k_decode_frames takes");

constexpr uint32_t kNoDiff = 0xFFFFFFFFu;

// Minimum of one unsigned 32-bit value per lane (wave_max_u32 on the complements; the result is wave-uniform).
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) { return ~wave_max_u32(~v); }

// The LDS plan of k_decode_frames (sela_decode.hip: decode_lds_bytes_for): one DecSubframeLds per subframe position | one
// DecWaveScratch per wave | sub_info[channels] | too_big[n_waves].  Nothing is added to it.
__host__ __device__ inline size_t verify_lds_bytes_for(uint32_t channels, int n_waves)
{
    return (size_t)channels * sizeof(DecSubframeLds) + (size_t)n_waves * sizeof(DecWaveScratch) + (size_t)channels * 4 + (size_t)n_waves * 4;
}

__global__ __launch_bounds__(kDecMaxWaves * 64) __attribute__((amdgpu_waves_per_eu(7, 8))) void k_verify_frames(const uint8_t* __restrict__ frames,
    const uint64_t* __restrict__ frame_offsets, uint32_t n_frames, uint32_t channels, const int16_t* __restrict__ pcm /* the original: frame f at f * 2048 * channels */,
    uint32_t* __restrict__ diff_count, uint32_t* __restrict__ first_diff, uint32_t* __restrict__ status, int32_t* __restrict__ ws_residues,
    uint32_t vec_shift_from /* as in k_decode_frames */, uint32_t synth_priorities /* as in k_decode_frames */,
    const uint32_t* __restrict__ n_frames_found /* or null: frames from *n_frames_found on are left alone */)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    const int n_waves = blockDim.x / 64;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / 64)), lane = threadIdx.x % 64;
    DecSubframeLds* const sub = reinterpret_cast<DecSubframeLds*>(dyn);
    DecWaveScratch* const scratch0 = reinterpret_cast<DecWaveScratch*>(dyn + (size_t)channels * sizeof(DecSubframeLds));
    DecWaveScratch* const scratch = scratch0 + wave;
    uint32_t* const sub_info = reinterpret_cast<uint32_t*>(dyn + (size_t)channels * sizeof(DecSubframeLds) + (size_t)n_waves * sizeof(DecWaveScratch));
    uint32_t* const too_big = sub_info + channels; // [n_waves]: this wave's subframe does not fit the fast plan

    const uint32_t f = blockIdx.x;
    if (f >= n_frames || (n_frames_found && f >= *n_frames_found))
        return;
    const bool vec_shift = f >= vec_shift_from;
    const uint8_t* const fb = frames + frame_offsets[f];
    const uint64_t fbytes = frame_offsets[f + 1] - frame_offsets[f];
    uint32_t flags = 0;
    for (uint32_t c = threadIdx.x; c < channels; c += blockDim.x)
        sub_info[c] = 0xFFFFFFFFu; // "no subframe delivered this channel"

    // ---- mode: every subframe of the frame must fit the fast plan ----------------------------------------------
    const bool fast_plan = channels <= (uint32_t)kDecMaxWaves;
    SubHeader hd = walk_headers(fb, fbytes, (uint32_t)wave < channels ? (uint32_t)wave : 0u);
    bool ok = block_header_ok(hd, channels);
    if (lane == 0)
        too_big[wave] = (fast_plan && (!ok || (hd.cw + 2 + hd.rw <= (uint32_t)kStreamCap && hd.order <= 2 * (uint32_t)kWave))) ? 0u : 1u;
    __syncthreads();
    bool fast = fast_plan;
    for (int w = 0; w < n_waves; w++)
        fast = fast && too_big[w] == 0;

    for (uint32_t c = wave; c < channels; c += n_waves) {
        if (c != (uint32_t)wave) {
            hd = walk_headers(fb, fbytes, c);
            ok = block_header_ok(hd, channels);
        }
        if (!ok) {
            flags |= SELA_HIP_FLAG_BAD_FRAME;
            continue;
        }
        DecSubframeLds* const sl = sub + c;
        const uint32_t nw = hd.cw + 2 + hd.rw;
        const uint32_t* const gw = reinterpret_cast<const uint32_t*>(fb + hd.p + 4); // the subframe's aligned words
        const int32_t* ws_c = nullptr;
        ParseProfile pp;
        if (fast) {
            for (uint32_t w = lane; w < nw + kStreamMargin; w += kWave) // the start bitmap
                sl->marks[w] = 0;
            wave_sync();
            const StreamWords sw = { gw, nw };
            flags |= parse_subframe<false>(sw, sl->marks, sl->pos, reinterpret_cast<uint16_t*>(&scratch->t), coef_values(scratch), hd.cw, hd.rw, hd.ck, hd.rk,
                hd.order, lane, pp);
        } else {
            int32_t* const wres = ws_residues + ((size_t)f * channels + c) * kBlock;
            const uint32_t n_frame_words = (uint32_t)((fbytes - hd.p - 4) / 4);
            flags |= parse_stream_serial(gw, 24, 24 + 32 * hd.cw, n_frame_words, hd.ck, hd.order, coef_values(scratch), lane);
            flags |= parse_stream_serial(gw, 32 * (hd.cw + 2), 32 * (hd.cw + 2 + hd.rw), n_frame_words, hd.rk, (uint32_t)kBlock, wres, lane);
            __threadfence(); // lane 0's stores to the workspace are read back by every lane
            ws_c = wres;
        }

        // dequantise (src/lpc/linear_predictor.cpp:16-28) + step-up
        SynthTables* const tables = &scratch->t;
        const uint32_t order = hd.order;
        const int32_t q_lo = (uint32_t)lane < order ? coef_values(scratch)[lane] : 0, q_hi = (uint32_t)lane + 64 < order ? coef_values(scratch)[lane + 64] : 0;
        wave_sync();
        // (the lane as dequant() sees it is made opaque here: the compiler otherwise selects the lane's table in front of the parse
        // and carries the pointer through it -- two spilled registers, which the budget of seven waves per SIMD does not have)
        int table_lane = lane;
        asm volatile("" : "+v"(table_lane));
        const double k_lo = (uint32_t)lane < order ? (order <= 1 ? 0.0 : dequant(table_lane, q_lo, flags)) : 0.0;
        const double k_hi = (uint32_t)lane + 64 < order ? dequant(table_lane + 64, q_hi, flags) : 0.0;
        step_up_regs(k_lo, k_hi, tables->a, (int)order, lane, flags);
        const bool fits24 = build_synth_table(tables->a, tables->tab, (int)order, lane);
        if (synth_priorities)
            set_wave_priority((int)((synth_priorities >> (order <= 48 ? 0 : (order <= 60 ? 8 : 16))) & 0xFF));
        if (vec_shift)
            synthesize_by_order<true>(order, gw, nw, hd.rk, sl->pos, ws_c, tables->tab, fits24, lane);
        else
            synthesize_by_order<false>(order, gw, nw, hd.rk, sl->pos, ws_c, tables->tab, fits24, lane);
        if (synth_priorities)
            __builtin_amdgcn_s_setprio(0);
        if (lane == 0)
            sub_info[hd.channel] = hd.type | (hd.parent << 8) | (c << 16);
    }
    __syncthreads();

    // ---- second pass of frame::FrameDecoder + interleave to int16, compared instead of stored ------------------------
    // What k_decode_frames would write at pcm_out[(f * 2048 + i) * channels + c] is held against pcm at the same place: the
    // values that differ are counted, the smallest differing i * channels + c is kept (a thread meets its indices in
    // ascending order: the first it finds is its smallest).
    uint32_t n_diff = 0, first = kNoDiff;
    const int16_t* const orig = pcm + (size_t)f * kBlock * channels;
    if (channels == 2 && ((uintptr_t)orig & 15) == 0) {
        // stereo: four samples of both channels per thread, one 16-byte load (wave-uniform case analysis)
        const uint32_t i0 = sub_info[0], i1 = sub_info[1];
        const bool have0 = i0 != 0xFFFFFFFFu, have1 = i1 != 0xFFFFFFFFu;
        const bool dep0 = have0 && (i0 & 0xFF) == 1, dep1 = have1 && (i1 & 0xFF) == 1;
        const uint32_t par0 = (i0 >> 8) & 0xFF, par1 = (i1 >> 8) & 0xFF; // parent channel of a dependent subframe (0 or 1, checked above)
        const uint2* s0 = reinterpret_cast<const uint2*>(sub[have0 ? i0 >> 16 : 0].smp);
        const uint2* s1 = reinterpret_cast<const uint2*>(sub[have1 ? i1 >> 16 : 0].smp);
        const uint4* in = reinterpret_cast<const uint4*>(orig);
        for (uint32_t i4 = threadIdx.x; i4 < (uint32_t)kBlock / 4; i4 += blockDim.x) {
            const uint4 o = in[i4];
            const uint2 zero = make_uint2(0, 0);
            const uint2 r0 = have0 ? s0[i4] : zero, r1 = have1 ? s1[i4] : zero; // raw subframe outputs, two samples per word
            // per 16-bit half: parent - difference (the parent's own, independent samples)
            auto sub16 = [](uint32_t a, uint32_t b) -> uint32_t { return ((a - (b & 0xFFFFu)) & 0xFFFFu) | ((a & 0xFFFF0000u) - (b & 0xFFFF0000u)); };
            uint2 a = r0, b = r1;
            if (dep0) {
                const uint2 pv = par0 == 0 ? r0 : r1;
                a = make_uint2(sub16(pv.x, r0.x), sub16(pv.y, r0.y));
            }
            if (dep1) {
                const uint2 pv = par1 == 0 ? r0 : r1;
                b = make_uint2(sub16(pv.x, r1.x), sub16(pv.y, r1.y));
            }
            // the four words the decoder stores (sample i: channel 0 | channel 1 << 16), against the original's
            const uint32_t x0 = ((a.x & 0xFFFFu) | (b.x << 16)) ^ o.x, x1 = ((a.x >> 16) | (b.x & 0xFFFF0000u)) ^ o.y;
            const uint32_t x2 = ((a.y & 0xFFFFu) | (b.y << 16)) ^ o.z, x3 = ((a.y >> 16) | (b.y & 0xFFFF0000u)) ^ o.w;
            if (x0 | x1 | x2 | x3) { // (rare: a handful of frames in thousands)
                const uint32_t x[4] = { x0, x1, x2, x3 };
#pragma unroll
                for (int w = 3; w >= 0; w--) { // (downwards: the smallest index is assigned last)
                    const uint32_t lo = x[w] & 0xFFFFu, hi = x[w] >> 16;
                    n_diff += (lo ? 1u : 0u) + (hi ? 1u : 0u);
                    if (x[w])
                        first = min(first, i4 * 8 + 2 * w + (lo ? 0u : 1u));
                }
            }
        }
    } else {
        for (uint32_t i = threadIdx.x; i < (uint32_t)kBlock; i += blockDim.x) {
            for (uint32_t c = 0; c < channels; c++) {
                const uint32_t info = sub_info[c];
                uint32_t v = info == 0xFFFFFFFFu ? 0u : (uint32_t)(uint16_t)sub[info >> 16].smp[i];
                if (info != 0xFFFFFFFFu && (info & 0xFF) == 1) {
                    const uint32_t pinfo = sub_info[(info >> 8) & 0xFF];
                    const uint32_t pv = pinfo == 0xFFFFFFFFu ? 0u : (uint32_t)(uint16_t)sub[pinfo >> 16].smp[i];
                    v = pv - v;
                }
                if ((uint16_t)v != (uint16_t)orig[(size_t)i * channels + c]) {
                    n_diff++;
                    first = min(first, i * channels + c);
                }
            }
        }
    }
    if (threadIdx.x == 0) {
        for (uint32_t c = 0; c < channels; c++) {
            const uint32_t info = sub_info[c];
            if (info == 0xFFFFFFFFu)
                flags |= SELA_HIP_FLAG_BAD_FRAME;
            else if ((info & 0xFF) == 1) {
                const uint32_t pinfo = sub_info[(info >> 8) & 0xFF];
                if (pinfo == 0xFFFFFFFFu || (pinfo & 0xFF) != 0)
                    // a parent that is itself dependent is refused by policy, as k_decode_frames refuses it.  (The reference defines a
                    // chain in stream order, and the 32-bit decoders decode it; against that order it reads an empty vector.)
                    flags |= SELA_HIP_FLAG_BAD_FRAME;
            }
        }
    }
    flags = wave_or(flags);
    if (lane == 0 && flags) {
        atomicOr(&status[0], flags);
        if (wave == 0 && (flags & SELA_HIP_FLAG_BAD_FRAME))
            atomicAdd(&status[1], 1u);
    }
    // within the wave, then across the waves through two words of each wave's synthesis table (dead behind the barrier above)
    n_diff = wave_sum_small(n_diff); // (at most 2048 * 8)
    first = wave_min_u32(first);
    uint32_t* const part = reinterpret_cast<uint32_t*>(&scratch->t);
    if (lane == 0)
        part[0] = n_diff, part[1] = first;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0, least = kNoDiff;
        for (int w = 0; w < n_waves; w++) {
            const uint32_t* const p = reinterpret_cast<const uint32_t*>(&scratch0[w].t);
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
size_t verify_lds_bytes(uint32_t channels) { return verify_lds_bytes_for(channels, decode_waves(channels)); }

hipError_t launch_verify_frames(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames, uint32_t channels, const int16_t* d_pcm,
    uint32_t* d_diff_counts, uint32_t* d_first_diff, uint32_t* d_status, void* d_workspace, hipStream_t stream, int recurrence_form, uint32_t synth_priorities,
    const uint32_t* d_n_found)
{
    if (n_frames == 0)
        return hipSuccess;
    if (channels == 0 || channels > (uint32_t)kDecMaxWaves)
        return hipErrorInvalidValue;
    const int n_waves = decode_waves(channels);
    int32_t* ws = reinterpret_cast<int32_t*>(((uintptr_t)d_workspace + 255) & ~(uintptr_t)255);
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
