// sela_decode32.hip -- k_decode_subframes32: subframes of ANY length decoded to 32-bit samples on the fast decoder's machinery
// (gfx950): the lane-parallel Rice parse and the tuned synthesis of sela_decode_core.inc with the length a run-time value.
// frame::FrameDecoder / sela_hip_decode_i32 and sela_hip_decode on streams whose frames are not 2048 samples long come here
// (sela_capi_generic.hip); k_generic_decode (sela_generic.hip, a serial walk) is only the judge of streams this kernel will not
// touch: misaligned or malformed frames, streams that run dry, coefficients outside the tables.
#include <hip/hip_runtime.h>

#include "sela_host.h"

#include "sela_synth.h"

namespace sela {

#include "sela_decode_core.inc"

#include "sela_segments.inc"

// ---- subframes of any length, 32-bit samples out ---------------------------------------------------------------------------------
// frame::FrameDecoder returns what the synthesis produces, untruncated (src/frame/frame_decoder.cpp:24-25,64-71), at each
// subframe's own samplesPerChannel, so the class -- and sela_hip_decode_i32 behind it -- cannot use k_decode_frames, whose
// samples pass through int16 and whose plan is 2048 samples.  One wave per subframe here:
//   * a subframe of at most 2048 samples whose words fit the parser's plan (every subframe the reference's CLI writes, and every
//     shorter one) runs the very parse and synthesis of k_decode_frames -- positions in LDS, residues decoded just in time;
//   * a longer one, or a stream beyond the plan, is parsed segment by segment (parse_segment above), the residues parked
//     where the samples will lie (dec_ws), and synthesised in place by the same recurrence with the length a run-time value.
// The samples land where k_generic_decode would have left them (dec_ws, info: k_generic_combine follows either).  The kernel
// takes a subframe or leaves it alone: anything it would have to judge -- a frame that is not whole words at an aligned
// place, a header the walk refuses, a stream that runs dry, a coefficient outside the tables or beyond int64 -- is counted in
// status[2], and the caller then runs the whole chunk on k_generic_decode, which knows what the reference does with such streams.
template <bool kVecShift>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(7, 8))) void k_decode_subframes32(const uint8_t* __restrict__ frames,
    const uint64_t* __restrict__ frame_offsets, uint64_t base_bytes, uint32_t n_frames, uint32_t channels, uint32_t stride,
    int32_t* __restrict__ dec_ws /* [n_frames][channels][stride] by subframe position */, GenericSubInfo* __restrict__ info, uint32_t* __restrict__ status,
    uint32_t standard_path /* 0: every subframe by segments (tests) */,
    const uint32_t* __restrict__ n_frames_found /* or null: frames from *n_frames_found on are not decoded (sela_hip_decode_payload_i32_device) */)
{
    __shared__ __attribute__((aligned(16))) DecSubframeLds sl;
    __shared__ DecWaveScratch scratch;
    const uint32_t sub = blockIdx.x;
    if (sub >= n_frames * channels)
        return;
    const int lane = threadIdx.x;
    const uint32_t f = sub / channels, c = sub % channels;
    if (n_frames_found && f >= *n_frames_found)
        return;
    const uint64_t at = frame_offsets[f] - base_bytes;
    const uint8_t* const fb = frames + at;
    const uint64_t fbytes = frame_offsets[f + 1] - frame_offsets[f];
    const SubHeader hd = walk_headers(fb, (at & 3) == 0 ? fbytes : 0 /* a frame at a place that is not word-aligned: not walked */, c);
    const bool mine = hd.ok && sela_subframe_decodable(&hd) && hd.n <= stride && hd.n != 0 && hd.n > hd.order; // (a subframe not longer than its order: the reference writes past its vector -- the judge's)
    uint32_t flags = 0;
    if (mine) {
        const uint32_t nw = hd.cw + 2 + hd.rw;
        const uint32_t* const gw = reinterpret_cast<const uint32_t*>(fb + hd.p + 4); // the subframe's aligned words
        SynthTables* const tables = &scratch.t;
        const uint32_t order = hd.order;
        int32_t* const samples = dec_ws + (size_t)sub * stride;
        // (in one piece: up to 2048 samples whose words fit the parser's plan -- its positions are one 16-bit word per codeword)
        const bool standard = standard_path && hd.n <= (uint32_t)kBlock && nw <= (uint32_t)kStreamCap;
        if (standard) {
            for (uint32_t w = lane; w < nw + kStreamMargin; w += kWave) // the start bitmap
                sl.marks[w] = 0;
            wave_sync();
            ParseProfile pp;
            const StreamWords sw = { gw, nw };
            flags |= parse_subframe<false>(sw, sl.marks, sl.pos, reinterpret_cast<uint16_t*>(tables), coef_values(&scratch), hd.cw, hd.rw, hd.ck, hd.rk, order, lane, pp, hd.n);
        } else {
            // the coefficients (src/frame/frame_decoder.cpp:19-23): bits [24, 24 + 32 cw) of the aligned words
            if (order)
                flags |= parse_stream_segments(gw, nw, 24, 24 + 32 * hd.cw, hd.ck, order, (256 * hd.cw + order - 1) / order + 1, &sl, reinterpret_cast<uint16_t*>(tables),
                    coef_values(&scratch), lane);
            // the residues (:24-29): bits [32 (cw + 2), 32 (cw + 2 + rw)), parked where the samples will lie
            if (hd.n)
                flags |= parse_stream_segments(gw, nw, 32 * (hd.cw + 2), 32 * nw, hd.rk, hd.n, (256 * hd.rw + hd.n - 1) / hd.n + 1, &sl, reinterpret_cast<uint16_t*>(tables),
                    samples, lane);
            // the lanes read each other's residues back: the stores have left the CU, nothing older is served from its vector cache
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        }
        const int32_t q_lo = (uint32_t)lane < order ? coef_values(&scratch)[lane] : 0, q_hi = (uint32_t)lane + 64 < order ? coef_values(&scratch)[lane + 64] : 0;
        wave_sync();
        const bool fits24 = predictor_table(order, q_lo, q_hi, tables, lane, flags);
        SynthOut<true> out32;
        out32.samples = samples;
        out32.n = hd.n;
        flags = wave_or(flags);
        if (flags == 0) // (a stream in trouble is the other kernel's)
            synthesize_by_order<kVecShift, true>(order, gw, nw, hd.rk, sl.pos, standard ? nullptr : samples, tables->tab, fits24, lane, out32);
    }
    flags = wave_or(flags);
    if (lane == 0) {
        GenericSubInfo si;
        si.channel = (uint8_t)hd.channel, si.type = (uint8_t)hd.type, si.parent = (uint8_t)hd.parent, si.n = hd.n;
        si.ok = mine && flags == 0 ? 1 : 0;
        if (!si.ok) {
            si.channel = si.type = si.parent = 0, si.n = 0;
            atomicAdd(&status[2], 1u);
        } else if (!(hd.n <= (uint32_t)kBlock && hd.cw + 2 + hd.rw <= (uint32_t)kStreamCap && standard_path))
            atomicAdd(&status[3], 1u); // (subframes that went by segments: tests and the probes ask)
        info[sub] = si;
    }
}

// ---- lpc::SampleGenerator on its own for any length (src/lpc/sample_generator.cpp:11-39; src/include/lpc.hpp:106-117): order +
// quantised reflection coefficients + n residues -> n samples, one wave per block, through the very dequantisation, step-up,
// table and recurrence the frame kernels run; the samples go out as the 32-bit values the reference's class returns.
__global__ __launch_bounds__(64) void k_lpc_decode_any(const int32_t* __restrict__ order_in, const int32_t* __restrict__ q_in, const int32_t* __restrict__ residues,
    uint32_t n_blocks, uint32_t n, int32_t* __restrict__ samples_out, int64_t* __restrict__ coefs_out /* [block][101] or null */, uint32_t* __restrict__ status)
{
    __shared__ DecWaveScratch scratch;
    const uint32_t b = blockIdx.x;
    if (b >= n_blocks)
        return;
    const int lane = threadIdx.x;
    uint32_t flags = 0;
    const int32_t o = order_in[b];
    if (o < 0 || o > kMaxOrder) {
        if (lane == 0)
            atomicOr(&status[0], (uint32_t)SELA_HIP_FLAG_BAD_FRAME);
        return;
    }
    const uint32_t order = (uint32_t)o;
    if (samples_out && (n == 0 || n <= order)) // src/lpc/sample_generator.cpp:14-22 writes samples[0] and samples[1 .. order]: past its vector
        flags |= SELA_HIP_FLAG_SHORT_BLOCK;
    const int32_t q_lo = (uint32_t)lane < order ? q_in[(size_t)b * kMaxOrder + lane] : 0;
    const int32_t q_hi = (uint32_t)lane + 64 < order ? q_in[(size_t)b * kMaxOrder + lane + 64] : 0;
    SynthTables* const tables = &scratch.t;
    step_up_from_q(order, q_lo, q_hi, tables->a, lane, flags);
    if (coefs_out) // lpc::LinearPredictor::linearPredictionCoefficients (src/lpc/linear_predictor.cpp:57-60)
        for (uint32_t i = lane; i <= order; i += kWave)
            coefs_out[(size_t)b * (kMaxOrder + 1) + i] = tables->a[i];
    if (samples_out) {
        const bool fits24 = build_synth_table(tables->a, tables->tab, (int)order, lane);
        SynthOut<true> out32;
        out32.samples = samples_out + (size_t)b * n;
        out32.n = n;
        synthesize_by_order<false, true>(order, nullptr, 0, 0, nullptr, residues + (size_t)b * n, tables->tab, fits24, lane, out32);
    }
    flags = wave_or(flags);
    if (lane == 0 && flags)
        atomicOr(&status[0], flags);
}

hipError_t launch_decode_subframes32(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint64_t base_bytes, uint32_t n_frames, uint32_t channels,
    uint32_t stride, int32_t* d_dec, GenericSubInfo* d_info, uint32_t* d_status, bool standard_path, hipStream_t stream, const uint32_t* d_n_found)
{
    const uint64_t subs = (uint64_t)n_frames * channels;
    if (subs == 0)
        return hipSuccess;
    if (subs <= kLonelyWaves) // (the recurrence's form for waves that have their SIMD nearly to themselves, vec_shift_from_for)
        hipLaunchKernelGGL(k_decode_subframes32<true>, dim3((uint32_t)subs), dim3(64), 0, stream, d_frames, d_frame_offsets, base_bytes, n_frames, channels, stride, d_dec,
            d_info, d_status, standard_path ? 1u : 0u, d_n_found);
    else
        hipLaunchKernelGGL(k_decode_subframes32<false>, dim3((uint32_t)subs), dim3(64), 0, stream, d_frames, d_frame_offsets, base_bytes, n_frames, channels, stride, d_dec,
            d_info, d_status, standard_path ? 1u : 0u, d_n_found);
    return hipGetLastError();
}

hipError_t launch_lpc_decode_any(const int32_t* d_order, const int32_t* d_q, const int32_t* d_residues, uint32_t n_blocks, uint32_t n, int32_t* d_samples,
    int64_t* d_coefs, uint32_t* d_status, hipStream_t stream)
{
    if (n_blocks)
        hipLaunchKernelGGL(k_lpc_decode_any, dim3(n_blocks), dim3(64), 0, stream, d_order, d_q, d_residues, n_blocks, n, d_samples, d_coefs, d_status);
    return hipGetLastError();
}

} // namespace sela
