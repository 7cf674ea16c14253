// sela_envelope.hip -- the envelope of a .sela stream, measured on the device: per frame, bucket of samples and channel the smallest
// and the largest value, the sum and the sum of squares of the int16 samples sela_hip_decode_n_device would write (gfx950;
// DESIGN.md 5.31).  A bucket is a power of two from 32 to 2048 samples, so a frame of 2048 samples holds 64 .. 1 of them.  The
// launches are the int16 family's sequence (launch_n_sequence, sela_generic.hip); launch_envelope_n_device plugs in
//
//   k_envelope_frames     the fused kernel: k_level_frames (sela_levels.hip) with a segmented reduction for its total.  One
//                         workgroup per frame, one wave per subframe: frame_prologue and decode_subframe of sela_decode_core.inc,
//                         the barrier, then the shared second pass -- and where the decoder stores a frame's interleaved int16
//                         samples, a wave takes a run of consecutive samples (a "chunk": a bucket, or several small ones side by
//                         side), reduces it over the groups of lanes that hold a bucket each, and writes those buckets' records.
//                         Nothing crosses waves, so there is no second barrier and no partial result in LDS; no decoded sample
//                         reaches global memory; the LDS plan is the decoder's, so the occupancy is the decoder's too.
//   k_envelope_channels   the same records from PCM that another kernel decoded into the workspace: the routes that are not fused
//                         (frames of any other length, frames of more than eight channels).  One workgroup per (frame, channel),
//                         a wave per bucket; it writes every slot of the frame, the zero records behind the frame's end too.
//
// Every figure is an integer, so it is exact and does not depend on the order of the additions.  A bucket has at most 2048
// samples: |sum| <= 2^26, sum_squares <= 2^41, and the two 15-bit halves of v * v <= 2^30 each add up to less than 2^26, so a
// 32-bit ladder per half carries the energy.
#include "sela_host.h"

#include "sela_group_reduce.h"
#include "sela_synth.h"

namespace sela {

#include "sela_decode_core.inc"

static_assert(kVerifyFusedChannels == (uint32_t)kDecMaxWaves, "the fused route takes what k_decode_frames takes");
static_assert(sizeof(struct sela_hip_envelope) == 16 && alignof(struct sela_hip_envelope) == 8, "the record of include/sela_hip.h");
static_assert(offsetof(struct sela_hip_envelope, min) == 0 && offsetof(struct sela_hip_envelope, max) == 2 && offsetof(struct sela_hip_envelope, sum) == 4
        && offsetof(struct sela_hip_envelope, sum_squares) == 8,
    "the words of a record");
static_assert(kEnvelopeMinBucket == 32 && kEnvelopeMaxBucket == (uint32_t)kBlock, "a 2048-sample frame holds whole buckets");

// What a lane, then a group of lanes, has seen of one bucket of one channel.  The extremes are kept biased so that both are
// unsigned maxima with 0 for "nothing seen": hi = v + 32768, lo = 32767 - v (0 .. 65535 each).
struct EnvelopeAcc {
    uint32_t hi = 0, lo = 0;
    uint32_t sum = 0;               // (mod 2^32: |sum| <= 2^26)
    uint32_t sq_low = 0, sq_high = 0; // the low 15 bits of v * v, and the rest, added separately
    __device__ __forceinline__ void take(int32_t v)
    {
        hi = max(hi, (uint32_t)(v + 32768));
        lo = max(lo, (uint32_t)(32767 - v));
        sum += (uint32_t)v;
        const uint32_t sq = (uint32_t)(v * v); // (32768^2 = 2^30)
        sq_low += sq & 0x7FFFu;
        sq_high += sq >> 15;
    }
    // word k of the record (little-endian: min | max << 16 | sum << 32, then sum_squares)
    __device__ __forceinline__ uint64_t word(uint32_t k) const
    {
        const uint32_t mn = (32767u - lo) & 0xFFFFu, mx = (hi - 32768u) & 0xFFFFu;
        return k == 0 ? ((uint64_t)sum << 32) | (mx << 16) | mn : ((uint64_t)sq_high << 15) + sq_low;
    }
};

// (group_reduce on one value per lane: sela_group_reduce.h)
__device__ __forceinline__ EnvelopeAcc group_reduce(const EnvelopeAcc& a, uint32_t lanes)
{
    const auto add = [](uint32_t x, uint32_t y) { return x + y; };
    const auto top = [](uint32_t x, uint32_t y) { return max(x, y); };
    EnvelopeAcc r;
    r.hi = group_reduce(a.hi, lanes, top);
    r.lo = group_reduce(a.lo, lanes, top);
    r.sum = group_reduce(a.sum, lanes, add);
    r.sq_low = group_reduce(a.sq_low, lanes, add);
    r.sq_high = group_reduce(a.sq_high, lanes, add);
    return r;
}

__global__ __launch_bounds__(kDecMaxWaves * 64) __attribute__((amdgpu_waves_per_eu(7, 8))) void k_envelope_frames(const uint8_t* __restrict__ frames,
    const uint64_t* __restrict__ frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t bucket /* 32 .. 2048, a power of two */,
    uint32_t slots /* records per frame and channel: ceil(stride / bucket) >= 2048 / bucket */, struct sela_hip_envelope* __restrict__ env /* [n_frames][slots][channels] */,
    uint32_t* __restrict__ status, int32_t* __restrict__ ws_residues, uint32_t vec_shift_from /* as in k_decode_frames */,
    uint32_t synth_priorities /* as in k_decode_frames */, const uint32_t* __restrict__ n_frames_found /* or null: frames from *n_frames_found on are left alone */)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    const int n_waves = blockDim.x / 64;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / 64)), lane = threadIdx.x % 64;
    const DecFrameLds l = carve_frame_lds(dyn, channels, n_waves);

    const uint32_t f = blockIdx.x;
    // (a stride below 2048 has no room for this route's records: k_route_n gives the route no frames then, and this holds it to that)
    if (f >= n_frames || (n_frames_found && f >= *n_frames_found) || slots < (uint32_t)kBlock / bucket)
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

    // ---- the second pass, reduced per bucket instead of stored --------------------------------------------------------
    // What k_decode_frames would write at pcm_out[(f * 2048 + i) * channels + c] goes into record [f][i / bucket][c].  A wave's
    // step covers `span` consecutive samples, a lane `each` of them (stereo: stereo_words' four of both channels; else one of one
    // channel), so a bucket lies on `lanes` = min(bucket, span) / each consecutive lanes.  A wave takes whole chunks of
    // max(bucket, span) samples: the lanes add up the chunk's steps, group_reduce joins the lanes of a bucket, and the last lanes
    // of each group write that bucket's record, one 8-byte word a lane.
    uint64_t* const out = reinterpret_cast<uint64_t*>(env + (size_t)f * slots * channels);
    const bool stereo = channels == 2;
    const uint32_t each = stereo ? 4u : 1u, span = 64u * each;
    const uint32_t chunk = max(bucket, span), steps = chunk / span, lanes = min(bucket, span) / each;
    const uint32_t chunks = (uint32_t)kBlock / chunk, chunks_shift = (uint32_t)__builtin_ctz(chunks);
    const uint32_t in_group = (uint32_t)lane & (lanes - 1);
    const uint32_t b_in_chunk = (uint32_t)lane / lanes; // (chunk / bucket buckets in a chunk: 1 unless the bucket is below the span)
    if (stereo) {
        const StereoPass sp = stereo_pass(l.sub, l.sub_info);
        for (uint32_t q = (uint32_t)wave; q < chunks; q += (uint32_t)n_waves) {
            EnvelopeAcc a0, a1;
            for (uint32_t j = 0; j < steps; j++) {
                const uint4 w = stereo_words(sp, q * (chunk / 4) + j * 64 + (uint32_t)lane);
                const uint32_t x[4] = { w.x, w.y, w.z, w.w };
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    a0.take((int32_t)(int16_t)(x[k] & 0xFFFFu));
                    a1.take((int32_t)x[k] >> 16);
                }
            }
            const EnvelopeAcc r0 = group_reduce(a0, lanes), r1 = group_reduce(a1, lanes);
            // the group's last four lanes: channel 0's two words, then channel 1's -- 32 consecutive bytes
            const uint32_t k = in_group - (lanes - 4);
            if (in_group >= lanes - 4) {
                const uint32_t b = q * (chunk / bucket) + b_in_chunk;
                out[(size_t)b * 4 + k] = k < 2 ? r0.word(k) : r1.word(k - 2);
            }
        }
    } else {
        for (uint32_t item = (uint32_t)wave; item < channels * chunks; item += (uint32_t)n_waves) {
            const uint32_t c = item >> chunks_shift, q = item & (chunks - 1);
            EnvelopeAcc a;
            for (uint32_t j = 0; j < steps; j++)
                a.take((int32_t)(int16_t)channel_value16(l.sub, l.sub_info, c, q * chunk + j * 64 + (uint32_t)lane));
            const EnvelopeAcc r = group_reduce(a, lanes);
            const uint32_t k = in_group - (lanes - 2);
            if (in_group >= lanes - 2) {
                const uint32_t b = q * (chunk / bucket) + b_in_chunk;
                out[((size_t)b * channels + c) * 2 + k] = r.word(k);
            }
        }
    }
    // the slots behind the frame's 2048 samples (a stride above 2048): zero records
    const uint32_t filled = (uint32_t)kBlock / bucket;
    for (uint32_t k = filled * channels * 2 + threadIdx.x; k < slots * channels * 2; k += blockDim.x)
        out[k] = 0;

    if (threadIdx.x == 0)
        flags |= layout_flags(l.sub_info, channels);
    flags = wave_or(flags);
    if (lane == 0 && flags) {
        atomicOr(&status[0], flags);
        if (wave == 0 && (flags & SELA_HIP_FLAG_BAD_FRAME))
            atomicAdd(&status[1], 1u);
    }
}

// ---- PCM another kernel decoded ---------------------------------------------------------------------------------------------
// One workgroup per (frame, channel), a wave per bucket: frame f's values lie at sample_offsets[f] * channels, interleaved (a
// strided 2-byte read: this is the cold route).  Every one of the frame's `slots` records is written: a partial last bucket over
// the samples it has, zero records from the frame's end on.  Frames from *n_a + *n_b on are left alone (the device's count of the
// route that ran: the other route's is 0 -- k_level_channels' rule).
constexpr uint32_t kEnvelopeThreads = 256;

__global__ __launch_bounds__(kEnvelopeThreads) void k_envelope_channels(const int16_t* __restrict__ decoded, const uint64_t* __restrict__ sample_offsets,
    uint32_t max_frames, uint32_t channels, uint32_t stride, uint32_t bucket, uint32_t slots, const uint32_t* __restrict__ n_a,
    const uint32_t* __restrict__ n_b /* or null */, struct sela_hip_envelope* __restrict__ env /* [max_frames][slots][channels] */)
{
    const uint32_t f = blockIdx.x, c = blockIdx.y;
    if (f >= min(*n_a + (n_b ? *n_b : 0u), max_frames))
        return;
    const uint64_t so = sample_offsets[f], in_frame = sample_offsets[f + 1] - so;
    const uint32_t n = (uint32_t)min(in_frame, (uint64_t)stride); // (never more than the decoder wrote)
    const int16_t* const d = decoded + so * channels + c;
    const uint32_t lane = threadIdx.x % 64;
    struct sela_hip_envelope* const out = env + (size_t)f * slots * channels + c; // slot b: out[b * channels]
    const uint32_t used = (n + bucket - 1) / bucket;                              // the slots that hold samples (<= slots: n <= stride)
    for (uint32_t b = threadIdx.x / 64; b < used; b += kEnvelopeThreads / 64) {
        const uint32_t from = b * bucket, to = min(from + bucket, n);
        EnvelopeAcc a;
        for (uint32_t i = from + lane; i < to; i += 64)
            a.take((int32_t)d[(size_t)i * channels]);
        EnvelopeAcc r;
        r.hi = wave_max_u32(a.hi), r.lo = wave_max_u32(a.lo);
        r.sum = wave_sum_small(a.sum), r.sq_low = wave_sum_small(a.sq_low), r.sq_high = wave_sum_small(a.sq_high);
        if (lane < 2) // (a lane per word of the record)
            reinterpret_cast<uint64_t*>(out + (size_t)b * channels)[lane] = r.word(lane);
    }
    // the slots at and behind the frame's end: zero records, a thread per word, no reduction
    for (uint64_t k = (uint64_t)used * 2 + threadIdx.x; k < (uint64_t)slots * 2; k += kEnvelopeThreads)
        reinterpret_cast<uint64_t*>(out + (size_t)(k / 2) * channels)[k & 1] = 0;
}

// the dynamic LDS launch_envelope_frames asks for (sela_hip_debug_envelope_lds_bytes: tests hold it against the decoder's)
size_t envelope_lds_bytes(uint32_t channels) { return decode_lds_bytes_for(channels, decode_waves(channels)); }

hipError_t launch_envelope_frames(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride, uint32_t bucket,
    struct sela_hip_envelope* d_env, uint32_t* d_status, void* d_workspace, hipStream_t stream, int recurrence_form, uint32_t synth_priorities, const uint32_t* d_n_found)
{
    if (n_frames == 0)
        return hipSuccess;
    const uint32_t slots = envelope_slots(stride, bucket);
    if (channels == 0 || channels > (uint32_t)kDecMaxWaves || slots == 0)
        return hipErrorInvalidValue;
    const int n_waves = decode_waves(channels);
    Carve carve(d_workspace); // (launch_decode's workspace: the route's kernel with a reduction for its stores)
    int32_t* const ws = carve_decode(carve, n_frames, channels);
    const size_t lds = envelope_lds_bytes(channels);
    if (lds > 64 * 1024) { // above the default dynamic-LDS limit (more than four channels); per device, so every time
        const hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(k_envelope_frames), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (err != hipSuccess)
            return err;
    }
    const uint32_t from = recurrence_form >= 0
        ? (recurrence_form ? 0u : n_frames)
        : vec_shift_from_for(n_frames, n_waves, resident_frames(reinterpret_cast<const void*>(k_envelope_frames), n_waves, lds, kResidencyEnvelope));
    hipLaunchKernelGGL(k_envelope_frames, dim3(n_frames), dim3(n_waves * 64), lds, stream, d_frames, d_frame_offsets, n_frames, channels, bucket, slots, d_env, d_status,
        ws, from, synth_priorities, d_n_found);
    return hipGetLastError();
}

hipError_t launch_envelope_channels(const int16_t* d_decoded, const uint64_t* d_sample_offsets, uint32_t max_frames, uint32_t channels, uint32_t stride, uint32_t bucket,
    const uint32_t* d_n_a, const uint32_t* d_n_b, struct sela_hip_envelope* d_env, hipStream_t stream)
{
    if (max_frames == 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_envelope_channels, dim3(max_frames, channels), dim3(kEnvelopeThreads), 0, stream, d_decoded, d_sample_offsets, max_frames, channels, stride,
        bucket, envelope_slots(stride, bucket), d_n_a, d_n_b, d_env);
    return hipGetLastError();
}

} // namespace sela

extern "C" size_t sela_hip_debug_envelope_lds_bytes(uint32_t channels)
{
    return channels == 0 || channels > sela::kVerifyFusedChannels ? 0 : sela::envelope_lds_bytes(channels);
}
