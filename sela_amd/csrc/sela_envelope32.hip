// sela_envelope32.hip -- the envelope of a 24- or 32-bit .sela stream, measured on the device: per frame, bucket of samples and
// channel the smallest and the largest value, the sum and the 128-bit sum of squares of the int32 samples
// sela_hip_decode_i32_device would write (gfx950).  A bucket is a power of two from 32 to 2048 samples.
//
// sela_hip_envelope_i32_device is sela_hip_levels_i32_device (sela_levels32.hip, 5.27) with sela_envelope.hip's segmented
// reduction for its total.  The launches are the int32 family's sequence (launch_i32_sequence, sela_generic.hip);
// launch_envelope_i32_device plugs in k_level32_begin as it is (status[2] = 0 and the two control words) and
//
//   k_envelope32_direct  one workgroup per (frame, slice of kVerify32Slice samples).  verify32_judge_layout decides whether the
//                        layout is DIRECT; for such a frame the value of channel c at i is dec[pos(c)][i], or dec[pos(parent)][i] -
//                        dec[pos(c)][i] mod 2^32: formed in registers.  No decoded sample is written.  Any other frame is marked
//                        and counted.
//   k_envelope32_rest    the marked frames, from the combine's samples and counts; with no marks and no control words, every frame
//                        of planar samples that already lie in device memory (sela_hip_envelope_samples_i32_device).
//
// Every bucket divides kVerify32Slice, so a slice holds whole buckets: a workgroup writes its buckets' final records straight
// into the caller's array -- no partial record in the workspace, no kernel that adds slices up.  A wave takes a "chunk" of
// max(bucket, span) consecutive samples of one channel (span: what the 64 lanes load in one step, 256 samples as int4s, 64
// otherwise): the lanes add up the chunk's steps, group_reduce joins the lanes that hold a bucket, and the last four lanes of
// each group store the record's four 8-byte words.  Nothing crosses waves; a chunk at or beyond the channel's end gets its zero
// words from a lane each, without a reduction.
//
// Every figure is an integer, so it is exact and does not depend on the launch's shape.  A bucket has at most 2048 samples:
// |sum| <= 2^42, sum_squares <= 2^73.  A lane holds up to 32 samples: its energy is a 64-bit low word and a count of its carries
// (four full-scale samples pass 2^64), its sum 64 bits; across the group both go as limbs of at most 22 bits (64 lanes of 2^22
// stay below 2^28), put together with their carries.  The extremes are kept biased, so that a lane that holds nothing of a bucket
// changes nothing: a sample that is not there is not a 0.
#include "sela_host.h"
#include "sela_group_reduce.h"
#include "sela_verify32_rule.h"

namespace sela {

namespace {

static_assert(sizeof(struct sela_hip_envelope32) == 32 && alignof(struct sela_hip_envelope32) == 8, "the record of include/sela_hip.h");
static_assert(offsetof(struct sela_hip_envelope32, min) == 0 && offsetof(struct sela_hip_envelope32, max) == 4 && offsetof(struct sela_hip_envelope32, sum) == 8
        && offsetof(struct sela_hip_envelope32, sum_squares_lo) == 16 && offsetof(struct sela_hip_envelope32, sum_squares_hi) == 24,
    "the words of a record");
static_assert(kVerify32Slice % kEnvelopeMaxBucket == 0 && kEnvelopeMinBucket == 32, "a slice holds whole buckets; a bucket holds whole groups of lanes");

constexpr uint32_t kRecordWords = 4;

// What a lane, then a group of lanes, has seen of one bucket of one channel.  The extremes are biased so that both are unsigned
// maxima with 0 for "nothing seen": hi = v + 2^31, lo = 2^31 - 1 - v (0 .. 2^32 - 1 each).
struct Envelope32Acc {
    uint32_t hi = 0, lo = 0;
    uint32_t carries = 0; // how often `low` wrapped; in a group's total: bits 64 .. of the energy
    uint64_t sum = 0;     // (mod 2^64: |sum| <= 2^42)
    uint64_t low = 0;
    // (on false: an element of a vector at or beyond the channel's end -- it is skipped by selects, so that the 16-byte load stays one)
    __device__ __forceinline__ void take(int32_t v, bool on = true)
    {
        hi = max(hi, on ? (uint32_t)v ^ 0x80000000u : 0u);
        lo = max(lo, on ? 0x7FFFFFFFu - (uint32_t)v : 0u);
        v = on ? v : 0;
        sum += (uint64_t)(int64_t)v;
        const uint32_t a = v < 0 ? 0u - (uint32_t)v : (uint32_t)v; // (INT32_MIN: 2^31)
        const uint64_t sq = (uint64_t)a * a;
        low += sq;
        carries += low < sq ? 1u : 0u;
    }
    // word k of the record (little-endian: min | max << 32, sum, the energy's low word, its high word)
    __device__ __forceinline__ uint64_t word(uint32_t k) const
    {
        const uint32_t mn = 0x7FFFFFFFu - lo, mx = hi ^ 0x80000000u;
        return k == 0 ? ((uint64_t)mx << 32) | mn : (k == 1 ? sum : (k == 2 ? low : (uint64_t)carries));
    }
};

// (the name is its own: one declared here would hide sela_group_reduce.h's)
__device__ __forceinline__ Envelope32Acc group_total(const Envelope32Acc& a, uint32_t lanes)
{
    const auto add = [](uint32_t x, uint32_t y) { return x + y; };
    const auto top = [](uint32_t x, uint32_t y) { return max(x, y); };
    Envelope32Acc r;
    r.hi = group_reduce(a.hi, lanes, top);
    r.lo = group_reduce(a.lo, lanes, top);
    // the sum, mod 2^64: limbs of 22, 22 and 20 bits
    const uint64_t s0 = group_reduce((uint32_t)a.sum & 0x3FFFFFu, lanes, add);
    const uint64_t s1 = group_reduce((uint32_t)(a.sum >> 22) & 0x3FFFFFu, lanes, add);
    const uint64_t s2 = group_reduce((uint32_t)(a.sum >> 44), lanes, add);
    r.sum = (s2 << 44) + (s1 << 22) + s0;
    // the energy, low + carries * 2^64 (a lane's is below 2^68): wave_sum_96's limbs, bits 0 .. 21, 22 .. 43, 44 .. 65, 66 ..
    const uint64_t l0 = group_reduce((uint32_t)a.low & 0x3FFFFFu, lanes, add);
    const uint64_t l1 = group_reduce((uint32_t)(a.low >> 22) & 0x3FFFFFu, lanes, add);
    const uint64_t l2 = group_reduce(((uint32_t)(a.low >> 44) | (a.carries << 20)) & 0x3FFFFFu, lanes, add);
    const uint32_t l3 = group_reduce(a.carries >> 2, lanes, add);
    r.low = l0 + (l1 << 22); // (below 2^51)
    const uint64_t l2_low = l2 << 44;
    r.low += l2_low;
    r.carries = (uint32_t)(l2 >> 20) + (r.low < l2_low ? 1u : 0u) + (l3 << 2);
    return r;
}

// The records of a frame's slice: `row(c, dec, par, n)` names channel c's samples -- dec, or par - dec mod 2^32 where par is not
// null, n of them.  kVec: the rows are 16-byte aligned and whole int4s long (stride % 4 == 0), so a lane takes four samples per
// load -- the last vector of a channel may reach beyond its end, never beyond the row: what lies there is not taken.  out: the
// frame's records, [slots][channels][kRecordWords]; this slice writes every word of its own slots (those below `slots`) once.
template <bool kVec, typename Row>
__device__ __forceinline__ void envelope_slice(uint32_t channels, uint32_t slice, bool refused, uint32_t bucket, uint32_t slots, uint64_t* __restrict__ out, Row row)
{
    constexpr uint32_t each = kVec ? 4u : 1u, span = 64u * each;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / 64)), lane = threadIdx.x % 64;
    const uint32_t chunk = max(bucket, span), steps = chunk / span, lanes = min(bucket, span) / each;
    const uint32_t per_chunk = chunk / bucket; // the buckets of a chunk: 1 unless the bucket is below the span
    const uint32_t lo = slice * kVerify32Slice, first_slot = lo / bucket;
    const uint32_t slice_slots = min(slots - first_slot, kVerify32Slice / bucket); // (first_slot < slots: lo < stride)
    const uint32_t chunks = (slice_slots + per_chunk - 1) / per_chunk;
    const uint32_t in_group = lane & (lanes - 1), b_in_chunk = lane / lanes;
    for (uint32_t item = wave; item < channels * chunks; item += kV32Waves) {
        const uint32_t c = item / chunks, q = item - c * chunks;
        const int32_t *dec, *par;
        uint32_t n;
        row(c, dec, par, n);
        const uint32_t end = refused ? 0u : min(n, lo + kVerify32Slice);
        const uint32_t from = lo + q * chunk, b0 = first_slot + q * per_chunk;
        if (from >= end) { // nothing of the channel here: zero words, a lane each
            const uint32_t b = b0 + lane / kRecordWords;
            if (lane < per_chunk * kRecordWords && b < slots)
                out[((size_t)b * channels + c) * kRecordWords + lane % kRecordWords] = 0;
            continue;
        }
        Envelope32Acc a;
        for (uint32_t j = 0; j < steps; j++) {
            const uint32_t i = from + j * span + lane * each;
            if (i >= end)
                continue;
            if (kVec) {
                int4 v = *reinterpret_cast<const int4*>(dec + i);
                if (par) {
                    const int4 p = *reinterpret_cast<const int4*>(par + i);
                    v.x = (int32_t)((uint32_t)p.x - (uint32_t)v.x), v.y = (int32_t)((uint32_t)p.y - (uint32_t)v.y);
                    v.z = (int32_t)((uint32_t)p.z - (uint32_t)v.z), v.w = (int32_t)((uint32_t)p.w - (uint32_t)v.w);
                }
                const uint32_t left = end - i;
                a.take(v.x);
                a.take(v.y, left > 1);
                a.take(v.z, left > 2);
                a.take(v.w, left > 3);
            } else {
                const int32_t d = dec[i];
                a.take(par ? (int32_t)((uint32_t)par[i] - (uint32_t)d) : d);
            }
        }
        const Envelope32Acc r = group_total(a, lanes);
        // the group's last four lanes: the record's four words -- 32 consecutive bytes.  A bucket of the chunk that lies at or
        // beyond the channel's end was reduced over nothing: its words are zeros, not the identity's extremes.
        const uint32_t b = b0 + b_in_chunk;
        if (in_group >= lanes - kRecordWords && b < slots) {
            const uint32_t k = in_group - (lanes - kRecordWords);
            out[((size_t)b * channels + c) * kRecordWords + k] = b * bucket >= end ? 0 : r.word(k);
        }
    }
}

template <bool kVec>
__global__ __launch_bounds__(kV32Threads) void k_envelope32_direct(const int32_t* __restrict__ dec_ws /* [frames][channels][stride] by position */,
    const GenericSubInfo* __restrict__ info, uint32_t max_frames, uint32_t channels, uint32_t stride, uint32_t bucket, uint32_t slots,
    const uint32_t* __restrict__ status, const uint32_t* __restrict__ n_frames_found /* or null */, uint32_t* __restrict__ ctl, uint32_t* __restrict__ marks /* [frames] */,
    uint64_t* __restrict__ env /* [max_frames][slots][channels][4] */)
{
    __shared__ uint32_t s_named[256], s_n[256]; // by channel: the subframes that name it, its subframe's length
    __shared__ uint16_t s_pos[256], s_ppos[256]; // by channel: its subframe's position, its parent's (kV32NoParent: independent)
    __shared__ uint32_t s_other;
    const uint32_t f = blockIdx.x, t = threadIdx.x;
    if (f >= frames_in_call(n_frames_found, max_frames))
        return;
    const size_t row = (size_t)f * channels;
    verify32_judge_layout(info + row, channels, t, s_named, s_n, s_pos, s_ppos, s_other);
    const bool first_slice = blockIdx.y == 0;
    if (s_other) { // the fallback's: marked and counted once
        if (first_slice && t == 0) {
            marks[f] = 1;
            atomicAdd(&ctl[0], 1u);
        }
        return;
    }
    if (first_slice && t == 0)
        marks[f] = 0;
    const bool refused = (status[0] & SELA_HIP_FLAG_STRIDE) != 0; // (refused for its stride: nothing is read)
    envelope_slice<kVec>(channels, blockIdx.y, refused, bucket, slots, env + (size_t)f * slots * channels * kRecordWords,
        [&](uint32_t c, const int32_t*& dec, const int32_t*& par, uint32_t& n) {
            dec = dec_ws + (row + s_pos[c]) * stride;
            par = s_ppos[c] == kV32NoParent ? nullptr : dec_ws + (row + s_ppos[c]) * stride;
            n = min(s_n[c], stride);
        });
}

// Samples by channel with their counts: the marked frames as k_generic_combine<false> left them in the workspace (frames below
// ctl[1]), or, with no marks, every frame of the caller's samples (counts or null: stride).
template <bool kVec>
__global__ __launch_bounds__(kV32Threads) void k_envelope32_rest(const int32_t* __restrict__ all /* [frames][channels][stride] by channel */,
    const uint32_t* __restrict__ counts /* or null */, uint32_t max_frames, uint32_t channels, uint32_t stride, uint32_t bucket, uint32_t slots,
    const uint32_t* __restrict__ status /* or null */, const uint32_t* __restrict__ ctl /* or null */, const uint32_t* __restrict__ marks /* or null */,
    uint64_t* __restrict__ env)
{
    const uint32_t f = blockIdx.x;
    if (f >= (ctl ? min(ctl[1], max_frames) : max_frames) || (marks && !marks[f]))
        return;
    const size_t row = (size_t)f * channels;
    const bool refused = status && (status[0] & SELA_HIP_FLAG_STRIDE) != 0;
    envelope_slice<kVec>(channels, blockIdx.y, refused, bucket, slots, env + (size_t)f * slots * channels * kRecordWords,
        [&](uint32_t c, const int32_t*& dec, const int32_t*& par, uint32_t& n) {
            dec = all + (row + c) * stride;
            par = nullptr;
            n = counts ? min(counts[row + c], stride) : stride;
        });
}

// int4 loads: every row starts at a multiple of 16 bytes (the workspace's pieces are 256-byte aligned)
bool rows_are_vectors32(const int32_t* d_rows, uint32_t stride) { return stride % 4 == 0 && ((uintptr_t)d_rows & 15) == 0; }

} // namespace

hipError_t launch_envelope32_direct(const int32_t* d_dec, const GenericSubInfo* d_info, uint32_t max_frames, const uint32_t* d_n_found, uint32_t channels,
    uint32_t stride, uint32_t bucket, const uint32_t* d_status, uint32_t* d_ctl, uint32_t* d_marks, struct sela_hip_envelope32* d_env, hipStream_t stream)
{
    const dim3 grid(max_frames, verify32_slices(stride));
    const uint32_t slots = envelope_slots(stride, bucket);
    uint64_t* const env = reinterpret_cast<uint64_t*>(d_env);
    if (slots == 0)
        return hipErrorInvalidValue;
    if (rows_are_vectors32(d_dec, stride))
        hipLaunchKernelGGL(k_envelope32_direct<true>, grid, dim3(kV32Threads), 0, stream, d_dec, d_info, max_frames, channels, stride, bucket, slots, d_status, d_n_found,
            d_ctl, d_marks, env);
    else
        hipLaunchKernelGGL(k_envelope32_direct<false>, grid, dim3(kV32Threads), 0, stream, d_dec, d_info, max_frames, channels, stride, bucket, slots, d_status, d_n_found,
            d_ctl, d_marks, env);
    return hipGetLastError();
}

hipError_t launch_envelope32_rest(const int32_t* d_all, const uint32_t* d_counts, uint32_t max_frames, uint32_t channels, uint32_t stride, uint32_t bucket,
    const uint32_t* d_status, const uint32_t* d_ctl, const uint32_t* d_marks, struct sela_hip_envelope32* d_env, hipStream_t stream)
{
    const dim3 grid(max_frames, verify32_slices(stride));
    const uint32_t slots = envelope_slots(stride, bucket);
    uint64_t* const env = reinterpret_cast<uint64_t*>(d_env);
    if (slots == 0)
        return hipErrorInvalidValue;
    const uint32_t* const flags = d_ctl ? d_status : nullptr; // (the caller's samples: no decoder has refused a stride)
    if (rows_are_vectors32(d_all, stride))
        hipLaunchKernelGGL(k_envelope32_rest<true>, grid, dim3(kV32Threads), 0, stream, d_all, d_counts, max_frames, channels, stride, bucket, slots, flags, d_ctl, d_marks,
            env);
    else
        hipLaunchKernelGGL(k_envelope32_rest<false>, grid, dim3(kV32Threads), 0, stream, d_all, d_counts, max_frames, channels, stride, bucket, slots, flags, d_ctl,
            d_marks, env);
    return hipGetLastError();
}

} // namespace sela
