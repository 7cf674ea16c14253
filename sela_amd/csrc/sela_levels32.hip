// sela_levels32.hip -- how loud a 24- or 32-bit .sela stream is, measured on the device: per frame and channel the peak, the sum
// and the 128-bit sum of squares of the int32 samples sela_hip_decode_i32_device would write (gfx950).
//
// sela_hip_levels_i32_device is sela_hip_verify_i32_device (sela_verify32.hip, 5.15) with a reduction where the compare is.  The
// launches are the int32 family's sequence (launch_i32_sequence, sela_generic.hip; its steps: sela_verify32.hip's head);
// launch_levels_i32_device plugs in
//
//   k_level32_begin    status[2] = 0 (it becomes the count of frames that are not silent) and the two control words.
//   k_level32_direct   one workgroup per (frame, slice of kVerify32Slice samples).  verify32_judge_layout decides whether the
//                      layout is DIRECT; for such a frame the value of channel c at i is dec[pos(c)][i], or dec[pos(parent)][i] -
//                      dec[pos(c)][i] mod 2^32: formed in registers and folded into the channel's partial record of this slice.
//                      No decoded sample is written.  Any other frame is marked and counted.
//   k_level32_rest     the rest step: the marked frames, from the combine's samples and counts; with no marks, every frame of planar samples
//                      that already lie in device memory (sela_hip_levels_samples_i32_device).
//   k_level32_sum      a thread per word of a record: the slices' partial records added up, status[2].
//
// Every figure is an integer, so it is exact and does not depend on the launch's shape: |v| <= 2^31, |sum| <= 65535 * 2^31 < 2^47,
// sum_squares <= 65535 * 2^62 < 2^78.  A thread's energy is a 64-bit low word and a count of its carries (four full-scale samples
// pass 2^64); a wave adds it in limbs of 22 bits (wave_sum_96), the waves meet in LDS, the slices in the workspace.  No atomic
// touches a record.
#include "sela_host.h"
#include "sela_verify32_rule.h"

namespace sela {

namespace {

static_assert(sizeof(sela_hip_level32) == 32 && alignof(sela_hip_level32) == 8, "the record of include/sela_hip.h");
static_assert(offsetof(sela_hip_level32, peak) == 0 && offsetof(sela_hip_level32, samples) == 4 && offsetof(sela_hip_level32, sum) == 8
        && offsetof(sela_hip_level32, sum_squares_lo) == 16 && offsetof(sela_hip_level32, sum_squares_hi) == 24,
    "the words of a record");

// What a thread has seen of one channel.
struct Level32Acc {
    uint32_t peak = 0, carries = 0; // (carries: how often `low` wrapped)
    int64_t sum = 0;
    uint64_t low = 0;
    __device__ __forceinline__ void take(int32_t v)
    {
        const uint32_t a = v < 0 ? 0u - (uint32_t)v : (uint32_t)v; // (INT32_MIN: 2^31)
        peak = max(peak, a);
        sum += v;
        const uint64_t sq = (uint64_t)a * a;
        low += sq;
        carries += low < sq ? 1u : 0u;
    }
};

// Samples [lo, end) of one channel: dec, or par - dec mod 2^32 where par is not null.  kVec: the rows are 16-byte aligned and
// whole int4s long (stride % 4 == 0), so a thread takes four samples per load -- the last vector of a channel may reach beyond
// `end`, never beyond the row: what lies there counts as 0, which changes no figure.
template <bool kVec>
__device__ __forceinline__ void fold_row(const int32_t* __restrict__ dec, const int32_t* __restrict__ par, uint32_t lo, uint32_t end, uint32_t t, Level32Acc& a)
{
    if (kVec) {
        for (uint32_t i = lo + 4 * t; i < end; i += 4 * kV32Threads) {
            int4 v = *reinterpret_cast<const int4*>(dec + i);
            if (par) {
                const int4 p = *reinterpret_cast<const int4*>(par + i);
                v.x = (int32_t)((uint32_t)p.x - (uint32_t)v.x), v.y = (int32_t)((uint32_t)p.y - (uint32_t)v.y);
                v.z = (int32_t)((uint32_t)p.z - (uint32_t)v.z), v.w = (int32_t)((uint32_t)p.w - (uint32_t)v.w);
            }
            const uint32_t left = end - i;
            a.take(v.x);
            a.take(left > 1 ? v.y : 0);
            a.take(left > 2 ? v.z : 0);
            a.take(left > 3 ? v.w : 0);
        }
    } else {
        for (uint32_t i = lo + t; i < end; i += kV32Threads) {
            const int32_t d = dec[i];
            a.take(par ? (int32_t)((uint32_t)par[i] - (uint32_t)d) : d);
        }
    }
}

// A wave's view of one channel in kPartWords words of LDS: peak | sum (low, high) | energy (three words).
constexpr uint32_t kPartWords = 6;
__device__ __forceinline__ void deposit_wave32(const Level32Acc& a, uint32_t* part)
{
    const uint32_t peak = wave_max_u32(a.peak);
    const uint64_t sum = wave_sum_64((uint64_t)a.sum);
    const Sum96 e = wave_sum_96(a.low, a.carries);
    if (threadIdx.x % 64 == 0) {
        part[0] = peak, part[1] = (uint32_t)sum, part[2] = (uint32_t)(sum >> 32);
        part[3] = (uint32_t)e.low, part[4] = (uint32_t)(e.low >> 32), part[5] = e.high;
    }
}

// Word k of the partial record of (slot, channel) that the waves' views in `parts` add up to; `samples` of this slice.  A partial
// record is a record: peak | samples << 32, sum, the energy's low word, its high word.
__device__ __forceinline__ uint64_t slice_word(uint32_t k, const uint32_t (*parts)[kPartWords], uint32_t samples)
{
    uint32_t peak = 0;
    uint64_t sum = 0, low = 0, high = 0;
    for (uint32_t w = 0; w < kV32Waves; w++) {
        const uint32_t* const p = parts[w];
        peak = max(peak, p[0]);
        sum += ((uint64_t)p[2] << 32) | p[1];
        const uint64_t l = ((uint64_t)p[4] << 32) | p[3];
        low += l;
        high += p[5] + (low < l ? 1u : 0u);
    }
    return k == 0 ? ((uint64_t)samples << 32) | peak : (k == 1 ? sum : (k == 2 ? low : high));
}

// The partial records of a frame's slice, channel by channel: `row(c, dec, par, n)` names channel c's samples.  One barrier per
// channel: the waves' views alternate between two places in LDS, and threads 0 .. 3 store one 8-byte word each.
template <bool kVec, typename Row>
__device__ __forceinline__ void fold_slice(uint32_t channels, uint32_t slice, bool refused, uint64_t* __restrict__ out /* [channels][4] */, Row row)
{
    __shared__ uint32_t s_part[2][kV32Waves][kPartWords];
    const uint32_t t = threadIdx.x;
    const uint32_t lo = slice * kVerify32Slice, hi = lo + kVerify32Slice;
    for (uint32_t c = 0; c < channels; c++) {
        const int32_t *dec, *par;
        uint32_t n;
        row(c, dec, par, n);
        const uint32_t end = refused ? 0u : min(n, hi);
        Level32Acc a;
        if (lo < end)
            fold_row<kVec>(dec, par, lo, end, t, a);
        deposit_wave32(a, s_part[c & 1][t / 64]);
        __syncthreads();
        if (t < 4)
            out[(size_t)c * 4 + t] = slice_word(t, s_part[c & 1], lo < end ? end - lo : 0u);
    }
}

// ctl[0]: the frames k_level32_direct leaves alone; ctl[1]: the frames the fallback takes (k_verify32_gate).  whole: the call
// has no decoder in front of it that writes the other status words.
__global__ __launch_bounds__(64) void k_level32_begin(uint32_t* __restrict__ status, uint32_t* __restrict__ ctl /* or null */, uint32_t whole)
{
    if (threadIdx.x == 0) {
        status[2] = 0;
        if (whole)
            status[0] = 0, status[1] = 0, status[3] = 0;
        if (ctl)
            ctl[0] = 0, ctl[1] = 0;
    }
}

template <bool kVec>
__global__ __launch_bounds__(kV32Threads) void k_level32_direct(const int32_t* __restrict__ dec_ws /* [frames][channels][stride] by position */,
    const GenericSubInfo* __restrict__ info, uint32_t max_frames, uint32_t channels, uint32_t stride, const uint32_t* __restrict__ status,
    const uint32_t* __restrict__ n_frames_found /* or null */, uint32_t* __restrict__ ctl, uint32_t* __restrict__ marks /* [frames] */,
    uint64_t* __restrict__ parts /* [max_frames][gridDim.y][channels][4] */)
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
    fold_slice<kVec>(channels, blockIdx.y, refused, parts + ((size_t)f * gridDim.y + blockIdx.y) * channels * 4,
        [&](uint32_t c, const int32_t*& dec, const int32_t*& par, uint32_t& n) {
            dec = dec_ws + (row + s_pos[c]) * stride;
            par = s_ppos[c] == kV32NoParent ? nullptr : dec_ws + (row + s_ppos[c]) * stride;
            n = min(s_n[c], stride);
        });
}

// Samples by channel with their counts: the marked frames as k_generic_combine<false> left them in the workspace (frames below
// ctl[1]), or, with no marks, every frame of the caller's samples (counts or null: stride).
template <bool kVec>
__global__ __launch_bounds__(kV32Threads) void k_level32_rest(const int32_t* __restrict__ all /* [frames][channels][stride] by channel */,
    const uint32_t* __restrict__ counts /* or null */, uint32_t max_frames, uint32_t channels, uint32_t stride, const uint32_t* __restrict__ status /* or null */,
    const uint32_t* __restrict__ ctl /* or null */, const uint32_t* __restrict__ marks /* or null */, uint64_t* __restrict__ parts)
{
    const uint32_t f = blockIdx.x;
    if (f >= (ctl ? min(ctl[1], max_frames) : max_frames) || (marks && !marks[f]))
        return;
    const size_t row = (size_t)f * channels;
    const bool refused = status && (status[0] & SELA_HIP_FLAG_STRIDE) != 0;
    fold_slice<kVec>(channels, blockIdx.y, refused, parts + ((size_t)f * gridDim.y + blockIdx.y) * channels * 4,
        [&](uint32_t c, const int32_t*& dec, const int32_t*& par, uint32_t& n) {
            dec = all + (row + c) * stride;
            par = nullptr;
            n = counts ? min(counts[row + c], stride) : stride;
        });
}

// A thread per 8-byte word of a record: words 0 .. 3 of (frame, channel) are threads 4 * (f * channels + c) + 0 .. 3.  The thread
// of a frame's first word also looks through the frame's peaks for status[2].
__global__ __launch_bounds__(kV32Threads) void k_level32_sum(const uint64_t* __restrict__ parts, uint32_t n_slices, uint32_t max_frames, uint32_t channels,
    const uint32_t* __restrict__ n_frames_found /* or null */, uint64_t* __restrict__ levels /* [max_frames][channels][4] */, uint32_t* __restrict__ status)
{
    const uint64_t word = (uint64_t)blockIdx.x * kV32Threads + threadIdx.x;
    const uint64_t record = word / 4;
    const uint32_t k = (uint32_t)(word % 4);
    const uint32_t f = (uint32_t)(record / channels), c = (uint32_t)(record % channels);
    uint32_t loud = 0;
    if (record < (uint64_t)frames_in_call(n_frames_found, max_frames) * channels) {
        const uint64_t* const p = parts + (size_t)f * n_slices * channels * 4;
        uint32_t peak = 0, samples = 0;
        uint64_t sum = 0, low = 0, high = 0;
        for (uint32_t s = 0; s < n_slices; s++) {
            const uint64_t* const q = p + ((size_t)s * channels + c) * 4;
            peak = max(peak, (uint32_t)q[0]);
            samples += (uint32_t)(q[0] >> 32);
            sum += q[1];
            low += q[2];
            high += q[3] + (low < q[2] ? 1u : 0u);
        }
        levels[word] = k == 0 ? ((uint64_t)samples << 32) | peak : (k == 1 ? sum : (k == 2 ? low : high));
        if (k == 0 && c == 0) {
            for (uint32_t i = 0; i < n_slices * channels && !peak; i++)
                peak = (uint32_t)p[(size_t)i * 4];
            loud = peak ? 1u : 0u;
        }
    }
    loud = wave_sum_small(loud);
    if (threadIdx.x % 64 == 0 && loud)
        atomicAdd(&status[2], loud);
}

// int4 loads: every row starts at a multiple of 16 bytes (the workspace's pieces are 256-byte aligned)
bool rows_are_vectors32(const int32_t* d_rows, uint32_t stride) { return stride % 4 == 0 && ((uintptr_t)d_rows & 15) == 0; }

uint32_t sum_blocks(uint32_t max_frames, uint32_t channels) { return (uint32_t)(((uint64_t)max_frames * channels * 4 + kV32Threads - 1) / kV32Threads); }

} // namespace

hipError_t launch_level32_begin(uint32_t* d_status, uint32_t* d_ctl, bool whole, hipStream_t stream)
{
    hipLaunchKernelGGL(k_level32_begin, dim3(1), dim3(64), 0, stream, d_status, d_ctl, whole ? 1u : 0u);
    return hipGetLastError();
}

hipError_t launch_level32_direct(const int32_t* d_dec, const GenericSubInfo* d_info, uint32_t max_frames, const uint32_t* d_n_found, uint32_t channels,
    uint32_t stride, const uint32_t* d_status, uint32_t* d_ctl, uint32_t* d_marks, uint64_t* d_parts, hipStream_t stream)
{
    const dim3 grid(max_frames, verify32_slices(stride));
    if (rows_are_vectors32(d_dec, stride))
        hipLaunchKernelGGL(k_level32_direct<true>, grid, dim3(kV32Threads), 0, stream, d_dec, d_info, max_frames, channels, stride, d_status, d_n_found, d_ctl, d_marks,
            d_parts);
    else
        hipLaunchKernelGGL(k_level32_direct<false>, grid, dim3(kV32Threads), 0, stream, d_dec, d_info, max_frames, channels, stride, d_status, d_n_found, d_ctl, d_marks,
            d_parts);
    return hipGetLastError();
}

hipError_t launch_level32_rest(const int32_t* d_all, const uint32_t* d_counts, uint32_t max_frames, const uint32_t* d_n_found, uint32_t channels, uint32_t stride,
    uint32_t* d_status, const uint32_t* d_ctl, const uint32_t* d_marks, uint64_t* d_parts, sela_hip_level32* d_levels, hipStream_t stream)
{
    const uint32_t n_slices = verify32_slices(stride);
    const dim3 grid(max_frames, n_slices);
    const uint32_t* const flags = d_ctl ? d_status : nullptr; // (the caller's samples: no decoder has refused a stride)
    if (rows_are_vectors32(d_all, stride))
        hipLaunchKernelGGL(k_level32_rest<true>, grid, dim3(kV32Threads), 0, stream, d_all, d_counts, max_frames, channels, stride, flags, d_ctl, d_marks, d_parts);
    else
        hipLaunchKernelGGL(k_level32_rest<false>, grid, dim3(kV32Threads), 0, stream, d_all, d_counts, max_frames, channels, stride, flags, d_ctl, d_marks, d_parts);
    hipLaunchKernelGGL(k_level32_sum, dim3(sum_blocks(max_frames, channels)), dim3(kV32Threads), 0, stream, d_parts, n_slices, max_frames, channels, d_n_found,
        reinterpret_cast<uint64_t*>(d_levels), d_status);
    return hipGetLastError();
}

} // namespace sela
