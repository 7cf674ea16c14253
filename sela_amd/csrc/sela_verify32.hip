// sela_verify32.hip -- a .sela stream checked against its int32 samples on the device, frame by frame (gfx950).
//
// sela_hip_verify_i32_device is sela_hip_decode_i32_device with a compare where the combine stores.  The launches are the int32
// family's sequence (launch_i32_sequence, sela_generic.hip): the sample index, a begin step, every subframe decoded into the
// workspace BY POSITION, a direct step, k_verify32_gate, k_generic_combine<false> on its count, a rest step that ends with a sum
// over the slices.  This file has the gate, and what launch_verify_i32_device plugs in:
//
//   k_verify32_begin   status[2] = 0 (it becomes the count of frames with a difference) and the two control words.
//   k_verify32_direct  one workgroup per (frame, slice of kVerify32Slice samples).  It reads the frame's GenericSubInfos and
//                      decides whether the layout is DIRECT: every channel 0 .. channels-1 named by exactly one subframe that
//                      is ok and of type 0 or 1, every type-1 subframe's parent named by a type-0 subframe at least as long.
//                      (What this project's encoders write, ragged frames included.)  For such a frame the value of channel c
//                      at i is dec[pos(c)][i], or dec[pos(parent)][i] - dec[pos(c)][i] mod 2^32: computed in registers and
//                      compared with the original.  No decoded sample is written.  Any other frame is marked and counted.
//   k_verify32_gate    one thread: the frames the fallback takes -- 0 when no frame was marked, else the call's own count.
//                      (The sequence's, for every call of the family; then k_generic_combine<false> on that count, into the
//                      workspace: frame_decoder.cpp's order of writes, its malformed frames.)
//   k_verify32_rest    the marked frames against the original, from the combine's samples and counts.
//   k_verify32_sum     a thread per frame: the slices' words added up, the frame's two words, status[2].
//
// Per frame: diff_count[f] = sum over the channels of #{ i < min(m, L) : decoded != original } + |m - L| (m: the decoder's
// count, L: the original's length), first_diff[f] = the smallest c * stride + i (0xFFFFFFFF: nothing differs).
#include "sela_host.h"
#include "sela_verify32_rule.h"

namespace sela {

namespace {

// Samples [lo, end) of one channel: dec (minus: par - dec mod 2^32 where par is not null) against org; a difference at i counts
// as index_base + i.  kVec: all three rows are 16-byte aligned and whole int4s long (stride % 4 == 0), so a thread takes four
// samples per load -- the last vector of a channel may reach beyond `end`, never beyond the row: what lies there is masked.
template <bool kVec>
__device__ __forceinline__ void compare_row(const int32_t* __restrict__ dec, const int32_t* __restrict__ par, const int32_t* __restrict__ org, uint32_t lo,
    uint32_t end, uint32_t index_base, uint32_t t, uint32_t& n_diff, uint32_t& first)
{
    if (kVec) {
        for (uint32_t i = lo + 4 * t; i < end; i += 4 * kV32Threads) {
            int4 v = *reinterpret_cast<const int4*>(dec + i);
            const int4 o = *reinterpret_cast<const int4*>(org + i);
            if (par) {
                const int4 p = *reinterpret_cast<const int4*>(par + i);
                v.x = (int32_t)((uint32_t)p.x - (uint32_t)v.x), v.y = (int32_t)((uint32_t)p.y - (uint32_t)v.y);
                v.z = (int32_t)((uint32_t)p.z - (uint32_t)v.z), v.w = (int32_t)((uint32_t)p.w - (uint32_t)v.w);
            }
            const uint32_t left = end - i;
            const uint32_t differ = (v.x != o.x ? 1u : 0u) | (left > 1 && v.y != o.y ? 2u : 0u) | (left > 2 && v.z != o.z ? 4u : 0u)
                | (left > 3 && v.w != o.w ? 8u : 0u);
            if (differ) {
                n_diff += (uint32_t)__popc(differ);
                first = min(first, index_base + i + (uint32_t)(__ffs((int)differ) - 1));
            }
        }
    } else {
        for (uint32_t i = lo + t; i < end; i += kV32Threads) {
            const int32_t d = dec[i];
            const int32_t v = par ? (int32_t)((uint32_t)par[i] - (uint32_t)d) : d;
            if (v != org[i]) {
                n_diff++;
                first = min(first, index_base + i);
            }
        }
    }
}

// the original's length of (frame row, channel): never more than stride
__device__ __forceinline__ uint32_t original_length(const uint32_t* __restrict__ lengths, size_t sub, uint32_t stride)
{
    return lengths ? min(lengths[sub], stride) : stride;
}

// a missing or an extra sample is a difference, found at the shorter of the two lengths
__device__ __forceinline__ void compare_lengths(uint32_t m, uint32_t L, uint32_t index_base, uint32_t& n_diff, uint32_t& first)
{
    if (m != L) {
        n_diff += m > L ? m - L : L - m;
        first = min(first, index_base + min(m, L));
    }
}

// ctl[0]: the frames k_verify32_direct leaves alone; ctl[1]: the frames the fallback takes (k_verify32_gate)
__global__ __launch_bounds__(64) void k_verify32_begin(uint32_t* __restrict__ status, uint32_t* __restrict__ ctl)
{
    if (threadIdx.x == 0)
        status[2] = 0, ctl[0] = 0, ctl[1] = 0;
}

template <bool kVec>
__global__ __launch_bounds__(kV32Threads) void k_verify32_direct(const int32_t* __restrict__ dec_ws /* [frames][channels][stride] by position */,
    const GenericSubInfo* __restrict__ info, uint32_t max_frames, uint32_t channels, uint32_t stride, const int32_t* __restrict__ samples,
    const uint32_t* __restrict__ lengths /* or null */, const uint32_t* __restrict__ status, const uint32_t* __restrict__ n_frames_found /* or null */,
    uint32_t* __restrict__ ctl, uint32_t* __restrict__ marks /* [frames] */, uint32_t* __restrict__ parts /* 2 x [max_frames][gridDim.y] */)
{
    __shared__ uint32_t s_named[256], s_n[256]; // by channel: the subframes that name it, its subframe's length
    __shared__ uint16_t s_pos[256], s_ppos[256]; // by channel: its subframe's position, its parent's (kV32NoParent: independent)
    __shared__ uint32_t s_other, s_count[kV32Waves], s_first[kV32Waves];
    const uint32_t f = blockIdx.x, t = threadIdx.x;
    if (f >= frames_in_call(n_frames_found, max_frames))
        return;
    const size_t row = (size_t)f * channels;
    const GenericSubInfo* const inf = info + row;
    verify32_judge_layout(inf, channels, t, s_named, s_n, s_pos, s_ppos, s_other);
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
    uint32_t n_diff = 0, first = kNoDiff;
    if (!(status[0] & SELA_HIP_FLAG_STRIDE)) { // (refused for its stride: nothing is compared)
        const uint32_t lo = blockIdx.y * kVerify32Slice, hi = lo + kVerify32Slice;
        for (uint32_t c = 0; c < channels; c++) {
            const uint32_t end = min(min(s_n[c], original_length(lengths, row + c, stride)), hi);
            if (lo >= end)
                continue;
            const int32_t* const dec = dec_ws + (row + s_pos[c]) * stride;
            const int32_t* const par = s_ppos[c] == kV32NoParent ? nullptr : dec_ws + (row + s_ppos[c]) * stride;
            compare_row<kVec>(dec, par, samples + (row + c) * stride, lo, end, c * stride, t, n_diff, first);
        }
        if (first_slice && t < channels)
            compare_lengths(s_n[t], original_length(lengths, row + t, stride), t * stride, n_diff, first);
    }
    leave_slice_words(n_diff, first, s_count, s_first, parts, (size_t)f * gridDim.y + blockIdx.y, (size_t)max_frames * gridDim.y);
}

__global__ __launch_bounds__(64) void k_verify32_gate(uint32_t max_frames, const uint32_t* __restrict__ n_frames_found /* or null */, uint32_t* __restrict__ ctl)
{
    if (threadIdx.x == 0)
        ctl[1] = ctl[0] ? frames_in_call(n_frames_found, max_frames) : 0u;
}

// The marked frames, as k_generic_combine<false> left them in the workspace (by channel, with their counts).
template <bool kVec>
__global__ __launch_bounds__(kV32Threads) void k_verify32_rest(const int32_t* __restrict__ all /* [frames][channels][stride] by channel */,
    const uint32_t* __restrict__ counts, uint32_t max_frames, uint32_t channels, uint32_t stride, const int32_t* __restrict__ samples,
    const uint32_t* __restrict__ lengths, const uint32_t* __restrict__ status, const uint32_t* __restrict__ ctl, const uint32_t* __restrict__ marks,
    uint32_t* __restrict__ parts)
{
    __shared__ uint32_t s_count[kV32Waves], s_first[kV32Waves];
    const uint32_t f = blockIdx.x, t = threadIdx.x;
    if (f >= ctl[1] || !marks[f])
        return;
    const size_t row = (size_t)f * channels;
    uint32_t n_diff = 0, first = kNoDiff;
    if (!(status[0] & SELA_HIP_FLAG_STRIDE)) {
        const uint32_t lo = blockIdx.y * kVerify32Slice, hi = lo + kVerify32Slice;
        for (uint32_t c = 0; c < channels; c++) {
            const uint32_t end = min(min(min(counts[row + c], stride), original_length(lengths, row + c, stride)), hi);
            if (lo < end)
                compare_row<kVec>(all + (row + c) * stride, nullptr, samples + (row + c) * stride, lo, end, c * stride, t, n_diff, first);
        }
        if (blockIdx.y == 0 && t < channels)
            compare_lengths(min(counts[row + t], stride), original_length(lengths, row + t, stride), t * stride, n_diff, first);
    }
    leave_slice_words(n_diff, first, s_count, s_first, parts, (size_t)f * gridDim.y + blockIdx.y, (size_t)max_frames * gridDim.y);
}

__global__ __launch_bounds__(kV32Threads) void k_verify32_sum(const uint32_t* __restrict__ parts, uint32_t n_slices, uint32_t max_frames,
    const uint32_t* __restrict__ n_frames_found /* or null */, uint32_t* __restrict__ diff_count, uint32_t* __restrict__ first_diff, uint32_t* __restrict__ status)
{
    const uint32_t f = blockIdx.x * kV32Threads + threadIdx.x;
    uint32_t lossy = 0;
    if (f < frames_in_call(n_frames_found, max_frames)) {
        uint32_t total = 0, least = kNoDiff;
        const size_t n_slots = (size_t)max_frames * n_slices;
        for (uint32_t s = 0; s < n_slices; s++) {
            total += parts[(size_t)f * n_slices + s];
            least = min(least, parts[n_slots + (size_t)f * n_slices + s]);
        }
        diff_count[f] = total;
        first_diff[f] = least;
        lossy = total ? 1u : 0u;
    }
    lossy = wave_sum_small(lossy);
    if (threadIdx.x % 64 == 0 && lossy)
        atomicAdd(&status[2], lossy);
}

// int4 loads: every row of the three arrays starts at a multiple of 16 bytes (the workspace's pieces are 256-byte aligned)
bool rows_are_vectors(const int32_t* d_samples, uint32_t stride) { return stride % 4 == 0 && ((uintptr_t)d_samples & 15) == 0; }

} // namespace

uint32_t verify32_slices(uint32_t stride) { return (stride + kVerify32Slice - 1) / kVerify32Slice; }

hipError_t launch_verify32_begin(uint32_t* d_status, uint32_t* d_ctl, hipStream_t stream)
{
    hipLaunchKernelGGL(k_verify32_begin, dim3(1), dim3(64), 0, stream, d_status, d_ctl);
    return hipGetLastError();
}

hipError_t launch_verify32_gate(uint32_t max_frames, const uint32_t* d_n_found, uint32_t* d_ctl, hipStream_t stream)
{
    hipLaunchKernelGGL(k_verify32_gate, dim3(1), dim3(64), 0, stream, max_frames, d_n_found, d_ctl);
    return hipGetLastError();
}

hipError_t launch_verify32_sum(const void* d_parts, uint32_t n_slices, uint32_t max_frames, const uint32_t* d_n_found, uint32_t* d_diff_counts, uint32_t* d_first_diff,
    uint32_t* d_status, hipStream_t stream)
{
    hipLaunchKernelGGL(k_verify32_sum, dim3((max_frames + kV32Threads - 1) / kV32Threads), dim3(kV32Threads), 0, stream, static_cast<const uint32_t*>(d_parts), n_slices,
        max_frames, d_n_found, d_diff_counts, d_first_diff, d_status);
    return hipGetLastError();
}

hipError_t launch_verify32_direct(const int32_t* d_dec, const GenericSubInfo* d_info, uint32_t max_frames, const uint32_t* d_n_found, uint32_t channels,
    uint32_t stride, const int32_t* d_samples, const uint32_t* d_lengths, const uint32_t* d_status, uint32_t* d_ctl, uint32_t* d_marks, void* d_parts,
    hipStream_t stream)
{
    const dim3 grid(max_frames, verify32_slices(stride));
    uint32_t* const parts = static_cast<uint32_t*>(d_parts);
    if (rows_are_vectors(d_samples, stride))
        hipLaunchKernelGGL(k_verify32_direct<true>, grid, dim3(kV32Threads), 0, stream, d_dec, d_info, max_frames, channels, stride, d_samples, d_lengths, d_status,
            d_n_found, d_ctl, d_marks, parts);
    else
        hipLaunchKernelGGL(k_verify32_direct<false>, grid, dim3(kV32Threads), 0, stream, d_dec, d_info, max_frames, channels, stride, d_samples, d_lengths, d_status,
            d_n_found, d_ctl, d_marks, parts);
    return hipGetLastError();
}

hipError_t launch_verify32_rest(const int32_t* d_all, const uint32_t* d_counts, uint32_t max_frames, const uint32_t* d_n_found, uint32_t channels, uint32_t stride,
    const int32_t* d_samples, const uint32_t* d_lengths, uint32_t* d_status, const uint32_t* d_ctl, const uint32_t* d_marks, void* d_parts,
    uint32_t* d_diff_counts, uint32_t* d_first_diff, hipStream_t stream)
{
    const uint32_t n_slices = verify32_slices(stride);
    const dim3 grid(max_frames, n_slices);
    uint32_t* const parts = static_cast<uint32_t*>(d_parts);
    if (rows_are_vectors(d_samples, stride))
        hipLaunchKernelGGL(k_verify32_rest<true>, grid, dim3(kV32Threads), 0, stream, d_all, d_counts, max_frames, channels, stride, d_samples, d_lengths, d_status, d_ctl,
            d_marks, parts);
    else
        hipLaunchKernelGGL(k_verify32_rest<false>, grid, dim3(kV32Threads), 0, stream, d_all, d_counts, max_frames, channels, stride, d_samples, d_lengths, d_status, d_ctl,
            d_marks, parts);
    hipLaunchKernelGGL(k_verify32_sum, dim3((max_frames + kV32Threads - 1) / kV32Threads), dim3(kV32Threads), 0, stream, parts, n_slices, max_frames, d_n_found,
        d_diff_counts, d_first_diff, d_status);
    return hipGetLastError();
}

} // namespace sela
