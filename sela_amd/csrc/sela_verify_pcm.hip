// sela_verify_pcm.hip -- a .sela stream checked against the packed interleaved 3- or 4-byte PCM it was made from, on the device,
// frame by frame (gfx950).
//
// sela_hip_verify_pcm_device is sela_hip_verify_i32_device (sela_verify32.hip, 5.15) with the original read where it lies: little-
// endian interleaved samples, frame f at sample_offsets[f] * channels * kBytes -- the layout sela_hip_decode_pcm_device writes.
// No unpacked copy of it is made.  The launches are the int32 family's sequence (launch_i32_sequence, sela_generic.hip; its steps:
// sela_verify32.hip's head); launch_verify_pcm_device plugs in k_verify32_begin and
//
//   k_verify_pcm<kBytes, false>  the direct step: one workgroup per (frame, tile of sela_pcm_layout.h), the tile clipped to the original's length
//                      L_f.  The tile's packed bytes are loaded into the LDS image as k_pcm_unpack loads them (aligned dwords, a
//                      run of kBytes per lane); the frame's layout is judged by k_verify32_direct's rule (sela_verify32_rule.h);
//                      a lane takes four consecutive samples of one channel out of the image, an int4 of the subframe as
//                      decoded (and of its parent for a type-1 subframe), and compares in registers.  Frames of any other
//                      layout are marked and counted.
//   k_verify_pcm<kBytes, true>   the rest step: the marked frames, from the combine's samples and counts; then
//   k_verify32_sum     on pcm_tiles(stride, channels) slices: the frame's two words, status[2].
//
// Per frame, with n_f = so[f + 1] - so[f] (at most stride), L_f = min(n_f, the samples the buffer still holds from so[f] on) and
// m_c the decoder's count of channel c: diff_count[f] = sum over c of #{ i < min(m_c, L_f) : decoded != original } + |m_c - L_f|,
// first_diff[f] = the smallest i * channels + c (0xFFFFFFFF: nothing differs).  A decoded value beyond 24 bits never equals a
// sign-extended 3-byte original.  Global stores: the frame's mark, the tile's two words, the control word's atomic.
#include "sela_host.h"
#include "sela_pcm_layout.h"
#include "sela_verify32_rule.h"

namespace sela {

namespace {

static_assert(kPcmThreads == kV32Threads, "one workgroup shape for the tile's loads and the layout's judge");

// a run of dwords at a 4-byte aligned place: one global (or LDS) access of 12 or 16 bytes
template <int kDwords>
struct __attribute__((packed, aligned(4))) Run {
    uint32_t d[kDwords];
};

template <int kBytes, bool kRest>
__global__ __launch_bounds__(kPcmThreads) void k_verify_pcm(const int32_t* __restrict__ dec_ws /* [frames][channels][stride]: by position; kRest: by channel */,
    const GenericSubInfo* __restrict__ info /* !kRest */, const uint32_t* __restrict__ counts /* kRest */, uint32_t max_frames, uint32_t channels, uint32_t stride,
    uint32_t n_tiles, const uint8_t* __restrict__ pcm, uint64_t pcm_samples, const uint64_t* __restrict__ sample_offsets, const uint32_t* __restrict__ status,
    const uint32_t* __restrict__ n_frames_found /* or null */, uint32_t* __restrict__ ctl, uint32_t* __restrict__ marks /* [frames] */,
    uint32_t* __restrict__ parts /* 2 x [max_frames][n_tiles] */)
{
    __shared__ uint32_t image[kPcmImageDwords];
    __shared__ uint32_t s_named[256], s_n[256]; // by channel: the subframes that name it, the decoder's count
    __shared__ uint16_t s_pos[256], s_ppos[256]; // by channel: its row of dec_ws in the frame, its parent's (kV32NoParent: none)
    __shared__ uint32_t s_other, s_count[kV32Waves], s_first[kV32Waves];
    const uint32_t f = blockIdx.x, t = threadIdx.x;
    const size_t row = (size_t)f * channels;
    if (kRest) {
        if (f >= ctl[1] || !marks[f])
            return;
        if (t < channels)
            s_n[t] = min(counts[row + t], stride), s_pos[t] = (uint16_t)t, s_ppos[t] = (uint16_t)kV32NoParent;
        __syncthreads();
    } else {
        if (f >= frames_in_call(n_frames_found, max_frames))
            return;
        verify32_judge_layout(info + row, channels, t, s_named, s_n, s_pos, s_ppos, s_other);
        if (s_other) { // the fallback's: marked and counted once
            if (blockIdx.y == 0 && t == 0) {
                marks[f] = 1;
                atomicAdd(&ctl[0], 1u);
            }
            return;
        }
        if (blockIdx.y == 0 && t == 0)
            marks[f] = 0;
    }
    const bool compare = !(status[0] & SELA_HIP_FLAG_STRIDE); // (refused for its stride: nothing is compared, no offset is read)
    // the original's frame: where it starts and how much of it the buffer holds -- clamped before anything is addressed
    uint64_t so = 0;
    uint32_t L = 0;
    if (compare) {
        const PcmHeld h = pcm_held_frame(sample_offsets[f], sample_offsets[f + 1], stride, pcm_samples);
        so = h.so, L = h.n;
    }
    const uint32_t tile_samples = pcm_tile_samples(channels);
    const bool vec = (stride & 3) == 0; // every row of dec_ws is then 16-byte aligned and whole int4s long
    const int32_t* const frame_dec = dec_ws + row * stride;
    for (uint32_t tile = blockIdx.y; tile < n_tiles; tile += gridDim.y) {
        uint32_t n_diff = 0, first = kNoDiff;
        if ((uint64_t)tile * tile_samples < L) {
            const PcmTile k = pcm_tile(so * channels * kBytes, tile, L, channels, kBytes);
            const PcmLoadPlan l = pcm_load_plan(k, kBytes);
            const uint8_t* const src = pcm + k.a0;
            for (uint32_t r = t; r < l.runs; r += kPcmThreads)
                *reinterpret_cast<Run<kBytes>*>(image + r * kBytes) = *reinterpret_cast<const Run<kBytes>*>(src + (size_t)r * kBytes * 4);
            for (uint32_t d = l.runs * kBytes + t; d < l.dwords; d += kPcmThreads)
                image[d] = *reinterpret_cast<const uint32_t*>(src + (size_t)d * 4);
            __syncthreads();
            const uint32_t items = k.items();
            for (uint32_t j = t; j < items; j += kPcmThreads) {
                const PcmItem it = k.item(j);
                const uint32_t m = s_n[it.c];
                if (it.s >= m) // (the decoder has nothing here: the missing samples are counted with the lengths)
                    continue;
                const uint32_t live = min(it.count, m - it.s);
                const int32_t* const dec = frame_dec + (size_t)s_pos[it.c] * stride + it.s;
                const uint32_t ppos = s_ppos[it.c];
                const int32_t* const par = ppos == kV32NoParent ? nullptr : frame_dec + (size_t)ppos * stride + it.s;
                int32_t v[4] = { 0, 0, 0, 0 };
                if (vec) { // (the vector may reach beyond the count, never beyond the row: what lies there is masked)
                    const int4 q = *reinterpret_cast<const int4*>(dec);
                    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
                    if (par) {
                        const int4 p = *reinterpret_cast<const int4*>(par);
                        v[0] = (int32_t)((uint32_t)p.x - (uint32_t)v[0]), v[1] = (int32_t)((uint32_t)p.y - (uint32_t)v[1]);
                        v[2] = (int32_t)((uint32_t)p.z - (uint32_t)v[2]), v[3] = (int32_t)((uint32_t)p.w - (uint32_t)v[3]);
                    }
                } else {
#pragma unroll
                    for (uint32_t i = 0; i < 4; i++)
                        if (i < live)
                            v[i] = par ? (int32_t)((uint32_t)par[i] - (uint32_t)dec[i]) : dec[i];
                }
                uint32_t differ = 0;
#pragma unroll
                for (uint32_t i = 0; i < 4; i++) {
                    if (i < live) {
                        const uint32_t at = k.at(it.c, it.s + i, kBytes);
                        const int32_t org = pcm_extract(image[at >> 2], image[(at >> 2) + 1], at & 3, kBytes);
                        differ |= v[i] != org ? 1u << i : 0u;
                    }
                }
                if (differ) {
                    n_diff += (uint32_t)__popc(differ);
                    first = min(first, (it.s + (uint32_t)(__ffs((int)differ) - 1)) * channels + it.c);
                }
            }
        }
        if (compare && tile == 0 && t < channels) { // a missing or an extra sample is a difference, found at the shorter of the two lengths
            const uint32_t m = s_n[t];
            if (m != L) {
                n_diff += m > L ? m - L : L - m;
                first = min(first, min(m, L) * channels + t);
            }
        }
        // (its barrier also closes the image: the next tile's loads come behind it)
        leave_slice_words(n_diff, first, s_count, s_first, parts, (size_t)f * n_tiles + tile, (size_t)max_frames * n_tiles);
    }
}

} // namespace

uint32_t verify_pcm_tiles(uint32_t stride, uint32_t channels)
{
    const uint32_t t = pcm_tile_samples(channels);
    return (uint32_t)(((uint64_t)stride + t - 1) / t);
}

// (frames above 65535 tiles a frame: the workgroups stride over them)
static dim3 verify_pcm_grid(uint32_t max_frames, uint32_t n_tiles) { return dim3(max_frames, n_tiles < 65535u ? n_tiles : 65535u); }

hipError_t launch_verify_pcm_direct(const int32_t* d_dec, const GenericSubInfo* d_info, uint32_t max_frames, const uint32_t* d_n_found, uint32_t channels,
    uint32_t stride, const void* d_pcm, uint32_t bytes_per_sample, uint64_t pcm_samples, const uint64_t* d_sample_offsets, const uint32_t* d_status, uint32_t* d_ctl,
    uint32_t* d_marks, void* d_parts, hipStream_t stream)
{
    const uint32_t n_tiles = verify_pcm_tiles(stride, channels);
    const dim3 grid = verify_pcm_grid(max_frames, n_tiles);
    const uint8_t* const pcm = static_cast<const uint8_t*>(d_pcm);
    uint32_t* const parts = static_cast<uint32_t*>(d_parts);
    if (bytes_per_sample == 3)
        hipLaunchKernelGGL((k_verify_pcm<3, false>), grid, dim3(kPcmThreads), 0, stream, d_dec, d_info, nullptr, max_frames, channels, stride, n_tiles, pcm, pcm_samples,
            d_sample_offsets, d_status, d_n_found, d_ctl, d_marks, parts);
    else
        hipLaunchKernelGGL((k_verify_pcm<4, false>), grid, dim3(kPcmThreads), 0, stream, d_dec, d_info, nullptr, max_frames, channels, stride, n_tiles, pcm, pcm_samples,
            d_sample_offsets, d_status, d_n_found, d_ctl, d_marks, parts);
    return hipGetLastError();
}

hipError_t launch_verify_pcm_rest(const int32_t* d_all, const uint32_t* d_counts, uint32_t max_frames, uint32_t channels, uint32_t stride, const void* d_pcm,
    uint32_t bytes_per_sample, uint64_t pcm_samples, const uint64_t* d_sample_offsets, const uint32_t* d_status, uint32_t* d_ctl, uint32_t* d_marks, void* d_parts,
    hipStream_t stream)
{
    const uint32_t n_tiles = verify_pcm_tiles(stride, channels);
    const dim3 grid = verify_pcm_grid(max_frames, n_tiles);
    const uint8_t* const pcm = static_cast<const uint8_t*>(d_pcm);
    uint32_t* const parts = static_cast<uint32_t*>(d_parts);
    if (bytes_per_sample == 3)
        hipLaunchKernelGGL((k_verify_pcm<3, true>), grid, dim3(kPcmThreads), 0, stream, d_all, nullptr, d_counts, max_frames, channels, stride, n_tiles, pcm, pcm_samples,
            d_sample_offsets, d_status, nullptr, d_ctl, d_marks, parts);
    else
        hipLaunchKernelGGL((k_verify_pcm<4, true>), grid, dim3(kPcmThreads), 0, stream, d_all, nullptr, d_counts, max_frames, channels, stride, n_tiles, pcm, pcm_samples,
            d_sample_offsets, d_status, nullptr, d_ctl, d_marks, parts);
    return hipGetLastError();
}

} // namespace sela
