// sela_digest_pcm.hip -- the CRC-32 of the packed interleaved 3- or 4-byte PCM a .sela stream decodes to, on the device: per frame
// the CRC of the bytes sela_hip_decode_pcm_device would write, and the track's from those (gfx950).
//
// The launches are the int32 family's sequence (launch_i32_sequence, sela_generic.hip; its steps: sela_verify32.hip's head);
// launch_digest_pcm_device plugs in
//
//   k_digest32_begin               the two control words (status[2] stays the largest samplesPerChannel, as the decode call leaves it).
//   k_digest32_tiles<kBytes, false>  the direct step: one workgroup per (frame, tile of sela_pcm_layout.h).  The frame's layout is
//                      judged by k_verify32_direct's rule (sela_verify32_rule.h); a lane takes four consecutive samples of one
//                      channel out of the subframes as decoded (an int4, and its parent's for a type-1 subframe) and places their
//                      low kBytes bytes into the tile's LDS image, as k_pcm_pack does -- with a frame byte offset of 0, so that
//                      every tile starts at image byte 0 (a tile is a multiple of 4 samples).  Where k_pcm_pack would store the
//                      image, this kernel takes its CRC out of LDS: 16-byte lines at the workgroup's stride, the lanes joined on
//                      the DPP ladder, the up to 15 bytes behind the last line by thread 0.  No decoded byte reaches global memory.
//                      Frames of any other layout are marked and counted.
//   k_digest32_tiles<kBytes, true>   the rest step: the marked frames, from the combine's samples and counts;
// then the folds of sela_digest.hip on the tiles' words: k_digest_slices (a frame's record), k_digest_fold and k_digest_track.
//
// The status words are the decode call's: what k_pcm_pack adds to them behind launch_decode_i32_device -- a frame whose channels
// disagree about its length (SELA_HIP_FLAG_BAD_FRAME, status[1]), the samples beyond a 3-byte container (status[3]) -- this kernel
// adds from the same tests.  Global stores: the frame's mark, the tile's word, those atomics.
#include "sela_host.h"

#include "sela_crc32_lanes.h"
#include "sela_pcm_layout.h"
#include "sela_verify32_rule.h"

namespace sela {

namespace {

static_assert(kPcmThreads == kV32Threads && kPcmThreads == kDigestThreads, "one workgroup shape for the judge, the image and the lines");
static_assert(kPcmImageDwords * 4 >= kPcmTileValues * 4 + 16, "a tile's bytes, and the line behind them, lie inside the image");

// ctl[0]: the frames the direct step leaves alone; ctl[1]: the frames the fallback takes (k_verify32_gate)
__global__ __launch_bounds__(64) void k_digest32_begin(uint32_t* __restrict__ ctl)
{
    if (threadIdx.x == 0)
        ctl[0] = 0, ctl[1] = 0;
}

template <int kBytes, bool kRest>
__global__ __launch_bounds__(kPcmThreads) void k_digest32_tiles(const int32_t* __restrict__ dec_ws /* [frames][channels][stride]: by position; kRest: by channel */,
    const GenericSubInfo* __restrict__ info /* !kRest */, const uint32_t* __restrict__ counts /* kRest */, uint32_t max_frames, uint32_t channels, uint32_t stride,
    uint32_t n_tiles, uint32_t tile_samples /* pcm_tile_samples(channels) */, uint32_t group_shift /* digest_pcm_group_shift(channels) */,
    const uint64_t* __restrict__ sample_offsets, uint32_t* __restrict__ status, const uint32_t* __restrict__ n_frames_found /* or null */,
    uint32_t* __restrict__ ctl, uint32_t* __restrict__ marks /* [frames] */, uint32_t* __restrict__ parts /* [max_frames][n_tiles] */, const DigestShape shape)
{
    __shared__ __attribute__((aligned(16))) uint32_t image[kPcmImageDwords];
    __shared__ uint32_t s_named[256], s_n[256]; // by channel: the subframes that name it, the decoder's count
    __shared__ uint16_t s_pos[256], s_ppos[256]; // by channel: its row of dec_ws in the frame, its parent's (kV32NoParent: none)
    __shared__ uint32_t s_other, s_wide, s_part[kDigestThreads / 64];
    const uint32_t f = blockIdx.x, t = threadIdx.x;
    const size_t row = (size_t)f * channels;
    if (t == 0)
        s_wide = 0;
    if (kRest) {
        if (f >= ctl[1] || !marks[f])
            return;
        if (t < channels)
            s_n[t] = counts[row + t], s_pos[t] = (uint16_t)t, s_ppos[t] = (uint16_t)kV32NoParent;
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
    if (status[0] & SELA_HIP_FLAG_STRIDE) // (refused for its stride: as k_pcm_pack, nothing is taken)
        return;
    // k_pcm_pack's test of a frame: every channel has the frame's length, which the stride holds (with the stride accepted, the
    // frame then also ends inside max_frames * stride samples)
    const uint64_t so0 = sample_offsets[f], so1 = sample_offsets[f + 1];
    const uint64_t n64 = so1 - so0;
    bool bad = so1 < so0 || n64 > stride;
    if (t < channels)
        bad |= s_n[t] != (uint32_t)n64;
    if (__syncthreads_or(bad)) {
        if (blockIdx.y == 0 && t == 0) {
            atomicOr(&status[0], (uint32_t)SELA_HIP_FLAG_BAD_FRAME);
            atomicAdd(&status[1], 1u);
        }
        return;
    }
    const uint32_t n = (uint32_t)n64; // (<= stride: every row of dec_ws holds it)
    const bool vec = (stride & 3) == 0; // every row of dec_ws is then 16-byte aligned and whole int4s long
    const int32_t* const frame_dec = dec_ws + row * stride;
    uint8_t* const image_bytes = reinterpret_cast<uint8_t*>(image);
    uint32_t wide = 0;
    for (uint32_t tile = blockIdx.y; tile < n_tiles; tile += gridDim.y) {
        if ((uint64_t)tile * tile_samples >= n)
            break;
        // pcm_tile(0, tile, n, channels, kBytes) without its divisions: its phase is 0, value j of the tile lies at image byte
        // j * kBytes.  An item is up to four consecutive samples of one channel (as PcmItem); the threads are laid over the items as
        // 2^group_shift neighbouring runs of a channel by 256 >> group_shift channels -- shifts and masks, no division.
        const uint32_t s0 = tile * tile_samples, s1 = n - s0 < tile_samples ? n : s0 + tile_samples;
        const uint32_t groups = (s1 - s0 + 3) / 4, tile_bytes = (s1 - s0) * channels * kBytes;
        for (uint32_t c = t >> group_shift; c < channels; c += kPcmThreads >> group_shift)
        for (uint32_t g = t & ((1u << group_shift) - 1); g < groups; g += 1u << group_shift) {
            const uint32_t s = s0 + 4 * g, count = s1 - s < 4 ? s1 - s : 4; // the item: samples s .. s + count - 1 of channel c
            const int32_t* const dec = frame_dec + (size_t)s_pos[c] * stride + s;
            const uint32_t ppos = s_ppos[c];
            const int32_t* const par = ppos == kV32NoParent ? nullptr : frame_dec + (size_t)ppos * stride + s;
            int32_t v[4] = { 0, 0, 0, 0 };
            if (vec) { // (the vector may reach beyond the frame's length, never beyond the row: what lies there is not placed)
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
                    if (i < count)
                        v[i] = par ? (int32_t)((uint32_t)par[i] - (uint32_t)dec[i]) : dec[i];
            }
#pragma unroll
            for (uint32_t i = 0; i < 4; i++) {
                if (i < count) {
                    const uint32_t value = (s + i - s0) * channels + c; // (< kPcmTileValues)
                    if (kBytes == 4) {
                        image[value] = (uint32_t)v[i];
                    } else {
#pragma unroll
                        for (uint32_t b = 0; b < 3; b++)
                            image_bytes[value * 3 + b] = (uint8_t)((uint32_t)v[i] >> (8 * b));
                        wide += v[i] < -(1 << 23) || v[i] >= (1 << 23) ? 1u : 0u;
                    }
                }
            }
        }
        __syncthreads();
        // the image's whole 16-byte lines: thread t takes lines t - pad, t - pad + 256, ... (the lines below 0 are empty)
        const uint32_t lines = tile_bytes / 16, tail = tile_bytes - 16 * lines;
        const uint32_t steps = (lines + kDigestThreads - 1) / kDigestThreads, pad = steps * kDigestThreads - lines;
        const uint4* const body = reinterpret_cast<const uint4*>(image);
        uint32_t r = 0;
        for (uint32_t j = 0; j < steps; j++) {
            const uint32_t q = t + j * kDigestThreads;
            if (j)
                r = crc_mul(r, shape.stride);
            if (q < pad)
                continue;
            const uint4 w = body[q - pad];
            r = crc_step32(crc_step32(crc_step32(crc_step32(r, w.x), w.y), w.z), w.w);
        }
        r = wave_crc(r, shape);
        if (t % 64 == 0)
            s_part[t / 64] = r;
        __syncthreads();
        if (t == 0) {
            uint32_t raw = waves_crc(s_part, 1, kDigestThreads / 64, shape);
            for (uint32_t i = 16 * lines; i < 16 * lines + tail; i++)
                raw = crc_raw_byte(raw, image_bytes[i]);
            parts[(size_t)f * n_tiles + tile] = raw;
        }
        __syncthreads(); // (closes the image and the waves' words: the next tile's samples come behind it)
    }
    if (kBytes == 3) { // one atomic per workgroup that found any
        if (wide)
            atomicAdd(&s_wide, wide);
        __syncthreads();
        if (t == 0 && s_wide)
            atomicAdd(&status[3], s_wide);
    }
}

// the threads' split over a tile's items: the largest power of two of neighbouring runs that a whole tile's runs per channel fill
uint32_t digest_pcm_group_shift(uint32_t channels)
{
    const uint32_t groups = pcm_tile_samples(channels) / 4;
    uint32_t shift = 0;
    while (shift < 8 && (2u << shift) <= groups)
        shift++;
    return shift;
}

// (frames above 65535 tiles a frame: the workgroups stride over them)
dim3 digest_pcm_grid(uint32_t max_frames, uint32_t n_tiles) { return dim3(max_frames, n_tiles < 65535u ? n_tiles : 65535u); }

} // namespace

// the bytes of a whole tile: the folds' slice
uint64_t digest_pcm_tile_bytes(uint32_t channels, uint32_t bytes_per_sample) { return (uint64_t)pcm_tile_samples(channels) * channels * bytes_per_sample; }

hipError_t launch_digest32_begin(uint32_t* d_ctl, hipStream_t stream)
{
    hipLaunchKernelGGL(k_digest32_begin, dim3(1), dim3(64), 0, stream, d_ctl);
    return hipGetLastError();
}

// one instance on its grid: the direct form reads the judge's records and the call's frame count, the rest form the combine's counts
template <int kBytes, bool kRest>
static hipError_t launch_tiles(const int32_t* d_samples, const GenericSubInfo* d_info, const uint32_t* d_counts, uint32_t max_frames, const uint32_t* d_n_found,
    uint32_t channels, uint32_t stride, const uint64_t* d_sample_offsets, uint32_t* d_status, uint32_t* d_ctl, uint32_t* d_marks, uint32_t* d_parts, hipStream_t stream)
{
    const uint32_t n_tiles = verify_pcm_tiles(stride, channels);
    hipLaunchKernelGGL((k_digest32_tiles<kBytes, kRest>), digest_pcm_grid(max_frames, n_tiles), dim3(kPcmThreads), 0, stream, d_samples, d_info, d_counts, max_frames,
        channels, stride, n_tiles, pcm_tile_samples(channels), digest_pcm_group_shift(channels), d_sample_offsets, d_status, d_n_found, d_ctl, d_marks, d_parts, kPcmShape);
    return hipGetLastError();
}

hipError_t launch_digest32_direct(const int32_t* d_dec, const GenericSubInfo* d_info, uint32_t max_frames, const uint32_t* d_n_found, uint32_t channels, uint32_t stride,
    uint32_t bytes_per_sample, const uint64_t* d_sample_offsets, uint32_t* d_status, uint32_t* d_ctl, uint32_t* d_marks, uint32_t* d_parts, hipStream_t stream)
{
    const auto launch = bytes_per_sample == 3 ? launch_tiles<3, false> : launch_tiles<4, false>;
    return launch(d_dec, d_info, nullptr, max_frames, d_n_found, channels, stride, d_sample_offsets, d_status, d_ctl, d_marks, d_parts, stream);
}

hipError_t launch_digest32_rest(const int32_t* d_all, const uint32_t* d_counts, uint32_t max_frames, uint32_t channels, uint32_t stride, uint32_t bytes_per_sample,
    const uint64_t* d_sample_offsets, uint32_t* d_status, uint32_t* d_ctl, uint32_t* d_marks, uint32_t* d_parts, hipStream_t stream)
{
    const auto launch = bytes_per_sample == 3 ? launch_tiles<3, true> : launch_tiles<4, true>;
    return launch(d_all, nullptr, d_counts, max_frames, nullptr, channels, stride, d_sample_offsets, d_status, d_ctl, d_marks, d_parts, stream);
}

} // namespace sela
