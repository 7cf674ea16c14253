// sela_pcm.hip -- packed interleaved 3- or 4-byte PCM <-> planar int32 on the device (declarations: sela_pcm.h;
// the index arithmetic: sela_pcm_layout.h, which tests/c/pcm_layout.cpp replays on the CPU).
//
// Both kernels: one workgroup per (frame, tile of samples), the grid from the arguments alone (the frames beyond 65535 by a
// stride over gridDim.y).  The tile's packed bytes stand in LDS as an image that starts at an aligned dword of global memory, so
// the packed side is moved as aligned dwords -- a run of 3 (four 3-byte samples) or 4 per lane -- and the planar side as up to
// four consecutive samples of a channel per lane; the transpose between the two is the LDS image.  No byte is loaded from
// global memory; bytes are stored only at the two ends of a frame (pcm_store_plan).
#include <hip/hip_runtime.h>

#include "sela_hip.h"
#include "sela_pcm.h"
#include "sela_pcm_layout.h"

namespace sela {
namespace {

// a run of dwords at a 4-byte aligned place: one global (or LDS) access of 12 or 16 bytes
template <int kDwords>
struct __attribute__((packed, aligned(4))) Run {
    uint32_t d[kDwords];
};

template <int kBytes>
__global__ __launch_bounds__(kPcmThreads) void k_pcm_unpack(const uint8_t* __restrict__ pcm, uint32_t n_frames, uint32_t channels, uint32_t n,
    int32_t* __restrict__ out /* [n_frames][channels][n] */)
{
    __shared__ uint32_t image[kPcmImageDwords];
    const uint32_t t = threadIdx.x;
    for (uint32_t f = blockIdx.y; f < n_frames; f += gridDim.y) {
        const PcmTile k = pcm_tile((uint64_t)f * n * channels * kBytes, blockIdx.x, n, channels, kBytes);
        const PcmLoadPlan l = pcm_load_plan(k, kBytes);
        const uint8_t* const src = pcm + k.a0;
        for (uint32_t r = t; r < l.runs; r += kPcmThreads)
            *reinterpret_cast<Run<kBytes>*>(image + r * kBytes) = *reinterpret_cast<const Run<kBytes>*>(src + (size_t)r * kBytes * 4);
        for (uint32_t d = l.runs * kBytes + t; d < l.dwords; d += kPcmThreads)
            image[d] = *reinterpret_cast<const uint32_t*>(src + (size_t)d * 4);
        __syncthreads();
        int32_t* const fo = out + (size_t)f * channels * n;
        // whole runs of four samples, one 16-byte store each; then each channel's last one to three samples
        const uint32_t items = k.items();
        for (uint32_t j = t; j < items; j += kPcmThreads) {
            const PcmItem it = k.item(j);
            if (it.count != 4)
                continue;
            Run<4> q;
#pragma unroll
            for (uint32_t i = 0; i < 4; i++) {
                const uint32_t at = k.at(it.c, it.s + i, kBytes);
                q.d[i] = (uint32_t)pcm_extract(image[at >> 2], image[(at >> 2) + 1], at & 3, kBytes);
            }
            *reinterpret_cast<Run<4>*>(fo + (size_t)it.c * n + it.s) = q;
        }
        const uint32_t rest = k.rest();
        for (uint32_t j = t; j < channels * rest; j += kPcmThreads) {
            const uint32_t c = j / rest, s = k.s1 - rest + (j - c * rest), at = k.at(c, s, kBytes);
            fo[(size_t)c * n + s] = pcm_extract(image[at >> 2], image[(at >> 2) + 1], at & 3, kBytes);
        }
        __syncthreads();
    }
}

// the low kBytes bytes of a sample into the image from byte `at` on (src/file/wav_file.cpp:262's rule); the bytes below `first` are left out
template <int kBytes>
__device__ inline void put_sample(uint8_t* image, uint32_t at, int32_t v, uint32_t first = 0)
{
#pragma unroll
    for (uint32_t b = 0; b < (uint32_t)kBytes; b++)
        if (b >= first)
            image[at + b] = (uint8_t)((uint32_t)v >> (8 * b));
}

template <int kBytes>
__global__ __launch_bounds__(kPcmThreads) void k_pcm_pack(const int32_t* __restrict__ samples /* [n_frames][channels][stride] */,
    const uint32_t* __restrict__ counts /* [n_frames][channels] */, const uint64_t* __restrict__ sample_offsets /* [n_frames + 1] */, uint32_t n_frames,
    uint32_t channels, uint32_t stride, uint8_t* __restrict__ pcm_out, uint32_t* __restrict__ status)
{
    __shared__ uint32_t image_dwords[kPcmImageDwords];
    __shared__ uint32_t s_wide;
    uint8_t* const image = reinterpret_cast<uint8_t*>(image_dwords);
    const uint32_t t = threadIdx.x;
    if (status[0] & SELA_HIP_FLAG_STRIDE) // (the decode in front refused the stride: nothing is written)
        return;
    if (t == 0)
        s_wide = 0;
    uint32_t wide = 0;
    for (uint32_t f = blockIdx.y; f < n_frames; f += gridDim.y) {
        const uint64_t so = sample_offsets[f], so1 = sample_offsets[f + 1];
        const uint64_t n64 = so1 - so;
        // every channel has the frame's length, and the frame ends inside n_frames * stride samples (a stream whose header walk
        // broke can say anything)
        bool bad = so1 < so || n64 > stride || so1 > (uint64_t)n_frames * stride;
        for (uint32_t c = t; c < channels; c += kPcmThreads)
            bad |= counts[(size_t)f * channels + c] != (uint32_t)n64;
        if (__syncthreads_or(bad)) { // (the barrier also closes the image of the frame before)
            if (t == 0 && blockIdx.x == 0) {
                atomicOr(&status[0], (uint32_t)SELA_HIP_FLAG_BAD_FRAME);
                atomicAdd(&status[1], 1u);
            }
            continue;
        }
        const uint32_t n = (uint32_t)n64;
        if (blockIdx.x * pcm_tile_samples(channels) >= n)
            continue;
        const PcmTile k = pcm_tile(so * channels * kBytes, blockIdx.x, n, channels, kBytes);
        const PcmStorePlan p = pcm_store_plan(k, n, kBytes);
        const int32_t* const fi = samples + (size_t)f * channels * stride;
        if (kBytes == 3 && p.lead && t == 0) // the value in front of the tile: its bytes from image byte 0 on
            put_sample<kBytes>(image, k.p - kBytes /* (below 0: only the bytes from `first` on exist) */, fi[(size_t)(channels - 1) * stride + k.s0 - 1], kBytes - k.p);
        const uint32_t items = k.items();
        for (uint32_t j = t; j < items; j += kPcmThreads) {
            const PcmItem it = k.item(j);
            const int32_t* const in = fi + (size_t)it.c * stride + it.s;
            int32_t v[4] = { 0, 0, 0, 0 };
            if (it.count == 4) {
                const Run<4> q = *reinterpret_cast<const Run<4>*>(in);
                v[0] = (int32_t)q.d[0], v[1] = (int32_t)q.d[1], v[2] = (int32_t)q.d[2], v[3] = (int32_t)q.d[3];
            } else {
#pragma unroll
                for (uint32_t i = 0; i < 3; i++)
                    if (i < it.count)
                        v[i] = in[i];
            }
#pragma unroll
            for (uint32_t i = 0; i < 4; i++) {
                if (i < it.count) {
                    put_sample<kBytes>(image, k.at(it.c, it.s + i, kBytes), v[i]);
                    if (kBytes == 3)
                        wide += v[i] < -(1 << 23) || v[i] >= (1 << 23) ? 1u : 0u;
                }
            }
        }
        __syncthreads();
        uint8_t* const dst = pcm_out + k.a0;
        if (t < p.head)
            dst[p.head_at + t] = image[p.head_at + t];
        if (t < p.tail)
            dst[p.tail_at + t] = image[p.tail_at + t];
        const uint32_t mid = p.mid_at >> 2;
        for (uint32_t r = t; r < p.runs; r += kPcmThreads)
            *reinterpret_cast<Run<kBytes>*>(dst + (size_t)(mid + r * kBytes) * 4) = *reinterpret_cast<const Run<kBytes>*>(image_dwords + mid + r * kBytes);
        for (uint32_t d = p.runs * kBytes + t; d < p.dwords; d += kPcmThreads)
            *reinterpret_cast<uint32_t*>(dst + (size_t)(mid + d) * 4) = image_dwords[mid + d];
    }
    if (kBytes == 3) { // one atomic per workgroup that found any
        if (wide)
            atomicAdd(&s_wide, wide);
        __syncthreads();
        if (t == 0 && s_wide)
            atomicAdd(&status[3], s_wide);
    }
}

dim3 pcm_grid(uint32_t n_frames, uint32_t channels, uint32_t samples) { return dim3(pcm_tiles(samples, channels), n_frames < 65535u ? n_frames : 65535u); }

} // namespace

hipError_t launch_pcm_unpack(const void* d_pcm, uint32_t bytes_per_sample, uint32_t n_frames, uint32_t channels, uint32_t n, int32_t* d_samples, hipStream_t stream)
{
    if (n_frames == 0)
        return hipSuccess;
    const dim3 grid = pcm_grid(n_frames, channels, n);
    if (bytes_per_sample == 3)
        hipLaunchKernelGGL(k_pcm_unpack<3>, grid, dim3(kPcmThreads), 0, stream, static_cast<const uint8_t*>(d_pcm), n_frames, channels, n, d_samples);
    else
        hipLaunchKernelGGL(k_pcm_unpack<4>, grid, dim3(kPcmThreads), 0, stream, static_cast<const uint8_t*>(d_pcm), n_frames, channels, n, d_samples);
    return hipGetLastError();
}

hipError_t launch_pcm_pack(const int32_t* d_samples, const uint32_t* d_counts, const uint64_t* d_sample_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride,
    uint32_t bytes_per_sample, void* d_pcm_out, uint32_t* d_status, hipStream_t stream)
{
    if (n_frames == 0)
        return hipSuccess;
    const dim3 grid = pcm_grid(n_frames, channels, stride);
    if (bytes_per_sample == 3)
        hipLaunchKernelGGL(k_pcm_pack<3>, grid, dim3(kPcmThreads), 0, stream, d_samples, d_counts, d_sample_offsets, n_frames, channels, stride,
            static_cast<uint8_t*>(d_pcm_out), d_status);
    else
        hipLaunchKernelGGL(k_pcm_pack<4>, grid, dim3(kPcmThreads), 0, stream, d_samples, d_counts, d_sample_offsets, n_frames, channels, stride,
            static_cast<uint8_t*>(d_pcm_out), d_status);
    return hipGetLastError();
}

} // namespace sela
