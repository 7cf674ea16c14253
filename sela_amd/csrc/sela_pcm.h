// sela_pcm.h -- packed 3- / 4-byte PCM on the device: what sela_pcm.hip (the two kernels), sela_capi_pcm.hip (the
// device-pointer calls) and sela_capi_generic.hip (the host-pointer calls on the leased context) share.
#ifndef SELA_PCM_H_
#define SELA_PCM_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sela_workspace.h"

namespace sela {

// k_pcm_unpack<3|4>: d_pcm [n_frames][n][channels] packed -> d_samples int32 [n_frames][channels][n].  Arguments checked by the caller.
hipError_t launch_pcm_unpack(const void* d_pcm, uint32_t bytes_per_sample, uint32_t n_frames, uint32_t channels, uint32_t n, int32_t* d_samples, hipStream_t stream);
// k_pcm_pack<3|4>: what launch_decode_i32_device leaves (samples [n_frames][channels][stride], counts, sample offsets) -> packed
// frames at sample_offsets[f] * channels * bytes_per_sample.  d_status: [0] is read (SELA_HIP_FLAG_STRIDE: nothing is written) and
// ORed into, [1] and [3] are added to.
hipError_t launch_pcm_pack(const int32_t* d_samples, const uint32_t* d_counts, const uint64_t* d_sample_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride,
    uint32_t bytes_per_sample, void* d_pcm_out, uint32_t* d_status, hipStream_t stream);

// sela_hip_encode_pcm_device / sela_hip_decode_pcm_device without their checks: the launches on `stream`, nothing waited for.
// SIZE_MAX: a shape the call refuses.
size_t encode_pcm_workspace_bytes(uint32_t n_frames, uint32_t channels, uint32_t n, Carve* at = nullptr);
size_t decode_pcm_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride, Carve* at = nullptr);
hipError_t launch_encode_pcm_device(const void* d_pcm, uint32_t bytes_per_sample, uint32_t n_frames, uint32_t channels, uint32_t n, bool lossless, uint8_t* d_frames,
    uint64_t frames_cap, uint64_t* d_frame_offsets, uint32_t* d_status, void* d_workspace, hipStream_t stream);
hipError_t launch_decode_pcm_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride,
    uint32_t bytes_per_sample, void* d_pcm_out, uint64_t* d_sample_offsets /* or null */, uint32_t* d_status, void* d_workspace, int mode, hipStream_t stream);

// sela_hip_encode_pcm / sela_hip_decode_pcm (sela_capi_generic.hip): the launches above on chunks of whole frames, on the calling
// thread's leased context and stream.  Arguments checked by the caller.
int generic_encode_pcm(const uint8_t* pcm, uint32_t bytes_per_sample, uint32_t n_frames, uint32_t channels, uint32_t n, bool lossless, uint8_t* frames_out,
    size_t frames_cap, uint64_t* frame_offsets_out);
int generic_decode_pcm(const uint8_t* frames, const uint64_t* frame_offsets, const uint64_t* sample_offsets /* the host's walk */, uint32_t n_frames, uint32_t channels,
    uint32_t stride, uint32_t bytes_per_sample, uint8_t* pcm_out, uint32_t* wide_samples /* or null: status[3] summed */);

} // namespace sela
#endif
