// sela_capi_pcm.hip -- the C boundary of the packed 3- / 4-byte PCM calls (include/sela_hip.h "24- and 32-bit PCM"; DESIGN.md 5.22;
// kernels: sela_pcm.hip).  The composed calls are the unpack in front of launch_encode_i32_device and the pack behind
// launch_decode_i32_device -- those two launches exactly as sela_hip_encode_i32_device_opt and sela_hip_decode_i32_device make
// them, on a piece of this call's workspace.  Every check comes before anything is enqueued.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "sela_generic.h"
#include "sela_hip.h"
#include "sela_host.h"
#include "sela_pcm.h"

namespace sela {

// The encode's workspace: the unpacked samples, int32 [n_frames][channels][n] | sela_hip_encode_i32_device's own.
struct EncodePcmWs {
    int32_t* samples;
    void* encode;
};
static EncodePcmWs carve_encode_pcm(Carve& c, uint32_t n_frames, uint32_t channels, uint32_t n)
{
    EncodePcmWs w;
    w.samples = c.take<int32_t>((uint64_t)n_frames * channels * n);
    Carve inner = c.sub(encode_i32_device_workspace_bytes(n_frames, channels, n));
    w.encode = inner.base();
    if (c.listing())
        encode_i32_device_workspace_bytes(n_frames, channels, n, false, &inner);
    return w;
}

size_t encode_pcm_workspace_bytes(uint32_t n_frames, uint32_t channels, uint32_t n, Carve* at)
{
    if (encode_i32_device_workspace_bytes(n_frames, channels, n) == SIZE_MAX)
        return SIZE_MAX;
    return measured(at, [&](Carve& c) { carve_encode_pcm(c, n_frames, channels, n); });
}

// The decode's workspace: sela_hip_decode_i32_device's own | its samples, int32 [max_frames][channels][stride] | its counts | the
// sample offsets of a caller that asks for none.
struct DecodePcmWs {
    void* decode;
    int32_t* samples;
    uint32_t* counts;
    uint64_t* offsets;
};
static DecodePcmWs carve_decode_pcm(Carve& c, uint32_t max_frames, uint32_t channels, uint32_t stride)
{
    const uint64_t subs = (uint64_t)max_frames * channels;
    DecodePcmWs w;
    Carve inner = c.sub(decode_i32_workspace_bytes(max_frames, channels, stride));
    w.decode = inner.base();
    if (c.listing())
        decode_i32_workspace_bytes(max_frames, channels, stride, &inner);
    w.samples = c.take<int32_t>(subs * stride);
    w.counts = c.take<uint32_t>(subs);
    w.offsets = c.take<uint64_t>((uint64_t)max_frames + 1);
    return w;
}

size_t decode_pcm_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride, Carve* at)
{
    if (decode_i32_workspace_bytes(max_frames, channels, stride) == SIZE_MAX)
        return SIZE_MAX;
    return measured(at, [&](Carve& c) { carve_decode_pcm(c, max_frames, channels, stride); });
}

hipError_t launch_encode_pcm_device(const void* d_pcm, uint32_t bytes_per_sample, uint32_t n_frames, uint32_t channels, uint32_t n, bool lossless, uint8_t* d_frames,
    uint64_t frames_cap, uint64_t* d_frame_offsets, uint32_t* d_status, void* d_workspace, hipStream_t stream)
{
    Carve c(d_workspace);
    const EncodePcmWs w = carve_encode_pcm(c, n_frames, channels, n);
    const hipError_t e = launch_pcm_unpack(d_pcm, bytes_per_sample, n_frames, channels, n, w.samples, stream);
    if (e != hipSuccess)
        return e;
    return launch_encode_i32_device(w.samples, false, n_frames, channels, n, d_frames, frames_cap, d_frame_offsets, d_status, w.encode, stream, lossless);
}

hipError_t launch_decode_pcm_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride,
    uint32_t bytes_per_sample, void* d_pcm_out, uint64_t* d_sample_offsets, uint32_t* d_status, void* d_workspace, int mode, hipStream_t stream)
{
    Carve c(d_workspace);
    const DecodePcmWs w = carve_decode_pcm(c, n_frames, channels, stride);
    uint64_t* const d_so = d_sample_offsets ? d_sample_offsets : w.offsets;
    const hipError_t e = launch_decode_i32_device(d_frames, d_frame_offsets, n_frames, nullptr, channels, stride, w.samples, w.counts, d_so, d_status, w.decode, mode, stream);
    if (e != hipSuccess)
        return e;
    return launch_pcm_pack(w.samples, w.counts, d_so, n_frames, channels, stride, bytes_per_sample, d_pcm_out, d_status, stream);
}

} // namespace sela

namespace {

int fail(int code, const std::string& what) { return sela::report_error(code, what); }
int launched(hipError_t e, const char* what) { return e == hipSuccess ? SELA_HIP_OK : sela::report_hip_error(e, what); }

// what every call here asks of its shape, in one order: the container, the channels, the length (a stride, or a frame's samples), the count
int check_pcm_shape(uint32_t bytes_per_sample, uint32_t n_frames, uint32_t channels, uint32_t length, bool is_stride)
{
    if (bytes_per_sample != 3 && bytes_per_sample != 4)
        return fail(SELA_HIP_EINVAL, "bytes_per_sample must be 3 or 4 (16-bit samples: sela_hip_encode_n_device / sela_hip_decode_n_device and the int16 host calls)");
    if (channels == 0 || channels > 255)
        return fail(SELA_HIP_EINVAL, "channels must be in 1..255");
    if (is_stride && length == 0)
        return fail(SELA_HIP_EINVAL, "stride must not be 0");
    if (!is_stride && (length == 0 || length > 65535))
        return fail(SELA_HIP_EINVAL, "samples_per_channel must be 1 .. 65535 (the subframe's field is 16 bits wide)");
    if ((uint64_t)n_frames * sela::generic_signals(channels, false) >= (1ull << 31))
        return fail(SELA_HIP_EINVAL, "n_frames * signals per frame must stay below 2^31");
    return SELA_HIP_OK;
}
int check_pcm_options(uint32_t options, bool* lossless)
{
    if (options & ~(uint32_t)SELA_HIP_ENCODE_LOSSLESS)
        return fail(SELA_HIP_EINVAL, "options: a bit this library does not know (SELA_HIP_ENCODE_LOSSLESS is the only one)");
    *lossless = options != 0;
    return SELA_HIP_OK;
}
int null_pointer() { return fail(SELA_HIP_EINVAL, "null device pointer"); }
bool misaligned(const void* p) { return ((uintptr_t)p & 3) != 0; }

} // namespace

extern "C" {

size_t sela_hip_encode_pcm_workspace_bytes(uint32_t n_frames, uint32_t channels, uint32_t samples_per_channel)
{
    return sela::encode_pcm_workspace_bytes(n_frames, channels, samples_per_channel);
}

size_t sela_hip_decode_pcm_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride)
{
    return sela::decode_pcm_workspace_bytes(max_frames, channels, stride);
}

// Whatever the container: the encoder refuses a zig-zag residue of 2^31 or more and a subframe of more than 65535 Rice words, and
// its Rice parameter is the minimum of a convex bits(k) over k = 0 .. 19 -- never worse than k = 19 (sela_hip.h).
size_t sela_hip_encode_pcm_bound_bytes(uint32_t n_frames, uint32_t channels, uint32_t samples_per_channel, uint32_t bytes_per_sample)
{
    (void)bytes_per_sample;
    return std::max(sela_hip_encode_bound_bytes_n(n_frames, channels, samples_per_channel), sela::generic_encode_bound_bytes(n_frames, channels, samples_per_channel));
}

int sela_hip_pcm_unpack_device(const void* d_pcm, uint32_t bytes_per_sample, uint32_t n_frames, uint32_t channels, uint32_t samples_per_channel, int32_t* d_samples,
    void* stream)
{
    const int rc = check_pcm_shape(bytes_per_sample, n_frames, channels, samples_per_channel, false);
    if (rc != SELA_HIP_OK)
        return rc;
    if (n_frames && (!d_pcm || !d_samples))
        return null_pointer();
    if (misaligned(d_pcm) || misaligned(d_samples))
        return fail(SELA_HIP_EINVAL, "d_pcm and d_samples must be 4-byte aligned");
    return launched(sela::launch_pcm_unpack(d_pcm, bytes_per_sample, n_frames, channels, samples_per_channel, d_samples, static_cast<hipStream_t>(stream)), "pcm_unpack launch");
}

int sela_hip_pcm_pack_device(const int32_t* d_samples, const uint32_t* d_counts, const uint64_t* d_sample_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride,
    uint32_t bytes_per_sample, void* d_pcm_out, uint32_t* d_status, void* stream)
{
    const int rc = check_pcm_shape(bytes_per_sample, n_frames, channels, stride, true);
    if (rc != SELA_HIP_OK)
        return rc;
    if (!d_status || !d_sample_offsets || (n_frames && (!d_samples || !d_counts || !d_pcm_out)))
        return null_pointer();
    if (misaligned(d_samples) || misaligned(d_counts) || misaligned(d_pcm_out) || misaligned(d_status) || ((uintptr_t)d_sample_offsets & 7))
        return fail(SELA_HIP_EINVAL, "d_samples, d_counts, d_pcm_out and d_status must be 4-byte aligned, d_sample_offsets 8-byte aligned");
    return launched(sela::launch_pcm_pack(d_samples, d_counts, d_sample_offsets, n_frames, channels, stride, bytes_per_sample, d_pcm_out, d_status,
                        static_cast<hipStream_t>(stream)),
        "pcm_pack launch");
}

int sela_hip_encode_pcm_device(const void* d_pcm, uint32_t bytes_per_sample, uint32_t n_frames, uint32_t channels, uint32_t samples_per_channel, uint32_t options,
    uint8_t* d_frames, size_t frames_cap, uint64_t* d_frame_offsets, uint32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream)
{
    int rc = check_pcm_shape(bytes_per_sample, n_frames, channels, samples_per_channel, false);
    if (rc != SELA_HIP_OK)
        return rc;
    bool lossless = false;
    if ((rc = check_pcm_options(options, &lossless)) != SELA_HIP_OK)
        return rc;
    if (!d_frame_offsets || !d_status || !d_workspace || (n_frames && (!d_pcm || !d_frames)))
        return null_pointer();
    if (misaligned(d_pcm) || misaligned(d_frames))
        return fail(SELA_HIP_EINVAL, "d_pcm and d_frames must be 4-byte aligned");
    if (workspace_bytes < sela::encode_pcm_workspace_bytes(n_frames, channels, samples_per_channel))
        return fail(SELA_HIP_ECAPACITY, "workspace smaller than sela_hip_encode_pcm_workspace_bytes()");
    return launched(sela::launch_encode_pcm_device(d_pcm, bytes_per_sample, n_frames, channels, samples_per_channel, lossless, d_frames, frames_cap, d_frame_offsets, d_status,
                        d_workspace, static_cast<hipStream_t>(stream)),
        "encode_pcm launch");
}

int sela_hip_decode_pcm_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride, uint32_t bytes_per_sample,
    void* d_pcm_out, uint64_t* d_sample_offsets, uint32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream)
{
    const int rc = check_pcm_shape(bytes_per_sample, n_frames, channels, stride, true);
    if (rc != SELA_HIP_OK)
        return rc;
    if (!d_frame_offsets || !d_status || !d_workspace || (n_frames && (!d_frames || !d_pcm_out)))
        return null_pointer();
    if (misaligned(d_frames) || misaligned(d_pcm_out))
        return fail(SELA_HIP_EINVAL, "d_frames and d_pcm_out must be 4-byte aligned");
    const size_t need = sela::decode_pcm_workspace_bytes(n_frames, channels, stride);
    if (need == SIZE_MAX || workspace_bytes < need)
        return fail(SELA_HIP_ECAPACITY, "workspace smaller than sela_hip_decode_pcm_workspace_bytes()");
    return launched(sela::launch_decode_pcm_device(d_frames, d_frame_offsets, n_frames, channels, stride, bytes_per_sample, d_pcm_out, d_sample_offsets, d_status, d_workspace,
                        sela::generic_standard_first_mode(), static_cast<hipStream_t>(stream)),
        "decode_pcm launch");
}

int sela_hip_decode_pcm_status_error(const uint32_t* status)
{
    if (!status)
        return fail(SELA_HIP_EINVAL, "null pointer");
    const uint32_t decode_status[4] = { status[0], status[1], status[2], 0 }; // ([3], the samples beyond a 3-byte container, is informational)
    return sela_hip_decode_status_error(decode_status);
}

int sela_hip_encode_pcm(const void* pcm, uint32_t bytes_per_sample, uint32_t n_frames, uint32_t channels, uint32_t samples_per_channel, uint32_t options,
    uint8_t* frames_out, size_t frames_cap, uint64_t* frame_offsets_out)
{
    int rc = check_pcm_shape(bytes_per_sample, n_frames, channels, samples_per_channel, false);
    if (rc != SELA_HIP_OK)
        return rc;
    bool lossless = false;
    if ((rc = check_pcm_options(options, &lossless)) != SELA_HIP_OK)
        return rc;
    if (!frame_offsets_out || (n_frames && (!pcm || !frames_out)))
        return fail(SELA_HIP_EINVAL, "null pointer");
    return sela::generic_encode_pcm(static_cast<const uint8_t*>(pcm), bytes_per_sample, n_frames, channels, samples_per_channel, lossless, frames_out, frames_cap,
        frame_offsets_out);
}

int sela_hip_decode_pcm(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t bytes_per_sample, void* pcm_out,
    size_t pcm_cap, uint32_t* wide_samples)
{
    const int rc = check_pcm_shape(bytes_per_sample, n_frames, channels, 1, true);
    if (rc != SELA_HIP_OK)
        return rc;
    if (!frame_offsets || (n_frames && (!frames || !pcm_out)))
        return fail(SELA_HIP_EINVAL, "null pointer");
    if (wide_samples)
        *wide_samples = 0;
    if (n_frames == 0)
        return SELA_HIP_OK;
    if (sela::check_frame_offsets(frame_offsets, n_frames) != SELA_HIP_OK)
        return SELA_HIP_EFORMAT;
    std::vector<uint64_t> sample_offsets((size_t)n_frames + 1);
    const uint32_t largest = sela::generic_index_samples(frames, frame_offsets, n_frames, channels, sample_offsets.data(), nullptr);
    if (largest == 0)
        return fail(SELA_HIP_EFORMAT, "malformed frame stream (the header walk breaks, or no subframe says a length)");
    if (sample_offsets[n_frames] * channels * bytes_per_sample > pcm_cap)
        return fail(SELA_HIP_ECAPACITY, "pcm_out too small (sela_hip_index_samples()[n_frames] * channels * bytes_per_sample bytes are needed)");
    return sela::generic_decode_pcm(frames, frame_offsets, sample_offsets.data(), n_frames, channels, largest, bytes_per_sample, static_cast<uint8_t*>(pcm_out),
        wide_samples);
}

} // extern "C"
