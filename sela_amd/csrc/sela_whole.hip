// sela_whole.hip -- a whole track with its tail (gfx950): the layout rule, the workspaces of
// sela_hip_encode_whole_device and sela_hip_encode_whole_pcm_device (5.25), and the splice that puts the long last frame behind
// the 2048-sample frames.
//
// The rule (include/sela_hip.h "a whole track"): N samples per channel are F = N / 2048 frames when F >= 1 -- the last of them
// 2048 + N % 2048 samples long -- and one frame of N samples below 2048.  It is written here once; the entry points
// (sela_capi.hip), the C++ host and the Python layer ask these functions.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "sela_host.h"

namespace sela {

namespace {
constexpr uint64_t kFrame = SELA_HIP_SAMPLES_PER_FRAME;
} // namespace

// the longest last frame of any track of at most max_samples samples per channel (0: no frame)
static uint32_t longest_last_frame(uint64_t max_samples) { return (uint32_t)std::min<uint64_t>(max_samples, 2 * kFrame - 1); }

// What both workspaces end in: the last frame as coded, in room for `bound_bytes`, and its head -- two offsets, and the four
// status words behind them.
static WholeLastWs carve_whole_last(Carve& c, size_t bound_bytes)
{
    WholeLastWs w;
    w.cap = (size_t)workspace_up(bound_bytes);
    w.frame = c.take<uint8_t>(w.cap);
    w.offsets = c.take<uint64_t>(2 + 2);
    w.status = reinterpret_cast<uint32_t*>(w.offsets + 2);
    return w;
}

// The 2048-sample frames' workspace | the last frame's any-length workspace | the last frame as coded | its head.  (Every
// shorter track is served from the same pieces: the sizes grow with the frames and with the length.)
WholeWs carve_whole(Carve& c, uint64_t max_samples, uint32_t channels)
{
    const uint32_t frames = (uint32_t)sela_hip_whole_frames(max_samples), last = std::max(longest_last_frame(max_samples), 1u);
    WholeWs w;
    w.main_bytes = encode_workspace_bytes(frames, channels); // (what the launch needs: the same on every device)
    w.last_bytes = encode_i32_device_workspace_bytes(1, channels, last);
    Carve main_ws = c.sub(w.main_bytes), last_ws = c.sub(w.last_bytes);
    w.main_workspace = main_ws.base();
    w.last_workspace = last_ws.base();
    if (c.listing()) { // (the two calls' own pieces, where they lie)
        encode_workspace_bytes(frames, channels, &main_ws);
        encode_i32_device_workspace_bytes(1, channels, last, false, &last_ws);
    }
    w.last = carve_whole_last(c, generic_encode_bound_bytes(1, channels, last));
    return w;
}

size_t whole_workspace_bytes(uint64_t max_samples, uint32_t channels, Carve* at)
{
    if (channels == 0 || channels > 255 || sela_hip_whole_frames(max_samples) * sela_hip_signals_per_frame(channels) >= (1ull << 31))
        return SIZE_MAX;
    return measured(at, [&](Carve& c) { carve_whole(c, max_samples, channels); });
}

// ---- the same track from packed 3- or 4-byte PCM: sela_hip_encode_whole_pcm_device ---------------------------------
// The 2048-sample frames' unpacked samples | sela_hip_encode_i32_device's workspace for them | the last frame's samples | its
// any-length workspace | the last frame as coded | its head.  (A track of whole frames only, or of one frame, uses the first or
// the second pair alone.)
WholePcmWs carve_whole_pcm(Carve& c, uint64_t max_samples, uint32_t channels)
{
    const uint32_t frames = (uint32_t)sela_hip_whole_frames(max_samples), last = std::max(longest_last_frame(max_samples), 1u);
    WholePcmWs w;
    w.main_samples = c.take<int32_t>((uint64_t)frames * channels * kFrame);
    Carve main_ws = c.sub(encode_i32_device_workspace_bytes(frames, channels, (uint32_t)kFrame));
    w.main_workspace = main_ws.base();
    if (c.listing()) // (the call's own pieces, where they lie)
        encode_i32_device_workspace_bytes(frames, channels, (uint32_t)kFrame, false, &main_ws);
    w.last_samples = c.take<int32_t>((uint64_t)channels * last);
    Carve last_ws = c.sub(encode_i32_device_workspace_bytes(1, channels, last));
    w.last_workspace = last_ws.base();
    if (c.listing())
        encode_i32_device_workspace_bytes(1, channels, last, false, &last_ws);
    w.last = carve_whole_last(c, sela_hip_encode_pcm_bound_bytes(1, channels, last, 4));
    return w;
}

size_t whole_pcm_workspace_bytes(uint64_t max_samples, uint32_t channels, Carve* at)
{
    if (channels == 0 || channels > 255 || sela_hip_whole_frames(max_samples) * generic_signals(channels, false) >= (1ull << 31))
        return SIZE_MAX;
    return measured(at, [&](Carve& c) { carve_whole_pcm(c, max_samples, channels); });
}

// ---- the splice ---------------------------------------------------------------------------------------------------------------
// The last frame was coded into the workspace (its own offsets {0, bytes} and status words beside it) while -- or after -- the
// 2048-sample frames were written: their plan left where they end in frame_offsets[last].  Copy the frame there if it ends
// inside frames_cap, say where it ends, and fold its status words into the call's.  Frames and their offsets are multiples of
// four bytes: whole words, one per lane and step.
constexpr int kSpliceThreads = 256;

__global__ __launch_bounds__(kSpliceThreads) void k_splice_tail(const uint32_t* __restrict__ last_frame, const uint64_t* __restrict__ last_offsets,
    const uint32_t* __restrict__ last_status, uint8_t* __restrict__ frames, uint64_t frames_cap, uint64_t* frame_offsets, uint32_t last, uint32_t* status)
{
    const uint64_t begin = frame_offsets[last], bytes = last_offsets[1], end = begin + bytes;
    const bool written = last_status[1] == 0 && end <= frames_cap;
    if (blockIdx.x == 0 && threadIdx.x == 0) { // (nobody reads these words in this launch: frame_offsets[last] is another one)
        frame_offsets[last + 1] = end;
        status[0] |= last_status[0];
        status[1] += written ? 0u : 1u;
    }
    if (!written)
        return;
    uint32_t* const out = reinterpret_cast<uint32_t*>(frames + begin);
    const uint32_t words = (uint32_t)(bytes >> 2);
    for (uint32_t i = blockIdx.x * kSpliceThreads + threadIdx.x; i < words; i += gridDim.x * kSpliceThreads)
        out[i] = last_frame[i];
}

hipError_t launch_whole_splice(const WholeLastWs& coded, uint32_t channels, uint8_t* d_frames, uint64_t frames_cap, uint64_t* d_frame_offsets, uint32_t last,
    uint32_t* d_status, hipStream_t stream)
{
    // (a stereo frame of 4095 samples is some 12 KB: a dozen workgroups; wide frames of many channels stride)
    const uint32_t grid = std::min(channels * 6u, 240u);
    hipLaunchKernelGGL(k_splice_tail, dim3(grid), dim3(kSpliceThreads), 0, stream, reinterpret_cast<const uint32_t*>(coded.frame), coded.offsets, coded.status, d_frames,
        frames_cap, d_frame_offsets, last, d_status);
    return hipGetLastError();
}

} // namespace sela

// ---- the layout rule: host only, no GPU ------------------------------------------------------------------------------------------
extern "C" {

uint64_t sela_hip_whole_frames(uint64_t n_samples) { return n_samples >= sela::kFrame ? n_samples / sela::kFrame : (n_samples ? 1 : 0); }

int sela_hip_whole_frame(uint64_t n_samples, uint64_t frame, uint64_t* first_sample, uint32_t* length)
{
    const uint64_t frames = sela_hip_whole_frames(n_samples);
    if (frame >= frames || !first_sample || !length)
        return sela::report_error(SELA_HIP_EINVAL, "sela_hip_whole_frame: no such frame, or a null pointer");
    *first_sample = frame * sela::kFrame;
    *length = (uint32_t)(frame + 1 < frames ? sela::kFrame : n_samples - frame * sela::kFrame);
    return SELA_HIP_OK;
}

size_t sela_hip_encode_whole_bound_bytes(uint64_t n_samples, uint32_t channels)
{
    const uint64_t frames = sela_hip_whole_frames(n_samples);
    if (frames == 0 || channels == 0 || channels > 255)
        return 0;
    const uint32_t last = (uint32_t)(n_samples - (frames - 1) * sela::kFrame);
    const uint64_t per_frame = sela_hip_encode_bound_bytes(1, channels);
    if (frames - 1 > (SIZE_MAX - sela_hip_encode_bound_bytes_n(1, channels, last)) / per_frame)
        return SIZE_MAX;
    return (size_t)((frames - 1) * per_frame) + sela_hip_encode_bound_bytes_n(1, channels, last);
}

size_t sela_hip_encode_whole_workspace_bytes(uint64_t max_samples, uint32_t channels) { return sela::whole_workspace_bytes(max_samples, channels); }

size_t sela_hip_encode_whole_pcm_bound_bytes(uint64_t n_samples, uint32_t channels, uint32_t bytes_per_sample)
{
    const uint64_t frames = sela_hip_whole_frames(n_samples);
    if (frames == 0 || channels == 0 || channels > 255 || (bytes_per_sample != 3 && bytes_per_sample != 4))
        return 0;
    const uint32_t last = (uint32_t)(n_samples - (frames - 1) * sela::kFrame);
    const size_t per_frame = sela_hip_encode_pcm_bound_bytes(1, channels, SELA_HIP_SAMPLES_PER_FRAME, bytes_per_sample),
                 last_frame = sela_hip_encode_pcm_bound_bytes(1, channels, last, bytes_per_sample);
    if (frames - 1 > (SIZE_MAX - last_frame) / per_frame)
        return SIZE_MAX;
    return (size_t)((frames - 1) * per_frame) + last_frame;
}

size_t sela_hip_encode_whole_pcm_workspace_bytes(uint64_t max_samples, uint32_t channels) { return sela::whole_pcm_workspace_bytes(max_samples, channels); }

} // extern "C"
