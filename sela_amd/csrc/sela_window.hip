// sela_window.hip -- sample windows of a stream: only the frames they touch are decoded (gfx950).
//
// Every frame of a .sela stream decodes on its own, so a window of a stream -- a player's seek, a random crop of a training
// batch -- needs the frames it overlaps and no others:
//
//   k_window_frames    the decoder with a clipped store.  Grid (window, j): workgroup (w, j) owns the output samples of window w
//                      that fall into the window's j-th frame, start / 2048 + j of its stream.  `cover`, the grid's second
//                      extent, is the most frames a window of that length can touch ((window_samples + 2046) / 2048 + 1): it
//                      depends on the length alone, so the launch is shaped on the host while the descriptors stay on the device.
//                      A workgroup whose frame is in the stream decodes it as k_decode_frames does -- one wave per subframe,
//                      frame_prologue and decode_subframe of sela_decode_core.inc, barrier -- and stores the shared second pass's
//                      values (parent - difference, mod 2^16) for its share of the window alone; one whose frame is not stores
//                      zeros for its share; one whose share is empty stores nothing.  Every output sample is written by exactly
//                      one workgroup: no pre-zeroing, no second kernel.  The LDS plan is the decoder's (decode_lds_bytes_for), so
//                      the occupancy is the decoder's too.
//
// The stores go sample by sample (channel_value16), consecutive lanes to consecutive samples: a window's base in the output has only
// its element's alignment (an odd start, an odd length, mono int16), which k_decode_frames' 16-byte stereo store cannot take.  In
// the code object a (sample, channel) is ~15 instructions for a channel of its own and ~22 for a difference channel -- one
// ds_read_u16, for a difference the parent's sub_info word and ds_read_u16 as well, the address, one global_store_short or
// _dword -- and a stereo frame is 32 such trips per lane, 64 two-byte stores per wave where the decoder issues 8 of 16 bytes.
// DESIGN.md 5.17 has what the whole kernel was measured to cost against k_decode_frames, and why it is not free.
//
// Generic mode (a subframe outside the LDS plan) parks its residues in the workspace by WORKGROUP, ((w * cover + j) * channels + c):
// two windows that share a frame decode it twice and must not share a slot.
//
// Scope: frames of 2048 samples, 1 .. 8 channels, 16-bit output (k_decode_frames_wide resolves difference channels over its own
// global output, which a clipped store does not have; streams of any other length need a search of sample_offsets).
#include "sela_host.h"

#include "sela_synth.h"

namespace sela {

#include "sela_decode_core.inc"

static_assert(sizeof(sela_hip_window) == 16, "a descriptor is read as two 64-bit words");

__global__ __launch_bounds__(kDecMaxWaves * 64) __attribute__((amdgpu_waves_per_eu(7, 8))) void k_window_frames(const uint8_t* __restrict__ frames,
    const uint64_t* __restrict__ frame_offsets, uint32_t n_frames_total, uint32_t channels, const sela_hip_window* __restrict__ windows, uint32_t window_samples,
    uint32_t format, void* __restrict__ out, uint32_t* __restrict__ window_flags /* [gridDim.x], zeroed */, uint32_t* __restrict__ status, int32_t* __restrict__ ws_residues,
    uint32_t vec_shift_from /* as in k_decode_frames, by the workgroup's place in the launch */, uint32_t synth_priorities /* as in k_decode_frames */)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    const int n_waves = blockDim.x / 64;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / 64)), lane = threadIdx.x % 64;
    const DecFrameLds l = carve_frame_lds(dyn, channels, n_waves);

    const uint32_t w = blockIdx.x, j = blockIdx.y;
    const uint64_t start = windows[w].start;
    const uint32_t first_frame = windows[w].first_frame;
    // the stream, cut at the table's end
    const uint32_t in_stream = first_frame < n_frames_total ? min(windows[w].n_frames, n_frames_total - first_frame) : 0u;
    const uint64_t q = start / (uint32_t)kBlock; // the window's first frame, within the stream
    const uint32_t r = (uint32_t)(start % (uint32_t)kBlock);
    // this workgroup's share of the window, [lo, hi): the samples of frame q + j (window_samples <= 2^24: nothing wraps)
    const uint32_t lo = j == 0 ? 0u : j * (uint32_t)kBlock - r;
    const uint32_t hi = min(window_samples, (j + 1) * (uint32_t)kBlock - r);
    if (lo >= hi)
        return;
    const uint32_t n_share = hi - lo;
    const uint32_t s0 = lo + r - j * (uint32_t)kBlock; // the share's first sample within its frame
    int16_t* const out16 = static_cast<int16_t*>(out) + ((size_t)w * window_samples + lo) * channels;        // [window][sample][channel]
    float* const outf = static_cast<float*>(out) + (size_t)w * channels * window_samples + lo;                // [window][channel][sample]
    const bool planar = format == SELA_HIP_WINDOW_F32_PLANAR;

    if (q >= in_stream || j >= in_stream - (uint32_t)q) { // (q is compared first: start + i is never formed)
        for (uint32_t t = threadIdx.x; t < n_share; t += blockDim.x)
            for (uint32_t c = 0; c < channels; c++) {
                if (planar)
                    outf[(size_t)c * window_samples + t] = 0.0f;
                else
                    out16[(size_t)t * channels + c] = 0;
            }
        return;
    }

    const uint32_t f = first_frame + (uint32_t)q + j;
    const uint32_t group = blockIdx.y * gridDim.x + blockIdx.x; // (the order workgroups are dispatched in)
    const bool vec_shift = group >= vec_shift_from;
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
        decode_subframe<false>(fb, fbytes, hd, fast, l.sub + c, l.scratch0 + wave, ws_residues, ((size_t)w * gridDim.y + j) * channels + c, vec_shift, synth_priorities,
            lane, flags, nullptr);
        if (lane == 0)
            l.sub_info[hd.channel] = sub_info_word(hd.type, hd.parent, c);
    }
    __syncthreads();

    // ---- the second pass, clipped to the window ---------------------------------------------------------------------------
    // What k_decode_frames writes for sample s0 + t of frame f goes to sample lo + t of the window.
    // Channel by channel: what sub_info says of a channel and of its parent is read once per channel, not once per sample.
    for (uint32_t c = 0; c < channels; c++)
        for (uint32_t t = threadIdx.x; t < n_share; t += blockDim.x) {
            const int16_t v = (int16_t)(uint16_t)channel_value16(l.sub, l.sub_info, c, s0 + t);
            if (planar)
                outf[(size_t)c * window_samples + t] = (float)v * (1.0f / 32768.0f); // (exact in binary32)
            else
                out16[(size_t)t * channels + c] = v;
        }
    if (threadIdx.x == 0)
        flags |= layout_flags(l.sub_info, channels);
    flags = wave_or(flags);
    if (lane == 0 && flags) {
        atomicOr(&status[0], flags);
        if (wave == 0 && (flags & SELA_HIP_FLAG_BAD_FRAME))
            atomicAdd(&status[1], 1u);
        if (atomicOr(&window_flags[w], flags) == 0) // the window's first flag, whichever wave of whichever of its frames brings it
            atomicAdd(&status[2], 1u);
    }
}

// d_status and the windows' flag words, zeroed ahead of k_window_frames.  A kernel and not hipMemsetAsync: a 16-byte memset node of
// this call, replayed from a captured graph, has left other values than zero in its target ("Open question": the
// cause is not known).  One launch clears both arrays, and a kernel node carries its arguments in the graph.
constexpr uint32_t kWindowClearThreads = 256;
__global__ __launch_bounds__(kWindowClearThreads) void k_window_clear(uint32_t* __restrict__ status, uint32_t* __restrict__ window_flags /* or null */, uint32_t n_windows)
{
    const uint32_t w = blockIdx.x * kWindowClearThreads + threadIdx.x;
    if (w < 4)
        status[w] = 0;
    if (window_flags && w < n_windows)
        window_flags[w] = 0;
}

// k_window_clear for the window calls of other files (sela_window32.hip): a word per window, or none where window_flags is null.
hipError_t launch_window_clear(uint32_t* d_status, uint32_t* d_window_flags, uint32_t n_windows, hipStream_t stream)
{
    const uint32_t groups = d_window_flags && n_windows ? (n_windows + kWindowClearThreads - 1) / kWindowClearThreads : 1u;
    hipLaunchKernelGGL(k_window_clear, dim3(groups), dim3(kWindowClearThreads), 0, stream, d_status, d_window_flags, d_window_flags ? n_windows : 0u);
    return hipGetLastError();
}

uint32_t window_cover(uint32_t window_samples) { return (uint32_t)(((uint64_t)window_samples + 2046) / (uint32_t)kBlock + 1); }

// The dynamic LDS a launch of k_window_frames asks for (sela_hip_debug_window_lds_bytes: tests hold it against the decoder's).
size_t window_lds_bytes(uint32_t channels) { return decode_lds_bytes_for(channels, decode_waves(channels)); }

// Generic mode's residues, one block per (workgroup, channel) | a flag word per window for the calls that pass no d_window_flags
// (launch_window_whole's kernels raise flags in the same words).
WindowWs carve_windows(Carve& c, uint32_t n_windows, uint32_t window_samples, uint32_t channels)
{
    WindowWs w;
    w.residues = c.take<int32_t>((uint64_t)n_windows * window_cover(window_samples) * channels * kBlock);
    w.flag_words = c.take<uint32_t>(n_windows);
    return w;
}
// The header's formula (include/sela_hip.h): the two pieces and the base's alignment.  The residues are whole blocks of 8 KiB,
// so the flag words start where they end and the carve fits (tests/test_workspace_cpu.py holds every shape to that).
size_t window_workspace_bytes(uint32_t n_windows, uint32_t window_samples, uint32_t channels, Carve* at)
{
    if (at)
        carve_windows(*at, n_windows, window_samples, channels);
    return (size_t)n_windows * window_cover(window_samples) * channels * kBlock * sizeof(int32_t) + (size_t)n_windows * sizeof(uint32_t) + 256;
}

// Clear, then decode: one serial chain on the caller's stream, capturable.  The arguments have been checked (sela_capi.hip).
hipError_t launch_window_frames(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames_total, uint32_t channels, const sela_hip_window* d_windows,
    uint32_t n_windows, uint32_t window_samples, uint32_t format, void* d_out, uint32_t* d_window_flags, uint32_t* d_status, void* d_workspace, hipStream_t stream,
    int recurrence_form, uint32_t synth_priorities)
{
    if (n_windows == 0) {
        hipLaunchKernelGGL(k_window_clear, dim3(1), dim3(kWindowClearThreads), 0, stream, d_status, static_cast<uint32_t*>(nullptr), 0u);
        return hipGetLastError();
    }
    if (channels == 0 || channels > (uint32_t)kDecMaxWaves)
        return hipErrorInvalidValue;
    const uint32_t cover = window_cover(window_samples);
    Carve carve(d_workspace);
    const WindowWs ws = carve_windows(carve, n_windows, window_samples, channels);
    uint32_t* const flags = d_window_flags ? d_window_flags : ws.flag_words;
    hipLaunchKernelGGL(k_window_clear, dim3((n_windows + kWindowClearThreads - 1) / kWindowClearThreads), dim3(kWindowClearThreads), 0, stream, d_status, flags, n_windows);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess)
        return err;
    const int n_waves = decode_waves(channels);
    const size_t lds = window_lds_bytes(channels);
    if (lds > 64 * 1024) { // above the default dynamic-LDS limit (more than four channels); per device, so every time
        err = hipFuncSetAttribute(reinterpret_cast<const void*>(k_window_frames), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (err != hipSuccess)
            return err;
    }
    const uint32_t groups = n_windows * cover; // (below 2^31: checked)
    const uint32_t from = recurrence_form >= 0
        ? (recurrence_form ? 0u : groups)
        : vec_shift_from_for(groups, n_waves, resident_frames(reinterpret_cast<const void*>(k_window_frames), n_waves, lds, kResidencyWindows));
    hipLaunchKernelGGL(k_window_frames, dim3(n_windows, cover), dim3(n_waves * 64), lds, stream, d_frames, d_frame_offsets, n_frames_total, channels, d_windows,
        window_samples, format, d_out, flags, d_status, ws.residues, from, synth_priorities);
    return hipGetLastError();
}

} // namespace sela

extern "C" size_t sela_hip_debug_window_lds_bytes(uint32_t channels)
{
    return channels == 0 || channels > (uint32_t)sela::kDecMaxWaves ? 0 : sela::window_lds_bytes(channels);
}
