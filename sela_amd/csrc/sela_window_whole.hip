// sela_window_whole.hip -- sample windows that reach the long last frame of a whole-track stream (gfx950), and, at
// the end of the file, the full decode of such a stream on the same last-frame kernel.
//
// A whole-track stream (5.19) is 2048-sample frames and ONE last frame of 1 .. 4095 samples.  Frame f still starts at sample
// 2048 f, so k_window_frames (sela_window.hip) keeps its arithmetic and its frames; the last frame is the any-length decoder's
// (sela_decode32.hip).  The call is both, one serial chain on the caller's stream:
//
//   k_tailwin_plan     a thread per window.  Finds the stream's last frame L inside the table and reads what it says its length
//                      is (frame_says_samples: sela_format.h's reader).  1 .. 4095 and not 2048: the window's descriptor is copied
//                      into the workspace with n_frames one less, and a WindowTail says which of the window's samples are L's.
//                      Anything else: the copy is the descriptor and the tail is empty.
//   k_window_clear, k_window_frames   launch_window_frames as it is, on the copies: status and flags cleared, every element of
//                      d_out written -- the share of L as the zeros of a stream that has ended there, without a flag.
//   k_tailwin_decode   grid (window, subframe), one wave each: the subframe of L at that position, by segments
//                      (parse_stream_segments, sela_segments.inc), predictor_table and synthesize_by_order with the length a
//                      run-time value -- k_decode_subframes32's non-standard path -- into the workspace as 32-bit samples, with
//                      a record of what the header said and of the flags met.  A wave whose window has no share returns at once.
//   k_tailwin_store    a workgroup per window.  Thread 0 turns the records into k_interleave16's list of writes (sela_generic.hip:
//                      independent subframes first, then dependent ones in subframe order, under the combine's rules); every
//                      thread runs them for its samples of the share and the values go out narrowed as that kernel narrows
//                      them, int16 interleaved or float planar, consecutive lanes to consecutive samples.  A frame the decode
//                      declined, or one whose layout the rules refuse, stores nothing (the zeros stay) and raises its flags:
//                      status[0], status[1] for BAD_FRAME, the window's word, and status[2] if it is the window's first flag.
//
// Two kernels behind the plan and not one: the decode is a wave of its own register budget with 4.4 KB of LDS, as
// k_decode_subframes32 is, and up to eight of them in one workgroup with a barrier would hold the whole group for the longest
// subframe; the store wants 256 lanes and none of the decoder's state.  An empty launch of either costs what a kernel that
// returns at once costs (5.13).
#include <hip/hip_runtime.h>

#include "sela_host.h"
#include "sela_decode_whole_plan.h"
#include "sela_window_tail.h"

#include "sela_synth.h"

namespace sela {

#include "sela_decode_core.inc"

#include "sela_segments.inc"

static_assert(sizeof(sela_hip_window) == 16, "a descriptor is copied as two 64-bit words");

#include "sela_tail_store.h" // TailSub, TailStoreList, tail_store_list, tail_store_sample: sela_window32.hip stores by them too

__global__ __launch_bounds__(kTailPlanThreads) void k_tailwin_plan(const uint8_t* __restrict__ frames, const uint64_t* __restrict__ frame_offsets, uint32_t n_frames_total,
    const sela_hip_window* __restrict__ windows, uint32_t n_windows, uint32_t window_samples, sela_hip_window* __restrict__ copies, WindowTail* __restrict__ tails)
{
    const uint32_t w = blockIdx.x * kTailPlanThreads + threadIdx.x;
    if (w >= n_windows)
        return;
    sela_hip_window d = windows[w];
    WindowTail t = {};
    const uint32_t n = window_stream_frames(d, n_frames_total);
    if (n != 0) {
        const uint32_t last = d.first_frame + n - 1;
        const uint32_t n_last = frame_says_samples(frames, frame_offsets, last);
        if (tail_length(n_last)) {
            t = window_tail_share(d.start, window_samples, n, n_last);
            t.frame = last;
            d.n_frames = n - 1;
        }
    }
    copies[w] = d;
    tails[w] = t;
}

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(7, 8))) void k_tailwin_decode(const uint8_t* __restrict__ frames,
    const uint64_t* __restrict__ frame_offsets, uint32_t channels, const WindowTail* __restrict__ tails, int32_t* __restrict__ dec_ws /* [window][position][kTailStride] */,
    TailSub* __restrict__ subs /* [window][position] */)
{
    __shared__ __attribute__((aligned(16))) DecSubframeLds sl;
    __shared__ DecWaveScratch scratch;
    const uint32_t w = blockIdx.x, c = blockIdx.y;
    const WindowTail t = tails[w];
    if (t.lo >= t.hi)
        return;
    const int lane = threadIdx.x;
    const uint64_t at = frame_offsets[t.frame], end = frame_offsets[t.frame + 1];
    const uint8_t* const fb = frames + at;
    const uint64_t fbytes = end >= at ? end - at : 0;
    const SubHeader hd = walk_headers(fb, (at & 3) == 0 ? fbytes : 0 /* a frame at a place that is not word-aligned: not walked */, c);
    // (k_decode_subframes32's own test, the stride being what a last frame may say)
    const bool mine = hd.ok && sela_subframe_decodable(&hd) && hd.n <= kTailMaxSamples && hd.n != 0 && hd.n > hd.order;
    uint32_t flags = 0;
    if (mine) {
        const uint32_t nw = hd.cw + 2 + hd.rw;
        const uint32_t* const gw = reinterpret_cast<const uint32_t*>(fb + hd.p + 4); // the subframe's aligned words
        SynthTables* const tables = &scratch.t;
        const uint32_t order = hd.order;
        int32_t* const samples = dec_ws + ((size_t)w * channels + c) * kTailStride;
        if (order)
            flags |= parse_stream_segments(gw, nw, 24, 24 + 32 * hd.cw, hd.ck, order, (256 * hd.cw + order - 1) / order + 1, &sl, reinterpret_cast<uint16_t*>(tables),
                coef_values(&scratch), lane);
        flags |= parse_stream_segments(gw, nw, 32 * (hd.cw + 2), 32 * nw, hd.rk, hd.n, (256 * hd.rw + hd.n - 1) / hd.n + 1, &sl, reinterpret_cast<uint16_t*>(tables), samples,
            lane);
        // the lanes read each other's residues back: the stores have left the CU, nothing older is served from its vector cache
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        const int32_t q_lo = (uint32_t)lane < order ? coef_values(&scratch)[lane] : 0, q_hi = (uint32_t)lane + 64 < order ? coef_values(&scratch)[lane + 64] : 0;
        wave_sync();
        const bool fits24 = predictor_table(order, q_lo, q_hi, tables, lane, flags);
        SynthOut<true> out32;
        out32.samples = samples;
        out32.n = hd.n;
        flags = wave_or(flags);
        if (flags == 0) // (a stream in trouble is declined: its share stays zero)
            synthesize_by_order<true, true>(order, gw, nw, hd.rk, sl.pos, samples, tables->tab, fits24, lane, out32);
    }
    flags = wave_or(flags);
    if (lane == 0) {
        TailSub s = {};
        s.ok = mine && flags == 0 ? 1 : 0;
        if (s.ok)
            s.channel = (uint8_t)hd.channel, s.type = (uint8_t)hd.type, s.parent = (uint8_t)hd.parent, s.n = hd.n;
        s.flags = s.ok ? 0u : (flags ? flags : (uint32_t)SELA_HIP_FLAG_BAD_FRAME);
        subs[(size_t)w * channels + c] = s;
    }
}

__global__ __launch_bounds__(kTailStoreThreads) void k_tailwin_store(const int32_t* __restrict__ dec_ws, const TailSub* __restrict__ subs, const WindowTail* __restrict__ tails,
    uint32_t channels /* <= kTailChannels */, uint32_t window_samples, uint32_t format, void* __restrict__ out, uint32_t* __restrict__ window_flags, uint32_t* __restrict__ status)
{
    __shared__ int32_t tab[kTailChannels][kTailStoreThreads];
    __shared__ TailStoreList list;
    const uint32_t w = blockIdx.x;
    const WindowTail tl = tails[w];
    if (tl.lo >= tl.hi)
        return;
    const uint32_t t = threadIdx.x;
    if (t == 0) {
        const uint32_t flags = tail_store_list(subs + (size_t)w * channels, channels, tl.n, list);
        if (flags) {
            atomicOr(&status[0], flags);
            if (flags & SELA_HIP_FLAG_BAD_FRAME)
                atomicAdd(&status[1], 1u);
            if (atomicOr(&window_flags[w], flags) == 0) // the window's first flag, whichever kernel brings it
                atomicAdd(&status[2], 1u);
        }
    }
    __syncthreads();
    if (!list.ok)
        return;
    const uint32_t n_share = tl.hi - tl.lo;
    const int32_t* const fd = dec_ws + (size_t)w * channels * kTailStride;
    const bool planar = format == SELA_HIP_WINDOW_F32_PLANAR;
    int16_t* const out16 = static_cast<int16_t*>(out) + ((size_t)w * window_samples + tl.lo) * channels; // [window][sample][channel]
    float* const outf = static_cast<float*>(out) + (size_t)w * channels * window_samples + tl.lo;         // [window][channel][sample]
    for (uint32_t base = 0; base < n_share; base += kTailStoreThreads) {
        const uint32_t j = base + t;
        if (j < n_share) {
            tail_store_sample(fd, list, tl.s0 + j /* (below tl.n: window_tail_share) */, tab, t);
            if (planar)
#pragma clang loop vectorize(disable) interleave(disable) // (one dword per store: d_out has a float's alignment and no more)
                for (uint32_t c = 0; c < channels; c++)
                    outf[(size_t)c * window_samples + j] = (float)(int16_t)(uint16_t)tab[c][t] * (1.0f / 32768.0f); // (exact in binary32)
            else if (channels == 1)
                out16[j] = (int16_t)(uint16_t)tab[0][t];
        }
        if (!planar && channels != 1) { // through the table: consecutive threads store consecutive int16
            __syncthreads();
            const uint32_t m = min(kTailStoreThreads, n_share - base) * channels;
            int16_t* const ob = out16 + (size_t)base * channels;
            for (uint32_t e = t; e < m; e += kTailStoreThreads) {
                const uint32_t s = e / channels, c = e - s * channels;
                ob[e] = (int16_t)(uint16_t)tab[c][s];
            }
            __syncthreads();
        }
    }
}

// launch_window_frames' own pieces | the copied descriptors | the tails | the subframe records | the decoded subframes.
struct WindowWholeWs {
    WindowWs frames;
    sela_hip_window* copies;
    WindowTail* tails;
    TailSub* subs;
    int32_t* dec;
};
static WindowWholeWs carve_window_whole(Carve& c, uint32_t n_windows, uint32_t window_samples, uint32_t channels)
{
    WindowWholeWs w;
    w.frames = carve_windows(c, n_windows, window_samples, channels);
    w.copies = c.take<sela_hip_window>(n_windows);
    w.tails = c.take<WindowTail>(n_windows);
    w.subs = c.take<TailSub>((uint64_t)n_windows * channels);
    w.dec = c.take<int32_t>((uint64_t)n_windows * channels * kTailStride);
    return w;
}

// The header's formula: the existing call's bytes, the four pieces and kWindowWholeSlack -- the four roundings that put each of
// them on a multiple of 256, less than 256 bytes each (tests/test_workspace_cpu.py holds the carve of every shape to this size).
constexpr size_t kWindowWholeSlack = 1024;
size_t window_whole_workspace_bytes(uint32_t n_windows, uint32_t window_samples, uint32_t channels, Carve* at)
{
    if (at)
        carve_window_whole(*at, n_windows, window_samples, channels);
    return window_workspace_bytes(n_windows, window_samples, channels)
        + (size_t)n_windows * (sizeof(sela_hip_window) + sizeof(WindowTail) + (size_t)channels * (sizeof(TailSub) + kTailStride * sizeof(int32_t))) + kWindowWholeSlack;
}

hipError_t launch_tailwin_plan(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames_total, const sela_hip_window* d_windows, uint32_t n_windows,
    uint32_t window_samples, sela_hip_window* d_copies, WindowTail* d_tails, hipStream_t stream)
{
    hipLaunchKernelGGL(k_tailwin_plan, dim3((n_windows + kTailPlanThreads - 1) / kTailPlanThreads), dim3(kTailPlanThreads), 0, stream, d_frames, d_frame_offsets, n_frames_total,
        d_windows, n_windows, window_samples, d_copies, d_tails);
    return hipGetLastError();
}

hipError_t launch_tailwin_decode(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t channels, const WindowTail* d_tails, uint32_t n_windows, int32_t* d_dec,
    void* d_subs, hipStream_t stream)
{
    hipLaunchKernelGGL(k_tailwin_decode, dim3(n_windows, channels), dim3(64), 0, stream, d_frames, d_frame_offsets, channels, d_tails, d_dec, static_cast<TailSub*>(d_subs));
    return hipGetLastError();
}

// Plan, the 2048-sample frames, the tails: one serial chain on the caller's stream, capturable.  The arguments have been checked
// (sela_capi.hip), as for launch_window_frames.
hipError_t launch_window_whole(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames_total, uint32_t channels, const sela_hip_window* d_windows,
    uint32_t n_windows, uint32_t window_samples, uint32_t format, void* d_out, uint32_t* d_window_flags, uint32_t* d_status, void* d_workspace, hipStream_t stream,
    int recurrence_form, uint32_t synth_priorities)
{
    if (n_windows == 0)
        return launch_window_frames(d_frames, d_frame_offsets, n_frames_total, channels, d_windows, 0, window_samples, format, d_out, d_window_flags, d_status,
            d_workspace, stream, recurrence_form, synth_priorities);
    if (channels == 0 || channels > kTailChannels)
        return hipErrorInvalidValue;
    Carve carve(d_workspace);
    const WindowWholeWs w = carve_window_whole(carve, n_windows, window_samples, channels);
    sela_hip_window* const d_copies = w.copies;
    WindowTail* const d_tails = w.tails;
    TailSub* const d_subs = w.subs;
    int32_t* const d_dec = w.dec;
    // the flag words of a call that passes none: where launch_window_frames keeps them, behind its residues (sela_window.hip)
    uint32_t* const flags = d_window_flags ? d_window_flags : w.frames.flag_words;
    hipLaunchKernelGGL(k_tailwin_plan, dim3((n_windows + kTailPlanThreads - 1) / kTailPlanThreads), dim3(kTailPlanThreads), 0, stream, d_frames, d_frame_offsets, n_frames_total,
        d_windows, n_windows, window_samples, d_copies, d_tails);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess)
        return err;
    err = launch_window_frames(d_frames, d_frame_offsets, n_frames_total, channels, d_copies, n_windows, window_samples, format, d_out, flags, d_status, d_workspace, stream,
        recurrence_form, synth_priorities);
    if (err != hipSuccess)
        return err;
    hipLaunchKernelGGL(k_tailwin_decode, dim3(n_windows, channels), dim3(64), 0, stream, d_frames, d_frame_offsets, channels, d_tails, d_dec, d_subs);
    hipLaunchKernelGGL(k_tailwin_store, dim3(n_windows), dim3(kTailStoreThreads), 0, stream, d_dec, d_subs, d_tails, channels, window_samples, format, d_out, flags, d_status);
    return hipGetLastError();
}

// ---- a full decode of a whole-track stream: sela_hip_decode_whole_device ------------------------------------------
// The 2048-sample decoder on frames 0 .. n - 2 and, beside it on a second stream, the long last frame: k_tailwin_decode as it is,
// on one "window" whose share is the whole frame, and a store of all its samples behind the others'.
//
//   k_whole_plan    one thread.  plan_decode_whole (sela_decode_whole_plan.h) on the device's bytes and count: the fast decoder's
//                   frame count, the WindowTail of L (or an empty one), *d_n_samples and all four status words.
//   k_whole_store   kWholeStoreBlocks workgroups, each with 256 samples of the frame (k_tailwin_store's table is 256 columns: a
//                   frame of 4095 samples in one workgroup would be sixteen rounds behind one another).  Every workgroup makes
//                   the list for itself; the first one reports the flags.  A declined frame stores nothing.
constexpr uint32_t kWholeStoreBlocks = kTailStride / kTailStoreThreads;

__global__ __launch_bounds__(64) void k_whole_plan(const uint8_t* __restrict__ frames, const uint64_t* __restrict__ frame_offsets, uint32_t n_frames,
    const uint32_t* __restrict__ n_found /* or null: n_frames is the count */, uint64_t pcm_capacity, WindowTail* __restrict__ tail, uint32_t* __restrict__ fast_frames,
    uint64_t* __restrict__ n_samples, uint32_t* __restrict__ status)
{
    if (threadIdx.x != 0 || blockIdx.x != 0)
        return;
    const uint32_t n = n_found ? min(*n_found, n_frames) : n_frames;
    const DecodeWholePlan p = plan_decode_whole(frames, frame_offsets, n, pcm_capacity);
    *tail = p.tail;
    *fast_frames = p.fast_frames;
    *n_samples = p.samples;
    status[0] = p.flags, status[1] = 0, status[2] = 0, status[3] = p.route;
}

__global__ __launch_bounds__(kTailStoreThreads) void k_whole_store(const int32_t* __restrict__ dec_ws, const TailSub* __restrict__ subs, const WindowTail* __restrict__ tail,
    uint32_t channels /* <= kTailChannels */, int16_t* __restrict__ pcm_out, uint32_t* __restrict__ status)
{
    __shared__ int32_t tab[kTailChannels][kTailStoreThreads];
    __shared__ TailStoreList list;
    const WindowTail tl = *tail;
    const uint32_t base = blockIdx.x * kTailStoreThreads;
    if (tl.lo >= tl.hi || base >= tl.n) // no long last frame, or none of its samples here (the first workgroup always has some)
        return;
    const uint32_t t = threadIdx.x;
    if (t == 0) {
        const uint32_t flags = tail_store_list(subs, channels, tl.n, list);
        if (flags && blockIdx.x == 0) { // status[1] counts L whatever it is declined for: none of it is decoded
            atomicOr(&status[0], flags);
            atomicAdd(&status[1], 1u);
        }
    }
    __syncthreads();
    if (!list.ok)
        return;
    const uint32_t here = min(kTailStoreThreads, tl.n - base);
    int16_t* const ob = pcm_out + ((size_t)SELA_HIP_SAMPLES_PER_FRAME * tl.frame + base) * channels; // frame L starts at sample 2048 L
    if (t < here)
        tail_store_sample(dec_ws, list, base + t, tab, t);
    __syncthreads();
    for (uint32_t e = t; e < here * channels; e += kTailStoreThreads) { // consecutive threads store consecutive int16
        const uint32_t s = e / channels, c = e - s * channels;
        ob[e] = (int16_t)(uint16_t)tab[c][s];
    }
}

// The fast decoder's workspace | the WindowTail of L | the fast decoder's frame count | the subframe records | the decoded subframes.
DecodeWholeWs carve_decode_whole(Carve& c, uint32_t max_frames, uint32_t channels)
{
    DecodeWholeWs w;
    Carve fast = c.sub(decode_workspace_bytes(max_frames, channels));
    w.fast_workspace = fast.base();
    if (c.listing()) // (the decoder's own piece, where it lies)
        decode_workspace_bytes(max_frames, channels, &fast);
    w.tail = c.take<WindowTail>(1);
    w.fast_frames = c.take<uint32_t>(1);
    w.subs = c.take<TailSub>(channels);
    w.dec = c.take<int32_t>((uint64_t)channels * kTailStride);
    return w;
}

// The header's formula: the fast decoder's bytes, a record and 4096 samples per channel, and kDecodeWholeSlack -- the four roundings
// that put each piece on a multiple of 256 with the two small pieces themselves (tests/test_decode_whole_cpu.py holds the carve
// of every shape to this size).
constexpr size_t kDecodeWholeSlack = 1024;
size_t decode_whole_workspace_bytes(uint32_t max_frames, uint32_t channels, Carve* at)
{
    if (at)
        carve_decode_whole(*at, max_frames, channels);
    return decode_workspace_bytes(max_frames, channels) + (size_t)channels * (sizeof(TailSub) + kTailStride * sizeof(int32_t)) + kDecodeWholeSlack;
}

hipError_t launch_decode_whole_plan(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t max_frames, const uint32_t* d_n_found, uint64_t pcm_capacity,
    const DecodeWholeWs& w, uint64_t* d_n_samples, uint32_t* d_status, hipStream_t stream)
{
    hipLaunchKernelGGL(k_whole_plan, dim3(1), dim3(64), 0, stream, d_frames, d_frame_offsets, max_frames, d_n_found, pcm_capacity, w.tail, w.fast_frames, d_n_samples,
        d_status);
    return hipGetLastError();
}

// (channels in 1 .. kTailChannels: the caller has checked)
hipError_t launch_decode_whole_tail(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t channels, const DecodeWholeWs& w, int16_t* d_pcm_out,
    uint32_t* d_status, hipStream_t stream)
{
    hipLaunchKernelGGL(k_tailwin_decode, dim3(1, channels), dim3(64), 0, stream, d_frames, d_frame_offsets, channels, w.tail, w.dec, static_cast<TailSub*>(w.subs));
    hipLaunchKernelGGL(k_whole_store, dim3(kWholeStoreBlocks), dim3(kTailStoreThreads), 0, stream, w.dec, static_cast<const TailSub*>(w.subs), w.tail, channels, d_pcm_out,
        d_status);
    return hipGetLastError();
}

} // namespace sela
