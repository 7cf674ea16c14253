// sela_window32.hip -- sample windows of 24- and 32-bit streams (gfx950): sela_hip_decode_windows_i32_device.
//
// k_window_frames (sela_window.hip) cuts its windows from the 2048-sample decoder's second pass, whose samples are 16 bits wide.
// Samples of up to 32 bits are the any-length decoder's (sela_decode32.hip), one wave per subframe into the workspace, so a window
// call for them is that decoder on the frames the windows touch and a store of the shares, as the long last frame of a whole-track
// stream is decoded for the int16 windows (sela_window_whole.hip).  One serial chain on the caller's stream:
//
//   k_window_clear      status and the windows' flag words (a kernel, not a memset node: sela_window.hip).
//   k_window32_decode   grid (window, j, subframe position), one wave each: the subframe of frame first_frame + start / 2048 + j at
//                       that position, to 32-bit samples in the workspace with a record of what its header said and of the flags
//                       met -- k_tailwin_decode's work, with k_decode_subframes32's choice of path: a subframe whose words fit the
//                       parser's plan (cw + 2 + rw <= kStreamCap) is parsed in one piece, positions in LDS and residues decoded
//                       just in time; a longer one goes by segments, the residues parked where the samples will lie.  A wave
//                       whose share of the window is empty, or whose frame lies outside the stream, returns at once.
//   k_window32_store    grid (window, j), a workgroup of 256: thread 0 turns the frame's records into the list of writes
//                       (tail_store_list, sela_tail_store.h) and raises the frame's flags; every thread then forms its samples
//                       of the share, 256 samples of every channel per round, in an LDS table in interleaved order, and the
//                       round goes out in the call's format.  A share whose frame is not taken -- declined by the decode, refused
//                       by the list's rules -- or lies behind the stream's end goes out as zeros by the same stores: every byte
//                       of d_out is written exactly once, by the workgroup that owns it, and there is no pre-clear.
//
// The formats: planar ones (int32, float) store one dword per lane and channel, consecutive lanes to consecutive samples;
// interleaved int32 reads the table in its own order, consecutive lanes to consecutive dwords; packed 3-byte samples form aligned
// dwords from two neighbouring table values each (sela_pcm24_edges.h) and store single bytes only at the two ragged ends of the
// share.
//
// Two kernels and not one, for sela_window_whole.hip's reasons: the decode is a wave of the decoder's register budget (65 / 69
// VGPRs, 12 bytes of scratch a lane, 5840 bytes of LDS), and up to eight of them behind one barrier would hold a workgroup for its
// longest subframe; the store wants 256 lanes (61 VGPRs, 8376 bytes of LDS, no scratch) and none of the decoder's state.
//
// Scope: frames of 2048 samples, 1 .. 8 channels, samples of up to 32 bits.
#include <hip/hip_runtime.h>

#include "sela_host.h"
#include "sela_pcm24_edges.h"
#include "sela_window_tail.h"

#include "sela_synth.h"

namespace sela {

#include "sela_decode_core.inc"

#include "sela_segments.inc"

#include "sela_tail_store.h"

static_assert(sizeof(sela_hip_window) == 16, "a descriptor is read as two 64-bit words");

// Workgroup (w, j)'s share [lo, hi) of window w: the samples that fall into the window's j-th frame; sample lo of the window is
// sample s0 of that frame, table frame `frame` when in_stream (k_window_frames' arithmetic: nothing is added to start).
struct Win32Share {
    uint32_t lo, hi, s0, frame;
    bool in_stream;
};
__device__ inline Win32Share window32_share(const sela_hip_window* __restrict__ windows, uint32_t w, uint32_t j, uint32_t n_frames_total, uint32_t window_samples)
{
    const sela_hip_window d = windows[w];
    const uint32_t in_stream = window_stream_frames(d, n_frames_total); // the stream, cut at the table's end
    const uint64_t q = d.start / (uint32_t)kBlock;
    const uint32_t r = (uint32_t)(d.start % (uint32_t)kBlock);
    Win32Share s;
    s.lo = j == 0 ? 0u : j * (uint32_t)kBlock - r; // (window_samples <= 2^24: nothing wraps)
    s.hi = min(window_samples, (j + 1) * (uint32_t)kBlock - r);
    s.s0 = s.lo + r - j * (uint32_t)kBlock;
    s.in_stream = q < in_stream && j < in_stream - (uint32_t)q; // (q is compared first: start + i is never formed)
    s.frame = s.in_stream ? d.first_frame + (uint32_t)q + j : 0u;
    return s;
}

template <bool kVecShift>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(7, 8))) void k_window32_decode(const uint8_t* __restrict__ frames,
    const uint64_t* __restrict__ frame_offsets, uint32_t n_frames_total, uint32_t channels, const sela_hip_window* __restrict__ windows, uint32_t window_samples,
    int32_t* __restrict__ dec_ws /* [window][j][position][kBlock] */, TailSub* __restrict__ subs /* [window][j][position] */,
    uint32_t standard_path /* 0: every subframe by segments (tests) */)
{
    __shared__ __attribute__((aligned(16))) DecSubframeLds sl;
    __shared__ DecWaveScratch scratch;
    const uint32_t w = blockIdx.x, j = blockIdx.y, c = blockIdx.z;
    const Win32Share sh = window32_share(windows, w, j, n_frames_total, window_samples);
    if (sh.lo >= sh.hi || !sh.in_stream)
        return;
    const int lane = threadIdx.x;
    const size_t slot = ((size_t)w * gridDim.y + j) * channels + c;
    const uint64_t at = frame_offsets[sh.frame], end = frame_offsets[sh.frame + 1];
    const uint8_t* const fb = frames + at;
    const uint64_t fbytes = end >= at ? end - at : 0;
    const SubHeader hd = walk_headers(fb, (at & 3) == 0 ? fbytes : 0 /* a frame at a place that is not word-aligned: not walked */, c);
    // (k_decode_subframes32's own test, the length being the one these windows are cut from)
    const bool mine = hd.ok && sela_subframe_decodable(&hd) && hd.n == (uint32_t)kBlock && hd.n > hd.order;
    uint32_t flags = 0;
    if (mine) {
        const uint32_t nw = hd.cw + 2 + hd.rw;
        const uint32_t* const gw = reinterpret_cast<const uint32_t*>(fb + hd.p + 4); // the subframe's aligned words
        SynthTables* const tables = &scratch.t;
        const uint32_t order = hd.order;
        int32_t* const samples = dec_ws + slot * kBlock;
        const bool standard = standard_path && nw <= (uint32_t)kStreamCap; // in one piece: the parser's positions are one 16-bit word per codeword
        if (standard) {
            for (uint32_t i = lane; i < nw + kStreamMargin; i += kWave) // the start bitmap
                sl.marks[i] = 0;
            wave_sync();
            ParseProfile pp;
            const StreamWords sw = { gw, nw };
            flags |= parse_subframe<false>(sw, sl.marks, sl.pos, reinterpret_cast<uint16_t*>(tables), coef_values(&scratch), hd.cw, hd.rw, hd.ck, hd.rk, order, lane, pp, hd.n);
        } else {
            if (order)
                flags |= parse_stream_segments(gw, nw, 24, 24 + 32 * hd.cw, hd.ck, order, (256 * hd.cw + order - 1) / order + 1, &sl, reinterpret_cast<uint16_t*>(tables),
                    coef_values(&scratch), lane);
            flags |= parse_stream_segments(gw, nw, 32 * (hd.cw + 2), 32 * nw, hd.rk, hd.n, (256 * hd.rw + hd.n - 1) / hd.n + 1, &sl, reinterpret_cast<uint16_t*>(tables), samples,
                lane);
            // the lanes read each other's residues back: the stores have left the CU, nothing older is served from its vector cache
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        }
        const int32_t q_lo = (uint32_t)lane < order ? coef_values(&scratch)[lane] : 0, q_hi = (uint32_t)lane + 64 < order ? coef_values(&scratch)[lane + 64] : 0;
        wave_sync();
        const bool fits24 = predictor_table(order, q_lo, q_hi, tables, lane, flags);
        SynthOut<true> out32;
        out32.samples = samples;
        out32.n = hd.n;
        flags = wave_or(flags);
        if (flags == 0) // (a stream in trouble is declined: its share is zeros)
            synthesize_by_order<kVecShift, true>(order, gw, nw, hd.rk, sl.pos, standard ? nullptr : samples, tables->tab, fits24, lane, out32);
    }
    flags = wave_or(flags);
    if (lane == 0) {
        TailSub s = {};
        s.ok = mine && flags == 0 ? 1 : 0;
        if (s.ok)
            s.channel = (uint8_t)hd.channel, s.type = (uint8_t)hd.type, s.parent = (uint8_t)hd.parent, s.n = hd.n;
        s.flags = s.ok ? 0u : (flags ? flags : (uint32_t)SELA_HIP_FLAG_BAD_FRAME);
        subs[slot] = s;
    }
}

constexpr uint32_t kWin32Threads = kTailStoreThreads;
constexpr uint32_t kWin32RoundValues = kWin32Threads * kTailChannels; // values of a round at most: 256 samples of eight channels

__global__ __launch_bounds__(kWin32Threads) void k_window32_store(const int32_t* __restrict__ dec_ws, const TailSub* __restrict__ subs, uint32_t n_frames_total,
    uint32_t channels /* <= kTailChannels */, const sela_hip_window* __restrict__ windows, uint32_t window_samples, uint32_t format, float scale /* F32_PLANAR: 2^-(sample_bits-1) */,
    void* __restrict__ out, uint32_t* __restrict__ window_flags, uint32_t* __restrict__ status)
{
    // the round's values in interleaved order behind the lead (sela_pcm24_edges.h): slot 1 + t * channels + c is channel c of the
    // round's sample t
    __shared__ int32_t vals[1 + kWin32RoundValues];
    __shared__ TailStoreList list;
    __shared__ int32_t carry;   // the last value of a round, the next round's lead
    __shared__ uint32_t wide;   // PCM24: values of the share outside [-2^23, 2^23)
    const uint32_t w = blockIdx.x, j = blockIdx.y;
    const Win32Share sh = window32_share(windows, w, j, n_frames_total, window_samples);
    if (sh.lo >= sh.hi)
        return;
    const uint32_t t = threadIdx.x;
    const size_t slot = ((size_t)w * gridDim.y + j) * channels;
    if (t == 0) {
        wide = 0;
        list.ok = 0, list.ops = 0;
        if (sh.in_stream) { // (behind the stream's end: zeros, and no flag)
            const uint32_t flags = tail_store_list(subs + slot, channels, (uint32_t)kBlock, list);
            if (flags) {
                atomicOr(&status[0], flags);
                if (flags & SELA_HIP_FLAG_BAD_FRAME)
                    atomicAdd(&status[1], 1u);
                if (atomicOr(&window_flags[w], flags) == 0) // the window's first flag, whichever of its frames brings it
                    atomicAdd(&status[2], 1u);
            }
        }
    }
    __syncthreads();
    const bool taken = list.ok != 0;
    const uint32_t n_share = sh.hi - sh.lo;
    const int32_t* const fd = dec_ws + slot * kBlock;
    const bool pcm24 = format == SELA_HIP_WINDOW_PCM24_INTERLEAVED;
    uint32_t n_wide = 0;
    for (uint32_t base = 0; base < n_share; base += kWin32Threads) {
        const uint32_t s = base + t;
        int32_t* const mine = vals + 1 + t * channels;
        if (pcm24 && t == 0 && base != 0)
            vals[0] = carry;
        if (s < n_share) {
            if (taken) {
                const uint32_t i = sh.s0 + s; // (below 2048: the share is the frame's)
                for (uint32_t k = 0; k < list.ops; k++) { // tail_store_sample's combine, on subframes kBlock apart and this table
                    if (i >= list.n[k])
                        continue;
                    int32_t v = fd[(size_t)list.sub[k] * kBlock + i];
                    const uint32_t p = list.parent[k];
                    if (p != kTailNoParent)
                        v = (int32_t)((uint32_t)mine[p] - (uint32_t)v);
                    mine[list.dst[k]] = v;
                }
                if (pcm24)
                    for (uint32_t c = 0; c < channels; c++)
                        n_wide += mine[c] < -(1 << 23) || mine[c] >= (1 << 23) ? 1u : 0u;
            } else {
                for (uint32_t c = 0; c < channels; c++)
                    mine[c] = 0;
            }
        }
        const uint32_t here = min(kWin32Threads, n_share - base), m = here * channels;
        if (format == SELA_HIP_WINDOW_I32_PLANAR || format == SELA_HIP_WINDOW_F32_PLANAR) { // [window][channel][sample]: a lane's own values
            if (s < n_share) {
                uint32_t* const o = static_cast<uint32_t*>(out) + (size_t)w * channels * window_samples + sh.lo + s;
#pragma clang loop vectorize(disable) interleave(disable) // (one dword per store: d_out has a dword's alignment and no more)
                for (uint32_t c = 0; c < channels; c++)
                    o[(size_t)c * window_samples] = format == SELA_HIP_WINDOW_I32_PLANAR ? (uint32_t)mine[c] : __float_as_uint((float)mine[c] * scale);
            }
        } else {
            __syncthreads(); // the table is whole
            const uint64_t v0 = ((uint64_t)w * window_samples + sh.lo + base) * channels; // the round's first value in d_out
            if (!pcm24) { // [window][sample][channel] int32: consecutive threads store consecutive dwords
                uint32_t* const o = static_cast<uint32_t*>(out) + v0;
                for (uint32_t e = t; e < m; e += kWin32Threads)
                    o[e] = (uint32_t)vals[1 + e];
            } else {
                uint8_t* const o = static_cast<uint8_t*>(out);
                const uint64_t b0 = 3 * v0, lead_at = b0 - 3; // (from_lead = at - lead_at, formed modulo 2^64 where b0 < 3)
                const Pcm24Span sp = pcm24_span(b0, b0 + 3ull * m, base == 0, base + kWin32Threads >= n_share);
                if (t < sp.head)
                    o[sp.head_at + t] = pcm24_byte(vals, (uint32_t)(sp.head_at + t - lead_at));
                for (uint32_t e = t; e < (uint32_t)sp.dwords; e += kWin32Threads)
                    *reinterpret_cast<uint32_t*>(o + sp.mid_at + 4ull * e) = pcm24_dword(vals, (uint32_t)(sp.mid_at + 4ull * e - lead_at));
                if (t < sp.tail)
                    o[sp.tail_at + t] = pcm24_byte(vals, (uint32_t)(sp.tail_at + t - lead_at));
                if (t == 0)
                    carry = vals[m];
            }
            __syncthreads(); // the next round overwrites the table
        }
    }
    if (pcm24) {
        if (n_wide)
            atomicAdd(&wide, n_wide);
        __syncthreads();
        if (t == 0 && wide)
            atomicAdd(&status[3], wide);
    }
}

// The subframe records | the decoded subframes, 2048 samples each | a flag word per window for a call that passes no d_window_flags
// (Window32Ws: sela_host.h).
Window32Ws carve_window32(Carve& c, uint32_t n_windows, uint32_t window_samples, uint32_t channels)
{
    const uint64_t slots = (uint64_t)n_windows * window_cover(window_samples) * channels;
    Window32Ws w;
    w.subs = c.take<TailSub>(slots);
    w.dec = c.take<int32_t>(slots * kBlock);
    w.flag_words = c.take<uint32_t>(n_windows);
    return w;
}

// The header's formula: the three pieces and kWindow32Slack -- the roundings that put the records' end and the flag words' end on
// a multiple of 256 (the samples are whole blocks of 8 KiB) and the base's alignment, less than 256 bytes each
// (tests/test_decode_windows_i32_cpu.py holds the carve of every shape to this size).
constexpr size_t kWindow32Slack = 1024;
size_t window32_workspace_bytes(uint32_t n_windows, uint32_t window_samples, uint32_t channels, Carve* at)
{
    if (at)
        carve_window32(*at, n_windows, window_samples, channels);
    return (size_t)n_windows * window_cover(window_samples) * channels * (sizeof(TailSub) + kBlock * sizeof(int32_t)) + (size_t)n_windows * sizeof(uint32_t) + kWindow32Slack;
}

// Clear, decode, store: one serial chain on the caller's stream, capturable.  The arguments have been checked (sela_capi.hip):
// 1 .. 8 channels, n_windows * cover * channels below 2^31, n_windows below 2^24 (256 n_windows work-items in the store's grid x).
hipError_t launch_window32(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames_total, uint32_t channels, const sela_hip_window* d_windows,
    uint32_t n_windows, uint32_t window_samples, uint32_t format, uint32_t sample_bits, void* d_out, uint32_t* d_window_flags, uint32_t* d_status, void* d_workspace,
    bool standard_path, hipStream_t stream)
{
    if (n_windows == 0)
        return launch_window_clear(d_status, nullptr, 0, stream);
    if (channels == 0 || channels > kTailChannels)
        return hipErrorInvalidValue;
    const uint32_t cover = window_cover(window_samples);
    Carve carve(d_workspace);
    const Window32Ws ws = carve_window32(carve, n_windows, window_samples, channels);
    uint32_t* const flags = d_window_flags ? d_window_flags : ws.flag_words;
    hipError_t err = launch_window_clear(d_status, flags, n_windows, stream);
    if (err != hipSuccess)
        return err;
    const dim3 grid(n_windows, cover, channels);
    if ((uint64_t)n_windows * cover * channels <= kLonelyWaves) // (the recurrence's form for waves that have their SIMD nearly to themselves: launch_decode_subframes32)
        hipLaunchKernelGGL(k_window32_decode<true>, grid, dim3(64), 0, stream, d_frames, d_frame_offsets, n_frames_total, channels, d_windows, window_samples, ws.dec, ws.subs,
            standard_path ? 1u : 0u);
    else
        hipLaunchKernelGGL(k_window32_decode<false>, grid, dim3(64), 0, stream, d_frames, d_frame_offsets, n_frames_total, channels, d_windows, window_samples, ws.dec, ws.subs,
            standard_path ? 1u : 0u);
    err = hipGetLastError();
    if (err != hipSuccess)
        return err;
    const float scale = format == SELA_HIP_WINDOW_F32_PLANAR ? __builtin_ldexpf(1.0f, 1 - (int)sample_bits) : 0.0f;
    hipLaunchKernelGGL(k_window32_store, dim3(n_windows, cover), dim3(kWin32Threads), 0, stream, ws.dec, ws.subs, n_frames_total, channels, d_windows, window_samples, format, scale,
        d_out, flags, d_status);
    return hipGetLastError();
}

} // namespace sela
