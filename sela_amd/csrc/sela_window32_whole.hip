// sela_window32_whole.hip -- sample windows of 24- and 32-bit WHOLE-TRACK streams (gfx950):
// sela_hip_decode_windows_i32_whole_device.
//
// A whole-track stream (5.19) is 2048-sample frames and ONE last frame L of 1 .. 4095 samples.  The call is to the 32-bit windows
// (sela_window32.hip, 5.23) what launch_window_whole (sela_window_whole.hip, 5.20) is to the int16 ones -- one serial chain on the
// caller's stream:
//
//   k_tailwin_plan      as it is: the descriptor copies with n_frames - 1 and the WindowTails.
//   launch_window32     on the copies: status and flags cleared, every byte of d_out written -- the share of L as the zeros of a
//                       stream that has ended there, without a flag.
//   k_tailwin_decode    as it is: the subframes of L as 32-bit samples at stride kTailStride, and their records.
//   k_tail32_store      a workgroup of 256 per window.  Thread 0 turns the records into the list of writes (tail_store_list) and
//                       raises the frame's flags as k_tailwin_store does; the share [lo, hi) of L then goes out as
//                       k_window32_store's shares do, in rounds of 256 samples through an LDS table in interleaved order: planar
//                       formats one dword per lane and channel to consecutive samples, interleaved int32 consecutive dwords,
//                       packed 3-byte samples as aligned dwords formed from neighbouring table values (sela_pcm24_edges.h) with
//                       single bytes only at the share's two ragged ends, the lead value carried from round to round.  It writes
//                       every byte of its share and no byte outside it; a declined frame stores nothing (the zeros stay).
//
// So the bytes of a taken share are written twice by the call -- zeros by launch_window32's store, the samples by this one, two
// launches in series on one stream -- where the plain call writes every byte exactly once.
//
// The store is a kernel of its own and not a second mode of k_window32_store: that kernel's share is one of `cover` slots of 2048
// samples read at stride 2048 and found by window32_share; this one's is the WindowTail's, up to 4095 samples at stride 4096.  The
// table's writes are strided by `channels` dwords (8-way on the 32 write banks at eight channels, as in k_window32_store): a share
// is sixteen rounds at most, behind global loads.
#include <hip/hip_runtime.h>

#include "sela_host.h"
#include "sela_pcm24_edges.h"
#include "sela_window_tail.h"

namespace sela {

#include "sela_tail_store.h"

constexpr uint32_t kTail32Threads = kTailStoreThreads;
constexpr uint32_t kTail32RoundValues = kTail32Threads * kTailChannels; // values of a round at most: 256 samples of eight channels

__global__ __launch_bounds__(kTail32Threads) void k_tail32_store(const int32_t* __restrict__ dec_ws /* [window][position][kTailStride] */, const TailSub* __restrict__ subs,
    const WindowTail* __restrict__ tails, uint32_t channels /* <= kTailChannels */, uint32_t window_samples, uint32_t format, float scale /* F32_PLANAR: 2^-(sample_bits-1) */,
    void* __restrict__ out, uint32_t* __restrict__ window_flags, uint32_t* __restrict__ status)
{
    // the round's values in interleaved order behind the lead (sela_pcm24_edges.h): slot 1 + t * channels + c is channel c of the
    // round's sample t
    __shared__ int32_t vals[1 + kTail32RoundValues];
    __shared__ TailStoreList list;
    __shared__ int32_t carry; // the last value of a round, the next round's lead
    __shared__ uint32_t wide; // PCM24: values of the share outside [-2^23, 2^23)
    const uint32_t w = blockIdx.x;
    const WindowTail tl = tails[w];
    if (tl.lo >= tl.hi)
        return;
    const uint32_t t = threadIdx.x;
    if (t == 0) {
        wide = 0;
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
    if (!list.ok) // declined: the zeros of launch_window32 stay
        return;
    const uint32_t n_share = tl.hi - tl.lo;
    const int32_t* const fd = dec_ws + (size_t)w * channels * kTailStride;
    const bool pcm24 = format == SELA_HIP_WINDOW_PCM24_INTERLEAVED;
    uint32_t n_wide = 0;
    for (uint32_t base = 0; base < n_share; base += kTail32Threads) {
        const uint32_t s = base + t;
        int32_t* const mine = vals + 1 + t * channels;
        if (pcm24 && t == 0 && base != 0)
            vals[0] = carry;
        if (s < n_share) {
            const uint32_t i = tl.s0 + s; // (below tl.n: window_tail_share)
            for (uint32_t k = 0; k < list.ops; k++) { // tail_store_sample's combine, on this table
                if (i >= list.n[k])
                    continue;
                int32_t v = fd[(size_t)list.sub[k] * kTailStride + i];
                const uint32_t p = list.parent[k];
                if (p != kTailNoParent)
                    v = (int32_t)((uint32_t)mine[p] - (uint32_t)v);
                mine[list.dst[k]] = v;
            }
            if (pcm24)
                for (uint32_t c = 0; c < channels; c++)
                    n_wide += mine[c] < -(1 << 23) || mine[c] >= (1 << 23) ? 1u : 0u;
        }
        const uint32_t here = min(kTail32Threads, n_share - base), m = here * channels;
        if (format == SELA_HIP_WINDOW_I32_PLANAR || format == SELA_HIP_WINDOW_F32_PLANAR) { // [window][channel][sample]: a lane's own values
            if (s < n_share) {
                uint32_t* const o = static_cast<uint32_t*>(out) + (size_t)w * channels * window_samples + tl.lo + s;
// (one dword per store: d_out has a dword's alignment and no more; not unrolled: eight channels' uniform addresses spill SGPRs)
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
                for (uint32_t c = 0; c < channels; c++)
                    o[(size_t)c * window_samples] = format == SELA_HIP_WINDOW_I32_PLANAR ? (uint32_t)mine[c] : __float_as_uint((float)mine[c] * scale);
            }
        } else {
            __syncthreads(); // the table is whole
            const uint64_t v0 = ((uint64_t)w * window_samples + tl.lo + base) * channels; // the round's first value in d_out
            if (!pcm24) { // [window][sample][channel] int32: consecutive threads store consecutive dwords
                uint32_t* const o = static_cast<uint32_t*>(out) + v0;
                for (uint32_t e = t; e < m; e += kTail32Threads)
                    o[e] = (uint32_t)vals[1 + e];
            } else {
                uint8_t* const o = static_cast<uint8_t*>(out);
                const uint64_t b0 = 3 * v0, lead_at = b0 - 3; // (from_lead = at - lead_at, formed modulo 2^64 where b0 < 3)
                const Pcm24Span sp = pcm24_span(b0, b0 + 3ull * m, base == 0, base + kTail32Threads >= n_share);
                if (t < sp.head)
                    o[sp.head_at + t] = pcm24_byte(vals, (uint32_t)(sp.head_at + t - lead_at));
                for (uint32_t e = t; e < (uint32_t)sp.dwords; e += kTail32Threads)
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

// launch_window32's own pieces | the copied descriptors | the tails | the subframe records of L | its decoded subframes.
struct Window32WholeWs {
    Window32Ws frames;
    sela_hip_window* copies;
    WindowTail* tails;
    void* subs;
    int32_t* dec;
};
static Window32WholeWs carve_window32_whole(Carve& c, uint32_t n_windows, uint32_t window_samples, uint32_t channels)
{
    Window32WholeWs w;
    w.frames = carve_window32(c, n_windows, window_samples, channels);
    w.copies = c.take<sela_hip_window>(n_windows);
    w.tails = c.take<WindowTail>(n_windows);
    w.subs = c.take<TailSub>((uint64_t)n_windows * channels);
    w.dec = c.take<int32_t>((uint64_t)n_windows * channels * kTailStride);
    return w;
}

// The header's formula: the plain call's bytes, the four pieces and kWindow32WholeSlack -- the four roundings that put each of them
// on a multiple of 256, less than 256 bytes each (tests/test_whole_pcm_cpu.py holds the carve of every shape to this size).
constexpr size_t kWindow32WholeSlack = 1024;
size_t window32_whole_workspace_bytes(uint32_t n_windows, uint32_t window_samples, uint32_t channels, Carve* at)
{
    if (at)
        carve_window32_whole(*at, n_windows, window_samples, channels);
    return window32_workspace_bytes(n_windows, window_samples, channels)
        + (size_t)n_windows * (sizeof(sela_hip_window) + sizeof(WindowTail) + (size_t)channels * (sizeof(TailSub) + kTailStride * sizeof(int32_t))) + kWindow32WholeSlack;
}

// Plan, the 2048-sample frames, the tails: one serial chain on the caller's stream, capturable.  The arguments have been checked
// (sela_capi.hip), as for launch_window32.
hipError_t launch_window32_whole(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames_total, uint32_t channels, const sela_hip_window* d_windows,
    uint32_t n_windows, uint32_t window_samples, uint32_t format, uint32_t sample_bits, void* d_out, uint32_t* d_window_flags, uint32_t* d_status, void* d_workspace,
    bool standard_path, hipStream_t stream)
{
    if (n_windows == 0)
        return launch_window32(d_frames, d_frame_offsets, n_frames_total, channels, d_windows, 0, window_samples, format, sample_bits, d_out, d_window_flags, d_status,
            d_workspace, standard_path, stream);
    if (channels == 0 || channels > kTailChannels)
        return hipErrorInvalidValue;
    Carve carve(d_workspace);
    const Window32WholeWs w = carve_window32_whole(carve, n_windows, window_samples, channels);
    // the flag words of a call that passes none: where launch_window32 keeps them
    uint32_t* const flags = d_window_flags ? d_window_flags : w.frames.flag_words;
    hipError_t err = launch_tailwin_plan(d_frames, d_frame_offsets, n_frames_total, d_windows, n_windows, window_samples, w.copies, w.tails, stream);
    if (err != hipSuccess)
        return err;
    err = launch_window32(d_frames, d_frame_offsets, n_frames_total, channels, w.copies, n_windows, window_samples, format, sample_bits, d_out, flags, d_status, d_workspace,
        standard_path, stream);
    if (err != hipSuccess)
        return err;
    err = launch_tailwin_decode(d_frames, d_frame_offsets, channels, w.tails, n_windows, w.dec, w.subs, stream);
    if (err != hipSuccess)
        return err;
    const float scale = format == SELA_HIP_WINDOW_F32_PLANAR ? __builtin_ldexpf(1.0f, 1 - (int)sample_bits) : 0.0f;
    hipLaunchKernelGGL(k_tail32_store, dim3(n_windows), dim3(kTail32Threads), 0, stream, w.dec, static_cast<const TailSub*>(w.subs), w.tails, channels, window_samples, format, scale,
        d_out, flags, d_status);
    return hipGetLastError();
}

} // namespace sela
