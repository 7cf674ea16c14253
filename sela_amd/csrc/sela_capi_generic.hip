// sela_capi_generic.hip -- the host side of the any-length / 32-bit route (kernels: sela_generic.hip; declarations:
// include/sela_hip.h "Blocks of any length" and "the frame classes' own value types").
//
// Plain synchronous calls on the calling thread's current device and a stream of the calling thread's own (GenericContext below:
// threads that code a frame at a time through the frame classes run side by side on the device instead of taking turns on
// the default stream): copy in, kernels, copy out, in chunks of frames that keep the device scratch bounded, ONE wait for the
// device per chunk (round 6: the encoder sizes its Rice words and frame bytes by an estimate instead of waiting for its plan,
// and what the host reads first lands in page-locked memory of the context).  The scratch is one grow-only device allocation
// per thread (a frame at a time through frame::FrameEncoder must not pay a hipMalloc / hipFree pair per call);
// sela_hip_thread_release() / sela_hip_shutdown() and the thread's end give it back.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "sela_crc32.h"
#include "sela_host.h"
#include "sela_lease.h"
#include "sela_pcm.h"
#include "sela_window_plan.h"

namespace {

using sela::Carve;
using sela::GenericMeta;
using sela::GenericSubInfo;

struct Arena { // one device allocation, handed out in aligned pieces for the length of a call
    uint8_t* base = nullptr;
    size_t cap = 0;
    Carve carve; // the pieces of the call in hand (sela_workspace.h), from `base`: hipMalloc's alignment is the carve's
    bool fits() const { return carve.end() <= cap; } // (asked after the pieces are taken: the callers' size estimates are checked, not trusted)
    void release()
    {
        if (base)
            (void)hipFree(base);
        base = nullptr, cap = 0, carve = Carve();
    }
    hipError_t reserve(size_t bytes)
    {
        carve = Carve(base);
        if (base && bytes <= cap)
            return hipSuccess;
        release();
        // (grow-only, and from a size that the batches of frame-at-a-time callers do not outgrow call after call: a regrowth is a
        // hipFree + hipMalloc, hundreds of microseconds in the middle of a batch)
        const size_t want = std::max<size_t>(bytes + (bytes >> 1), (size_t)16 << 20);
        const hipError_t e = hipMalloc(reinterpret_cast<void**>(&base), want);
        if (e != hipSuccess) {
            base = nullptr;
            return e;
        }
        cap = want;
        carve = Carve(base);
        return hipSuccess;
    }
    template <typename T>
    T* take(size_t count) { return carve.take<T>(std::max<size_t>(count, 1)); }
};

// What a calling thread needs on a device: scratch and a stream of its own (threads that code a frame at a time through the
// frame classes run side by side on the device instead of taking turns on the default stream).  Leased like the fast path's
// contexts (sela_lease.h): a thread that ends parks its set for the next thread on that device.
struct PinnedScratch { // page-locked host memory for what a call reads back first (status words, offsets, a small call's whole output)
    uint8_t* base = nullptr;
    size_t cap = 0;
    void release()
    {
        if (base)
            (void)hipHostFree(base);
        base = nullptr, cap = 0;
    }
    uint8_t* reserve(size_t bytes) // null when the runtime has none to give: the caller copies into its own (pageable) memory then
    {
        if (base && bytes <= cap)
            return base;
        release();
        const size_t want = std::max<size_t>(bytes + (bytes >> 1), (size_t)3 << 20); // (grow-only; a regrowth is a hipHostFree + hipHostMalloc: milliseconds)
        if (hipHostMalloc(reinterpret_cast<void**>(&base), want, hipHostMallocDefault) != hipSuccess) {
            base = nullptr;
            return nullptr;
        }
        cap = want;
        return base;
    }
};

// A context's stream.  The runtime serves all streams through a few hardware queues (four) and gives a new stream the queue with the
// fewest streams on it at that moment; two contexts whose streams share a queue take turns on the device instead of running side
// by side.  With three coalesced decode jobs in flight, runs of the reference's thread loop over the frame classes came in two kinds:
// 280-300 M samples/s at 64 threads, or 180-190 (6 of 16 runs; with GPU_MAX_HW_QUEUES=8 or 16: 0 of 12).  So streams are made four
// at a time, one after the other, and handed out in that order, and the park hands back the context parked last: the contexts in use
// together are the ones created in a row, on different queues (2 of 16 runs of the slow kind since; the runtime's placement is
// not ours to decide, only to make less likely to hurt).
hipError_t fresh_stream(int dev, hipStream_t* out)
{
    static std::mutex mu;
    static std::vector<hipStream_t> bank[64];
    const int d = dev >= 0 && dev < 64 ? dev : 0;
    std::lock_guard<std::mutex> lock(mu);
    if (bank[d].empty()) {
        for (int i = 0; i < 4; i++) {
            hipStream_t s = nullptr;
            const hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
            if (e != hipSuccess) {
                if (bank[d].empty())
                    return e;
                (void)hipGetLastError();
                break;
            }
            bank[d].insert(bank[d].begin(), s); // (handed out from the back: in the order of creation)
        }
    }
    *out = bank[d].back();
    bank[d].pop_back();
    return hipSuccess;
}

struct GenericContext : sela::CurrentDevice {
    int device = -1;
    hipStream_t stream = nullptr;
    Arena arena;
    PinnedScratch pinned;
    hipError_t open() { return stream ? hipSuccess : fresh_stream(device, &stream); } // (on the context's device, before its first use)
    // what the lease asks of it (sela_lease.h)
    static constexpr size_t kParked = 64;
    static GenericContext* make(int dev)
    {
        GenericContext* c = new GenericContext;
        c->device = dev;
        return c;
    }
    bool serves(int dev) const { return device == dev; } // (its stream and scratch are that device's: another device, another context)
    void tidy() {}
    void destroy()
    {
        arena.release();
        pinned.release();
        if (stream)
            (void)hipStreamDestroy(stream);
        stream = nullptr;
    }
};
thread_local sela::ContextLease<GenericContext> g_lease;

// What every entry point of the route opens with: a device, and the calling thread's context on it.
struct Call {
    int rc; // SELA_HIP_OK, or the failure, reported
    GenericContext* ctx = nullptr;
    Call()
    {
        if ((rc = sela::device_ready()) != SELA_HIP_OK)
            return;
        int dev = -1;
        hipError_t e = hipGetDevice(&dev);
        if (e == hipSuccess && (ctx = g_lease.get(dev)))
            e = ctx->open();
        if (e != hipSuccess)
            rc = sela::report_hip_error(e, "the calling thread's scratch and stream");
    }
    Arena& arena() const { return ctx->arena; }
    hipStream_t stream() const { return ctx->stream; }
};

std::atomic<int> g_standard_first_mode{-1}; // sela_hip_debug_standard_first
std::atomic<int> g_standard_chunks{0};
std::atomic<long long> g_segment_subframes{0}; // subframes k_decode_subframes32 parsed by segments (sela_hip_debug_segment_subframes)

constexpr size_t kPiece = 256; // what take() may add per piece
constexpr size_t kChunkBudget = (size_t)768 << 20; // device scratch per chunk of frames

} // namespace

namespace sela {

void generic_release() { g_lease.give_back(); }
int generic_standard_first_mode() { return g_standard_first_mode.load(std::memory_order_relaxed); }
void generic_shutdown() { g_lease.shutdown(); }

size_t generic_encode_bound_bytes(uint32_t n_frames, uint32_t channels, uint32_t n)
{
    // first-minimum k is no worse than k = 19: (u >> 19) + 20 bits per value, u < 2^31 (beyond: ERANGE); a subframe holds at most
    // 65535 words (beyond: ERANGE)
    const uint64_t res_words = std::min<uint64_t>(65535, ((uint64_t)n * (4095 + 20) + 31) / 32);
    return (size_t)n_frames * (4 + (size_t)channels * (SELA_SUBFRAME_HEADER_BYTES + 4 * ((size_t)kCoefWordsCap + res_words)));
}

// input: int16 [n_frames][n][channels] (in16) or int32 [n_frames][channels][n]
// One submission per chunk of frames: copy in, analyse, plan, pack, assemble, copy out -- the Rice words and the frame bytes go
// to scratch sized by an ESTIMATE (4.5 bytes per sample: what 32-bit noise costs; 16-bit audio needs half), the kernels stay
// inside it whatever the data, and only a chunk whose plan turns out larger is packed and assembled again at its exact size
// (round 5 waited for the plan before it sized anything: two trips to the device per call).  What the host reads back first --
// status, sizes, offsets, and a small call's frames -- lands in page-locked memory of the calling thread's context.
constexpr size_t kEagerBytes = (size_t)4 << 20;

int generic_encode(const void* input, bool in16, uint32_t n_frames, uint32_t channels, uint32_t n, uint8_t* frames_out, size_t frames_cap,
    uint64_t* frame_offsets_out, bool lossless /* SELA_HIP_ENCODE_LOSSLESS */, bool paired /* sela_hip_encode_paired*: DESIGN.md 5.18 */)
{
    const Call call;
    if (call.rc != SELA_HIP_OK)
        return call.rc;
    Arena& g_arena = call.arena();
    const uint32_t n_sig = generic_signals(channels, paired);
    const size_t in_frame_bytes = (size_t)n * channels * (in16 ? 2 : 4);
    const size_t est_frame_bytes = ((size_t)n * channels * 9) / 2 + (size_t)channels * 192 + 64; // words and frame bytes, each (a subframe: 12 bytes of header, up to 32 coefficient words)
    const size_t per_frame = (size_t)n_sig * n * 8 + (size_t)n_sig * (kMaxOrder * 4 + sizeof(GenericMeta) + 2 * kPiece) + in_frame_bytes + (size_t)channels * 12 + 8
        + 2 * est_frame_bytes;
    const uint32_t chunk = (uint32_t)std::max<size_t>(1, std::min<size_t>(n_frames, kChunkBudget / per_frame));
    uint64_t base_bytes = 0;
    frame_offsets_out[0] = 0;
    const hipStream_t st = call.stream();
    for (uint32_t f0 = 0; f0 < n_frames; f0 += chunk) {
        const uint32_t cf = std::min(chunk, n_frames - f0);
        const size_t blocks = (size_t)cf * n_sig, subs = (size_t)cf * channels;
        const size_t est_words = ((size_t)cf * est_frame_bytes + 3) / 4, est_bytes = est_words * 4;
        const size_t fixed = blocks * n * 8 + blocks * (kMaxOrder * 4 + sizeof(GenericMeta)) + cf * in_frame_bytes + (subs + 1) * 12 + ((size_t)cf + 1) * 8 + 64 + 16 * kPiece
            + est_words * 4 + 8 + est_bytes;
        hipError_t e = g_arena.reserve(fixed);
        if (e != hipSuccess)
            return report_hip_error(e, "generic encode: scratch");
        void* d_in = g_arena.take<uint8_t>(cf * in_frame_bytes);
        int32_t* d_sig = g_arena.take<int32_t>(blocks * n);
        int32_t* d_res = g_arena.take<int32_t>(blocks * n);
        int32_t* d_q = g_arena.take<int32_t>(blocks * kMaxOrder);
        GenericMeta* d_meta = g_arena.take<GenericMeta>(blocks);
        // what the host reads back first, in one piece: status (4 x u32) | total words | frame offsets
        const size_t head_words = 3 + (size_t)cf + 1;
        uint64_t* d_head = g_arena.take<uint64_t>(head_words);
        uint32_t* d_status = reinterpret_cast<uint32_t*>(d_head);
        uint64_t* d_offsets = d_head + 3;
        uint64_t* d_word_base = g_arena.take<uint64_t>(subs + 1);
        uint32_t* d_chosen = g_arena.take<uint32_t>(subs);
        uint32_t* d_words = g_arena.take<uint32_t>(est_words + 2);
        uint8_t* d_frames = g_arena.take<uint8_t>(est_bytes);
        if (!g_arena.fits())
            return report_error(SELA_HIP_ENOMEM, "generic encode: internal scratch estimate too small");
        const bool eager = est_bytes <= kEagerBytes;
        uint8_t* const pin = call.ctx->pinned.reserve(head_words * 8 + (eager ? est_bytes : 0));
        std::vector<uint64_t> head_pageable;
        uint64_t* head = reinterpret_cast<uint64_t*>(pin);
        if (!pin) {
            head_pageable.resize(head_words);
            head = head_pageable.data();
        }
        uint8_t* const eager_frames = pin && eager ? pin + head_words * 8 : nullptr;
        e = hipMemcpyAsync(d_in, static_cast<const uint8_t*>(input) + (size_t)f0 * in_frame_bytes, cf * in_frame_bytes, hipMemcpyHostToDevice, st);
        if (e == hipSuccess)
            e = hipMemsetAsync(d_head, 0, 24, st);
        if (e == hipSuccess)
            e = hipMemsetAsync(d_words, 0, (est_words + 2) * 4, st);
        if (e == hipSuccess)
            e = launch_generic_analyse(d_in, in16, cf, channels, n_sig, n, d_sig, d_res, d_q, d_meta, st, lossless, paired);
        if (e == hipSuccess)
            e = launch_generic_plan(d_meta, cf, channels, n_sig, base_bytes, d_offsets, d_word_base, d_chosen, d_status, d_head + 2, st, paired);
        if (e == hipSuccess)
            e = launch_generic_emit(d_meta, cf, channels, n_sig, n, d_res, d_q, d_chosen, d_word_base, d_words, est_words, d_offsets, base_bytes, d_frames, est_bytes, st);
        if (e == hipSuccess)
            e = hipMemcpyAsync(head, d_head, head_words * 8, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && eager_frames)
            e = hipMemcpyAsync(eager_frames, d_frames, est_bytes, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess)
            e = hipStreamSynchronize(st);
        if (e != hipSuccess)
            return report_hip_error(e, "generic encode");
        uint32_t status[4];
        std::memcpy(status, head, 16);
        const uint64_t total_words = head[2];
        std::memcpy(frame_offsets_out + f0, head + 3, ((size_t)cf + 1) * 8);
        const int rc = judge_encode(status[0], kJudgeEncode, "encode");
        if (rc != SELA_HIP_OK)
            return rc;
        const uint64_t chunk_bytes = frame_offsets_out[f0 + cf] - base_bytes;
        if (frame_offsets_out[f0 + cf] > frames_cap)
            return report_error(SELA_HIP_ECAPACITY, "frames_out too small (see sela_hip_encode_bound_bytes_n)");
        if (total_words <= est_words && chunk_bytes <= est_bytes) {
            if (eager_frames) {
                std::memcpy(frames_out + base_bytes, eager_frames, (size_t)chunk_bytes);
            } else {
                e = hipMemcpyAsync(frames_out + base_bytes, d_frames, chunk_bytes, hipMemcpyDeviceToHost, st);
                if (e == hipSuccess)
                    e = hipStreamSynchronize(st);
            }
        } else { // (rare: data that codes to more than 4.5 bytes per sample) pack and assemble again, at the plan's exact sizes
            uint8_t* extra = nullptr;
            const size_t words_bytes = (size_t)workspace_up(((size_t)total_words + 2) * 4); // (of an allocation of this call's own, no workspace: the frames behind the words)
            e = hipMalloc(reinterpret_cast<void**>(&extra), words_bytes + chunk_bytes + 256);
            if (e != hipSuccess)
                return report_hip_error(e, "generic encode: stream scratch");
            uint32_t* d_words2 = reinterpret_cast<uint32_t*>(extra);
            uint8_t* d_frames2 = extra + words_bytes;
            e = hipMemsetAsync(d_words2, 0, ((size_t)total_words + 2) * 4, st);
            if (e == hipSuccess)
                e = launch_generic_emit(d_meta, cf, channels, n_sig, n, d_res, d_q, d_chosen, d_word_base, d_words2, total_words, d_offsets, base_bytes, d_frames2, chunk_bytes, st);
            if (e == hipSuccess)
                e = hipMemcpyAsync(frames_out + base_bytes, d_frames2, chunk_bytes, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess)
                e = hipStreamSynchronize(st);
            (void)hipFree(extra);
        }
        if (e != hipSuccess)
            return report_hip_error(e, "generic encode: emit");
        base_bytes += chunk_bytes;
    }
    return SELA_HIP_OK;
}

// Walk a stream's headers on the host: per frame the first subframe's samplesPerChannel (running total in sample_offsets, if
// given), the largest samplesPerChannel of any subframe (returned; 0 when the walk falls off a frame), and whether every
// subframe says exactly 2048.
uint32_t generic_index_samples(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, uint64_t* sample_offsets,
    bool* all_standard)
{
    uint32_t largest = 0;
    bool standard = true, broken = false;
    uint64_t total = 0;
    for (uint32_t f = 0; f < n_frames; f++) {
        if (sample_offsets)
            sample_offsets[f] = total;
        const uint8_t* fb = frames + frame_offsets[f];
        const uint64_t fbytes = frame_offsets[f + 1] >= frame_offsets[f] ? frame_offsets[f + 1] - frame_offsets[f] : 0;
        uint64_t p = 4;
        uint32_t first = 0;
        for (uint32_t c = 0; c < channels; c++) {
            SelaSubframeHeader h = {}; // (n is read, and counts, even when only the residue words run past the frame)
            p = sela_subframe_read_bytes(fb, fbytes, p, &h);
            if (c == 0)
                first = h.n;
            largest = std::max(largest, h.n);
            standard = standard && h.n == SELA_HIP_SAMPLES_PER_FRAME;
            if (p == 0) {
                broken = true;
                break;
            }
        }
        total += first;
    }
    if (sample_offsets)
        sample_offsets[n_frames] = total;
    if (all_standard)
        *all_standard = standard && !broken;
    return broken ? 0 : largest;
}

// One of: samples_out + counts_out (32-bit, planar, stride), or pcm_out + sample_offsets (16-bit interleaved).
// Every chunk's subframes are first offered to k_decode_subframes32 (the fast decoder's lane-parallel parse and tuned synthesis
// with 32-bit samples, any length); a chunk in which that kernel leaves anything alone -- a frame that is not whole words at
// an aligned place, a malformed header, a stream that runs dry, coefficients outside the tables -- is decoded again by
// k_generic_decode, which reproduces what the reference does with such streams (or reports them).
int generic_decode(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, int32_t* samples_out, uint32_t stride,
    uint32_t* counts_out, int16_t* pcm_out, const uint64_t* sample_offsets)
{
    const Call call;
    if (call.rc != SELA_HIP_OK)
        return call.rc;
    Arena& g_arena = call.arena();
    if (check_frame_offsets(frame_offsets, n_frames) != SELA_HIP_OK)
        return SELA_HIP_EFORMAT;
    if (stride == 0)
        stride = 1;
    const size_t per_frame = (size_t)channels * stride * 8 + (size_t)channels * (sizeof(GenericSubInfo) + 4) + 16 + (size_t)channels * stride * (pcm_out ? 2 : 0);
    const uint32_t chunk = (uint32_t)std::max<size_t>(1, std::min<size_t>(n_frames, kChunkBudget / per_frame));
    const hipStream_t st = call.stream();
    for (uint32_t f0 = 0; f0 < n_frames; f0 += chunk) {
        const uint32_t cf = std::min(chunk, n_frames - f0);
        const size_t subs = (size_t)cf * channels;
        const uint64_t base_bytes = frame_offsets[f0], in_bytes = frame_offsets[f0 + cf] - base_bytes;
        const uint64_t s0 = pcm_out ? sample_offsets[f0] : 0, chunk_samples = pcm_out ? sample_offsets[f0 + cf] - s0 : 0;
        const size_t need = in_bytes + 8 + ((size_t)cf + 1) * 16 + subs * stride * 8 + subs * (sizeof(GenericSubInfo) + 4) + (size_t)chunk_samples * channels * 2 + 64
            + 12 * kPiece;
        hipError_t e = g_arena.reserve(need);
        if (e != hipSuccess)
            return report_hip_error(e, "generic decode: scratch");
        uint8_t* d_frames = g_arena.take<uint8_t>(in_bytes + 8);
        uint64_t* d_offsets = g_arena.take<uint64_t>((size_t)cf + 1);
        int32_t* d_dec = g_arena.take<int32_t>(subs * stride);
        int32_t* d_all = g_arena.take<int32_t>(subs * stride);
        GenericSubInfo* d_info = g_arena.take<GenericSubInfo>(subs);
        // what the host reads back first, in one piece: status (4 x u32) | a count per (frame, channel)
        uint32_t* d_tail = g_arena.take<uint32_t>(4 + subs);
        uint32_t* d_status = d_tail;
        uint32_t* d_counts = d_tail + 4;
        uint64_t* d_sample_offsets = pcm_out ? g_arena.take<uint64_t>((size_t)cf + 1) : nullptr;
        int16_t* d_pcm = pcm_out ? g_arena.take<int16_t>((size_t)chunk_samples * channels) : nullptr;
        if (!g_arena.fits())
            return report_error(SELA_HIP_ENOMEM, "generic decode: internal scratch estimate too small");
        // A small chunk's samples travel with the status, one wait for the device instead of two (a call of one frame -- the
        // frame classes' kind -- is mostly waits); what they are worth is known when both have arrived.  Both land in
        // page-locked memory of the calling thread's context (a copy into pageable memory is staged by the runtime, and waits)
        // -- unless the caller's own buffer is page-locked (a coalesced batch's staging, sela_hip_host_alloc): then the samples
        // go there at once (through the context's buffer and a memcpy, a batch of 50 stereo frames cost its leader 0.8 MB of
        // copying more).  The frame offsets take the same way in: from page-locked memory the copy is queued, not staged.
        const size_t out_bytes = pcm_out ? (size_t)chunk_samples * channels * 2 : subs * stride * sizeof(int32_t);
        const bool eager = out_bytes <= kEagerBytes;
        const size_t tail_bytes = ((4 + subs) * 4 + 15) & ~(size_t)15, offsets_bytes = (((size_t)cf + 1) * 8 + 15) & ~(size_t)15;
        uint8_t* const user_out = pcm_out ? reinterpret_cast<uint8_t*>(pcm_out + s0 * channels) : reinterpret_cast<uint8_t*>(samples_out + (size_t)f0 * channels * stride);
        bool user_locked = false;
        if (eager) {
            hipPointerAttribute_t attr;
            user_locked = hipPointerGetAttributes(&attr, user_out) == hipSuccess && attr.type == hipMemoryTypeHost;
            (void)hipGetLastError(); // (ordinary memory is not an error)
        }
        uint8_t* const pin = call.ctx->pinned.reserve(tail_bytes + offsets_bytes + (eager && !user_locked ? out_bytes : 0));
        const uint64_t* offsets_src = frame_offsets + f0;
        if (pin) {
            std::memcpy(pin + tail_bytes, frame_offsets + f0, ((size_t)cf + 1) * 8);
            offsets_src = reinterpret_cast<const uint64_t*>(pin + tail_bytes);
        }
        e = hipMemcpyAsync(d_frames, frames + base_bytes, in_bytes, hipMemcpyHostToDevice, st);
        if (e == hipSuccess)
            e = hipMemcpyAsync(d_offsets, offsets_src, ((size_t)cf + 1) * 8, hipMemcpyHostToDevice, st);
        std::vector<uint64_t> local;
        if (e == hipSuccess && pcm_out) { // positions relative to the chunk's first sample
            local.resize((size_t)cf + 1);
            for (uint32_t i = 0; i <= cf; i++)
                local[i] = sample_offsets[f0 + i] - s0;
            e = hipMemcpyAsync(d_sample_offsets, local.data(), local.size() * 8, hipMemcpyHostToDevice, st);
        }
        const int mode = g_standard_first_mode.load(std::memory_order_relaxed); // -1: the product; 0: the serial kernel alone; 1: as -1; 2: offered, every subframe by segments
        const bool offer = mode != 0, standard_path = mode != 2;
        std::vector<uint32_t> tail_pageable;
        uint32_t* tail = reinterpret_cast<uint32_t*>(pin);
        if (!pin) {
            tail_pageable.resize(4 + subs);
            tail = tail_pageable.data();
        }
        uint8_t* const eager_out = pin && eager && !user_locked ? pin + tail_bytes + offsets_bytes : nullptr;
        const void* const device_out = pcm_out ? static_cast<const void*>(d_pcm) : static_cast<const void*>(d_all);
        // samples_out and the device's channel-major array have one layout ([frame][channel][stride]): ONE copy (a copy per
        // channel cost 13 us each: 7 ms for 256 stereo frames).  What lies behind a channel's count is not defined.
        for (int attempt = offer ? 0 : 1; attempt < 2; attempt++) {
            if (e == hipSuccess)
                e = hipMemsetAsync(d_tail, 0, (4 + subs) * 4, st);
            if (e == hipSuccess)
                e = launch_generic_decode(d_frames, d_offsets, base_bytes, cf, channels, stride, d_dec, d_info, d_all, d_counts, d_sample_offsets, d_pcm, d_status,
                    attempt == 0, standard_path, st);
            if (e == hipSuccess)
                e = hipMemcpyAsync(tail, d_tail, (4 + subs) * 4, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess && eager)
                e = hipMemcpyAsync(eager_out ? eager_out : user_out, device_out, out_bytes, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess)
                e = hipStreamSynchronize(st);
            if (e != hipSuccess)
                return report_hip_error(e, "generic decode");
            if (attempt == 0 && tail[2] == 0) { // (the fast kernel took every subframe and every one came out clean)
                g_standard_chunks.fetch_add(1, std::memory_order_relaxed);
                g_segment_subframes.fetch_add(tail[3], std::memory_order_relaxed);
                break;
            }
        }
        const uint32_t* const status = tail;
        // (what the reference itself leaves undefined is reported, never decoded silently: the decoders' one policy, sela_host.h)
        const int verdict = judge_decode(status[0], kJudgeJob | SELA_HIP_FLAG_SHORT_BLOCK, kRouteHost32, "decode");
        if (verdict != SELA_HIP_OK)
            return verdict;
        if (!pcm_out)
            std::memcpy(counts_out + (size_t)f0 * channels, tail + 4, subs * 4);
        if (eager_out) {
            std::memcpy(user_out, eager_out, out_bytes);
        } else if (!eager) {
            e = hipMemcpyAsync(user_out, device_out, out_bytes, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess)
                e = hipStreamSynchronize(st);
        }
        if (e != hipSuccess)
            return report_hip_error(e, "generic decode: copy out");
    }
    return SELA_HIP_OK;
}

// The host-pointer calls that decode a stream and keep something other than the samples -- sela_hip_verify, _verify_i32,
// _verify_pcm, _levels, _levels_i32 -- and sela_hip_decode_pcm: their *_device launch
// on chunks of whole frames, on the calling thread's context and stream (frame_chunks).  Per chunk the frames and their offsets
// (relative to a 4-byte aligned base) go in, with what the call uploads beside them; what it reads back lands behind the chunk's ONE
// wait; the first chunk whose status words fail ends the call with that code.  What a call brings is its `Op`:
//   per_frame                       the scratch a frame costs, roughly: it picks the chunk size (kChunkBudget), nothing else
//   workspace_bytes(cf)             its launch's workspace for cf frames
//   pieces(c, f0, cf)               its pieces of the arena, between the frame offsets and the workspace.  Run on a measuring
//                                   Carve to size the arena and on the arena's to take them, so the two cannot disagree
//   submit(.., f0, cf, d_ws, ..)    its upload, its launch and its copies back, all on the stream
//   finish(f0, cf)                  behind the wait: the status words judged, the results handed on
namespace {
std::atomic<uint32_t> g_pcm_chunk_frames{0}; // sela_hip_debug_pcm_chunk_frames: this many frames a chunk (0: the budget decides)
uint32_t pcm_chunk(uint32_t n_frames, size_t per_frame)
{
    const uint32_t forced = g_pcm_chunk_frames.load(std::memory_order_relaxed);
    const size_t chunk = forced ? forced : kChunkBudget / per_frame;
    return (uint32_t)std::max<size_t>(1, std::min<size_t>(n_frames, chunk));
}

template <typename T>
T* piece(Carve& c, uint64_t count) { return c.take<T>(std::max<uint64_t>(count, 1)); }

template <typename Op>
int frame_chunks(const Call& call, const char* who, const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, Op& op)
{
    Arena& arena = call.arena();
    const std::string name(who);
    const uint32_t chunk = pcm_chunk(n_frames, op.per_frame);
    const hipStream_t st = call.stream();
    const int mode = g_standard_first_mode.load(std::memory_order_relaxed);
    std::vector<uint64_t> local;
    for (uint32_t f0 = 0; f0 < n_frames; f0 += chunk) {
        const uint32_t cf = std::min(chunk, n_frames - f0);
        const uint64_t base_bytes = frame_offsets[f0] & ~(uint64_t)3, in_bytes = frame_offsets[f0 + cf] - base_bytes;
        const size_t ws_bytes = op.workspace_bytes(cf);
        if (ws_bytes == SIZE_MAX)
            return report_error(SELA_HIP_EINVAL, name + ": the chunk is too large");
        uint8_t *d_frames = nullptr, *d_ws = nullptr;
        uint64_t* d_offsets = nullptr;
        const auto pieces = [&](Carve& c) {
            d_frames = piece<uint8_t>(c, in_bytes + 8);
            d_offsets = piece<uint64_t>(c, (uint64_t)cf + 1);
            op.pieces(c, f0, cf);
            d_ws = piece<uint8_t>(c, ws_bytes);
        };
        hipError_t e = arena.reserve(measured(nullptr, pieces));
        if (e != hipSuccess)
            return report_hip_error(e, (name + ": scratch").c_str());
        pieces(arena.carve);
        local.resize((size_t)cf + 1);
        for (uint32_t i = 0; i <= cf; i++)
            local[i] = frame_offsets[f0 + i] - base_bytes;
        e = hipMemcpyAsync(d_frames, frames + base_bytes, in_bytes, hipMemcpyHostToDevice, st);
        if (e == hipSuccess)
            e = hipMemcpyAsync(d_offsets, local.data(), local.size() * 8, hipMemcpyHostToDevice, st);
        if (e == hipSuccess)
            e = op.submit(d_frames, d_offsets, f0, cf, d_ws, mode, st);
        if (e == hipSuccess)
            e = hipStreamSynchronize(st);
        if (e != hipSuccess)
            return report_hip_error(e, who);
        const int rc = op.finish(f0, cf);
        if (rc != SELA_HIP_OK)
            return rc;
    }
    return SELA_HIP_OK;
}

// The two judges of a chunk's status words: as sela_hip_decode_n_status_error judges (the int16 calls), as
// sela_hip_decode_status_error judges (the int32 ones).  status[2] is the call's own count there, not the largest frame.
int judge_n(const uint32_t* status)
{
    const uint32_t route_status[4] = { status[0], status[1], 0, status[3] };
    return sela_hip_decode_n_status_error(route_status);
}
int judge_i32(const uint32_t* status)
{
    const uint32_t decode_status[4] = { status[0], status[1], 0, 0 };
    return sela_hip_decode_status_error(decode_status);
}

// The three verify calls: a `Ref` -- the reference data (its pieces of the arena, its upload), the launch and the judge -- and
// behind it status (4 x u32) | diff_counts [cf] | first_diff [cf], read back in one piece.
struct VerifyPcm { // int16, interleaved, where sela_hip_decode writes it (sample_offsets)
    const int16_t* pcm;
    const uint64_t* sample_offsets;
    uint32_t channels, stride;
    int recurrence_form;
    int16_t* d_pcm;
    uint64_t values(uint32_t f0, uint32_t cf) const { return (sample_offsets[f0 + cf] - sample_offsets[f0]) * channels; }
    void take(Carve& c, uint32_t f0, uint32_t cf) { d_pcm = piece<int16_t>(c, values(f0, cf)); }
    hipError_t upload(uint32_t f0, uint32_t cf, hipStream_t st) const
    {
        const uint64_t n = values(f0, cf);
        return n ? hipMemcpyAsync(d_pcm, pcm + sample_offsets[f0] * channels, (size_t)n * 2, hipMemcpyHostToDevice, st) : hipSuccess;
    }
    hipError_t launch(const uint8_t* d_frames, const uint64_t* d_offsets, uint32_t cf, uint32_t* d_tail, void* d_ws, int mode, hipStream_t st) const
    {
        return launch_verify_n_device(d_frames, d_offsets, cf, nullptr, channels, stride, d_pcm, d_tail + 4, d_tail + 4 + cf, nullptr, d_tail, d_ws, mode, recurrence_form,
            0, st);
    }
    static constexpr auto judge = judge_n;
};
struct VerifySamples { // int32 [frame][channel][stride], lengths or null
    const int32_t* samples;
    const uint32_t* lengths;
    uint32_t channels, stride;
    int32_t* d_samples;
    uint32_t* d_lengths;
    void take(Carve& c, uint32_t, uint32_t cf)
    {
        d_samples = piece<int32_t>(c, (uint64_t)cf * channels * stride);
        d_lengths = lengths ? piece<uint32_t>(c, (uint64_t)cf * channels) : nullptr;
    }
    hipError_t upload(uint32_t f0, uint32_t cf, hipStream_t st) const
    {
        const size_t subs = (size_t)cf * channels;
        hipError_t e = hipMemcpyAsync(d_samples, samples + (size_t)f0 * channels * stride, subs * stride * 4, hipMemcpyHostToDevice, st);
        if (e == hipSuccess && lengths)
            e = hipMemcpyAsync(d_lengths, lengths + (size_t)f0 * channels, subs * 4, hipMemcpyHostToDevice, st);
        return e;
    }
    hipError_t launch(const uint8_t* d_frames, const uint64_t* d_offsets, uint32_t cf, uint32_t* d_tail, void* d_ws, int mode, hipStream_t st) const
    {
        return launch_verify_i32_device(d_frames, d_offsets, cf, nullptr, channels, stride, d_samples, d_lengths, d_tail + 4, d_tail + 4 + cf, nullptr, d_tail, d_ws, mode, st);
    }
    static constexpr auto judge = judge_i32;
};
struct VerifyPacked { // packed interleaved PCM of 3 or 4 bytes a sample, where sela_hip_decode_pcm writes it (sample_offsets)
    const uint8_t* pcm;
    uint64_t pcm_samples;
    const uint64_t* sample_offsets;
    uint32_t channels, stride, bytes_per_sample;
    uint8_t* d_pcm;
    uint32_t chunk_f0; // the first frame of the chunk d_pcm holds
    uint64_t held(uint32_t f0) const { return pcm_samples - std::min(sample_offsets[f0], pcm_samples); } // samples the original holds from the chunk's first frame on
    uint64_t samples(uint32_t f0, uint32_t cf) const { return std::min(sample_offsets[f0 + cf] - sample_offsets[f0], held(f0)); }
    size_t bytes(uint32_t f0, uint32_t cf) const { return (size_t)samples(f0, cf) * channels * bytes_per_sample; }
    void take(Carve& c, uint32_t f0, uint32_t cf) { d_pcm = piece<uint8_t>(c, bytes(f0, cf) + 4), chunk_f0 = f0; }
    hipError_t upload(uint32_t f0, uint32_t cf, hipStream_t st) const
    {
        const size_t n = bytes(f0, cf);
        return n ? hipMemcpyAsync(d_pcm, pcm + sample_offsets[f0] * channels * bytes_per_sample, n, hipMemcpyHostToDevice, st) : hipSuccess;
    }
    hipError_t launch(const uint8_t* d_frames, const uint64_t* d_offsets, uint32_t cf, uint32_t* d_tail, void* d_ws, int mode, hipStream_t st) const
    {
        return launch_verify_pcm_device(d_frames, d_offsets, cf, nullptr, channels, stride, d_pcm, bytes_per_sample, held(chunk_f0), d_tail + 4, d_tail + 4 + cf, nullptr,
            d_tail, d_ws, mode, st);
    }
    static constexpr auto judge = judge_i32;
};

template <typename Ref>
struct VerifyOp {
    size_t per_frame;
    size_t (*workspace)(uint32_t, uint32_t, uint32_t);
    Ref ref;
    uint32_t *diff_counts, *first_diff;
    uint32_t lossy = 0;
    uint32_t* d_tail = nullptr;
    std::vector<uint32_t> tail;
    size_t workspace_bytes(uint32_t cf) const { return workspace(cf, ref.channels, ref.stride); }
    void pieces(Carve& c, uint32_t f0, uint32_t cf)
    {
        ref.take(c, f0, cf);
        d_tail = piece<uint32_t>(c, 4 + 2 * (uint64_t)cf);
    }
    hipError_t submit(const uint8_t* d_frames, const uint64_t* d_offsets, uint32_t f0, uint32_t cf, void* d_ws, int mode, hipStream_t st)
    {
        tail.resize(4 + 2 * (size_t)cf);
        hipError_t e = ref.upload(f0, cf, st);
        if (e == hipSuccess)
            e = ref.launch(d_frames, d_offsets, cf, d_tail, d_ws, mode, st);
        if (e == hipSuccess)
            e = hipMemcpyAsync(tail.data(), d_tail, tail.size() * 4, hipMemcpyDeviceToHost, st);
        return e;
    }
    int finish(uint32_t f0, uint32_t cf)
    {
        const int rc = Ref::judge(tail.data());
        if (rc != SELA_HIP_OK)
            return rc;
        std::memcpy(diff_counts + f0, tail.data() + 4, (size_t)cf * 4);
        std::memcpy(first_diff + f0, tail.data() + 4 + cf, (size_t)cf * 4);
        lossy += tail[2];
        return SELA_HIP_OK;
    }
};

template <typename Ref>
int verify_chunks(const Call& call, const char* who, const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, size_t per_frame,
    size_t (*workspace_bytes)(uint32_t, uint32_t, uint32_t), Ref ref, uint32_t* diff_counts, uint32_t* first_diff, uint32_t* lossy_frames)
{
    VerifyOp<Ref> op{ per_frame, workspace_bytes, ref, diff_counts, first_diff };
    const int rc = frame_chunks(call, who, frames, frame_offsets, n_frames, op);
    if (rc == SELA_HIP_OK && lossy_frames)
        *lossy_frames = op.lossy;
    return rc;
}

// The two levels calls and the envelope: no reference; status (4 x u32) | the chunk's records (`records` of them a frame), read
// back in two pieces, the records straight into the caller's.  `Launch`: the call's *_device launch on (d_frames, d_offsets, cf, d_levels, d_status, d_ws, mode, stream).
template <typename Record, typename Launch>
struct LevelsOp {
    size_t per_frame;
    size_t (*workspace)(uint32_t, uint32_t, uint32_t);
    int (*judge)(const uint32_t*);
    uint32_t channels, stride;
    uint32_t records;
    Record* levels;
    Launch launch;
    uint32_t* d_status = nullptr;
    Record* d_levels = nullptr;
    uint32_t status[4] = { 0, 0, 0, 0 };
    size_t workspace_bytes(uint32_t cf) const { return workspace(cf, channels, stride); }
    void pieces(Carve& c, uint32_t, uint32_t cf)
    {
        d_status = piece<uint32_t>(c, 4);
        d_levels = piece<Record>(c, (uint64_t)cf * records);
    }
    hipError_t submit(const uint8_t* d_frames, const uint64_t* d_offsets, uint32_t f0, uint32_t cf, void* d_ws, int mode, hipStream_t st)
    {
        hipError_t e = launch(d_frames, d_offsets, cf, d_levels, d_status, d_ws, mode, st);
        if (e == hipSuccess)
            e = hipMemcpyAsync(status, d_status, sizeof(status), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess)
            e = hipMemcpyAsync(levels + (size_t)f0 * records, d_levels, (size_t)cf * records * sizeof(Record), hipMemcpyDeviceToHost, st);
        return e;
    }
    int finish(uint32_t, uint32_t) const { return judge(status); }
};
template <typename Record, typename Launch>
int levels_chunks(const Call& call, const char* who, const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride,
    uint32_t records, size_t per_frame, size_t (*workspace_bytes)(uint32_t, uint32_t, uint32_t), int (*judge)(const uint32_t*), Record* levels, Launch launch)
{
    LevelsOp<Record, Launch> op{ per_frame, workspace_bytes, judge, channels, stride, records, levels, launch };
    return frame_chunks(call, who, frames, frame_offsets, n_frames, op);
}
} // namespace

// The stride is the stream's largest samplesPerChannel (the host's walk).
int generic_verify(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, const int16_t* pcm, uint32_t* diff_counts,
    uint32_t* first_diff, uint32_t* lossy_frames, int recurrence_form)
{
    if (lossy_frames)
        *lossy_frames = 0;
    const Call call;
    if (call.rc != SELA_HIP_OK)
        return call.rc;
    if (check_frame_offsets(frame_offsets, n_frames) != SELA_HIP_OK)
        return SELA_HIP_EFORMAT;
    std::vector<uint64_t> sample_offsets((size_t)n_frames + 1);
    const uint32_t largest = generic_index_samples(frames, frame_offsets, n_frames, channels, sample_offsets.data(), nullptr);
    if (n_frames && largest == 0)
        return report_error(SELA_HIP_EFORMAT, "malformed frame stream (the header walk breaks, or no subframe says a length)");
    const uint32_t stride = std::max(largest, 1u);
    const size_t per_frame = (size_t)channels * stride * (4 + (channels > 8 ? 4 : 0) + 2 + 2) + (size_t)channels * sizeof(GenericSubInfo) + 64;
    return verify_chunks(call, "verify", frames, frame_offsets, n_frames, per_frame, verify_workspace_bytes,
        VerifyPcm{ pcm, sample_offsets.data(), channels, stride, recurrence_form, nullptr }, diff_counts, first_diff, lossy_frames);
}

// sela_hip_levels.  The stride is the stream's largest samplesPerChannel (the host's walk).
int generic_levels(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, sela_hip_level* levels, int recurrence_form)
{
    const Call call;
    if (call.rc != SELA_HIP_OK)
        return call.rc;
    if (check_frame_offsets(frame_offsets, n_frames) != SELA_HIP_OK)
        return SELA_HIP_EFORMAT;
    const uint32_t largest = generic_index_samples(frames, frame_offsets, n_frames, channels, nullptr, nullptr);
    if (n_frames && largest == 0)
        return report_error(SELA_HIP_EFORMAT, "malformed frame stream (the header walk breaks, or no subframe says a length)");
    const uint32_t stride = std::max(largest, 1u);
    const size_t per_frame = (size_t)channels * stride * (4 + (channels > 8 ? 4 : 0) + 2) + (size_t)channels * (sizeof(GenericSubInfo) + sizeof(sela_hip_level)) + 64;
    return levels_chunks(call, "levels", frames, frame_offsets, n_frames, channels, stride, channels, per_frame, levels_workspace_bytes, judge_n, levels,
        [=](const uint8_t* d_frames, const uint64_t* d_offsets, uint32_t cf, sela_hip_level* d_levels, uint32_t* d_status, void* d_ws, int mode, hipStream_t st) {
            return launch_levels_n_device(d_frames, d_offsets, cf, nullptr, channels, stride, d_levels, nullptr, d_status, d_ws, mode, recurrence_form, 0, st);
        });
}

// sela_hip_envelope: generic_levels' walk and chunks, at the caller's stride (a longer frame is the status
// words' SELA_HIP_FLAG_STRIDE, judged like every other flag).
int generic_envelope(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride, uint32_t bucket,
    struct sela_hip_envelope* env, int recurrence_form)
{
    const Call call;
    if (call.rc != SELA_HIP_OK)
        return call.rc;
    if (check_frame_offsets(frame_offsets, n_frames) != SELA_HIP_OK)
        return SELA_HIP_EFORMAT;
    const uint32_t largest = generic_index_samples(frames, frame_offsets, n_frames, channels, nullptr, nullptr);
    if (n_frames && largest == 0)
        return report_error(SELA_HIP_EFORMAT, "malformed frame stream (the header walk breaks, or no subframe says a length)");
    const uint32_t records = envelope_slots(stride, bucket) * channels; // (fits 32 bits: sela_hip_envelope refuses a shape where it does not)
    const size_t per_frame = (size_t)channels * stride * (4 + (channels > 8 ? 4 : 0) + 2) + (size_t)channels * sizeof(GenericSubInfo) + (size_t)records * sizeof(struct sela_hip_envelope) + 64;
    return levels_chunks(call, "envelope", frames, frame_offsets, n_frames, channels, stride, records, per_frame, levels_workspace_bytes, judge_n, env,
        [=](const uint8_t* d_frames, const uint64_t* d_offsets, uint32_t cf, struct sela_hip_envelope* d_env, uint32_t* d_status, void* d_ws, int mode, hipStream_t st) {
            return launch_envelope_n_device(d_frames, d_offsets, cf, nullptr, channels, stride, bucket, d_env, nullptr, d_status, d_ws, mode, recurrence_form, 0, st);
        });
}

// sela_hip_digest: generic_levels' walk and chunks.  Per chunk status (4 x u32) | the two track words | the
// records come back, the records into the caller's where it wants them; the chunk's track word joins the call's by crc_combine.
namespace {
struct DigestOp {
    size_t per_frame;
    uint32_t channels, stride;
    int recurrence_form;
    struct sela_hip_digest* digests; // or null
    uint32_t crc = 0;
    uint64_t bytes = 0;
    uint32_t* d_status = nullptr;
    uint64_t* d_track = nullptr;
    struct sela_hip_digest* d_digests = nullptr;
    uint32_t status[4] = { 0, 0, 0, 0 };
    uint64_t track[2] = { 0, 0 };
    size_t workspace_bytes(uint32_t cf) const { return digest_workspace_bytes(cf, channels, stride); }
    void pieces(Carve& c, uint32_t, uint32_t cf)
    {
        d_status = piece<uint32_t>(c, 4);
        d_track = piece<uint64_t>(c, 2);
        d_digests = piece<struct sela_hip_digest>(c, cf);
    }
    hipError_t submit(const uint8_t* d_frames, const uint64_t* d_offsets, uint32_t f0, uint32_t cf, void* d_ws, int mode, hipStream_t st)
    {
        hipError_t e = launch_digest_n_device(d_frames, d_offsets, cf, nullptr, channels, stride, d_digests, d_track, nullptr, d_status, d_ws, mode, recurrence_form, 0, st);
        if (e == hipSuccess)
            e = hipMemcpyAsync(status, d_status, sizeof(status), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess)
            e = hipMemcpyAsync(track, d_track, sizeof(track), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && digests)
            e = hipMemcpyAsync(digests + f0, d_digests, (size_t)cf * sizeof(struct sela_hip_digest), hipMemcpyDeviceToHost, st);
        return e;
    }
    int finish(uint32_t, uint32_t)
    {
        const int rc = judge_n(status);
        if (rc != SELA_HIP_OK)
            return rc;
        crc = crc_combine(crc, (uint32_t)track[0], track[1]);
        bytes += track[1];
        return SELA_HIP_OK;
    }
};
} // namespace

int generic_digest(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, struct sela_hip_digest* digests, uint32_t* track_crc32,
    uint64_t* track_bytes, int recurrence_form)
{
    const Call call;
    if (call.rc != SELA_HIP_OK)
        return call.rc;
    if (check_frame_offsets(frame_offsets, n_frames) != SELA_HIP_OK)
        return SELA_HIP_EFORMAT;
    const uint32_t largest = generic_index_samples(frames, frame_offsets, n_frames, channels, nullptr, nullptr);
    if (n_frames && largest == 0)
        return report_error(SELA_HIP_EFORMAT, "malformed frame stream (the header walk breaks, or no subframe says a length)");
    const uint32_t stride = std::max(largest, 1u);
    const size_t per_frame = (size_t)channels * stride * (4 + (channels > 8 ? 4 : 0) + 2) + (size_t)channels * sizeof(GenericSubInfo) + sizeof(struct sela_hip_digest) + 64;
    DigestOp op{ per_frame, channels, stride, recurrence_form, digests };
    const int rc = frame_chunks(call, "digest", frames, frame_offsets, n_frames, op);
    if (rc == SELA_HIP_OK && track_crc32)
        *track_crc32 = op.crc;
    if (rc == SELA_HIP_OK && track_bytes)
        *track_bytes = op.bytes;
    return rc;
}

// The caller has walked the stream: the offsets never decrease, the largest samplesPerChannel fits the stride.
int generic_verify_i32(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride, const int32_t* samples,
    const uint32_t* lengths, uint32_t* diff_counts, uint32_t* first_diff, uint32_t* lossy_frames)
{
    const Call call;
    if (call.rc != SELA_HIP_OK)
        return call.rc;
    const size_t per_frame = (size_t)channels * stride * 12 + (size_t)channels * (sizeof(GenericSubInfo) + 8) + 64;
    return verify_chunks(call, "verify_i32", frames, frame_offsets, n_frames, per_frame, verify_i32_workspace_bytes,
        VerifySamples{ samples, lengths, channels, stride, nullptr, nullptr }, diff_counts, first_diff, lossy_frames);
}

// sela_hip_levels_i32.  The caller has walked the stream, as for generic_verify_i32.
int generic_levels_i32(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride, sela_hip_level32* levels)
{
    const Call call;
    if (call.rc != SELA_HIP_OK)
        return call.rc;
    const size_t per_frame = (size_t)channels * stride * 8 + (size_t)channels * (sizeof(GenericSubInfo) + 8 + sizeof(sela_hip_level32) * (1 + verify32_slices(stride))) + 64;
    return levels_chunks(call, "levels_i32", frames, frame_offsets, n_frames, channels, stride, channels, per_frame, levels_i32_workspace_bytes, judge_i32, levels,
        [=](const uint8_t* d_frames, const uint64_t* d_offsets, uint32_t cf, sela_hip_level32* d_levels, uint32_t* d_status, void* d_ws, int mode, hipStream_t st) {
            return launch_levels_i32_device(d_frames, d_offsets, cf, nullptr, channels, stride, d_levels, nullptr, d_status, d_ws, mode, st);
        });
}

// sela_hip_envelope_i32: generic_levels_i32's chunks at the caller's stride, ceil(stride / bucket) * channels
// records a frame (a longer frame is the status words' SELA_HIP_FLAG_STRIDE, judged like every other flag).  The caller has
// walked the stream.
int generic_envelope_i32(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride, uint32_t bucket,
    struct sela_hip_envelope32* env)
{
    const Call call;
    if (call.rc != SELA_HIP_OK)
        return call.rc;
    const uint32_t records = envelope_slots(stride, bucket) * channels; // (fits 32 bits: sela_hip_envelope_i32 refuses a shape where it does not)
    const size_t per_frame = (size_t)channels * stride * 8 + (size_t)channels * (sizeof(GenericSubInfo) + 8) + (size_t)records * sizeof(struct sela_hip_envelope32)
        + 8 * (size_t)verify32_slices(stride) + 64;
    return levels_chunks(call, "envelope_i32", frames, frame_offsets, n_frames, channels, stride, records, per_frame, envelope_i32_workspace_bytes, judge_i32, env,
        [=](const uint8_t* d_frames, const uint64_t* d_offsets, uint32_t cf, struct sela_hip_envelope32* d_env, uint32_t* d_status, void* d_ws, int mode, hipStream_t st) {
            return launch_envelope_i32_device(d_frames, d_offsets, cf, nullptr, channels, stride, bucket, d_env, nullptr, d_status, d_ws, mode, st);
        });
}

// sela_hip_decode_windows: the *_device launch on chunks of WINDOWS, on the calling thread's context and stream.
// Per chunk only the frames its windows touch go in (plan_windows: the distinct covering frames back to back, the descriptors
// on that compacted table; runs of neighbouring frames are gathered with one memcpy each, the whole with one copy); status
// (4 x u32) | window flags [cw] and the output come back behind the chunk's ONE wait.  The verdict is given at the end, on
// the flags of all chunks: the output and the flags are the caller's either way.
namespace {
thread_local uint64_t g_windows_staged_bytes = 0; // sela_hip_debug_windows_staged_bytes
}
void windows_staged_bytes_reset() { g_windows_staged_bytes = 0; }

int generic_decode_windows(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames_total, uint32_t channels, const sela_hip_window* windows,
    uint32_t n_windows, uint32_t window_samples, uint32_t format, void* out, uint32_t* window_flags, int recurrence_form, bool whole, bool wide, uint32_t sample_bits)
{
    const Call call;
    if (call.rc != SELA_HIP_OK)
        return call.rc;
    if (check_frame_offsets(frame_offsets, n_frames_total) != SELA_HIP_OK)
        return SELA_HIP_EFORMAT;
    Arena& g_arena = call.arena();
    const hipStream_t st = call.stream();
    // (wide, DESIGN.md 5.23: sela_hip_decode_windows_i32 -- the same plan and staging, launch_window32 and its formats behind; wide and
    // whole, 5.25: launch_window32_whole)
    const size_t out_per_window = (size_t)window_samples * channels * (wide ? (format == SELA_HIP_WINDOW_PCM24_INTERLEAVED ? 3 : 4) : format == SELA_HIP_WINDOW_F32_PLANAR ? 4 : 2);
    // (an estimate for the chunk's size only -- what a chunk needs is reserved exactly below: a 16-bit frame is about 5 bytes a sample at most)
    const size_t per_window = out_per_window + (size_t)(window_cover(window_samples) + (whole ? 2 : 0)) * channels * kBlock * (sizeof(int32_t) + 5) + 64;
    const uint32_t chunk = (uint32_t)std::max<size_t>(1, std::min<size_t>(n_windows, kChunkBudget / per_window));
    WindowPlan plan;
    std::vector<uint8_t> staged;
    std::vector<uint32_t> tail;
    uint32_t flags = 0;
    for (uint32_t w0 = 0; w0 < n_windows; w0 += chunk) {
        const uint32_t cw = std::min(chunk, n_windows - w0);
        if (whole)
            plan_windows_whole(frames, frame_offsets, n_frames_total, windows + w0, cw, window_samples, &plan);
        else
            plan_windows(frame_offsets, n_frames_total, windows + w0, cw, window_samples, &plan);
        const size_t in_bytes = (size_t)plan.staged_bytes(), n_staged = plan.frames.size(), out_bytes = (size_t)cw * out_per_window;
        const size_t ws_bytes = wide ? (whole ? window32_whole_workspace_bytes : window32_workspace_bytes)(cw, window_samples, channels, nullptr)
            : whole                   ? window_whole_workspace_bytes(cw, window_samples, channels)
                                      : window_workspace_bytes(cw, window_samples, channels);
        hipError_t e = g_arena.reserve(in_bytes + 8 + (n_staged + 1) * 8 + (size_t)cw * sizeof(sela_hip_window) + out_bytes + (4 + (size_t)cw) * 4 + ws_bytes + 8 * kPiece);
        if (e != hipSuccess)
            return report_hip_error(e, "decode_windows: scratch");
        uint8_t* d_frames = g_arena.take<uint8_t>(in_bytes + 8);
        uint64_t* d_offsets = g_arena.take<uint64_t>(n_staged + 1);
        sela_hip_window* d_windows = g_arena.take<sela_hip_window>(cw);
        uint8_t* d_out = g_arena.take<uint8_t>(out_bytes);
        uint32_t* d_tail = g_arena.take<uint32_t>(4 + (size_t)cw);
        uint8_t* d_ws = g_arena.take<uint8_t>(ws_bytes);
        if (!g_arena.fits())
            return report_error(SELA_HIP_ENOMEM, "decode_windows: internal scratch estimate too small");
        staged.resize(in_bytes);
        for (size_t i = 0; i < n_staged;) { // a run of neighbouring frames is one piece of the caller's stream
            size_t k = i + 1;
            while (k < n_staged && plan.frames[k] == plan.frames[k - 1] + 1)
                k++;
            if (plan.offsets[k] > plan.offsets[i])
                std::memcpy(staged.data() + plan.offsets[i], frames + frame_offsets[plan.frames[i]], (size_t)(plan.offsets[k] - plan.offsets[i]));
            i = k;
        }
        g_windows_staged_bytes += in_bytes;
        tail.assign(4 + (size_t)cw, 0);
        uint8_t* const user_out = static_cast<uint8_t*>(out) + (size_t)w0 * out_per_window;
        if (in_bytes)
            e = hipMemcpyAsync(d_frames, staged.data(), in_bytes, hipMemcpyHostToDevice, st);
        if (e == hipSuccess)
            e = hipMemcpyAsync(d_offsets, plan.offsets.data(), (n_staged + 1) * 8, hipMemcpyHostToDevice, st);
        if (e == hipSuccess)
            e = hipMemcpyAsync(d_windows, plan.windows.data(), (size_t)cw * sizeof(sela_hip_window), hipMemcpyHostToDevice, st);
        if (e == hipSuccess && wide)
            e = (whole ? launch_window32_whole : launch_window32)(d_frames, d_offsets, (uint32_t)n_staged, channels, d_windows, cw, window_samples, format, sample_bits,
                d_out, d_tail + 4, d_tail, d_ws, g_standard_first_mode.load(std::memory_order_relaxed) != 2, st);
        else if (e == hipSuccess)
            e = (whole ? launch_window_whole : launch_window_frames)(d_frames, d_offsets, (uint32_t)n_staged, channels, d_windows, cw, window_samples, format, d_out,
                d_tail + 4, d_tail, d_ws, st, recurrence_form, 0);
        if (e == hipSuccess)
            e = hipMemcpyAsync(tail.data(), d_tail, tail.size() * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess)
            e = hipMemcpyAsync(user_out, d_out, out_bytes, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess)
            e = hipStreamSynchronize(st);
        if (e != hipSuccess)
            return report_hip_error(e, "decode_windows");
        flags |= tail[0] | (tail[1] ? SELA_HIP_FLAG_BAD_FRAME : 0u);
        if (window_flags)
            std::memcpy(window_flags + w0, tail.data() + 4, (size_t)cw * 4);
    }
    // the fast route's verdict (sela_hip_decode_n_status_error, status[3] == 1) -- with the output and the flags already delivered
    return judge_decode(flags, SELA_HIP_FLAG_STRIDE | kJudgeJob, kRouteFast, "decode_windows");
}

int generic_lpc_encode(const int32_t* samples, uint32_t n_blocks, uint32_t n, int32_t* order_out, int32_t* q_out, int32_t* residues_out)
{
    const Call call;
    if (call.rc != SELA_HIP_OK)
        return call.rc;
    Arena& g_arena = call.arena();
    const size_t per_block = (size_t)n * 12 + kMaxOrder * 4 + sizeof(GenericMeta) + 16;
    const uint32_t chunk = (uint32_t)std::max<size_t>(1, std::min<size_t>(n_blocks, kChunkBudget / per_block));
    std::vector<GenericMeta> meta;
    const hipStream_t st = call.stream();
    for (uint32_t b0 = 0; b0 < n_blocks; b0 += chunk) {
        const uint32_t cb = std::min(chunk, n_blocks - b0);
        hipError_t e = g_arena.reserve((size_t)cb * per_block + 8 * kPiece);
        if (e != hipSuccess)
            return report_hip_error(e, "lpc_encode: scratch");
        int32_t* d_in = g_arena.take<int32_t>((size_t)cb * n);
        int32_t* d_sig = g_arena.take<int32_t>((size_t)cb * n);
        int32_t* d_res = g_arena.take<int32_t>((size_t)cb * n);
        int32_t* d_q = g_arena.take<int32_t>((size_t)cb * kMaxOrder);
        GenericMeta* d_meta = g_arena.take<GenericMeta>(cb);
        if (!g_arena.fits())
            return report_error(SELA_HIP_ENOMEM, "lpc_encode: internal scratch estimate too small");
        e = hipMemcpyAsync(d_in, samples + (size_t)b0 * n, (size_t)cb * n * 4, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) // a "frame" of one channel per block
            e = launch_generic_analyse(d_in, false, cb, 1, 1, n, d_sig, d_res, d_q, d_meta, st);
        meta.resize(cb);
        if (e == hipSuccess)
            e = hipMemcpyAsync(meta.data(), d_meta, (size_t)cb * sizeof(GenericMeta), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess)
            e = hipMemcpyAsync(q_out + (size_t)b0 * kMaxOrder, d_q, (size_t)cb * kMaxOrder * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess)
            e = hipMemcpyAsync(residues_out + (size_t)b0 * n, d_res, (size_t)cb * n * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess)
            e = hipStreamSynchronize(st);
        if (e != hipSuccess)
            return report_hip_error(e, "lpc_encode");
        uint32_t flags = 0;
        for (uint32_t i = 0; i < cb; i++) {
            order_out[b0 + i] = (int32_t)meta[i].order;
            flags |= meta[i].flags;
        }
        // (a residue beyond the zig-zag's range or a long Rice stream is the Rice stage's business, not this one's)
        const int rc = judge_encode(flags, SELA_HIP_FLAG_SHORT_BLOCK | SELA_HIP_FLAG_COEF_OVERFLOW, "lpc_encode");
        if (rc != SELA_HIP_OK)
            return rc;
    }
    return SELA_HIP_OK;
}

int generic_lpc_decode(const int32_t* order, const int32_t* q, const int32_t* residues, uint32_t n_blocks, uint32_t n, int32_t* samples_out, int64_t* coefs_out)
{
    const Call call;
    if (call.rc != SELA_HIP_OK)
        return call.rc;
    Arena& g_arena = call.arena();
    constexpr size_t kCoefs = kMaxOrder + 1;
    const hipStream_t st = call.stream();
    const size_t per_block = (size_t)n * 8 + kMaxOrder * 4 + 4 + kCoefs * 8;
    const uint32_t chunk = (uint32_t)std::max<size_t>(1, std::min<size_t>(n_blocks, kChunkBudget / per_block));
    for (uint32_t b0 = 0; b0 < n_blocks; b0 += chunk) {
        const uint32_t cb = std::min(chunk, n_blocks - b0);
        hipError_t e = g_arena.reserve((size_t)cb * per_block + 64 + 8 * kPiece);
        if (e != hipSuccess)
            return report_hip_error(e, "lpc_decode: scratch");
        int32_t* d_order = g_arena.take<int32_t>(cb);
        int32_t* d_q = g_arena.take<int32_t>((size_t)cb * kMaxOrder);
        int32_t* d_res = samples_out ? g_arena.take<int32_t>((size_t)cb * n) : nullptr;
        int32_t* d_out = samples_out ? g_arena.take<int32_t>((size_t)cb * n) : nullptr;
        int64_t* d_coefs = coefs_out ? g_arena.take<int64_t>((size_t)cb * kCoefs) : nullptr;
        uint32_t* d_status = g_arena.take<uint32_t>(4);
        if (!g_arena.fits())
            return report_error(SELA_HIP_ENOMEM, "lpc_decode: internal scratch estimate too small");
        e = hipMemcpyAsync(d_order, order + b0, (size_t)cb * 4, hipMemcpyHostToDevice, st);
        if (e == hipSuccess)
            e = hipMemcpyAsync(d_q, q + (size_t)b0 * kMaxOrder, (size_t)cb * kMaxOrder * 4, hipMemcpyHostToDevice, st);
        if (e == hipSuccess && d_res)
            e = hipMemcpyAsync(d_res, residues + (size_t)b0 * n, (size_t)cb * n * 4, hipMemcpyHostToDevice, st);
        if (e == hipSuccess)
            e = hipMemsetAsync(d_status, 0, 16, st);
        if (e == hipSuccess && d_coefs)
            e = hipMemsetAsync(d_coefs, 0, (size_t)cb * kCoefs * 8, st);
        if (e == hipSuccess)
            e = launch_lpc_decode_any(d_order, d_q, d_res, cb, n, d_out, d_coefs, d_status, st);
        uint32_t status[4] = {};
        if (e == hipSuccess)
            e = hipMemcpyAsync(status, d_status, 16, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && samples_out)
            e = hipMemcpyAsync(samples_out + (size_t)b0 * n, d_out, (size_t)cb * n * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && coefs_out)
            e = hipMemcpyAsync(coefs_out + (size_t)b0 * kCoefs, d_coefs, (size_t)cb * kCoefs * 8, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess)
            e = hipStreamSynchronize(st);
        if (e != hipSuccess)
            return report_hip_error(e, "lpc_decode");
        const int verdict = judge_decode(status[0], kJudgeLpc | SELA_HIP_FLAG_SHORT_BLOCK, kRouteLpc, "lpc_decode");
        if (verdict != SELA_HIP_OK)
            return verdict;
    }
    return SELA_HIP_OK;
}

// sela_hip_encode_pcm / sela_hip_decode_pcm: the device calls' launches (sela_capi_pcm.hip) on chunks of whole
// frames, on the calling thread's context and stream, past the coalescer.  What travels is the packed bytes: 3 per sample of a
// 24-bit container, not 4.  The chunks are sized by pcm_chunk (kChunkBudget of scratch, or sela_hip_debug_pcm_chunk_frames); the
// decode runs on frame_chunks (above).
//
// Per chunk ONE wait where the frames fit the estimate generic_encode sizes its own by (4.5 bytes a sample); a chunk that codes
// to more is encoded again into room of the size its offsets ask for.
int generic_encode_pcm(const uint8_t* pcm, uint32_t bytes_per_sample, uint32_t n_frames, uint32_t channels, uint32_t n, bool lossless, uint8_t* frames_out,
    size_t frames_cap, uint64_t* frame_offsets_out)
{
    const Call call;
    if (call.rc != SELA_HIP_OK)
        return call.rc;
    Arena& arena = call.arena();
    const hipStream_t st = call.stream();
    const size_t in_frame_bytes = (size_t)n * channels * bytes_per_sample;
    const size_t est_frame_bytes = ((size_t)n * channels * 9) / 2 + (size_t)channels * 192 + 64;
    const size_t per_frame = encode_pcm_workspace_bytes(1, channels, n) + in_frame_bytes + est_frame_bytes + 8;
    const uint32_t chunk = pcm_chunk(n_frames, per_frame);
    uint64_t base_bytes = 0;
    frame_offsets_out[0] = 0;
    std::vector<uint64_t> head;
    for (uint32_t f0 = 0; f0 < n_frames; f0 += chunk) {
        const uint32_t cf = std::min(chunk, n_frames - f0);
        const size_t ws_bytes = encode_pcm_workspace_bytes(cf, channels, n);
        const size_t head_words = 2 + (size_t)cf + 1; // status (4 x u32) | frame offsets
        head.assign(head_words, 0);
        size_t cap = (size_t)cf * est_frame_bytes;
        for (int attempt = 0; attempt < 2; attempt++) {
            hipError_t e = arena.reserve(cf * in_frame_bytes + head_words * 8 + cap + ws_bytes + 8 * kPiece);
            if (e != hipSuccess)
                return report_hip_error(e, "encode_pcm: scratch");
            uint8_t* d_in = arena.take<uint8_t>(cf * in_frame_bytes);
            uint64_t* d_head = arena.take<uint64_t>(head_words);
            uint8_t* d_frames = arena.take<uint8_t>(cap);
            uint8_t* d_ws = arena.take<uint8_t>(ws_bytes);
            if (!arena.fits())
                return report_error(SELA_HIP_ENOMEM, "encode_pcm: internal scratch estimate too small");
            e = hipMemcpyAsync(d_in, pcm + (size_t)f0 * in_frame_bytes, cf * in_frame_bytes, hipMemcpyHostToDevice, st);
            if (e == hipSuccess)
                e = launch_encode_pcm_device(d_in, bytes_per_sample, cf, channels, n, lossless, d_frames, cap, d_head + 2, reinterpret_cast<uint32_t*>(d_head), d_ws, st);
            if (e == hipSuccess)
                e = hipMemcpyAsync(head.data(), d_head, head_words * 8, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess)
                e = hipStreamSynchronize(st);
            if (e != hipSuccess)
                return report_hip_error(e, "encode_pcm");
            uint32_t status[4];
            std::memcpy(status, head.data(), 16);
            const int rc = judge_encode(status[0], kJudgeEncode, "encode_pcm");
            if (rc != SELA_HIP_OK)
                return rc;
            const uint64_t chunk_bytes = head[2 + cf];
            if (base_bytes + chunk_bytes > frames_cap)
                return report_error(SELA_HIP_ECAPACITY, "frames_out too small (see sela_hip_encode_pcm_bound_bytes)");
            if (status[1] == 0) {
                e = hipMemcpyAsync(frames_out + base_bytes, d_frames, (size_t)chunk_bytes, hipMemcpyDeviceToHost, st);
                if (e == hipSuccess)
                    e = hipStreamSynchronize(st);
                if (e != hipSuccess)
                    return report_hip_error(e, "encode_pcm: copy out");
                for (uint32_t i = 1; i <= cf; i++)
                    frame_offsets_out[f0 + i] = base_bytes + head[2 + i];
                base_bytes += chunk_bytes;
                break;
            }
            if (attempt == 1)
                return report_error(SELA_HIP_ENODEV, "encode_pcm: a chunk did not fit the room its own offsets asked for");
            cap = (size_t)chunk_bytes; // (rare: more than 4.5 bytes a sample)
        }
    }
    return SELA_HIP_OK;
}

// sela_hip_decode_pcm on frame_chunks: nothing uploaded beside the frames; the chunk's packed PCM | status (4 x u32), read back in
// two pieces, the PCM straight into the caller's at the chunk's sample offset.
namespace {
struct DecodePcmOp {
    size_t per_frame;
    const uint64_t* sample_offsets;
    uint32_t channels, stride, bytes_per_sample;
    uint8_t* pcm_out;
    uint32_t* wide_samples;
    uint8_t* d_out = nullptr;
    uint32_t* d_status = nullptr;
    uint32_t status[4] = {};
    size_t value_bytes() const { return (size_t)channels * bytes_per_sample; }
    size_t workspace_bytes(uint32_t cf) const { return decode_pcm_workspace_bytes(cf, channels, stride); }
    void pieces(Carve& c, uint32_t, uint32_t cf)
    {
        d_out = piece<uint8_t>(c, (uint64_t)cf * stride * value_bytes());
        d_status = piece<uint32_t>(c, 4);
    }
    hipError_t submit(const uint8_t* d_frames, const uint64_t* d_offsets, uint32_t f0, uint32_t cf, void* d_ws, int mode, hipStream_t st)
    {
        const size_t out_bytes = (size_t)(sample_offsets[f0 + cf] - sample_offsets[f0]) * value_bytes();
        hipError_t e = launch_decode_pcm_device(d_frames, d_offsets, cf, channels, stride, bytes_per_sample, d_out, nullptr, d_status, d_ws, mode, st);
        if (e == hipSuccess)
            e = hipMemcpyAsync(status, d_status, 16, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && out_bytes)
            e = hipMemcpyAsync(pcm_out + (size_t)sample_offsets[f0] * value_bytes(), d_out, out_bytes, hipMemcpyDeviceToHost, st);
        return e;
    }
    int finish(uint32_t, uint32_t) const
    {
        const int rc = sela_hip_decode_pcm_status_error(status);
        if (rc == SELA_HIP_OK && wide_samples)
            *wide_samples += status[3];
        return rc;
    }
};
} // namespace

// The caller has walked the stream: the offsets never decrease, stride is the largest samplesPerChannel, sample_offsets the walk's.
int generic_decode_pcm(const uint8_t* frames, const uint64_t* frame_offsets, const uint64_t* sample_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride,
    uint32_t bytes_per_sample, uint8_t* pcm_out, uint32_t* wide_samples)
{
    const Call call;
    if (call.rc != SELA_HIP_OK)
        return call.rc;
    const size_t per_frame = decode_pcm_workspace_bytes(1, channels, stride) + (size_t)stride * channels * bytes_per_sample + 16;
    DecodePcmOp op{ per_frame, sample_offsets, channels, stride, bytes_per_sample, pcm_out, wide_samples };
    return frame_chunks(call, "decode_pcm", frames, frame_offsets, n_frames, op);
}

// sela_hip_digest_pcm: generic_levels_i32's chunks with DigestOp's outputs.  Per chunk status (4 x u32) | the two
// track words | the records come back; the chunk's track word joins the call's by crc_combine, its status[3] the count of samples
// beyond a 3-byte container.  The caller has walked the stream, as for generic_levels_i32.
namespace {
struct DigestPcmOp {
    size_t per_frame;
    uint32_t channels, stride, bytes_per_sample;
    struct sela_hip_digest* digests; // or null
    uint32_t crc = 0, wide = 0;
    uint64_t bytes = 0;
    uint32_t* d_status = nullptr;
    uint64_t* d_track = nullptr;
    struct sela_hip_digest* d_digests = nullptr;
    uint32_t status[4] = { 0, 0, 0, 0 };
    uint64_t track[2] = { 0, 0 };
    size_t workspace_bytes(uint32_t cf) const { return digest_pcm_workspace_bytes(cf, channels, stride); }
    void pieces(Carve& c, uint32_t, uint32_t cf)
    {
        d_status = piece<uint32_t>(c, 4);
        d_track = piece<uint64_t>(c, 2);
        d_digests = piece<struct sela_hip_digest>(c, cf);
    }
    hipError_t submit(const uint8_t* d_frames, const uint64_t* d_offsets, uint32_t f0, uint32_t cf, void* d_ws, int mode, hipStream_t st)
    {
        hipError_t e = launch_digest_pcm_device(d_frames, d_offsets, cf, nullptr, channels, stride, bytes_per_sample, d_digests, d_track, nullptr, d_status, d_ws, mode, st);
        if (e == hipSuccess)
            e = hipMemcpyAsync(status, d_status, sizeof(status), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess)
            e = hipMemcpyAsync(track, d_track, sizeof(track), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && digests)
            e = hipMemcpyAsync(digests + f0, d_digests, (size_t)cf * sizeof(struct sela_hip_digest), hipMemcpyDeviceToHost, st);
        return e;
    }
    int finish(uint32_t, uint32_t)
    {
        const int rc = sela_hip_decode_pcm_status_error(status);
        if (rc != SELA_HIP_OK)
            return rc;
        crc = crc_combine(crc, (uint32_t)track[0], track[1]);
        bytes += track[1];
        wide += status[3];
        return SELA_HIP_OK;
    }
};
} // namespace

int generic_digest_pcm(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride, uint32_t bytes_per_sample,
    struct sela_hip_digest* digests, uint32_t* track_crc32, uint64_t* track_bytes, uint32_t* wide_samples)
{
    const Call call;
    if (call.rc != SELA_HIP_OK)
        return call.rc;
    const size_t per_frame = (size_t)channels * stride * 8 + (size_t)channels * (sizeof(GenericSubInfo) + 8) + (size_t)verify_pcm_tiles(stride, channels) * 8
        + sizeof(struct sela_hip_digest) + 64;
    DigestPcmOp op{ per_frame, channels, stride, bytes_per_sample, digests };
    const int rc = frame_chunks(call, "digest_pcm", frames, frame_offsets, n_frames, op);
    if (rc == SELA_HIP_OK && track_crc32)
        *track_crc32 = op.crc;
    if (rc == SELA_HIP_OK && track_bytes)
        *track_bytes = op.bytes;
    if (rc == SELA_HIP_OK && wide_samples)
        *wide_samples = op.wide;
    return rc;
}

// sela_hip_verify_pcm: verify_chunks on the packed original.
int generic_verify_pcm(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t bytes_per_sample, const uint8_t* pcm,
    uint64_t pcm_samples, uint32_t* diff_counts, uint32_t* first_diff, uint32_t* lossy_frames)
{
    const Call call;
    if (call.rc != SELA_HIP_OK)
        return call.rc;
    std::vector<uint64_t> sample_offsets((size_t)n_frames + 1);
    const uint32_t stride = std::max(generic_index_samples(frames, frame_offsets, n_frames, channels, sample_offsets.data(), nullptr), 1u);
    const size_t per_frame = (size_t)channels * stride * (8 + bytes_per_sample) + (size_t)channels * (sizeof(GenericSubInfo) + 8) + (size_t)verify_pcm_tiles(stride, channels) * 8 + 64;
    return verify_chunks(call, "verify_pcm", frames, frame_offsets, n_frames, per_frame, verify_pcm_workspace_bytes,
        VerifyPacked{ pcm, pcm_samples, sample_offsets.data(), channels, stride, bytes_per_sample, nullptr, 0 }, diff_counts, first_diff, lossy_frames);
}

} // namespace sela

extern "C" void sela_hip_debug_pcm_chunk_frames(uint32_t frames) { sela::g_pcm_chunk_frames.store(frames, std::memory_order_relaxed); }

extern "C" {
void sela_hip_debug_standard_first(int mode) { g_standard_first_mode.store(mode, std::memory_order_relaxed); }
int sela_hip_debug_standard_chunks(void) { return g_standard_chunks.load(std::memory_order_relaxed); }
long long sela_hip_debug_segment_subframes(void) { return g_segment_subframes.load(std::memory_order_relaxed); }
void sela_hip_debug_generic_wrap_taps(int on) { sela::set_generic_wrap_taps(on); }
}

extern "C" uint64_t sela_hip_debug_windows_staged_bytes(void) { return sela::g_windows_staged_bytes; }
