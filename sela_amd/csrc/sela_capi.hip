// sela_capi.hip -- the extern "C" boundary of libsela_hip.so (declared in include/sela_hip.h).
//
// Plain pointers and sizes only.  The *_device entry points enqueue kernels on the caller's stream;
// the host-pointer entry points (one-shot and streaming jobs) stage through a per-thread, grow-only set
// of device buffers.  There is no CPU fallback anywhere: without a HIP device every call fails with
// SELA_HIP_ENODEV.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>

#include <chrono>
#include <condition_variable>
#include <deque>
#include <thread>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "sela_coalescer.h"
#include "sela_crc32.h"
#include "sela_decode_whole_plan.h"
#include "sela_host.h"
#include "sela_lease.h"
#include "sela_pcm.h"
#include "sela_salvage_walk.h"
#include "sela_salvage_walk_unaligned.h"

namespace {

thread_local std::string g_error;

int fail(int code, const std::string& what)
{
    g_error = what;
    return code;
}

int fail_hip(hipError_t e, const char* where)
{
    return fail(e == hipErrorOutOfMemory ? SELA_HIP_ENOMEM : SELA_HIP_ENODEV, std::string(where) + ": " + hipGetErrorString(e));
}

// ---- the verdicts on what the kernels report (sela_host.h): one ordered table per direction ---------------------------------------
struct Verdict {
    uint32_t flag;
    uint32_t routes; // the decoder's routes (1 << sela::DecodeRoute) this row speaks for
    int code;
    bool named; // the text opens with the caller's name
    const char* text;
};
constexpr uint32_t kEveryRoute = ~0u, kLpcOnly = 1u << sela::kRouteLpc;
// What the reference itself leaves undefined (COEF_OVERFLOW, Q_RANGE, SHORT_BLOCK) is reported, never decoded silently.
const Verdict kDecodeVerdicts[] = {
    { SELA_HIP_FLAG_STRIDE, kEveryRoute, SELA_HIP_ECAPACITY, false, "stride is smaller than the largest samplesPerChannel of the stream (status[2])" },
    { SELA_HIP_FLAG_BAD_FRAME, 1u << sela::kRouteDevice32, SELA_HIP_EFORMAT, false,
        "malformed frame (decreasing offsets, sync word, sizes, an order above 100, a Rice parameter above 31, a channel or parent that does not exist, or channels of different lengths)" },
    { SELA_HIP_FLAG_BAD_FRAME, 1u << sela::kRouteHost32, SELA_HIP_EFORMAT, false,
        "malformed frame (sync word, sizes, an order above 100, a Rice parameter above 31, a channel or parent that does not exist, or channels of different lengths)" },
    { SELA_HIP_FLAG_BAD_FRAME, 1u << sela::kRouteFast, SELA_HIP_EFORMAT, false, "malformed frame stream (bad sync word or subframe header)" },
    { SELA_HIP_FLAG_BAD_FRAME, 1u << sela::kRouteWalk, SELA_HIP_EFORMAT, false,
        "malformed frame stream (the header walk breaks, frame offsets decrease, or no subframe says a length)" },
    { SELA_HIP_FLAG_BAD_FRAME, kLpcOnly, SELA_HIP_EINVAL, true, "order outside 0..100" },
    { SELA_HIP_FLAG_RICE_OVERRUN, kEveryRoute, SELA_HIP_EFORMAT, false, "a Rice stream ended before all its values were read" },
    { SELA_HIP_FLAG_COEF_OVERFLOW, kEveryRoute, SELA_HIP_ERANGE, true, "a predictor coefficient left the int64 range" },
    { SELA_HIP_FLAG_Q_RANGE, kEveryRoute, SELA_HIP_ERANGE, true,
        "a quantised reflection coefficient outside [-64, 63] (the reference indexes past its tables, src/lpc/linear_predictor.cpp:23-26)" },
    { SELA_HIP_FLAG_SHORT_BLOCK, ~kLpcOnly, SELA_HIP_ERANGE, true,
        "a subframe without samples or not longer than its predictor order (the reference writes past its vector, src/lpc/sample_generator.cpp:14-22)" },
    { SELA_HIP_FLAG_SHORT_BLOCK, kLpcOnly, SELA_HIP_ERANGE, true,
        "a block without samples or not longer than its predictor order (the reference writes past its vector, src/lpc/sample_generator.cpp:14-22)" },
    { SELA_HIP_FLAG_INTERNAL, kEveryRoute, SELA_HIP_ENODEV, true, "a bounded wait inside a kernel ran out" },
};
const Verdict kEncodeVerdicts[] = {
    { SELA_HIP_FLAG_SHORT_BLOCK, kEveryRoute, SELA_HIP_ERANGE, true,
        "a block is not longer than its predictor order (the reference reads past its vector there, src/lpc/residue_generator.cpp:104-110)" },
    { SELA_HIP_FLAG_RICE_RANGE, kEveryRoute, SELA_HIP_ERANGE, true, "a residue is beyond the reference's int32 zig-zag (|value| >= 2^30)" },
    { SELA_HIP_FLAG_COEF_OVERFLOW, kEveryRoute, SELA_HIP_ERANGE, true, "a predictor coefficient left the int64 range" },
    { SELA_HIP_FLAG_WORDS_CAP, kEveryRoute, SELA_HIP_ERANGE, true, "a Rice stream needs more words than a subframe's 16-bit count can say" },
};
template <size_t N>
int judge(const Verdict (&table)[N], uint32_t flags, uint32_t route, const char* who)
{
    for (const Verdict& v : table)
        if ((flags & v.flag) && (v.routes & route))
            return fail(v.code, v.named ? std::string(who) + ": " + v.text : std::string(v.text));
    return SELA_HIP_OK;
}

} // namespace
namespace sela {
int report_error(int code, const std::string& what) { return fail(code, what); }
int report_hip_error(hipError_t e, const char* where) { return fail_hip(e, where); }
int device_ready()
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(SELA_HIP_ENODEV, "no HIP device visible (the SELA MI355X path has no CPU fallback)");
    return SELA_HIP_OK;
}
int check_frame_offsets(const uint64_t* frame_offsets, uint32_t n_frames)
{
    return frame_offsets_ascend(frame_offsets, n_frames) ? SELA_HIP_OK : fail(SELA_HIP_EFORMAT, "frame offsets must not decrease");
}
int judge_decode(uint32_t flags, uint32_t judged, DecodeRoute route, const char* who) { return judge(kDecodeVerdicts, flags & judged, 1u << route, who); }
int judge_encode(uint32_t flags, uint32_t judged, const char* who) { return judge(kEncodeVerdicts, flags & judged, kEveryRoute, who); }
} // namespace sela
namespace {

// ---- page-locked host memory (sela_hip_host_alloc) ---------------------------------------------------------
// Copies from and to pageable memory go through the runtime's own staging and block the calling thread;
// from page-locked memory hipMemcpyAsync really is asynchronous, which is what the chunk pipeline below
// needs.  Pinning is slow (page by page), so freed blocks are kept and handed out again.
struct PinnedPool {
    struct Block {
        void* ptr;
        size_t cap;
        bool pinned;
    };
    std::mutex mu;
    std::vector<Block> live, idle;
    size_t idle_bytes = 0;
    static constexpr size_t kIdleCap = (size_t)1 << 30; // blocks kept for reuse beyond this are unpinned and freed, oldest first

    void* take(size_t bytes)
    {
        std::lock_guard<std::mutex> lock(mu);
        size_t best = idle.size();
        for (size_t i = 0; i < idle.size(); i++)
            if (idle[i].cap >= bytes && idle[i].cap <= 2 * bytes + 4096 && (best == idle.size() || idle[i].cap < idle[best].cap))
                best = i;
        Block b;
        if (best != idle.size()) {
            b = idle[best];
            idle.erase(idle.begin() + (std::ptrdiff_t)best);
            idle_bytes -= b.cap;
        } else {
            b.cap = (bytes + 4095) & ~(size_t)4095;
            b.ptr = nullptr;
            // (portable + mapped: one worker's kernels read and write these blocks from whichever device it is bound to)
            b.pinned = hipHostMalloc(&b.ptr, b.cap, hipHostMallocPortable | hipHostMallocMapped) == hipSuccess && b.ptr;
            if (!b.pinned) { // no device (CPU-only container code still runs): ordinary memory
                (void)hipGetLastError();
                b.ptr = std::aligned_alloc(4096, b.cap);
                if (!b.ptr)
                    return nullptr;
            }
        }
        live.push_back(b);
        return b.ptr;
    }
    void give(void* p)
    {
        std::lock_guard<std::mutex> lock(mu);
        for (size_t i = 0; i < live.size(); i++)
            if (live[i].ptr == p) {
                idle.push_back(live[i]);
                idle_bytes += live[i].cap;
                live.erase(live.begin() + (std::ptrdiff_t)i);
                while (idle_bytes > kIdleCap && idle.size() > 1) { // (the block just returned stays: it is the likeliest to be asked for again)
                    const Block old = idle.front();
                    idle.erase(idle.begin());
                    idle_bytes -= old.cap;
                    if (old.pinned)
                        (void)hipHostFree(old.ptr);
                    else
                        std::free(old.ptr);
                }
                return;
            }
    }
    void trim()
    {
        std::lock_guard<std::mutex> lock(mu);
        for (Block& b : idle) {
            if (b.pinned)
                (void)hipHostFree(b.ptr);
            else
                std::free(b.ptr);
        }
        idle.clear();
        idle_bytes = 0;
    }
};
PinnedPool& pool()
{
    static PinnedPool* p = new PinnedPool; // (never destroyed: the HIP runtime may already be gone at exit)
    return *p;
}

// Grow-only device scratch used by the host-pointer API (one set per calling thread).
struct DeviceBuffer {
    void* ptr = nullptr;
    size_t cap = 0;
    hipError_t reserve(size_t bytes)
    {
        if (bytes <= cap)
            return hipSuccess;
        if (ptr)
            (void)hipFree(ptr);
        ptr = nullptr;
        cap = 0;
        const size_t want = bytes + bytes / 4 + 4096;
        hipError_t e = hipMalloc(&ptr, want);
        if (e == hipSuccess)
            cap = want;
        return e;
    }
    void release()
    {
        if (ptr)
            (void)hipFree(ptr);
        ptr = nullptr;
        cap = 0;
    }
};
// page-locked host scratch owned by the library (frame offsets on their way in or out)
struct HostBuffer {
    void* ptr = nullptr;
    size_t cap = 0;
    hipError_t reserve(size_t bytes)
    {
        if (bytes <= cap)
            return hipSuccess;
        release();
        const size_t want = bytes + bytes / 4 + 4096;
        hipError_t e = hipHostMalloc(&ptr, want, hipHostMallocPortable | hipHostMallocMapped);
        if (e == hipSuccess) {
            cap = want;
            std::memset(ptr, 0, want); // (tickets and flags the device leaves here are compared with what was there before)
        } else
            ptr = nullptr;
        return e;
    }
    void release()
    {
        if (ptr)
            (void)hipHostFree(ptr);
        ptr = nullptr;
        cap = 0;
    }
};

// Host-pointer decodes run as a chunked pipeline (encodes: see job_feed_encode_launch): the copy-in of every chunk is queued, in order
// on one stream, as soon as the chunk is fed (kSets chunks deep); the kernels of consecutive chunks alternate
// between streams (a chunk of this size leaves the device in its launch tail for a good part of its run time, so
// neighbours overlap); a chunk is copied out as soon as its kernels have finished.  Nothing in the issue path
// waits for the device until a buffer set comes round again.
constexpr uint32_t kHostChunkFrames = 1024; // (for up to eight channels, see chunk_frames())
constexpr uint32_t kSets = 8;
constexpr uint32_t kRunStreams = 2;

struct ChunkSet { // one chunk of a decode job in flight
    DeviceBuffer pcm, frames, workspace;
    hipEvent_t copied_in = nullptr, ran = nullptr, copied_out = nullptr;
};

struct HostContext : sela::CurrentDevice {
    ChunkSet set[kSets];
    DeviceBuffer status;      // device-side status words (decode kernels of a job report through job_flags instead)
    // encode jobs: one launch per feed (see job_feed_encode)
    DeviceBuffer enc_pcm, enc_workspace, enc_ready, enc_words; // enc_words: the job's stream position (two cells in turn), 4 status words, the stagers' four words (EncodeHostLink::stage_started)
    hipEvent_t enc_prev = nullptr; // behind the newest work on the encode stream
    HostBuffer enc_mirror;                                     // page-locked: offsets + status per feed
    uint64_t* enc_mirror_mapped = nullptr;
    HostBuffer job_offsets_host; // decode: the frame offsets of every feed of the running job, where the kernels read them
    HostBuffer job_flags;     // decode: one byte per (frame, wave), zeroed by the host, written by the kernels (over the link) on errors only
    const uint64_t* job_offsets_mapped = nullptr; // device addresses of the two host buffers
    uint8_t* job_flags_mapped = nullptr;
    hipStream_t s_in = nullptr, s_out = nullptr, s_run[kRunStreams] = { nullptr, nullptr };
    int device = -1;
    bool job_open = false;
    int staged_device = -1; // the device whose staging path this context's open job holds (staged_path_acquire), or -1
    // the buffers belong to the device that was current when they were allocated
    bool bind_current_device()
    {
        int dev = -1;
        if (hipGetDevice(&dev) != hipSuccess)
            return false;
        if (dev != device) {
            release();
            device = dev;
        }
        return true;
    }
    // Four streams, because the runtime multiplexes streams onto four hardware queues and two streams on one queue
    // serialise (an event record of one sits in front of the other's kernels).  Encode jobs use them as copy-in,
    // two kernel streams and copy-out; decode jobs as copy-in and three kernel + copy-out streams.
    hipError_t streams()
    {
        hipError_t e = hipSuccess;
        for (hipStream_t* s : { &s_in, &s_run[0], &s_run[1], &s_out })
            if (!*s && (e = hipStreamCreateWithFlags(s, hipStreamNonBlocking)) != hipSuccess)
                return e;
        for (ChunkSet& c : set)
            for (hipEvent_t* ev : { &c.copied_in, &c.ran, &c.copied_out })
                if (!*ev && (e = hipEventCreateWithFlags(ev, hipEventDisableTiming)) != hipSuccess)
                    return e;
        if (!enc_prev)
            e = hipEventCreateWithFlags(&enc_prev, hipEventDisableTiming);
        return e;
    }
    // decode: a chunk's kernel and copy-out share a stream, three streams in turn (the fourth copies in)
    hipStream_t decode_stream(uint32_t chunk) const
    {
        const hipStream_t run[3] = { s_run[0], s_run[1], s_out };
        return run[chunk % 3];
    }
    void sync_all()
    {
        for (hipStream_t s : { s_in, s_out, s_run[0], s_run[1] })
            if (s)
                (void)hipStreamSynchronize(s);
    }
    void release()
    {
        for (ChunkSet& c : set) {
            c.pcm.release();
            c.frames.release();
            c.workspace.release();
            for (hipEvent_t* ev : { &c.copied_in, &c.ran, &c.copied_out }) {
                if (*ev)
                    (void)hipEventDestroy(*ev);
                *ev = nullptr;
            }
        }
        status.release();
        if (enc_prev)
            (void)hipEventDestroy(enc_prev);
        enc_prev = nullptr;
        enc_pcm.release();
        enc_workspace.release();
        enc_ready.release();
        enc_words.release();
        enc_mirror.release();
        job_offsets_host.release();
        job_flags.release();
        for (hipStream_t* s : { &s_in, &s_out, &s_run[0], &s_run[1] }) {
            if (*s)
                (void)hipStreamDestroy(*s);
            *s = nullptr;
        }
    }
    // what the lease asks of it (sela_lease.h)
    static constexpr size_t kParked = 16; // more idle ones than this are freed instead (a context holds up to a few hundred MB of HBM)
    static HostContext* make(int dev);
    bool serves(int) const { return true; } // (a thread keeps its context when it changes device: bind_current_device)
    void tidy();
    void destroy() { release(); }
};
// A thread's context is LEASED (sela_lease.h): creating one (four streams, 25 events, a dozen device and page-locked buffers)
// takes the runtime about 10 ms -- three times what a 3-minute track takes file to file.
std::atomic<int> g_contexts_created{ 0 }; // debug: sela_hip_debug_contexts_created
void staged_path_release(int device);     // (below)

HostContext* HostContext::make(int)
{
    g_contexts_created.fetch_add(1, std::memory_order_relaxed);
    return new HostContext; // (bound to the device, and filled, by the job that begins on it)
}
void HostContext::tidy()
{
    if (!job_open)
        return;
    // a thread that ended in the middle of a job: nothing of it may be left in flight or marked
    sync_all();
    release();
    job_open = false;
    if (staged_device >= 0) // (its job held the device's staging path: nobody else will give it back)
        staged_path_release(staged_device);
    staged_device = -1;
}
thread_local sela::ContextLease<HostContext> g_lease;
inline HostContext& ctx() { return g_lease.held ? *g_lease.held : *g_lease.get(HostContext::current_device()); }

// Per-thread kernel timing (bench.py's roofline leg): events bracketing the kernels of the last call.
struct KernelTiming {
    bool enabled = false;
    hipEvent_t ev[4] = { nullptr, nullptr, nullptr, nullptr };
    int recorded = 0; // number of kernels bracketed by the last call
    hipEvent_t* events()
    {
        if (!enabled)
            return nullptr;
        for (auto& e : ev)
            if (!e && hipEventCreate(&e) != hipSuccess)
                return nullptr;
        return ev;
    }
};
thread_local KernelTiming g_timing;
thread_local uint64_t* g_phase_cycles = nullptr; // debug: per-block phase cycle counts (sela_hip_debug_phase_buffer)
thread_local int g_force_plain_fir = 0;          // debug: sela_hip_debug_force_plain_fir
thread_local int g_self_blocks = -1;             // debug: sela_hip_debug_mean_workers
thread_local int g_team_lanes = -1;              // debug: sela_hip_debug_encode_teams
thread_local int g_fused_device = 0;             // debug: sela_hip_debug_encode_fused
thread_local int g_stage_wait_naps = -1;         // debug: sela_hip_debug_stage_wait
thread_local int g_reissued_feeds = 0;           // debug: sela_hip_debug_reissued_feeds
thread_local int g_recurrence_form = -1;         // debug: sela_hip_debug_decode_recurrence

// The staging kernel asks for whole CUs and the blocks that wait for it never leave theirs: two jobs staging on one
// device at once (two host threads on one GPU) can keep each other's stagers off the device until the bounded waits run
// out.  So one job per device stages at a time; a job that finds the path taken uses the copy engine instead.
std::mutex g_staged_mu;
bool g_staged_busy[64] = {};
bool staged_path_acquire(int device)
{
    if (device < 0 || device >= 64)
        return false;
    std::lock_guard<std::mutex> lock(g_staged_mu);
    if (g_staged_busy[device])
        return false;
    g_staged_busy[device] = true;
    return true;
}
void staged_path_release(int device)
{
    if (device < 0 || device >= 64)
        return;
    std::lock_guard<std::mutex> lock(g_staged_mu);
    g_staged_busy[device] = false;
}

// Frames per decode chunk: kHostChunkFrames for up to eight channels; beyond that a chunk keeps about the bytes of
// 1024 eight-channel frames (a 255-channel frame is 1 MB of PCM: chunks are sized by what they move, and the chunk
// buffers -- PCM and the generic-mode workspace of every set -- by the chunk).
uint32_t chunk_frames(uint32_t channels)
{
    return channels <= 8 ? kHostChunkFrames : std::max(16u, kHostChunkFrames * 8 / channels);
}
// Size of chunk number `index` of a decode job that has `available` frames at hand.  It opens with two shorter
// chunks: its copy-outs run back to back from the moment the first chunk is done, so the job is as long as the way
// to that moment plus the bare copy of the PCM -- provided every later chunk is decoded by the time the copy-out
// before it ends, which is what keeps the first chunks from being shorter still.
uint32_t next_chunk_frames(uint32_t index, uint32_t available, uint32_t channels)
{
    const uint32_t full = chunk_frames(channels);
    uint32_t want = full;
    if (index < 2)
        want = std::min<uint32_t>(want, std::max(8u, (index ? 640u : 384u) * full / kHostChunkFrames));
    if (want < available && available - want < want / 4) // (no stub of a last chunk: split what is left in two)
        want = (available + 1) / 2;
    return want < available ? want : available;
}

uint32_t flags_to_error(uint32_t flags)
{
    return flags & (SELA_HIP_FLAG_WORDS_CAP | SELA_HIP_FLAG_RICE_RANGE | SELA_HIP_FLAG_COEF_OVERFLOW);
}

} // namespace

// ---- streaming jobs ----------------------------------------------------------------------------------------
struct EncodeFeed {      // one feed of an encode job = one launch
    uint32_t first = 0, n_frames = 0;
    size_t mirror_at = 0;        // where the launch reports (offsets, status) in ctx().enc_mirror
    hipEvent_t done = nullptr;   // recorded behind the launch
    void* bounce_in = nullptr;   // page-locked copy of a feed that came from ordinary memory
    const int16_t* host_src = nullptr;   // the feed's PCM in page-locked host memory, as the host sees it ...
    const int16_t* mapped_src = nullptr; // ... and as the device sees it
    bool reissued = false;       // went through the copy-engine path a second time (see job_reissue_encode)
};

struct sela_hip_job {
    bool encode = false;
    bool lossless = false; // encode: SELA_HIP_ENCODE_LOSSLESS (sela_hip_encode_begin_opt), for every feed
    uint32_t channels = 0, total_frames = 0;
    uint32_t fed = 0;      // frames handed to feed() so far
    int error = SELA_HIP_OK;
    // ---- decode: chunks
    uint32_t issued = 0;       // chunks whose copies and kernel are enqueued
    uint32_t final_chunks = 0; // chunks whose results are complete in host memory
    std::vector<uint32_t> chunk_first, chunk_frames; // per issued chunk
    int16_t* pcm_out = nullptr;   // where the copy-outs land: the caller's buffer if it is page-locked, else a page-locked bounce buffer
    int16_t* pcm_caller = nullptr; // the caller's buffer
    bool pcm_bounce = false;
    uint32_t frames_moved = 0;     // frames copied from the bounce buffer to the caller's so far
    std::vector<void*> bounce_frames; // page-locked copies of feeds that came from ordinary memory
    size_t offsets_used = 0; // entries of ctx().job_offsets_host taken by the feeds so far
    // ---- encode: feeds
    uint8_t* frames_out = nullptr; // the caller's buffer
    size_t frames_cap = 0;
    uint64_t* offsets_out = nullptr;
    uint8_t* out_host = nullptr;   // where the kernels' stores land as the host sees it: frames_out, or a page-locked bounce buffer
    uint8_t* out_mapped = nullptr; // ... as the device sees it
    bool out_bounce = false;
    std::vector<EncodeFeed> feeds;
    size_t mirror_used = 0;
    bool staged = false;      // this job's feeds have their PCM fetched by the staging kernel (one such job per device at a time)
    bool holds_staged_path = false; // (taken at begin, given back at end -- also by a job that fell back to the copy engine on the way)
    uint32_t feeds_final = 0; // feeds whose launch has finished: their bytes and offsets are complete in host memory
    uint32_t frames_final = 0;
    uint64_t bytes_final = 0, bytes_copied = 0; // (bytes_copied: bounce buffer -> frames_out)
};

namespace {

int job_fail(sela_hip_job* job, int code)
{
    if (job->error == SELA_HIP_OK)
        job->error = code;
    return code;
}

// Decode into ordinary memory: the chunks that have arrived in the page-locked bounce buffer go on to the caller's.
void job_move_decoded(sela_hip_job* job)
{
    if (!job->pcm_bounce || job->final_chunks == 0)
        return;
    const uint32_t n = job->final_chunks;
    const uint32_t frames = job->chunk_first[n - 1] + job->chunk_frames[n - 1];
    if (frames > job->frames_moved) {
        const size_t frame_samples = (size_t)sela::kBlock * job->channels;
        std::memcpy(job->pcm_caller + job->frames_moved * frame_samples, job->pcm_out + job->frames_moved * frame_samples,
            (size_t)(frames - job->frames_moved) * frame_samples * sizeof(int16_t));
        job->frames_moved = frames;
    }
}

// Results of decode chunk `i` are in host memory once its copy-out has finished.
int job_finalize(sela_hip_job* job, uint32_t upto /* chunks */)
{
    while (job->final_chunks < upto) {
        ChunkSet& c = ctx().set[job->final_chunks % kSets];
        // (chunk i and chunk i + kSets share the event; waiting for the later record covers the earlier one)
        hipError_t e = hipEventSynchronize(c.copied_out);
        if (e != hipSuccess)
            return job_fail(job, fail_hip(e, "copy-out"));
        job->final_chunks++;
    }
    job_move_decoded(job);
    return SELA_HIP_OK;
}

hipError_t reserve_chunk_buffers(uint32_t channels)
{
    const size_t frame_pcm = (size_t)sela::kBlock * channels * sizeof(int16_t);
    const uint32_t frames = chunk_frames(channels);
    for (ChunkSet& c : ctx().set) {
        hipError_t e;
        if ((e = c.pcm.reserve(frames * frame_pcm + 16)) != hipSuccess
            || (e = c.workspace.reserve(sela::decode_workspace_bytes(frames, channels))) != hipSuccess)
            return e;
    }
    return hipSuccess;
}

// The address the device uses for page-locked host memory, or null for ordinary (pageable) memory.
void* device_view(const void* host)
{
    hipPointerAttribute_t attr;
    void* dev = nullptr;
    if (host && hipPointerGetAttributes(&attr, host) == hipSuccess && attr.type == hipMemoryTypeHost
        && hipHostGetDevicePointer(&dev, const_cast<void*>(host), 0) == hipSuccess)
        return dev;
    (void)hipGetLastError(); // (not an error: the caller falls back to a bounce buffer)
    return nullptr;
}

// ---- encode jobs ---------------------------------------------------------------------------------------------------
// One feed = one launch of k_encode_blocks (and, beside it on the copy-in stream, of k_stage_in, whose workgroups fetch
// the feed's PCM from page-locked host memory frame by frame): the blocks encode each frame as it lands, and the last
// block of every group of frames (kGroupFrames) writes the group's finished bytes straight to their place in frames_out
// and their offsets to page-locked memory (finish_group).  No copy engine, no hand-over: the host enqueues one kernel
// per feed and an event behind it; a feed's bytes and offsets are final when its event has fired.  Feeds run one
// after the other on one stream; the job's stream position passes from launch to launch in device memory
// (enc_words).  Buffers that are not page-locked go through page-locked bounce buffers.
constexpr uint32_t kStageWorkgroups = 8;         // of k_stage_in, four waves each with eight 16-byte loads in flight per lane (6: 0.95 ms, 16: 0.90, 24: 0.99)
constexpr uint32_t kEncodeLaunchFrames = 1u << 14; // a feed larger than this is cut (the device buffers -- 27 KB of workspace per stereo frame -- are sized for it)

// Enqueue the launch of feed number `index` (its PCM in page-locked memory, its place in the mirror and its event are
// in `feed`).  staged: the PCM is fetched by the staging kernel beside the launch; otherwise by the copy engine in
// front of it.
hipError_t issue_encode_feed(sela_hip_job* job, EncodeFeed& feed, size_t index, bool staged)
{
    const size_t frame_pcm = (size_t)sela::kBlock * job->channels * sizeof(int16_t);
    const hipStream_t s = ctx().s_run[0];
    hipError_t e;
    sela::EncodeHostLink link;
    link.mirror = ctx().enc_mirror_mapped + feed.mirror_at;
    // (two cells in turn: a launch reads where the one before left the stream and leaves its own end in the other)
    uint64_t* const pos = static_cast<uint64_t*>(ctx().enc_words.ptr);
    link.pos_in = pos + (index & 1);
    link.pos_out = pos + ((index + 1) & 1);
    link.host_pcm = feed.mapped_src;
    link.pcm_ready = static_cast<uint64_t*>(ctx().enc_ready.ptr);
    link.stage_workgroups = kStageWorkgroups;
    link.stage_stream = ctx().s_in;
    link.stage_started = pos + 4;
    link.wait_naps = g_stage_wait_naps;
    // what fills the device's copy of the PCM waits for the launch before this one, which reads it (and for the
    // allocation that may just have cleared the marks)
    if ((e = hipEventRecord(ctx().enc_prev, s)) != hipSuccess || (e = hipStreamWaitEvent(ctx().s_in, ctx().enc_prev, 0)) != hipSuccess)
        return e;
    if (!staged) { // (the stagers copy stereo frames; anything else goes in by the copy engine, ahead of the launch)
        if ((e = hipMemcpyAsync(ctx().enc_pcm.ptr, feed.host_src, feed.n_frames * frame_pcm, hipMemcpyHostToDevice, ctx().s_in)) != hipSuccess
            || (e = hipEventRecord(ctx().enc_prev, ctx().s_in)) != hipSuccess || (e = hipStreamWaitEvent(s, ctx().enc_prev, 0)) != hipSuccess)
            return e;
        link.host_pcm = nullptr;
    }
    uint32_t* d_status = reinterpret_cast<uint32_t*>(pos + 2);
    e = sela::launch_encode(static_cast<const int16_t*>(ctx().enc_pcm.ptr), feed.n_frames, job->channels, job->out_mapped, job->frames_cap, nullptr, d_status,
        ctx().enc_workspace.ptr, nullptr, s, nullptr, nullptr, &link, g_force_plain_fir, g_self_blocks, 0, nullptr, 0, 0, nullptr, false, job->lossless);
    if (e == hipSuccess && !feed.done)
        e = hipEventCreateWithFlags(&feed.done, hipEventDisableTiming);
    if (e == hipSuccess)
        e = hipEventRecord(feed.done, s);
    return e;
}

int job_feed_encode_launch(sela_hip_job* job, const int16_t* pcm, uint32_t nf)
{
    const size_t frame_pcm = (size_t)sela::kBlock * job->channels * sizeof(int16_t);
    const hipStream_t s = ctx().s_run[0];
    hipError_t e;
    EncodeFeed feed;
    feed.first = job->fed;
    feed.n_frames = nf;
    feed.mirror_at = job->mirror_used;
    feed.host_src = pcm;
    feed.mapped_src = static_cast<const int16_t*>(device_view(pcm));
    if (!feed.mapped_src) { // ordinary memory: through a page-locked copy (kept until the job ends)
        feed.bounce_in = pool().take(nf * frame_pcm);
        if (!feed.bounce_in)
            return job_fail(job, fail(SELA_HIP_ENOMEM, "page-locked bounce buffer"));
        std::memcpy(feed.bounce_in, pcm, nf * frame_pcm);
        feed.host_src = static_cast<const int16_t*>(feed.bounce_in);
        if (!(feed.mapped_src = static_cast<const int16_t*>(device_view(feed.bounce_in)))) {
            pool().give(feed.bounce_in);
            return job_fail(job, fail(SELA_HIP_ENODEV, "page-locked memory is not visible to the device"));
        }
    }
    // (grow-only; the launches of a job run in order on one stream, so growing waits for the last one)
    const size_t need_pcm = nf * frame_pcm + 16, need_ws = sela::encode_workspace_bytes(nf, job->channels), need_ready = (size_t)nf * 8;
    if (need_pcm > ctx().enc_pcm.cap || need_ws > ctx().enc_workspace.cap || need_ready > ctx().enc_ready.cap) {
        if ((e = hipStreamSynchronize(s)) != hipSuccess || (e = ctx().enc_pcm.reserve(need_pcm)) != hipSuccess
            || (e = ctx().enc_workspace.reserve(need_ws)) != hipSuccess || (e = ctx().enc_ready.reserve(need_ready)) != hipSuccess
            // (the "frame copied in" words carry the bare ticket -- and a checksum -- and another process's tickets count from the same start)
            || (e = hipMemsetAsync(ctx().enc_ready.ptr, 0, ctx().enc_ready.cap, s)) != hipSuccess) {
            if (feed.bounce_in)
                pool().give(feed.bounce_in);
            return job_fail(job, fail_hip(e, "hipMalloc"));
        }
    }
    e = issue_encode_feed(job, feed, job->feeds.size(), job->staged && job->channels == 2);
    if (e != hipSuccess) {
        if (feed.bounce_in)
            pool().give(feed.bounce_in);
        if (feed.done)
            (void)hipEventDestroy(feed.done);
        return job_fail(job, fail_hip(e, "encode launch"));
    }
    job->mirror_used += (size_t)nf + 2;
    job->fed += nf;
    job->feeds.push_back(feed);
    return SELA_HIP_OK;
}

// A launch whose bounded wait for the staging kernel ran out (SELA_HIP_FLAG_INTERNAL: the device was kept so busy by
// other work that the stagers got no compute units in time) has coded frames that were not there: its bytes, its
// sizes -- and with them the stream position every later feed started from -- are void.  Feed `from` and everything
// queued behind it are issued again, PCM by the copy engine this time (nothing waits for a kernel beside it there).
// A busy device costs time, never the result; only a feed that fails this way too is an error.
int job_reissue_encode(sela_hip_job* job, size_t from)
{
    hipError_t e;
    ctx().sync_all(); // (nothing of the void launches is left running)
    job->staged = false;
    uint64_t* const pos = static_cast<uint64_t*>(ctx().enc_words.ptr);
    const uint64_t start = job->bytes_final; // the stream behind the last good feed
    if ((e = hipMemcpyAsync(pos + (from & 1), &start, 8, hipMemcpyHostToDevice, ctx().s_run[0])) != hipSuccess
        || (e = hipStreamSynchronize(ctx().s_run[0])) != hipSuccess) // (`start` is a local)
        return job_fail(job, fail_hip(e, "encode re-issue"));
    for (size_t k = from; k < job->feeds.size(); k++) {
        job->feeds[k].reissued = true;
        g_reissued_feeds++;
        if ((e = issue_encode_feed(job, job->feeds[k], k, false)) != hipSuccess)
            return job_fail(job, fail_hip(e, "encode re-issue"));
    }
    return SELA_HIP_OK;
}

int job_feed_encode(sela_hip_job* job, const int16_t* pcm, uint32_t n_frames)
{
    const size_t frame_samples = (size_t)sela::kBlock * job->channels;
    for (uint32_t done = 0; done < n_frames;) {
        const uint32_t nf = std::min(kEncodeLaunchFrames, n_frames - done);
        const int rc = job_feed_encode_launch(job, pcm + done * frame_samples, nf);
        if (rc != SELA_HIP_OK)
            return rc;
        done += nf;
    }
    return SELA_HIP_OK;
}

// How far the stream has got in host memory: the feeds, in order, whose launch has finished.  Fills offsets_out for
// their frames, and moves their bytes out of the bounce buffer if there is one.  (Finer steps -- a word per group of
// frames written by the kernel behind the group's bytes -- were dropped with the release fence they need: it costs an
// L2 write-back per group.)
int job_encode_progress(sela_hip_job* job, bool wait)
{
    const uint64_t* mirror = static_cast<const uint64_t*>(ctx().enc_mirror.ptr);
    while (job->feeds_final < job->feeds.size()) {
        EncodeFeed& f = job->feeds[job->feeds_final];
        const hipError_t q = wait ? hipEventSynchronize(f.done) : hipEventQuery(f.done);
        if (q == hipErrorNotReady) {
            (void)hipGetLastError();
            break;
        }
        if (q != hipSuccess)
            return job_fail(job, fail_hip(q, "encode kernels"));
        const uint64_t* m = mirror + f.mirror_at;
        const uint64_t st = m[f.n_frames + 1];
        const uint32_t flags = (uint32_t)st, overflow = (uint32_t)(st >> 32);
        if (flags & SELA_HIP_FLAG_INTERNAL) {
            if (f.reissued)
                return job_fail(job, fail(SELA_HIP_ENODEV, "a wait inside the encode kernel ran out (internal error)"));
            const int rc = job_reissue_encode(job, job->feeds_final);
            if (rc != SELA_HIP_OK)
                return rc;
            continue; // (this feed again, now behind its new event)
        }
        if (flags_to_error(flags)) {
            char msg[160];
            std::snprintf(msg, sizeof msg, "a block left the range the .sela format can carry (flags 0x%x)", flags);
            return job_fail(job, fail(SELA_HIP_ERANGE, msg));
        }
        for (uint32_t i = 0; i <= f.n_frames; i++)
            job->offsets_out[(size_t)f.first + i] = m[i];
        uint32_t fits = f.n_frames; // (a frame that ends beyond the capacity was not written, nor was any frame behind it)
        while (fits > 0 && m[fits] > job->frames_cap)
            fits--;
        if (m[fits] <= job->frames_cap) {
            job->frames_final = f.first + fits;
            job->bytes_final = m[fits];
        }
        if (job->out_bounce && job->bytes_final > job->bytes_copied) {
            std::memcpy(job->frames_out + job->bytes_copied, job->out_host + job->bytes_copied, (size_t)(job->bytes_final - job->bytes_copied));
            job->bytes_copied = job->bytes_final;
        }
        if (overflow)
            return job_fail(job, fail(SELA_HIP_ECAPACITY, "frames_out too small (see sela_hip_encode_bound_bytes)"));
        if (f.bounce_in) { // (a final feed is never issued again: its page-locked copy can go)
            pool().give(f.bounce_in);
            f.bounce_in = nullptr;
            f.host_src = f.mapped_src = nullptr;
        }
        job->feeds_final++;
    }
    return SELA_HIP_OK;
}

// A decode chunk needs nothing from the host once it is queued (its output size is known): copy-in on the copy
// stream; then, on one of three streams in turn, the kernel and right behind it -- no event in between -- the
// copy-out, so that the copy-outs of neighbouring chunks come from different streams (on ONE stream the copy engine
// idles ~20 us between two copies).  The kernels read the frame offsets where the host staged them (page-locked
// memory, two words per workgroup over the link): the first kernel starts as soon as the first chunk's frames are on
// the device.  (Measured and dropped: copy-in on the chunk's own stream as well -- the runtime keeps about three
// copies in flight and starts them in the order they were queued, so a copy-out that waits for its kernel holds up
// the copy-ins queued behind it: 0.90 -> 1.11 ms.)
// `k_offsets` = the chunk's first entry of the feed's staged offsets (absolute in `frames`), as the device sees it.
int job_issue_decode(sela_hip_job* job, const uint8_t* frames, const uint64_t* offsets, const uint64_t* k_offsets, uint32_t nf)
{
    const uint32_t i = job->issued;
    ChunkSet& c = ctx().set[i % kSets];
    const hipStream_t s = ctx().decode_stream(i);
    hipError_t e;
    if (i >= kSets) {
        // chunk i - kSets used this set.  The host goes no further ahead than that chunk's kernel (which also keeps
        // the queues short); the copy-in must not overwrite frames that kernel reads, the kernel not PCM on its way out.
        if ((e = hipEventSynchronize(c.ran)) != hipSuccess)
            return job_fail(job, fail_hip(e, "kernels"));
        if ((e = hipStreamWaitEvent(s, c.copied_out, 0)) != hipSuccess)
            return job_fail(job, fail_hip(e, "hipStreamWaitEvent"));
    }
    const uint64_t bytes = offsets[nf] - offsets[0];
    if ((size_t)bytes + 16 > c.frames.cap) {
        if (i >= kSets && (e = hipEventSynchronize(c.copied_out)) != hipSuccess) // (nothing of the set's last use is in flight)
            return job_fail(job, fail_hip(e, "copy-out"));
        if ((e = c.frames.reserve((size_t)bytes + 16)) != hipSuccess)
            return job_fail(job, fail_hip(e, "hipMalloc"));
    }
    if ((bytes && (e = hipMemcpyAsync(c.frames.ptr, frames + offsets[0], (size_t)bytes, hipMemcpyHostToDevice, ctx().s_in)) != hipSuccess)
        || (e = hipEventRecord(c.copied_in, ctx().s_in)) != hipSuccess || (e = hipStreamWaitEvent(s, c.copied_in, 0)) != hipSuccess)
        return job_fail(job, fail_hip(e, "H2D frames"));
    // the kernel adds the feed's absolute offsets to its base: bias the base so that offsets[0] lands on the chunk's copy
    const uint8_t* d_base = static_cast<const uint8_t*>(c.frames.ptr) - offsets[0];
    uint8_t* flags = ctx().job_flags_mapped + (size_t)job->fed * sela::decode_waves(job->channels);
    e = sela::launch_decode(d_base, k_offsets, nf, job->channels, static_cast<int16_t*>(c.pcm.ptr), static_cast<uint32_t*>(ctx().status.ptr),
        c.workspace.ptr, s, nullptr, nullptr, flags, g_recurrence_form);
    if (e != hipSuccess || (e = hipEventRecord(c.ran, s)) != hipSuccess)
        return job_fail(job, fail_hip(e, "decode launch"));
    const size_t frame_pcm = (size_t)sela::kBlock * job->channels * sizeof(int16_t);
    if ((e = hipMemcpyAsync(job->pcm_out + (size_t)job->fed * sela::kBlock * job->channels, c.pcm.ptr, nf * frame_pcm, hipMemcpyDeviceToHost, s)) != hipSuccess
        || (e = hipEventRecord(c.copied_out, s)) != hipSuccess)
        return job_fail(job, fail_hip(e, "D2H pcm"));
    job->chunk_first.push_back(job->fed);
    job->chunk_frames.push_back(nf);
    job->issued++;
    job->fed += nf;
    return SELA_HIP_OK;
}

// One feed of a decode job: stage its offsets, queue its chunks.
int job_feed_decode(sela_hip_job* job, const uint8_t* frames, const uint64_t* offsets, uint32_t n_frames)
{
    if (n_frames == 0)
        return SELA_HIP_OK;
    // (sized at begin for the whole job: total_frames entries + one more per feed, and a feed has at least a frame)
    uint64_t* staged = static_cast<uint64_t*>(ctx().job_offsets_host.ptr) + job->offsets_used;
    const uint64_t* mapped = ctx().job_offsets_mapped + job->offsets_used;
    std::memcpy(staged, offsets, ((size_t)n_frames + 1) * 8);
    job->offsets_used += (size_t)n_frames + 1;
    if (!device_view(frames + offsets[0])) {
        // ordinary memory: through a page-locked copy (kept until the job ends).  Copies from pageable memory go through
        // the runtime's own staging, and with several host threads decoding at once their results were seen to arrive
        // behind the event that should cover them (tests/test_gpu_round3.py::test_four_threads_encode_on_one_gpu).
        const size_t bytes = (size_t)(offsets[n_frames] - offsets[0]);
        void* copy = pool().take(bytes ? bytes : 1);
        if (!copy)
            return job_fail(job, fail(SELA_HIP_ENOMEM, "page-locked bounce buffer"));
        std::memcpy(copy, frames + offsets[0], bytes);
        job->bounce_frames.push_back(copy);
        frames = static_cast<const uint8_t*>(copy) - offsets[0];
    }
    for (uint32_t done = 0; done < n_frames;) {
        const uint32_t nf = next_chunk_frames(job->issued, n_frames - done, job->channels);
        const int rc = job_issue_decode(job, frames, offsets + done, mapped + done, nf);
        if (rc != SELA_HIP_OK)
            return rc;
        done += nf;
    }
    return SELA_HIP_OK;
}

// Decode: which chunks have arrived in host memory by now (no waiting).
int job_drain_ready(sela_hip_job* job)
{
    if (job->encode)
        return job_encode_progress(job, false);
    while (job->final_chunks < job->issued && hipEventQuery(ctx().set[job->final_chunks % kSets].copied_out) == hipSuccess)
        job->final_chunks++;
    (void)hipGetLastError(); // (hipErrorNotReady from the query is not an error)
    job_move_decoded(job);
    return SELA_HIP_OK;
}

void job_progress(const sela_hip_job* job, uint32_t* frames_final, uint64_t* bytes_final)
{
    if (job->encode) {
        if (frames_final)
            *frames_final = job->frames_final;
        if (bytes_final)
            *bytes_final = job->bytes_final;
        return;
    }
    const uint32_t n = job->final_chunks;
    if (frames_final)
        *frames_final = n ? job->chunk_first[n - 1] + job->chunk_frames[n - 1] : 0;
    if (bytes_final)
        *bytes_final = 0;
}

int job_begin(sela_hip_job** out, bool encode, uint32_t channels, uint32_t total_frames)
{
    if (!out)
        return fail(SELA_HIP_EINVAL, "null job pointer");
    *out = nullptr;
    if (channels == 0 || channels > 255)
        return fail(SELA_HIP_EINVAL, "channels must be in 1..255");
    if (!encode && channels > sela::decode_max_channels())
        return fail(SELA_HIP_EINVAL, "too many channels for the on-chip decoder (sela_hip_decode_max_channels)");
    int rc = sela_hip_init(-1);
    if (rc != SELA_HIP_OK)
        return rc;
    if (!ctx().bind_current_device())
        return fail(SELA_HIP_ENODEV, "hipGetDevice failed");
    if (ctx().job_open)
        return fail(SELA_HIP_EINVAL, "this thread already has an open job");
    hipError_t e = ctx().streams();
    if (e == hipSuccess)
        e = ctx().status.reserve(16);
    if (e == hipSuccess && encode) {
        // (offsets + status per feed, a feed has at least a frame)
        if ((e = ctx().enc_mirror.reserve((3 * (size_t)total_frames + 4) * 8)) == hipSuccess
            && (e = ctx().enc_words.reserve(16 + 16 + 32)) == hipSuccess
            && (e = hipHostGetDevicePointer((void**)&ctx().enc_mirror_mapped, ctx().enc_mirror.ptr, 0)) == hipSuccess)
            e = hipMemsetAsync(ctx().enc_words.ptr, 0, 16 + 16 + 32, ctx().s_run[0]); // the job's stream position: 0
    }
    if (e == hipSuccess && !encode) {
        const size_t n_flags = (size_t)total_frames * sela::decode_waves(channels) + 1;
        if ((e = reserve_chunk_buffers(channels)) == hipSuccess
            && (e = ctx().job_offsets_host.reserve((2 * (size_t)total_frames + 2) * 8)) == hipSuccess
            && (e = ctx().job_flags.reserve(n_flags)) == hipSuccess
            && (e = hipHostGetDevicePointer((void**)&ctx().job_offsets_mapped, ctx().job_offsets_host.ptr, 0)) == hipSuccess
            && (e = hipHostGetDevicePointer((void**)&ctx().job_flags_mapped, ctx().job_flags.ptr, 0)) == hipSuccess)
            std::memset(ctx().job_flags.ptr, 0, n_flags);
    }
    if (e != hipSuccess)
        return fail_hip(e, "hipMalloc");
    sela_hip_job* job = new sela_hip_job;
    job->encode = encode;
    job->channels = channels;
    job->total_frames = total_frames;
    job->staged = job->holds_staged_path = encode && channels == 2 && staged_path_acquire(ctx().device);
    ctx().staged_device = job->holds_staged_path ? ctx().device : -1;
    ctx().job_open = true;
    *out = job;
    return SELA_HIP_OK;
}

int job_end(sela_hip_job* job, uint32_t* frames_final, uint64_t* bytes_final)
{
    int rc = job->error;
    hipError_t e = hipSuccess;
    if (job->encode) {
        // (also after an error: nothing of the job may still be running when its buffers go back)
        if ((e = hipStreamSynchronize(ctx().s_run[0])) != hipSuccess && rc == SELA_HIP_OK)
            rc = fail_hip(e, "encode kernels");
        if (rc == SELA_HIP_OK)
            rc = job_encode_progress(job, true);
        for (EncodeFeed& f : job->feeds) {
            if (f.bounce_in)
                pool().give(f.bounce_in);
            if (f.done)
                (void)hipEventDestroy(f.done);
        }
        if (job->out_bounce && job->out_host)
            pool().give(job->out_host);
    } else {
        if (rc == SELA_HIP_OK)
            rc = job_finalize(job, job->issued);
        if (rc != SELA_HIP_OK)
            ctx().sync_all(); // (nothing may still be reading or writing the bounce buffers)
        for (void* b : job->bounce_frames)
            pool().give(b);
        if (job->pcm_bounce && job->pcm_out)
            pool().give(job->pcm_out);
    }
    uint32_t seen_flags = 0;
    if (rc == SELA_HIP_OK && !job->encode && job->issued) {
        // every frame is decoded (bad ones to silence) before the verdict; the kernels left their flags in host memory
        const uint8_t* flags = static_cast<const uint8_t*>(ctx().job_flags.ptr);
        const size_t n = (size_t)job->fed * sela::decode_waves(job->channels);
        for (size_t i = 0; i < n; i++)
            seen_flags |= flags[i];
    }
    if (rc != SELA_HIP_OK) { // leave nothing in flight behind an error
        const std::string msg = sela_hip_last_error();
        ctx().sync_all();
        (void)fail(rc, msg);
    }
    job_progress(job, frames_final, bytes_final);
    ctx().job_open = false;
    if (job->holds_staged_path)
        staged_path_release(ctx().device);
    ctx().staged_device = -1;
    delete job;
    if (rc != SELA_HIP_OK)
        return rc;
    return sela::judge_decode(seen_flags, sela::kJudgeJob, sela::kRouteFast, "decode"); // (not SHORT_BLOCK, not INTERNAL)
}


// ---- does a device-pointer launch have the device to itself? ------------------------------------------------------------------
// The encode kernels take a schedule of wave priorities that FALLS with a wave's progress (sela_encode.hip, the note on
// priorities): on its own a launch of one fill finishes 7 % sooner with it, beside another stream's kernels the same schedule
// starves the neighbour and costs 6 %.  Whether there is a neighbour the library can tell for its own launches: every
// device-pointer call leaves an event on its stream, and a call looks at the events of the OTHER streams -- one still pending
// means that stream's kernels will run beside this launch's.  (Decided when the launch is queued; work the library does not
// know of is not seen: then the schedule is merely not the best one.  Events, not the streams themselves, are kept: a caller
// may destroy its stream.)
struct Flights {
    struct Entry {
        hipStream_t stream;
        hipEvent_t done;
    };
    std::mutex mu;
    std::vector<Entry> entries[64]; // by device
    bool others_pending(int dev, hipStream_t stream)
    {
        std::lock_guard<std::mutex> lock(mu);
        for (const Entry& e : entries[dev])
            if (e.stream != stream && hipEventQuery(e.done) == hipErrorNotReady)
                return true;
        return false;
    }
    void note(int dev, hipStream_t stream)
    {
        std::lock_guard<std::mutex> lock(mu);
        std::vector<Entry>& v = entries[dev];
        Entry* mine = nullptr;
        for (Entry& e : v)
            if (e.stream == stream)
                mine = &e;
        if (!mine && v.size() >= 16) // streams come and go: an entry whose work is done is as good as a new one
            for (Entry& e : v)
                if (hipEventQuery(e.done) != hipErrorNotReady) {
                    mine = &e;
                    mine->stream = stream;
                    break;
                }
        if (!mine) {
            if (v.size() >= 64)
                return; // (not tracked: at worst a launch is taken to be alone)
            Entry e{ stream, nullptr };
            if (hipEventCreateWithFlags(&e.done, hipEventDisableTiming) != hipSuccess)
                return;
            v.push_back(e);
            mine = &v.back();
        }
        (void)hipEventRecord(mine->done, stream);
    }
    void release_all() // sela_hip_shutdown: the events go back to the runtime, each on its device
    {
        std::lock_guard<std::mutex> lock(mu);
        int before = -1;
        (void)hipGetDevice(&before);
        for (int dev = 0; dev < 64; dev++) {
            if (entries[dev].empty())
                continue;
            (void)hipSetDevice(dev);
            for (Entry& e : entries[dev])
                (void)hipEventDestroy(e.done);
            entries[dev].clear();
        }
        if (before >= 0)
            (void)hipSetDevice(before);
    }
};
// A stream that is being captured into a graph must not be touched by the bookkeeping: the event record would be captured too,
// and a query of that event afterwards fails.  Such a launch counts as having neighbours (no schedule) and leaves no mark.
bool stream_is_capturing(hipStream_t stream)
{
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    return stream && hipStreamIsCapturing(stream, &st) == hipSuccess && st != hipStreamCaptureStatusNone;
}
Flights& flights()
{
    static Flights* f = new Flights; // (never destroyed: events outlive the statics' teardown)
    return *f;
}
std::atomic<int64_t> g_forced_priorities{ -1 }; // debug (sela_hip_debug_priorities): a fixed schedule for every launch; -1: by the neighbours
std::atomic<int> g_launches_alone{ 0 };         // debug: launches that were given the falling schedule
constexpr uint32_t kFallingPriorities = 0x00010203u; // 3, 2, 1, 0 by quarters of a wave's work (least significant byte first)
constexpr uint32_t kHeavySubframesFirst = 0x00010000u; // the decoder: orders above 60 at priority 1 through their synthesis (launch_decode)

uint32_t launch_priorities(hipStream_t stream, int& dev)
{
    dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) {
        dev = -1;
        return 0;
    }
    const int64_t forced = g_forced_priorities.load(std::memory_order_relaxed);
    if (forced >= 0)
        return (uint32_t)forced;
    if (stream_is_capturing(stream) || flights().others_pending(dev, stream))
        return 0;
    g_launches_alone.fetch_add(1, std::memory_order_relaxed);
    return kFallingPriorities;
}

// ---- an encode launch cut in two (round 6: built, measured, OFF) ------------------------------------------------------------------
// One fill of team waves ends in a tail: the last waves walk alone while most SIMDs idle, and plan + assemble -- 30 us during which
// one CU works -- wait behind it.  Round 5 measured from outside that two encoders on two streams, each on its share of the track,
// finish 6 % sooner than one launch (tools/split_probe.py: 0.434 -> 0.408 ms per call).  Round 6 built it inside the call -- a launch
// the library gives to teams of 16 runs as two halves on the caller's stream and a side stream of the device, the first half's
// plan + assemble under the second half's tail, the second half's frames placed behind the first's by its plan kernel
// (k_plan_frames' base); same bytes, offsets and status words (tests) -- and it is SLOWER: one lane 12.16-12.20 G samples/s at every
// share from 40 to 70 % against 12.48 uncut (profiles/r06/split_sweep.txt): the two event hand-overs between the streams cost more
// than the 15 us of plan + assemble they hide.  So the library never cuts by itself; the form stays behind
// sela_hip_debug_encode_split (bench.py --encode-split N) for the comparison.  Never while kernel timing is on, with a trace or phase
// buffer, with a kernel forced by a debug hook, or into a stream that is being captured.
//
// A side lane: per device a stream of the library's own and the two events that cross to it and back -- `forked`, recorded on the
// caller's stream for the side stream to wait on, and `side_done`, recorded on the side stream for the caller's to wait on.  (In a
// stream that is being captured the side stream joins the capture at the first crossing and leaves it at the second.)  Whoever
// holds `mu` enqueues through it; the work of successive holders still overlaps on the device.  The library has two, which never
// wait on each other: the encode split's, taken with try_to_lock, and the whole-track calls' (fork_join below), taken blocking.
struct SideLane {
    std::mutex mu;
    hipStream_t side[64] = {};
    hipEvent_t forked[64] = {}, side_done[64] = {};
    bool ready(int dev)
    {
        if (side[dev])
            return true;
        if (hipStreamCreateWithFlags(&side[dev], hipStreamNonBlocking) != hipSuccess) {
            side[dev] = nullptr;
            return false;
        }
        if (hipEventCreateWithFlags(&forked[dev], hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&side_done[dev], hipEventDisableTiming) != hipSuccess) {
            (void)hipStreamDestroy(side[dev]);
            side[dev] = nullptr;
            return false;
        }
        return true;
    }
    void release_all()
    {
        std::lock_guard<std::mutex> lock(mu);
        int before = -1;
        (void)hipGetDevice(&before);
        for (int dev = 0; dev < 64; dev++)
            if (side[dev]) {
                (void)hipSetDevice(dev);
                (void)hipStreamSynchronize(side[dev]);
                (void)hipEventDestroy(forked[dev]);
                (void)hipEventDestroy(side_done[dev]);
                (void)hipStreamDestroy(side[dev]);
                side[dev] = nullptr;
            }
        if (before >= 0)
            (void)hipSetDevice(before);
    }
};
struct Splitter : SideLane {
    std::map<const void*, std::pair<uint32_t, uint32_t>> last; // workspace -> (frames of the launch, frames of its first half; 0: whole)
    void release_all()
    {
        SideLane::release_all();
        std::lock_guard<std::mutex> lock(mu);
        last.clear();
    }
};
Splitter& splitter()
{
    static Splitter* s = new Splitter; // (never destroyed: streams outlive the statics' teardown)
    return *s;
}
SideLane& whole_lane()
{
    static SideLane* l = new SideLane;
    return *l;
}

// The fork and join of the whole-track device calls, written once: `side_work(side stream)` beside `main_work()`
// on the caller's stream `st`, both behind whatever `st` holds already, and `st` behind both when this returns.  Each returns a
// SELA_HIP_ code, its error reported.  The lane's mutex is held from before the fork until the join is enqueued; the main work is
// enqueued only behind side work that was enqueued whole; the join is enqueued on every path past the fork -- also after a failure
// in between: a side stream that has joined a capture must leave it -- and the first failure is the one reported.  `name` opens
// the texts; `ran_on`, if given, is told the device.
template <typename SideWork, typename MainWork>
int fork_join(SideLane& lane, hipStream_t st, const char* name, SideWork side_work, MainWork main_work, int* ran_on = nullptr)
{
    const std::string who = std::string(name) + ": ";
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64)
        return fail(SELA_HIP_ENODEV, who + "no current device");
    std::lock_guard<std::mutex> lock(lane.mu);
    if (!lane.ready(dev))
        return fail(SELA_HIP_ENODEV, who + "no side stream");
    const hipStream_t side = lane.side[dev];
    // fork: the side stream follows whatever produced the call's input, and the workspace's previous user, on the caller's stream
    hipError_t e = hipEventRecord(lane.forked[dev], st);
    if (e == hipSuccess)
        e = hipStreamWaitEvent(side, lane.forked[dev], 0);
    if (e != hipSuccess)
        return fail_hip(e, (who + "fork").c_str());
    int rc = side_work(side);
    if (rc == SELA_HIP_OK && (e = hipEventRecord(lane.side_done[dev], side)) != hipSuccess)
        rc = fail_hip(e, (who + "join").c_str());
    if (rc == SELA_HIP_OK)
        rc = main_work();
    if ((e = hipStreamWaitEvent(st, lane.side_done[dev], 0)) != hipSuccess && rc == SELA_HIP_OK)
        rc = fail_hip(e, (who + "join").c_str());
    if (ran_on)
        *ran_on = dev;
    return rc;
}
std::atomic<int> g_encode_split{ 0 };    // debug (sela_hip_debug_encode_split): 0 never (the product), 1..999: every launch of teams of 16, that share to the first half
std::atomic<int> g_launches_split{ 0 };
// The workspace of a launch cut in two: the first half's, the second half's (each launch_encode's own, sela_workspace.h).
struct SplitWs {
    void *first, *second;
    size_t end; // what both need of the caller's workspace
};
SplitWs carve_encode_split(sela::Carve& c, uint32_t first, uint32_t rest, uint32_t channels)
{
    sela::Carve a = c.sub(sela::encode_workspace_bytes(first, channels)), b = c.sub(sela::encode_workspace_bytes(rest, channels));
    if (c.listing()) { // (the halves' own pieces, where they lie)
        sela::encode_workspace_bytes(first, channels, &a);
        sela::encode_workspace_bytes(rest, channels, &b);
    }
    return { a.base(), b.base(), (size_t)c.end() };
}
uint32_t split_of_last_launch(const void* d_workspace, uint32_t n_frames)
{
    std::lock_guard<std::mutex> lock(splitter().mu);
    const auto it = splitter().last.find(d_workspace);
    return it != splitter().last.end() && it->second.first == n_frames ? it->second.second : 0u;
}

} // namespace

// ---- the stages on their own (sela_hip.h): plain synchronous calls, device buffers of their own -----------------------------
namespace {

// device memory for the length of one call
struct Scratch {
    std::vector<void*> blocks;
    ~Scratch()
    {
        for (void* b : blocks)
            (void)hipFree(b);
    }
    template <typename T>
    T* take(size_t count, hipError_t& err)
    {
        void* p = nullptr;
        if (err == hipSuccess)
            err = hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T));
        if (p)
            blocks.push_back(p);
        return static_cast<T*>(p);
    }
    template <typename T>
    T* upload(const T* host, size_t count, hipError_t& err)
    {
        T* d = take<T>(count, err);
        if (err == hipSuccess && count)
            err = hipMemcpy(d, host, count * sizeof(T), hipMemcpyHostToDevice);
        return d;
    }
};

} // namespace

extern "C" {

const char* sela_hip_last_error(void) { return g_error.c_str(); }

int sela_hip_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess)
        return 0;
    return n;
}

int sela_hip_init(int device)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(SELA_HIP_ENODEV, "no HIP device visible (the SELA MI355X path has no CPU fallback)");
    if (device >= n)
        return fail(SELA_HIP_EINVAL, "device index out of range");
    if (device >= 0) {
        e = hipSetDevice(device);
        if (e != hipSuccess)
            return fail_hip(e, "hipSetDevice");
    }
    return SELA_HIP_OK;
}

void sela_hip_thread_release(void)
{
    g_lease.give_back();
    sela::generic_release();
}

void sela_hip_shutdown(void)
{
    g_lease.shutdown();
    sela::generic_shutdown();
    flights().release_all();
    splitter().release_all();
    whole_lane().release_all();
    pool().trim();
}

void* sela_hip_host_alloc(size_t bytes) { return pool().take(bytes ? bytes : 1); }

void sela_hip_host_free(void* p)
{
    if (p)
        pool().give(p);
}

void sela_hip_debug_phase_buffer(uint64_t* d_cycles) { g_phase_cycles = d_cycles; }

void sela_hip_debug_force_plain_fir(int enable) { g_force_plain_fir = enable & 3; }

void sela_hip_debug_mean_workers(int self_blocks) { g_self_blocks = self_blocks; }
void sela_hip_debug_encode_teams(int lanes) { g_team_lanes = lanes; }
void sela_hip_debug_encode_fused(int enable) { g_fused_device = enable != 0; }
void sela_hip_debug_priorities(uint32_t team_quarters) { g_forced_priorities.store((int64_t)team_quarters, std::memory_order_relaxed); }
void sela_hip_debug_priorities_adaptive(void) { g_forced_priorities.store(-1, std::memory_order_relaxed); }
int sela_hip_debug_launches_alone(void) { return g_launches_alone.load(std::memory_order_relaxed); }
int sela_hip_debug_block_forms(const void* d_workspace, uint32_t n_frames, uint32_t channels, uint32_t* counts_out, uint8_t* forms_out)
{
    if (!d_workspace || !counts_out || channels == 0)
        return fail(SELA_HIP_EINVAL, "bad argument");
    counts_out[0] = counts_out[1] = counts_out[2] = 0;
    const size_t blocks = (size_t)n_frames * sela_hip_signals_per_frame(channels);
    std::vector<sela::BlockMeta> meta(blocks);
    hipError_t e = hipDeviceSynchronize();
    // (the records open the workspace, launch_encode -- or, after a launch that was cut in two, each half's workspace)
    const uint32_t first = split_of_last_launch(d_workspace, n_frames);
    const size_t n_sig = sela_hip_signals_per_frame(channels);
    if (e == hipSuccess && blocks) {
        const size_t head = first ? (size_t)first * n_sig : blocks;
        if (!first)
            e = hipMemcpy(meta.data(), sela::encode_block_records(d_workspace, n_frames, channels), blocks * sizeof(sela::BlockMeta), hipMemcpyDeviceToHost);
        else {
            sela::Carve c(d_workspace);
            const SplitWs halves = carve_encode_split(c, first, n_frames - first, channels);
            e = hipMemcpy(meta.data(), sela::encode_block_records(halves.first, first, channels), head * sizeof(sela::BlockMeta), hipMemcpyDeviceToHost);
            if (e == hipSuccess)
                e = hipMemcpy(meta.data() + head, sela::encode_block_records(halves.second, n_frames - first, channels), (blocks - head) * sizeof(sela::BlockMeta),
                    hipMemcpyDeviceToHost);
        }
    }
    if (e != hipSuccess)
        return fail_hip(e, "block forms");
    for (size_t b = 0; b < blocks; b++) {
        const uint32_t form = (meta[b].flags & sela::kBlockFormPlain) ? 2 : ((meta[b].flags & sela::kBlockFormTwoPass) ? 1 : 0);
        counts_out[form]++;
        if (forms_out)
            forms_out[b] = (uint8_t)form;
    }
    return SELA_HIP_OK;
}
void sela_hip_debug_keep_both_candidates(int on) { sela::set_keep_both_candidates(on); }
void sela_hip_debug_encode_split(int mode) { g_encode_split.store(mode < 0 || mode > 999 ? 0 : mode, std::memory_order_relaxed); }
int sela_hip_debug_launches_split(void) { return g_launches_split.load(std::memory_order_relaxed); }
void sela_hip_debug_encode_hashes(int on) { sela::set_encode_hashes(on); }
int sela_hip_debug_encode_kernel(uint32_t n_frames, uint32_t channels) { return sela::encode_team_lanes(n_frames, channels, g_team_lanes); }

void sela_hip_debug_stage_wait(int naps) { g_stage_wait_naps = naps; }

int sela_hip_debug_reissued_feeds(void) { return g_reissued_feeds; }
void sela_hip_debug_decode_recurrence(int form) { g_recurrence_form = form < 0 ? -1 : (form != 0); }
int sela_hip_debug_contexts_created(void) { return g_contexts_created.load(std::memory_order_relaxed); }

void sela_hip_enable_kernel_timing(int enable) { g_timing.enabled = enable != 0; }

int sela_hip_kernel_times(float* ms_out, int capacity)
{
    const int n = g_timing.recorded < capacity ? g_timing.recorded : capacity;
    for (int i = 0; i < n; i++) {
        if (hipEventSynchronize(g_timing.ev[i + 1]) != hipSuccess || hipEventElapsedTime(&ms_out[i], g_timing.ev[i], g_timing.ev[i + 1]) != hipSuccess)
            return 0;
    }
    return n;
}

uint32_t sela_hip_signals_per_frame(uint32_t channels) { return channels == 2 ? 3u : channels; }

size_t sela_hip_encode_workspace_bytes(uint32_t n_frames, uint32_t channels)
{
    // (room for the two workspaces of a launch that the debug hook cuts in two, at any share: the fixed parts -- the rings -- twice)
    const size_t whole = sela::encode_workspace_bytes(n_frames, channels);
    return sela::encode_split_frames(n_frames, channels, 500) ? whole + sela::encode_workspace_bytes(0, channels) + 65536 : whole;
}

size_t sela_hip_decode_workspace_bytes(uint32_t n_frames, uint32_t channels) { return sela::decode_workspace_bytes(n_frames, channels); }

uint32_t sela_hip_decode_max_channels(void) { return sela::decode_max_channels(); }

size_t sela_hip_encode_bound_bytes(uint32_t n_frames, uint32_t channels)
{
    return (size_t)n_frames * sela_frame_bytes(channels, channels * (uint32_t)sela::kSlotWords);
}

namespace {
// sela_hip_encode_device and, with lossless, sela_hip_encode_device_opt: the checks, the choice of kernels, the launch
int encode_device_call(const int16_t* d_pcm, uint32_t n_frames, uint32_t channels, uint8_t* d_frames, size_t frames_cap,
    uint64_t* d_frame_offsets, uint32_t* d_status, void* d_workspace, size_t workspace_bytes, sela_hip_trace* d_trace, void* stream, bool lossless)
{
    if (channels == 0 || channels > 255)
        return fail(SELA_HIP_EINVAL, "channels must be in 1..255");
    if (!d_frame_offsets || !d_status || (n_frames && (!d_pcm || !d_frames || !d_workspace)))
        return fail(SELA_HIP_EINVAL, "null device pointer");
    if (((uintptr_t)d_pcm & 3) || ((uintptr_t)d_frames & 3))
        return fail(SELA_HIP_EINVAL, "d_pcm and d_frames must be 4-byte aligned");
    if (workspace_bytes < sela::encode_workspace_bytes(n_frames, channels))
        return fail(SELA_HIP_ECAPACITY, "workspace smaller than sela_hip_encode_workspace_bytes()");
    hipEvent_t* ev = n_frames ? g_timing.events() : nullptr;
    g_timing.recorded = ev ? 3 : 0;
    sela::EncodeHostLink fused = {}; // (debug hook: the one-launch form on device pointers -- nothing mirrored, no stream position, no stagers)
    fused.wait_naps = -1;
    const bool use_fused = g_fused_device && !d_trace && !g_phase_cycles;
    if (use_fused)
        g_timing.recorded = ev ? 1 : 0;
    int dev = -1;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const uint32_t priorities = launch_priorities(st, dev);
    // cut in two?  (see Splitter)
    uint32_t first = 0;
    SplitWs halves = {};
    const int split_mode = g_encode_split.load(std::memory_order_relaxed);
    if (dev >= 0 && n_frames && split_mode > 0 && !ev && !d_trace && !g_phase_cycles && !use_fused && g_team_lanes < 0 && !stream_is_capturing(st)) {
        first = sela::encode_split_frames(n_frames, channels, split_mode);
        sela::Carve c(d_workspace);
        if (first && (halves = carve_encode_split(c, first, n_frames - first, channels)).end > workspace_bytes)
            first = 0;
    }
    hipError_t e = hipSuccess;
    bool split_done = false;
    if (first) {
        Splitter& sp = splitter();
        std::unique_lock<std::mutex> lock(sp.mu, std::try_to_lock); // (one split launch at a time per process: a second caller is not alone anyway)
        if (lock.owns_lock() && sp.ready(dev)) {
            const uint32_t rest = n_frames - first;
            void* const ws2 = halves.second;
            const int16_t* const pcm2 = d_pcm + (size_t)first * SELA_HIP_SAMPLES_PER_FRAME * channels;
            const hipStream_t side = sp.side[dev];
            e = hipEventRecord(sp.forked[dev], st);
            if (e == hipSuccess)
                e = hipStreamWaitEvent(side, sp.forked[dev], 0);
            if (e == hipSuccess) // the first half's blocks, on the caller's stream
                e = sela::launch_encode(d_pcm, first, channels, d_frames, frames_cap, d_frame_offsets, d_status, d_workspace, nullptr, st, nullptr, nullptr, nullptr,
                    g_force_plain_fir, g_self_blocks, 16, nullptr, priorities, 1, nullptr, false, lossless);
            if (e == hipSuccess) // the second half's, beside them
                e = sela::launch_encode(pcm2, rest, channels, d_frames, frames_cap, d_frame_offsets + first, d_status, ws2, nullptr, side, nullptr, nullptr, nullptr,
                    g_force_plain_fir, g_self_blocks, 16, nullptr, priorities, 1, nullptr, false, lossless);
            if (e == hipSuccess)
                e = hipEventRecord(sp.side_done[dev], side);
            if (e == hipSuccess) // the first half's plan + assemble, under the second half's tail
                e = sela::launch_encode(d_pcm, first, channels, d_frames, frames_cap, d_frame_offsets, d_status, d_workspace, nullptr, st, nullptr, nullptr, nullptr,
                    g_force_plain_fir, g_self_blocks, 16, nullptr, priorities, 2, nullptr, false, lossless);
            if (e == hipSuccess)
                e = hipStreamWaitEvent(st, sp.side_done[dev], 0);
            if (e == hipSuccess) // the second half's frames behind the first's
                e = sela::launch_encode(pcm2, rest, channels, d_frames, frames_cap, d_frame_offsets + first, d_status, ws2, nullptr, st, nullptr, nullptr, nullptr,
                    g_force_plain_fir, g_self_blocks, 16, nullptr, priorities, 2, d_frame_offsets + first, true, lossless);
            sp.last[d_workspace] = std::make_pair(n_frames, first);
            g_launches_split.fetch_add(1, std::memory_order_relaxed);
            split_done = true;
        }
    }
    if (!split_done) {
        e = sela::launch_encode(d_pcm, n_frames, channels, d_frames, frames_cap, d_frame_offsets, d_status, d_workspace,
            d_trace, st, ev, g_phase_cycles, use_fused ? &fused : nullptr, g_force_plain_fir, g_self_blocks, g_team_lanes, nullptr,
            priorities, 0, nullptr, false, lossless);
        if (n_frames) {
            std::lock_guard<std::mutex> lock(splitter().mu);
            const auto it = splitter().last.find(d_workspace);
            if (it != splitter().last.end())
                it->second = std::make_pair(n_frames, 0u);
        }
    }
    if (e != hipSuccess)
        return fail_hip(e, "encode launch");
    if (dev >= 0 && n_frames)
        if (!stream_is_capturing(static_cast<hipStream_t>(stream)))
            flights().note(dev, static_cast<hipStream_t>(stream));
    return SELA_HIP_OK;
}

// what every *_opt call asks first: SELA_HIP_OK and whether the call is a lossless one, or the refusal, reported
int encode_options(uint32_t options, bool* lossless)
{
    if (options & ~(uint32_t)SELA_HIP_ENCODE_LOSSLESS)
        return fail(SELA_HIP_EINVAL, "options: a bit this library does not know (SELA_HIP_ENCODE_LOSSLESS is the only one)");
    *lossless = options != 0;
    return SELA_HIP_OK;
}
} // namespace

int sela_hip_encode_device(const int16_t* d_pcm, uint32_t n_frames, uint32_t channels, uint8_t* d_frames, size_t frames_cap,
    uint64_t* d_frame_offsets, uint32_t* d_status, void* d_workspace, size_t workspace_bytes, sela_hip_trace* d_trace, void* stream)
{
    return encode_device_call(d_pcm, n_frames, channels, d_frames, frames_cap, d_frame_offsets, d_status, d_workspace, workspace_bytes, d_trace, stream, false);
}

int sela_hip_encode_device_opt(const int16_t* d_pcm, uint32_t n_frames, uint32_t channels, uint8_t* d_frames, size_t frames_cap,
    uint64_t* d_frame_offsets, uint32_t* d_status, void* d_workspace, size_t workspace_bytes, sela_hip_trace* d_trace, void* stream, uint32_t options)
{
    bool lossless = false;
    const int rc = encode_options(options, &lossless);
    if (rc != SELA_HIP_OK)
        return rc;
    if (lossless && d_trace)
        return fail(SELA_HIP_EINVAL, "SELA_HIP_ENCODE_LOSSLESS with d_trace: the trace is the reference's arithmetic");
    if (lossless && g_phase_cycles)
        return fail(SELA_HIP_EINVAL, "SELA_HIP_ENCODE_LOSSLESS while sela_hip_debug_phase_buffer is set: the phase counts are the plain kernels'");
    return encode_device_call(d_pcm, n_frames, channels, d_frames, frames_cap, d_frame_offsets, d_status, d_workspace, workspace_bytes, d_trace, stream, lossless);
}

namespace {
// The decoder's counterpart of the encoder's schedule: a launch that has the device to itself raises its heavy subframes.
// *dev: the current device, or -1 (then nothing is to be noted in flights() after the launch).
uint32_t decode_synth_priorities(uint32_t n_frames, void* stream, int* dev)
{
    uint32_t synth_priorities = 0;
    if (n_frames && hipGetDevice(dev) == hipSuccess && *dev >= 0 && *dev < 64) {
        const int64_t forced = g_forced_priorities.load(std::memory_order_relaxed);
        synth_priorities = forced >= 0 ? (forced ? kHeavySubframesFirst : 0u)
                                       : (stream_is_capturing(static_cast<hipStream_t>(stream)) || flights().others_pending(*dev, static_cast<hipStream_t>(stream)) ? 0u : kHeavySubframesFirst);
    } else {
        *dev = -1;
    }
    return synth_priorities;
}

// A launch of the 2048-sample decoder or of what runs it (decode, decode_n, verify): ask for the priorities, launch, and leave
// the launch in flights() unless the stream is capturing.  launch: uint32_t synth_priorities -> hipError_t; what: fail_hip's text.
extern "C++" template <typename Launch>
int launch_with_priorities(uint32_t n_frames, void* stream, const char* what, Launch launch)
{
    int dev = -1;
    const hipError_t e = launch(decode_synth_priorities(n_frames, stream, &dev));
    if (e != hipSuccess)
        return fail_hip(e, what);
    if (dev >= 0)
        if (!stream_is_capturing(static_cast<hipStream_t>(stream)))
            flights().note(dev, static_cast<hipStream_t>(stream));
    return SELA_HIP_OK;
}

// sela_hip_decode_device's launch, arguments checked; d_n_found (or null): the device's own count of frames to decode
int decode_device_launch(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames, uint32_t channels,
    int16_t* d_pcm_out, uint32_t* d_status, void* d_workspace, void* stream, const uint32_t* d_n_found)
{
    hipEvent_t* ev = n_frames ? g_timing.events() : nullptr;
    g_timing.recorded = ev ? 1 : 0;
    return launch_with_priorities(n_frames, stream, "decode launch", [&](uint32_t synth_priorities) {
        return sela::launch_decode(d_frames, d_frame_offsets, n_frames, channels, d_pcm_out, d_status, d_workspace, static_cast<hipStream_t>(stream), ev,
            g_phase_cycles, nullptr, g_recurrence_form, synth_priorities, d_n_found);
    });
}

int launched(hipError_t e, const char* what) { return e == hipSuccess ? SELA_HIP_OK : fail_hip(e, what); }

// A payload call's workspace: the index's, then the call's own, each its launch's own description (sela_workspace.h).
struct PayloadWs {
    void* own;
    size_t end; // what both need of the caller's workspace
};
PayloadWs carve_payload(void* d_workspace, size_t payload_bytes, size_t own_bytes)
{
    sela::Carve c(d_workspace);
    c.sub(sela::index_workspace_bytes(payload_bytes)); // (launch_index is given d_workspace itself: the same base)
    return { c.sub(own_bytes).base(), (size_t)c.end() };
}

// the index's own checks (sela_hip_index_frames_device); SELA_HIP_OK or the failure, reported
int check_index_args(const uint8_t* d_payload, size_t payload_bytes, uint32_t channels, const uint64_t* d_frame_offsets, const uint32_t* d_n_frames,
    const void* d_workspace)
{
    if (channels == 0 || channels > 255)
        return fail(SELA_HIP_EINVAL, "channels must be in 1..255");
    if (!d_frame_offsets || !d_n_frames || !d_workspace || (payload_bytes && !d_payload))
        return fail(SELA_HIP_EINVAL, "null device pointer");
    if ((uintptr_t)d_payload & 3)
        return fail(SELA_HIP_EINVAL, "d_payload must be 4-byte aligned");
    if (payload_bytes / 4 >= 0xFFFFFFFFull)
        return fail(SELA_HIP_EINVAL, "payloads of 16 GiB and more are not indexed on the device (32-bit word indices)");
    return SELA_HIP_OK;
}
} // namespace

int sela_hip_decode_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames, uint32_t channels,
    int16_t* d_pcm_out, uint32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream)
{
    if (channels == 0 || channels > 255)
        return fail(SELA_HIP_EINVAL, "channels must be in 1..255");
    if (channels > sela::decode_max_channels())
        return fail(SELA_HIP_EINVAL, "too many channels for the on-chip decoder (sela_hip_decode_max_channels)");
    if (!d_status || (n_frames && (!d_frames || !d_frame_offsets || !d_pcm_out || !d_workspace)))
        return fail(SELA_HIP_EINVAL, "null device pointer");
    if ((uintptr_t)d_frames & 3)
        return fail(SELA_HIP_EINVAL, "d_frames must be 4-byte aligned");
    if (workspace_bytes < sela::decode_workspace_bytes(n_frames, channels))
        return fail(SELA_HIP_ECAPACITY, "workspace smaller than sela_hip_decode_workspace_bytes()");
    return decode_device_launch(d_frames, d_frame_offsets, n_frames, channels, d_pcm_out, d_status, d_workspace, stream, nullptr);
}

size_t sela_hip_index_workspace_bytes(size_t payload_bytes, uint32_t max_frames)
{
    (void)max_frames; // (every word of the payload may be a candidate, whatever the cap)
    return sela::index_workspace_bytes(payload_bytes);
}

int sela_hip_index_frames_device(const uint8_t* d_payload, size_t payload_bytes, uint32_t max_frames, uint32_t channels,
    uint64_t* d_frame_offsets, uint32_t* d_n_frames, void* d_workspace, size_t workspace_bytes, void* stream)
{
    const int rc = check_index_args(d_payload, payload_bytes, channels, d_frame_offsets, d_n_frames, d_workspace);
    if (rc != SELA_HIP_OK)
        return rc;
    if (workspace_bytes < sela::index_workspace_bytes(payload_bytes))
        return fail(SELA_HIP_ECAPACITY, "workspace smaller than sela_hip_index_workspace_bytes()");
    return launched(sela::launch_index(d_payload, payload_bytes, max_frames, channels, d_frame_offsets, d_n_frames, d_workspace, static_cast<hipStream_t>(stream)),
        "index launch");
}

int sela_hip_decode_payload_device(const uint8_t* d_payload, size_t payload_bytes, uint32_t max_frames, uint32_t channels,
    int16_t* d_pcm_out, uint64_t* d_frame_offsets, uint32_t* d_n_frames, uint32_t* d_status, void* d_workspace, size_t workspace_bytes,
    void* stream)
{
    const int rc = check_index_args(d_payload, payload_bytes, channels, d_frame_offsets, d_n_frames, d_workspace);
    if (rc != SELA_HIP_OK)
        return rc;
    if (channels > sela::decode_max_channels())
        return fail(SELA_HIP_EINVAL, "too many channels for the on-chip decoder (sela_hip_decode_max_channels)");
    if (!d_status || (max_frames && !d_pcm_out))
        return fail(SELA_HIP_EINVAL, "null device pointer");
    const PayloadWs ws = carve_payload(d_workspace, payload_bytes, sela::decode_workspace_bytes(max_frames, channels));
    if (workspace_bytes < ws.end)
        return fail(SELA_HIP_ECAPACITY, "workspace smaller than sela_hip_index_workspace_bytes() + sela_hip_decode_workspace_bytes()");
    const hipError_t e = sela::launch_index(d_payload, payload_bytes, max_frames, channels, d_frame_offsets, d_n_frames, d_workspace,
        static_cast<hipStream_t>(stream));
    if (e != hipSuccess)
        return fail_hip(e, "index launch");
    return decode_device_launch(d_payload, d_frame_offsets, max_frames, channels, d_pcm_out, d_status, ws.own, stream, d_n_frames);
}

// ---- salvage: the frames of a damaged payload (the walk: sela_salvage_walk.h, the device: sela_salvage.hip) ------
uint32_t sela_hip_salvage_frames(const uint8_t* payload, size_t payload_bytes, uint32_t max_frames, uint32_t channels, sela_hip_salvaged* records,
    uint64_t* totals)
{
    return sela::salvage_walk(payload, payload_bytes, max_frames, channels, records, totals);
}

size_t sela_hip_salvage_workspace_bytes(size_t payload_bytes, uint32_t max_frames)
{
    return sela::salvage_workspace_bytes(payload_bytes, max_frames);
}

namespace {
// both salvage calls' checks: the index's cases and codes; d_out null for the walk alone
int salvage_call(const uint8_t* d_payload, size_t payload_bytes, uint32_t max_frames, uint32_t channels, uint8_t* d_out, size_t out_cap, uint64_t* d_frame_offsets,
    sela_hip_salvaged* d_records, uint64_t* d_totals, void* d_workspace, size_t workspace_bytes, void* stream, bool copy, bool unaligned = false)
{
    if (channels == 0 || channels > 255)
        return fail(SELA_HIP_EINVAL, "channels must be in 1..255");
    if (!d_totals || !d_workspace || (payload_bytes && !d_payload) || (!copy && max_frames && !d_records) || (copy && (!d_frame_offsets || (out_cap && !d_out))))
        return fail(SELA_HIP_EINVAL, "null device pointer");
    if ((uintptr_t)d_payload & 3)
        return fail(SELA_HIP_EINVAL, "d_payload must be 4-byte aligned");
    if (copy && ((uintptr_t)d_out & 3))
        return fail(SELA_HIP_EINVAL, "d_out must be 4-byte aligned");
    if (unaligned && (uint64_t)payload_bytes >= (1ull << 32))
        return fail(SELA_HIP_EINVAL, "payloads of 4 GiB and more are not salvaged at any byte on the device (32-bit byte offsets)");
    if (payload_bytes / 4 >= 0xFFFFFFFFull)
        return fail(SELA_HIP_EINVAL, "payloads of 16 GiB and more are not indexed on the device (32-bit word indices)");
    if (copy && out_cap && payload_bytes && (uintptr_t)d_out < (uintptr_t)d_payload + payload_bytes && (uintptr_t)d_payload < (uintptr_t)d_out + out_cap)
        return fail(SELA_HIP_EINVAL, "d_out must not overlap the payload");
    if (unaligned) {
        if (workspace_bytes < sela::salvage_unaligned_workspace_bytes(payload_bytes, max_frames))
            return fail(SELA_HIP_ECAPACITY, "workspace smaller than sela_hip_salvage_unaligned_workspace_bytes()");
        return launched(sela::launch_salvage_unaligned(d_payload, payload_bytes, max_frames, channels, d_records, d_totals, copy && out_cap ? d_out : nullptr,
                            out_cap, d_frame_offsets, d_workspace, static_cast<hipStream_t>(stream)),
            "salvage launch");
    }
    if (workspace_bytes < sela::salvage_workspace_bytes(payload_bytes, max_frames))
        return fail(SELA_HIP_ECAPACITY, "workspace smaller than sela_hip_salvage_workspace_bytes()");
    return launched(sela::launch_salvage(d_payload, payload_bytes, max_frames, channels, d_records, d_totals, copy && out_cap ? d_out : nullptr, out_cap,
                        d_frame_offsets, d_workspace, static_cast<hipStream_t>(stream)),
        "salvage launch");
}
} // namespace

int sela_hip_salvage_frames_device(const uint8_t* d_payload, size_t payload_bytes, uint32_t max_frames, uint32_t channels, sela_hip_salvaged* d_records,
    uint64_t* d_totals, void* d_workspace, size_t workspace_bytes, void* stream)
{
    return salvage_call(d_payload, payload_bytes, max_frames, channels, nullptr, 0, nullptr, d_records, d_totals, d_workspace, workspace_bytes, stream, false);
}

int sela_hip_salvage_payload_device(const uint8_t* d_payload, size_t payload_bytes, uint32_t max_frames, uint32_t channels, uint8_t* d_out, size_t out_cap,
    uint64_t* d_frame_offsets, sela_hip_salvaged* d_records, uint64_t* d_totals, void* d_workspace, size_t workspace_bytes, void* stream)
{
    return salvage_call(d_payload, payload_bytes, max_frames, channels, d_out, out_cap, d_frame_offsets, d_records, d_totals, d_workspace, workspace_bytes, stream, true);
}

// ---- salvage at any byte (the walk: sela_salvage_walk_unaligned.h, the device: sela_salvage_unaligned.hip) ----------
uint32_t sela_hip_salvage_frames_unaligned(const uint8_t* payload, size_t payload_bytes, uint32_t max_frames, uint32_t channels, sela_hip_salvaged* records,
    uint64_t* totals)
{
    return sela::salvage_walk_unaligned(payload, payload_bytes, max_frames, channels, records, totals);
}

size_t sela_hip_salvage_unaligned_workspace_bytes(size_t payload_bytes, uint32_t max_frames)
{
    return sela::salvage_unaligned_workspace_bytes(payload_bytes, max_frames);
}

int sela_hip_salvage_frames_unaligned_device(const uint8_t* d_payload, size_t payload_bytes, uint32_t max_frames, uint32_t channels, sela_hip_salvaged* d_records,
    uint64_t* d_totals, void* d_workspace, size_t workspace_bytes, void* stream)
{
    return salvage_call(d_payload, payload_bytes, max_frames, channels, nullptr, 0, nullptr, d_records, d_totals, d_workspace, workspace_bytes, stream, false, true);
}

int sela_hip_salvage_payload_unaligned_device(const uint8_t* d_payload, size_t payload_bytes, uint32_t max_frames, uint32_t channels, uint8_t* d_out, size_t out_cap,
    uint64_t* d_frame_offsets, sela_hip_salvaged* d_records, uint64_t* d_totals, void* d_workspace, size_t workspace_bytes, void* stream)
{
    return salvage_call(d_payload, payload_bytes, max_frames, channels, d_out, out_cap, d_frame_offsets, d_records, d_totals, d_workspace, workspace_bytes, stream, true,
        true);
}

// ---- the decode and verify calls of any length on device pointers, each in two forms ---------------
// A call is its own check of its arguments, its workspace formula and its launch.  What it is given -- frames with their
// offsets, or a payload that the device indexes first -- is a FORM, and the form runs the call:
//   frames:  the call's check; d_frames and its offsets; the capacity; the launch.
//   payload: the index's checks; the call's check; the capacity of both workspaces; launch_index; the launch on the rest of the
//            workspace with the device's own count of frames.
// check: n_frames -> SELA_HIP_OK or the failure, reported; launch: (d_frames, d_frame_offsets, max_frames, d_n_found, d_workspace)
// -> the same.  Nothing is allocated on the way to the launch.  (sela_hip_decode_device and its payload twin, above, check other
// things -- no stride, no pointer without frames -- and would need a shape of their own: they stay written out.)
extern "C++" {
namespace {
// Formula: (max_frames, channels, stride) -> bytes.  The calls sized by their table name their sela:: function; a call sized by
// something else (the windows) brings a closure over what it is sized by.
template <typename Formula>
struct DeviceCallOf {
    const char* name; // "decode_i32": the capacity's text names sela_hip_<name>_workspace_bytes()
    Formula workspace_bytes; // SIZE_MAX: more than any device holds
    uint32_t channels, stride;
    void* d_workspace;
    size_t capacity;
    hipStream_t stream;
};
using DeviceCall = DeviceCallOf<size_t (*)(uint32_t max_frames, uint32_t channels, uint32_t stride)>;

struct FramesForm {
    const uint8_t* d_frames;
    const uint64_t* d_frame_offsets;
    uint32_t n_frames;
    template <typename Formula, typename Check, typename Launch>
    int operator()(const DeviceCallOf<Formula>& c, Check check, Launch launch) const
    {
        const int rc = check(n_frames);
        if (rc != SELA_HIP_OK)
            return rc;
        if (!d_frame_offsets || (n_frames && !d_frames))
            return fail(SELA_HIP_EINVAL, "null device pointer");
        if ((uintptr_t)d_frames & 3)
            return fail(SELA_HIP_EINVAL, "d_frames must be 4-byte aligned");
        const size_t need = c.workspace_bytes(n_frames, c.channels, c.stride);
        if (need == SIZE_MAX || c.capacity < need)
            return fail(SELA_HIP_ECAPACITY, std::string("workspace smaller than sela_hip_") + c.name + "_workspace_bytes()");
        return launch(d_frames, d_frame_offsets, n_frames, static_cast<const uint32_t*>(nullptr), c.d_workspace);
    }
};

struct PayloadForm {
    const uint8_t* d_payload;
    size_t payload_bytes;
    uint32_t max_frames;
    uint64_t* d_frame_offsets;
    uint32_t* d_n_frames;
    template <typename Formula, typename Check, typename Launch>
    int operator()(const DeviceCallOf<Formula>& c, Check check, Launch launch) const
    {
        int rc = check_index_args(d_payload, payload_bytes, c.channels, d_frame_offsets, d_n_frames, c.d_workspace);
        if (rc == SELA_HIP_OK)
            rc = check(max_frames);
        if (rc != SELA_HIP_OK)
            return rc;
        const size_t own_bytes = c.workspace_bytes(max_frames, c.channels, c.stride);
        const PayloadWs ws = carve_payload(c.d_workspace, payload_bytes, own_bytes == SIZE_MAX ? 0 : own_bytes);
        if (own_bytes == SIZE_MAX || c.capacity < ws.end)
            return fail(SELA_HIP_ECAPACITY, std::string("workspace smaller than sela_hip_index_workspace_bytes() + sela_hip_") + c.name + "_workspace_bytes()");
        rc = launched(sela::launch_index(d_payload, payload_bytes, max_frames, c.channels, d_frame_offsets, d_n_frames, c.d_workspace, c.stream), "index launch");
        if (rc != SELA_HIP_OK)
            return rc;
        return launch(d_payload, d_frame_offsets, max_frames, d_n_frames, ws.own);
    }
};

// what every one of these calls checks first, and how it says that a pointer is missing
int check_frames_shape(uint32_t n_frames, uint32_t channels, uint32_t stride)
{
    if (channels == 0 || channels > 255)
        return fail(SELA_HIP_EINVAL, "channels must be in 1..255");
    if (stride == 0)
        return fail(SELA_HIP_EINVAL, "stride must not be 0");
    if ((uint64_t)n_frames * channels >= (1ull << 31))
        return fail(SELA_HIP_EINVAL, "n_frames * channels must stay below 2^31");
    return SELA_HIP_OK;
}
int need_pointers(bool all_there) { return all_there ? SELA_HIP_OK : fail(SELA_HIP_EINVAL, "null device pointer"); }

// sela_hip_decode_i32_device / sela_hip_decode_payload_i32_device (5.11)
template <typename Form>
int decode_i32_call(const Form& form, uint32_t channels, uint32_t stride, int32_t* d_samples_out, uint32_t* d_counts_out, uint64_t* d_sample_offsets,
    uint32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream)
{
    const DeviceCall c = { "decode_i32", sela::decode_i32_workspace_bytes, channels, stride, d_workspace, workspace_bytes, static_cast<hipStream_t>(stream) };
    return form(
        c,
        [&](uint32_t n_frames) {
            const int rc = check_frames_shape(n_frames, channels, stride);
            return rc != SELA_HIP_OK ? rc : need_pointers(d_status && d_workspace && (!n_frames || (d_samples_out && d_counts_out)));
        },
        [&](const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t max_frames, const uint32_t* d_n_found, void* d_ws) {
            return launched(sela::launch_decode_i32_device(d_frames, d_frame_offsets, max_frames, d_n_found, channels, stride, d_samples_out, d_counts_out,
                                d_sample_offsets, d_status, d_ws, sela::generic_standard_first_mode(), c.stream),
                "decode_i32 launch");
        });
}

// sela_hip_decode_n_device / sela_hip_decode_payload_n_device (5.13)
template <typename Form>
int decode_n_call(const Form& form, uint32_t channels, uint32_t stride, int16_t* d_pcm_out, uint64_t* d_sample_offsets, uint32_t* d_status, void* d_workspace,
    size_t workspace_bytes, void* stream)
{
    const DeviceCall c = { "decode_n", sela::decode_n_workspace_bytes, channels, stride, d_workspace, workspace_bytes, static_cast<hipStream_t>(stream) };
    return form(
        c,
        [&](uint32_t n_frames) {
            const int rc = check_frames_shape(n_frames, channels, stride);
            return rc != SELA_HIP_OK ? rc : need_pointers(d_status && d_workspace && (!n_frames || d_pcm_out));
        },
        [&](const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t max_frames, const uint32_t* d_n_found, void* d_ws) {
            return launch_with_priorities(max_frames, stream, "decode_n launch", [&](uint32_t synth_priorities) {
                return sela::launch_decode_n_device(d_frames, d_frame_offsets, max_frames, d_n_found, channels, stride, d_pcm_out, d_sample_offsets, d_status, d_ws,
                    sela::generic_standard_first_mode(), g_recurrence_form, synth_priorities, c.stream);
            });
        });
}

// sela_hip_verify_device / sela_hip_verify_payload_device (5.14): the decode_n call with the compare's arrays
template <typename Form>
int verify_call(const Form& form, uint32_t channels, uint32_t stride, const int16_t* d_pcm, uint32_t* d_diff_counts, uint32_t* d_first_diff,
    uint64_t* d_sample_offsets, uint32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream)
{
    const DeviceCall c = { "verify", sela::verify_workspace_bytes, channels, stride, d_workspace, workspace_bytes, static_cast<hipStream_t>(stream) };
    return form(
        c,
        [&](uint32_t n_frames) {
            int rc = check_frames_shape(n_frames, channels, stride);
            if (rc == SELA_HIP_OK)
                rc = need_pointers(d_status && d_workspace && (!n_frames || (d_pcm && d_diff_counts && d_first_diff)));
            if (rc == SELA_HIP_OK && (((uintptr_t)d_pcm & 1) || ((uintptr_t)d_diff_counts & 3) || ((uintptr_t)d_first_diff & 3)))
                rc = fail(SELA_HIP_EINVAL, "d_pcm must be 2-byte aligned, d_diff_counts and d_first_diff 4-byte aligned");
            return rc;
        },
        [&](const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t max_frames, const uint32_t* d_n_found, void* d_ws) {
            return launch_with_priorities(max_frames, stream, "verify launch", [&](uint32_t synth_priorities) {
                return sela::launch_verify_n_device(d_frames, d_frame_offsets, max_frames, d_n_found, channels, stride, d_pcm, d_diff_counts, d_first_diff,
                    d_sample_offsets, d_status, d_ws, sela::generic_standard_first_mode(), g_recurrence_form, synth_priorities, c.stream);
            });
        });
}

// sela_hip_levels_device / sela_hip_levels_payload_device (5.26): the verify call with the records for the compare's arrays
template <typename Form>
int levels_call(const Form& form, uint32_t channels, uint32_t stride, sela_hip_level* d_levels, uint64_t* d_sample_offsets, uint32_t* d_status, void* d_workspace,
    size_t workspace_bytes, void* stream)
{
    const DeviceCall c = { "levels", sela::levels_workspace_bytes, channels, stride, d_workspace, workspace_bytes, static_cast<hipStream_t>(stream) };
    return form(
        c,
        [&](uint32_t n_frames) {
            int rc = check_frames_shape(n_frames, channels, stride);
            if (rc == SELA_HIP_OK)
                rc = need_pointers(d_status && d_workspace && (!n_frames || d_levels));
            if (rc == SELA_HIP_OK && ((uintptr_t)d_levels & 7))
                rc = fail(SELA_HIP_EINVAL, "d_levels must be 8-byte aligned");
            return rc;
        },
        [&](const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t max_frames, const uint32_t* d_n_found, void* d_ws) {
            return launch_with_priorities(max_frames, stream, "levels launch", [&](uint32_t synth_priorities) {
                return sela::launch_levels_n_device(d_frames, d_frame_offsets, max_frames, d_n_found, channels, stride, d_levels, d_sample_offsets, d_status, d_ws,
                    sela::generic_standard_first_mode(), g_recurrence_form, synth_priorities, c.stream);
            });
        });
}

// sela_hip_digest_device / sela_hip_digest_payload_device (5.28): levels_call's checks in its order, with the track's two words
template <typename Form>
int digest_call(const Form& form, uint32_t channels, uint32_t stride, struct sela_hip_digest* d_digests, uint64_t* d_track, uint64_t* d_sample_offsets,
    uint32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream)
{
    const DeviceCall c = { "digest", sela::digest_workspace_bytes, channels, stride, d_workspace, workspace_bytes, static_cast<hipStream_t>(stream) };
    return form(
        c,
        [&](uint32_t n_frames) {
            int rc = check_frames_shape(n_frames, channels, stride);
            if (rc == SELA_HIP_OK)
                rc = need_pointers(d_status && d_workspace && d_track && (!n_frames || d_digests));
            if (rc == SELA_HIP_OK && (((uintptr_t)d_digests & 7) || ((uintptr_t)d_track & 7)))
                rc = fail(SELA_HIP_EINVAL, "d_digests and d_track must be 8-byte aligned");
            return rc;
        },
        [&](const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t max_frames, const uint32_t* d_n_found, void* d_ws) {
            return launch_with_priorities(max_frames, stream, "digest launch", [&](uint32_t synth_priorities) {
                return sela::launch_digest_n_device(d_frames, d_frame_offsets, max_frames, d_n_found, channels, stride, d_digests, d_track, d_sample_offsets, d_status,
                    d_ws, sela::generic_standard_first_mode(), g_recurrence_form, synth_priorities, c.stream);
            });
        });
}

// sela_hip_envelope_device / sela_hip_envelope_payload_device (5.31): levels_call's checks in its order, the bucket with the shape;
// the workspace is the levels call's
template <typename Form>
int envelope_call(const Form& form, uint32_t channels, uint32_t stride, uint32_t bucket, struct sela_hip_envelope* d_env, uint64_t* d_sample_offsets, uint32_t* d_status,
    void* d_workspace, size_t workspace_bytes, void* stream)
{
    const DeviceCall c = { "envelope", sela::levels_workspace_bytes, channels, stride, d_workspace, workspace_bytes, static_cast<hipStream_t>(stream) };
    return form(
        c,
        [&](uint32_t n_frames) {
            int rc = check_frames_shape(n_frames, channels, stride);
            if (rc == SELA_HIP_OK && !sela::envelope_bucket_ok(bucket))
                rc = fail(SELA_HIP_EINVAL, "bucket must be one of 32, 64, 128, 256, 512, 1024, 2048");
            if (rc == SELA_HIP_OK)
                rc = need_pointers(d_status && d_workspace && (!n_frames || d_env));
            if (rc == SELA_HIP_OK && ((uintptr_t)d_env & 7))
                rc = fail(SELA_HIP_EINVAL, "d_env must be 8-byte aligned");
            return rc;
        },
        [&](const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t max_frames, const uint32_t* d_n_found, void* d_ws) {
            return launch_with_priorities(max_frames, stream, "envelope launch", [&](uint32_t synth_priorities) {
                return sela::launch_envelope_n_device(d_frames, d_frame_offsets, max_frames, d_n_found, channels, stride, bucket, d_env, d_sample_offsets, d_status, d_ws,
                    sela::generic_standard_first_mode(), g_recurrence_form, synth_priorities, c.stream);
            });
        });
}

// sela_hip_digest_pcm_device / sela_hip_digest_payload_pcm_device (5.29): digest_call's checks in its order, then the container's, as
// in verify_pcm_call; the decode_i32 call's launch shape
template <typename Form>
int digest_pcm_call(const Form& form, uint32_t channels, uint32_t stride, uint32_t bytes_per_sample, struct sela_hip_digest* d_digests, uint64_t* d_track,
    uint64_t* d_sample_offsets, uint32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream)
{
    const DeviceCall c = { "digest_pcm", sela::digest_pcm_workspace_bytes, channels, stride, d_workspace, workspace_bytes, static_cast<hipStream_t>(stream) };
    return form(
        c,
        [&](uint32_t n_frames) {
            int rc = check_frames_shape(n_frames, channels, stride);
            if (rc == SELA_HIP_OK)
                rc = need_pointers(d_status && d_workspace && d_track && (!n_frames || d_digests));
            if (rc == SELA_HIP_OK && (((uintptr_t)d_digests & 7) || ((uintptr_t)d_track & 7)))
                rc = fail(SELA_HIP_EINVAL, "d_digests and d_track must be 8-byte aligned");
            if (rc == SELA_HIP_OK && bytes_per_sample != 3 && bytes_per_sample != 4)
                rc = fail(SELA_HIP_EINVAL, "bytes_per_sample must be 3 or 4 (16-bit samples: sela_hip_digest_device)");
            if (rc == SELA_HIP_OK && ((uintptr_t)d_sample_offsets & 7))
                rc = fail(SELA_HIP_EINVAL, "d_sample_offsets must be 8-byte aligned");
            return rc;
        },
        [&](const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t max_frames, const uint32_t* d_n_found, void* d_ws) {
            return launched(sela::launch_digest_pcm_device(d_frames, d_frame_offsets, max_frames, d_n_found, channels, stride, bytes_per_sample, d_digests, d_track,
                                d_sample_offsets, d_status, d_ws, sela::generic_standard_first_mode(), c.stream),
                "digest_pcm launch");
        });
}

// The shape checks of the int16 window calls, device and host pointers alike (5.17, 5.20): codes and texts in this order.
// `more_channels` is the call that a caller with more than eight channels is sent to.
int check_windows_shape(uint32_t channels, uint32_t n_windows, uint32_t window_samples, uint32_t format, const char* more_channels)
{
    if (channels == 0 || channels > 8)
        return fail(SELA_HIP_EINVAL, std::string("channels must be in 1..8: the windows are cut from the on-chip decoder's second pass (more channels: ") + more_channels + ", then crop)");
    if (window_samples == 0 || window_samples > (1u << 24))
        return fail(SELA_HIP_EINVAL, "window_samples must be in 1..2^24");
    if (format != SELA_HIP_WINDOW_I16_INTERLEAVED && format != SELA_HIP_WINDOW_F32_PLANAR)
        return fail(SELA_HIP_EINVAL, "format must be SELA_HIP_WINDOW_I16_INTERLEAVED or SELA_HIP_WINDOW_F32_PLANAR");
    if ((uint64_t)n_windows * sela::window_cover(window_samples) >= (1ull << 31))
        return fail(SELA_HIP_EINVAL, "n_windows * cover must stay below 2^31 (cover = (window_samples + 2046) / 2048 + 1)");
    return SELA_HIP_OK;
}
// sela_hip_decode_windows_device (5.17), in the frames form: the table is the form's, the windows are the call's.  Its workspace
// is sized by the windows and not by the table, so its formula is sela_hip_decode_windows_workspace_bytes itself, closed over
// the call's own arguments (the form asks it only after the check has passed them); the call has no stride.
int windows_call(const FramesForm& form, uint32_t channels, const sela_hip_window* d_windows, uint32_t n_windows, uint32_t window_samples, uint32_t format,
    void* d_out, uint32_t* d_window_flags, uint32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream, bool whole /* 5.20: the same checks, the long last frame's kernels behind */)
{
    const auto formula = [=](uint32_t /* the table's frames */, uint32_t, uint32_t) {
        return whole ? sela::window_whole_workspace_bytes(n_windows, window_samples, channels) : sela::window_workspace_bytes(n_windows, window_samples, channels);
    };
    const DeviceCallOf<decltype(formula)> c = { whole ? "decode_windows_whole" : "decode_windows", formula, channels, 0, d_workspace, workspace_bytes, static_cast<hipStream_t>(stream) };
    return form(
        c,
        [&](uint32_t) {
            int rc = check_windows_shape(channels, n_windows, window_samples, format, "sela_hip_decode_device");
            if (rc == SELA_HIP_OK)
                rc = need_pointers(d_status && (!n_windows || (d_windows && d_out && d_workspace)));
            if (rc == SELA_HIP_OK && (((uintptr_t)d_windows & 7) || ((uintptr_t)d_out & (format == SELA_HIP_WINDOW_F32_PLANAR ? 3 : 1)) || ((uintptr_t)d_window_flags & 3) || ((uintptr_t)d_status & 3)))
                rc = fail(SELA_HIP_EINVAL, "d_windows must be 8-byte aligned, d_out aligned to its element, d_window_flags and d_status 4-byte aligned");
            return rc;
        },
        [&](const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames_total, const uint32_t*, void* d_ws) {
            return launch_with_priorities(n_windows * sela::window_cover(window_samples), stream, "decode_windows launch", [&](uint32_t synth_priorities) {
                const auto launch = whole ? sela::launch_window_whole : sela::launch_window_frames;
                return launch(d_frames, d_frame_offsets, n_frames_total, channels, d_windows, n_windows,
                    window_samples, format, d_out, d_window_flags, d_status, d_ws, c.stream, g_recurrence_form, synth_priorities);
            });
        });
}

// The shape checks of the 24- and 32-bit window calls, device and host pointers alike (5.23, 5.25): check_windows_shape's order
// and codes -- the format's place holds the wider formats and F32's sample_bits, the product counts the channels too (a wave per
// subframe) and is followed by a bound on n_windows alone (the store's grid).
int check_windows_i32_shape(uint32_t channels, uint32_t n_windows, uint32_t window_samples, uint32_t format, uint32_t sample_bits)
{
    if (channels == 0 || channels > 8)
        return fail(SELA_HIP_EINVAL, "channels must be in 1..8: a frame's subframes are combined in one workgroup's table (more channels: sela_hip_decode_i32_device, then crop)");
    if (window_samples == 0 || window_samples > (1u << 24))
        return fail(SELA_HIP_EINVAL, "window_samples must be in 1..2^24");
    if (format < SELA_HIP_WINDOW_F32_PLANAR || format > SELA_HIP_WINDOW_PCM32_INTERLEAVED)
        return fail(SELA_HIP_EINVAL, "format must be SELA_HIP_WINDOW_F32_PLANAR, _I32_PLANAR, _PCM24_INTERLEAVED or _PCM32_INTERLEAVED (int16: sela_hip_decode_windows_device)");
    if (format == SELA_HIP_WINDOW_F32_PLANAR && (sample_bits == 0 || sample_bits > 32))
        return fail(SELA_HIP_EINVAL, "sample_bits must be in 1..32 with SELA_HIP_WINDOW_F32_PLANAR");
    if ((uint64_t)n_windows * sela::window_cover(window_samples) * channels >= (1ull << 31))
        return fail(SELA_HIP_EINVAL, "n_windows * cover * channels must stay below 2^31 (cover = (window_samples + 2046) / 2048 + 1)");
    if (n_windows >= (1u << 24))
        return fail(SELA_HIP_EINVAL, "n_windows must stay below 2^24 (a workgroup of 256 per window and covering frame: a launch holds fewer than 2^32 work-items per dimension)");
    return SELA_HIP_OK;
}
// sela_hip_decode_windows_i32_device (5.23): windows_call with the wider formats; d_out is a dword's.
int windows_i32_call(const FramesForm& form, uint32_t channels, const sela_hip_window* d_windows, uint32_t n_windows, uint32_t window_samples, uint32_t format,
    uint32_t sample_bits, void* d_out, uint32_t* d_window_flags, uint32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream,
    bool whole /* 5.25: the same checks, the long last frame's kernels behind */)
{
    const auto formula = [=](uint32_t /* the table's frames */, uint32_t, uint32_t) {
        return whole ? sela::window32_whole_workspace_bytes(n_windows, window_samples, channels) : sela::window32_workspace_bytes(n_windows, window_samples, channels);
    };
    const DeviceCallOf<decltype(formula)> c = { whole ? "decode_windows_i32_whole" : "decode_windows_i32", formula, channels, 0, d_workspace, workspace_bytes, static_cast<hipStream_t>(stream) };
    return form(
        c,
        [&](uint32_t) {
            int rc = check_windows_i32_shape(channels, n_windows, window_samples, format, sample_bits);
            if (rc == SELA_HIP_OK)
                rc = need_pointers(d_status && (!n_windows || (d_windows && d_out && d_workspace)));
            if (rc == SELA_HIP_OK && (((uintptr_t)d_windows & 7) || ((uintptr_t)d_out & 3) || ((uintptr_t)d_window_flags & 3) || ((uintptr_t)d_status & 3)))
                rc = fail(SELA_HIP_EINVAL, "d_windows must be 8-byte aligned, d_out, d_window_flags and d_status 4-byte aligned");
            return rc;
        },
        [&](const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames_total, const uint32_t*, void* d_ws) {
            const auto launch = whole ? sela::launch_window32_whole : sela::launch_window32;
            return launched(launch(d_frames, d_frame_offsets, n_frames_total, channels, d_windows, n_windows, window_samples, format, sample_bits, d_out, d_window_flags,
                                d_status, d_ws, sela::generic_standard_first_mode() != 2, c.stream),
                "decode_windows_i32 launch");
        });
}

// sela_hip_verify_i32_device / sela_hip_verify_payload_i32_device (5.15): the decode_i32 call with the compare's arrays
template <typename Form>
int verify_i32_call(const Form& form, uint32_t channels, uint32_t stride, const int32_t* d_samples, const uint32_t* d_lengths, uint32_t* d_diff_counts,
    uint32_t* d_first_diff, uint64_t* d_sample_offsets, uint32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream)
{
    const DeviceCall c = { "verify_i32", sela::verify_i32_workspace_bytes, channels, stride, d_workspace, workspace_bytes, static_cast<hipStream_t>(stream) };
    return form(
        c,
        [&](uint32_t n_frames) {
            int rc = check_frames_shape(n_frames, channels, stride);
            if (rc == SELA_HIP_OK)
                rc = need_pointers(d_status && d_workspace && (!n_frames || (d_samples && d_diff_counts && d_first_diff)));
            if (rc == SELA_HIP_OK && (((uintptr_t)d_samples & 3) || ((uintptr_t)d_lengths & 3) || ((uintptr_t)d_diff_counts & 3) || ((uintptr_t)d_first_diff & 3)))
                rc = fail(SELA_HIP_EINVAL, "d_samples, d_lengths, d_diff_counts and d_first_diff must be 4-byte aligned");
            return rc;
        },
        [&](const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t max_frames, const uint32_t* d_n_found, void* d_ws) {
            return launched(sela::launch_verify_i32_device(d_frames, d_frame_offsets, max_frames, d_n_found, channels, stride, d_samples, d_lengths, d_diff_counts,
                                d_first_diff, d_sample_offsets, d_status, d_ws, sela::generic_standard_first_mode(), c.stream),
                "verify_i32 launch");
        });
}

// sela_hip_levels_i32_device / sela_hip_levels_payload_i32_device (5.27): levels_call's checks in its order, the decode_i32 call's launch shape
template <typename Form>
int levels_i32_call(const Form& form, uint32_t channels, uint32_t stride, sela_hip_level32* d_levels, uint64_t* d_sample_offsets, uint32_t* d_status,
    void* d_workspace, size_t workspace_bytes, void* stream)
{
    const DeviceCall c = { "levels_i32", sela::levels_i32_workspace_bytes, channels, stride, d_workspace, workspace_bytes, static_cast<hipStream_t>(stream) };
    return form(
        c,
        [&](uint32_t n_frames) {
            int rc = check_frames_shape(n_frames, channels, stride);
            if (rc == SELA_HIP_OK)
                rc = need_pointers(d_status && d_workspace && (!n_frames || d_levels));
            if (rc == SELA_HIP_OK && ((uintptr_t)d_levels & 7))
                rc = fail(SELA_HIP_EINVAL, "d_levels must be 8-byte aligned");
            return rc;
        },
        [&](const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t max_frames, const uint32_t* d_n_found, void* d_ws) {
            return launched(sela::launch_levels_i32_device(d_frames, d_frame_offsets, max_frames, d_n_found, channels, stride, d_levels, d_sample_offsets, d_status, d_ws,
                                sela::generic_standard_first_mode(), c.stream),
                "levels_i32 launch");
        });
}

// sela_hip_envelope_i32_device / sela_hip_envelope_payload_i32_device (5.32): levels_i32_call's checks in its order, the bucket with
// the shape as in envelope_call; the workspace is the verify_i32 call's
template <typename Form>
int envelope_i32_call(const Form& form, uint32_t channels, uint32_t stride, uint32_t bucket, struct sela_hip_envelope32* d_env, uint64_t* d_sample_offsets,
    uint32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream)
{
    const DeviceCall c = { "envelope_i32", sela::envelope_i32_workspace_bytes, channels, stride, d_workspace, workspace_bytes, static_cast<hipStream_t>(stream) };
    return form(
        c,
        [&](uint32_t n_frames) {
            int rc = check_frames_shape(n_frames, channels, stride);
            if (rc == SELA_HIP_OK && !sela::envelope_bucket_ok(bucket))
                rc = fail(SELA_HIP_EINVAL, "bucket must be one of 32, 64, 128, 256, 512, 1024, 2048");
            if (rc == SELA_HIP_OK)
                rc = need_pointers(d_status && d_workspace && (!n_frames || d_env));
            if (rc == SELA_HIP_OK && ((uintptr_t)d_env & 7))
                rc = fail(SELA_HIP_EINVAL, "d_env must be 8-byte aligned");
            return rc;
        },
        [&](const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t max_frames, const uint32_t* d_n_found, void* d_ws) {
            return launched(sela::launch_envelope_i32_device(d_frames, d_frame_offsets, max_frames, d_n_found, channels, stride, bucket, d_env, d_sample_offsets, d_status,
                                d_ws, sela::generic_standard_first_mode(), c.stream),
                "envelope_i32 launch");
        });
}

// sela_hip_verify_pcm_device / sela_hip_verify_payload_pcm_device (5.24): the verify_i32 call's checks in its order, then the
// container's and the original's alignment
template <typename Form>
int verify_pcm_call(const Form& form, uint32_t channels, uint32_t stride, const void* d_pcm, uint32_t bytes_per_sample, uint64_t pcm_samples, uint32_t* d_diff_counts,
    uint32_t* d_first_diff, uint64_t* d_sample_offsets, uint32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream)
{
    const DeviceCall c = { "verify_pcm", sela::verify_pcm_workspace_bytes, channels, stride, d_workspace, workspace_bytes, static_cast<hipStream_t>(stream) };
    return form(
        c,
        [&](uint32_t n_frames) {
            int rc = check_frames_shape(n_frames, channels, stride);
            if (rc == SELA_HIP_OK)
                rc = need_pointers(d_status && d_workspace && (!n_frames || (d_pcm && d_diff_counts && d_first_diff)));
            if (rc == SELA_HIP_OK && (((uintptr_t)d_diff_counts & 3) || ((uintptr_t)d_first_diff & 3)))
                rc = fail(SELA_HIP_EINVAL, "d_diff_counts and d_first_diff must be 4-byte aligned");
            if (rc == SELA_HIP_OK && bytes_per_sample != 3 && bytes_per_sample != 4)
                rc = fail(SELA_HIP_EINVAL, "bytes_per_sample must be 3 or 4 (16-bit samples: sela_hip_verify_device)");
            if (rc == SELA_HIP_OK && ((uintptr_t)d_pcm & 3))
                rc = fail(SELA_HIP_EINVAL, "d_pcm must be 4-byte aligned");
            if (rc == SELA_HIP_OK && ((uintptr_t)d_sample_offsets & 7))
                rc = fail(SELA_HIP_EINVAL, "d_sample_offsets must be 8-byte aligned");
            return rc;
        },
        [&](const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t max_frames, const uint32_t* d_n_found, void* d_ws) {
            return launched(sela::launch_verify_pcm_device(d_frames, d_frame_offsets, max_frames, d_n_found, channels, stride, d_pcm, bytes_per_sample, pcm_samples,
                                d_diff_counts, d_first_diff, d_sample_offsets, d_status, d_ws, sela::generic_standard_first_mode(), c.stream),
                "verify_pcm launch");
        });
}
} // namespace
} // extern "C++"

size_t sela_hip_decode_i32_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride)
{
    return sela::decode_i32_workspace_bytes(max_frames, channels, stride);
}

int sela_hip_decode_i32_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride,
    int32_t* d_samples_out, uint32_t* d_counts_out, uint64_t* d_sample_offsets, uint32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream)
{
    return decode_i32_call(FramesForm{ d_frames, d_frame_offsets, n_frames }, channels, stride, d_samples_out, d_counts_out, d_sample_offsets, d_status, d_workspace,
        workspace_bytes, stream);
}

int sela_hip_decode_payload_i32_device(const uint8_t* d_payload, size_t payload_bytes, uint32_t max_frames, uint32_t channels, uint32_t stride,
    int32_t* d_samples_out, uint32_t* d_counts_out, uint64_t* d_sample_offsets, uint64_t* d_frame_offsets, uint32_t* d_n_frames, uint32_t* d_status,
    void* d_workspace, size_t workspace_bytes, void* stream)
{
    return decode_i32_call(PayloadForm{ d_payload, payload_bytes, max_frames, d_frame_offsets, d_n_frames }, channels, stride, d_samples_out, d_counts_out,
        d_sample_offsets, d_status, d_workspace, workspace_bytes, stream);
}

// sela_hip_decode_i32's verdict on the device's status words
int sela_hip_decode_status_error(const uint32_t* status)
{
    if (!status)
        return fail(SELA_HIP_EINVAL, "null pointer");
    return sela::judge_decode(status[0] | (status[1] ? SELA_HIP_FLAG_BAD_FRAME : 0u), ~0u, sela::kRouteDevice32, "decode");
}

// ---- the any-length / 32-bit encode on device pointers ------------------------------------------
namespace {
// what sela_hip_encode_i32_device and sela_hip_encode_n_device check alike, then the launch; no lease, no coalescer, no wait
int encode_i32_device_call(const void* d_input, bool in16, uint32_t n_frames, uint32_t channels, uint32_t n, uint8_t* d_frames, size_t frames_cap,
    uint64_t* d_frame_offsets, uint32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream, bool lossless = false, bool paired = false)
{
    if (channels == 0 || channels > 255)
        return fail(SELA_HIP_EINVAL, "channels must be in 1..255");
    if (n == 0 || n > 65535)
        return fail(SELA_HIP_EINVAL, "samples_per_channel must be 1 .. 65535 (the subframe's field is 16 bits wide)");
    if ((uint64_t)n_frames * sela::generic_signals(channels, paired) >= (1ull << 31))
        return fail(SELA_HIP_EINVAL, "n_frames * signals per frame must stay below 2^31");
    if (!d_frame_offsets || !d_status || !d_workspace || (n_frames && (!d_input || !d_frames)))
        return fail(SELA_HIP_EINVAL, "null device pointer");
    if (((uintptr_t)d_frames & 3) || ((uintptr_t)d_input & (in16 ? 1 : 3)))
        return fail(SELA_HIP_EINVAL, "d_frames must be 4-byte aligned, the samples aligned to their type");
    if (workspace_bytes < sela::encode_i32_device_workspace_bytes(n_frames, channels, n, paired))
        return fail(SELA_HIP_ECAPACITY, paired ? "workspace smaller than sela_hip_encode_paired_workspace_bytes()" : "workspace smaller than sela_hip_encode_i32_workspace_bytes()");
    return launched(sela::launch_encode_i32_device(d_input, in16, n_frames, channels, n, d_frames, frames_cap, d_frame_offsets, d_status, d_workspace,
                        static_cast<hipStream_t>(stream), lossless, paired),
        paired ? "encode_paired launch" : "encode_i32 launch");
}

// what every paired call asks first: its own options word -- 0 or SELA_HIP_ENCODE_LOSSLESS
int paired_options(uint32_t options, bool* lossless)
{
    if (options & ~(uint32_t)SELA_HIP_ENCODE_LOSSLESS)
        return fail(SELA_HIP_EINVAL, "options: a paired call takes 0 or SELA_HIP_ENCODE_LOSSLESS");
    *lossless = options != 0;
    return SELA_HIP_OK;
}
} // namespace

size_t sela_hip_encode_i32_workspace_bytes(uint32_t n_frames, uint32_t channels, uint32_t samples_per_channel)
{
    return sela::encode_i32_device_workspace_bytes(n_frames, channels, samples_per_channel);
}

int sela_hip_encode_i32_device(const int32_t* d_samples, uint32_t n_frames, uint32_t channels, uint32_t samples_per_channel, uint8_t* d_frames, size_t frames_cap,
    uint64_t* d_frame_offsets, uint32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream)
{
    return encode_i32_device_call(d_samples, false, n_frames, channels, samples_per_channel, d_frames, frames_cap, d_frame_offsets, d_status, d_workspace,
        workspace_bytes, stream);
}

int sela_hip_encode_n_device(const int16_t* d_pcm, uint32_t n_frames, uint32_t channels, uint32_t samples_per_channel, uint8_t* d_frames, size_t frames_cap,
    uint64_t* d_frame_offsets, uint32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream)
{
    return encode_i32_device_call(d_pcm, true, n_frames, channels, samples_per_channel, d_frames, frames_cap, d_frame_offsets, d_status, d_workspace,
        workspace_bytes, stream);
}

int sela_hip_encode_i32_device_opt(const int32_t* d_samples, uint32_t n_frames, uint32_t channels, uint32_t samples_per_channel, uint8_t* d_frames, size_t frames_cap,
    uint64_t* d_frame_offsets, uint32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream, uint32_t options)
{
    bool lossless = false;
    const int rc = encode_options(options, &lossless);
    return rc != SELA_HIP_OK ? rc : encode_i32_device_call(d_samples, false, n_frames, channels, samples_per_channel, d_frames, frames_cap, d_frame_offsets, d_status,
                                        d_workspace, workspace_bytes, stream, lossless);
}

int sela_hip_encode_n_device_opt(const int16_t* d_pcm, uint32_t n_frames, uint32_t channels, uint32_t samples_per_channel, uint8_t* d_frames, size_t frames_cap,
    uint64_t* d_frame_offsets, uint32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream, uint32_t options)
{
    bool lossless = false;
    const int rc = encode_options(options, &lossless);
    return rc != SELA_HIP_OK ? rc : encode_i32_device_call(d_pcm, true, n_frames, channels, samples_per_channel, d_frames, frames_cap, d_frame_offsets, d_status,
                                        d_workspace, workspace_bytes, stream, lossless);
}

// ---- channel pairs: the any-length kernels over channels + channels / 2 signals -----------------------------
uint32_t sela_hip_paired_signals_per_frame(uint32_t channels) { return sela::generic_signals(channels, true); }

size_t sela_hip_encode_paired_workspace_bytes(uint32_t n_frames, uint32_t channels, uint32_t samples_per_channel)
{
    return sela::encode_i32_device_workspace_bytes(n_frames, channels, samples_per_channel, true);
}

int sela_hip_encode_paired_i32_device(const int32_t* d_samples, uint32_t n_frames, uint32_t channels, uint32_t samples_per_channel, uint8_t* d_frames,
    size_t frames_cap, uint64_t* d_frame_offsets, uint32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream, uint32_t options)
{
    bool lossless = false;
    const int rc = paired_options(options, &lossless);
    return rc != SELA_HIP_OK ? rc : encode_i32_device_call(d_samples, false, n_frames, channels, samples_per_channel, d_frames, frames_cap, d_frame_offsets, d_status,
                                        d_workspace, workspace_bytes, stream, lossless, true);
}

int sela_hip_encode_paired_n_device(const int16_t* d_pcm, uint32_t n_frames, uint32_t channels, uint32_t samples_per_channel, uint8_t* d_frames,
    size_t frames_cap, uint64_t* d_frame_offsets, uint32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream, uint32_t options)
{
    bool lossless = false;
    const int rc = paired_options(options, &lossless);
    return rc != SELA_HIP_OK ? rc : encode_i32_device_call(d_pcm, true, n_frames, channels, samples_per_channel, d_frames, frames_cap, d_frame_offsets, d_status,
                                        d_workspace, workspace_bytes, stream, lossless, true);
}

// the any-length route's verdict after its plan (generic_encode in sela_capi_generic.hip): the flags, then the capacity
int sela_hip_encode_status_error(const uint32_t* status)
{
    if (!status)
        return fail(SELA_HIP_EINVAL, "null pointer");
    const int rc = sela::judge_encode(status[0], sela::kJudgeEncode, "encode");
    if (rc != SELA_HIP_OK)
        return rc;
    if (status[1])
        return fail(SELA_HIP_ECAPACITY, "d_frames too small: status[1] frames were not written (d_frame_offsets[n_frames] bytes are needed)");
    return SELA_HIP_OK;
}

size_t sela_hip_decode_n_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride)
{
    return sela::decode_n_workspace_bytes(max_frames, channels, stride);
}

int sela_hip_decode_n_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride,
    int16_t* d_pcm_out, uint64_t* d_sample_offsets, uint32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream)
{
    return decode_n_call(FramesForm{ d_frames, d_frame_offsets, n_frames }, channels, stride, d_pcm_out, d_sample_offsets, d_status, d_workspace, workspace_bytes, stream);
}

int sela_hip_decode_payload_n_device(const uint8_t* d_payload, size_t payload_bytes, uint32_t max_frames, uint32_t channels, uint32_t stride,
    int16_t* d_pcm_out, uint64_t* d_sample_offsets, uint64_t* d_frame_offsets, uint32_t* d_n_frames, uint32_t* d_status, void* d_workspace,
    size_t workspace_bytes, void* stream)
{
    return decode_n_call(PayloadForm{ d_payload, payload_bytes, max_frames, d_frame_offsets, d_n_frames }, channels, stride, d_pcm_out, d_sample_offsets, d_status,
        d_workspace, workspace_bytes, stream);
}

// sela_hip_decode's verdict, by the route the device took (status[3]): the any-length route's as sela_hip_decode_i32's, the fast
// kernels' as the streaming job's, and a stream the header walk refused: malformed, whatever else it says
int sela_hip_decode_n_status_error(const uint32_t* status)
{
    if (!status)
        return fail(SELA_HIP_EINVAL, "null pointer");
    const uint32_t flags = status[0] | (status[1] ? SELA_HIP_FLAG_BAD_FRAME : 0u);
    if (status[3] == 2)
        return sela::judge_decode(flags, ~0u, sela::kRouteDevice32, "decode");
    if (status[3] == 1)
        return sela::judge_decode(flags, SELA_HIP_FLAG_STRIDE | sela::kJudgeJob, sela::kRouteFast, "decode");
    return sela::judge_decode(flags, SELA_HIP_FLAG_STRIDE | SELA_HIP_FLAG_BAD_FRAME, sela::kRouteWalk, "decode");
}

size_t sela_hip_verify_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride)
{
    return sela::verify_workspace_bytes(max_frames, channels, stride);
}

int sela_hip_verify_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride, const int16_t* d_pcm,
    uint32_t* d_diff_counts, uint32_t* d_first_diff, uint64_t* d_sample_offsets, uint32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream)
{
    return verify_call(FramesForm{ d_frames, d_frame_offsets, n_frames }, channels, stride, d_pcm, d_diff_counts, d_first_diff, d_sample_offsets, d_status, d_workspace,
        workspace_bytes, stream);
}

int sela_hip_verify_payload_device(const uint8_t* d_payload, size_t payload_bytes, uint32_t max_frames, uint32_t channels, uint32_t stride, const int16_t* d_pcm,
    uint32_t* d_diff_counts, uint32_t* d_first_diff, uint64_t* d_sample_offsets, uint64_t* d_frame_offsets, uint32_t* d_n_frames, uint32_t* d_status,
    void* d_workspace, size_t workspace_bytes, void* stream)
{
    return verify_call(PayloadForm{ d_payload, payload_bytes, max_frames, d_frame_offsets, d_n_frames }, channels, stride, d_pcm, d_diff_counts, d_first_diff,
        d_sample_offsets, d_status, d_workspace, workspace_bytes, stream);
}

// Host pointers, synchronous: on the any-length route's leased context and stream (generic_verify), past the coalescer; the
// calling thread's open streaming job lives in the fast path's context and is left alone.
int sela_hip_verify(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, const int16_t* pcm, uint32_t* diff_counts,
    uint32_t* first_diff, uint32_t* lossy_frames)
{
    if (channels == 0 || channels > 255)
        return fail(SELA_HIP_EINVAL, "channels must be in 1..255");
    if ((uint64_t)n_frames * channels >= (1ull << 31))
        return fail(SELA_HIP_EINVAL, "n_frames * channels must stay below 2^31");
    if (!frame_offsets || (n_frames && (!frames || !pcm || !diff_counts || !first_diff)))
        return fail(SELA_HIP_EINVAL, "null pointer");
    return sela::generic_verify(frames, frame_offsets, n_frames, channels, pcm, diff_counts, first_diff, lossy_frames, g_recurrence_form);
}

size_t sela_hip_levels_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride)
{
    return sela::levels_workspace_bytes(max_frames, channels, stride);
}

int sela_hip_levels_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride, sela_hip_level* d_levels,
    uint64_t* d_sample_offsets, uint32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream)
{
    return levels_call(FramesForm{ d_frames, d_frame_offsets, n_frames }, channels, stride, d_levels, d_sample_offsets, d_status, d_workspace, workspace_bytes, stream);
}

int sela_hip_levels_payload_device(const uint8_t* d_payload, size_t payload_bytes, uint32_t max_frames, uint32_t channels, uint32_t stride, sela_hip_level* d_levels,
    uint64_t* d_sample_offsets, uint64_t* d_frame_offsets, uint32_t* d_n_frames, uint32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream)
{
    return levels_call(PayloadForm{ d_payload, payload_bytes, max_frames, d_frame_offsets, d_n_frames }, channels, stride, d_levels, d_sample_offsets, d_status,
        d_workspace, workspace_bytes, stream);
}

// Host pointers, synchronous: where sela_hip_verify runs (generic_levels); no frames need no device.
int sela_hip_levels(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, sela_hip_level* levels)
{
    if (channels == 0 || channels > 255)
        return fail(SELA_HIP_EINVAL, "channels must be in 1..255");
    if ((uint64_t)n_frames * channels >= (1ull << 31))
        return fail(SELA_HIP_EINVAL, "n_frames * channels must stay below 2^31");
    if (!frame_offsets || (n_frames && (!frames || !levels)))
        return fail(SELA_HIP_EINVAL, "null pointer");
    if (n_frames == 0)
        return SELA_HIP_OK;
    return sela::generic_levels(frames, frame_offsets, n_frames, channels, levels, g_recurrence_form);
}

// ---- envelope (5.31) ----------------------------------------------------------------------------------------------------------------
uint32_t sela_hip_envelope_slots(uint32_t stride, uint32_t bucket) { return sela::envelope_slots(stride, bucket); }

size_t sela_hip_envelope_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride)
{
    return sela::levels_workspace_bytes(max_frames, channels, stride);
}

int sela_hip_envelope_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride, uint32_t bucket,
    struct sela_hip_envelope* d_env, uint64_t* d_sample_offsets, uint32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream)
{
    return envelope_call(FramesForm{ d_frames, d_frame_offsets, n_frames }, channels, stride, bucket, d_env, d_sample_offsets, d_status, d_workspace, workspace_bytes,
        stream);
}

int sela_hip_envelope_payload_device(const uint8_t* d_payload, size_t payload_bytes, uint32_t max_frames, uint32_t channels, uint32_t stride, uint32_t bucket,
    struct sela_hip_envelope* d_env, uint64_t* d_sample_offsets, uint64_t* d_frame_offsets, uint32_t* d_n_frames, uint32_t* d_status, void* d_workspace, size_t workspace_bytes,
    void* stream)
{
    return envelope_call(PayloadForm{ d_payload, payload_bytes, max_frames, d_frame_offsets, d_n_frames }, channels, stride, bucket, d_env, d_sample_offsets, d_status,
        d_workspace, workspace_bytes, stream);
}

// Host pointers, synchronous: where sela_hip_levels runs (generic_envelope); no frames need no device.
int sela_hip_envelope(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride, uint32_t bucket,
    struct sela_hip_envelope* env)
{
    if (channels == 0 || channels > 255)
        return fail(SELA_HIP_EINVAL, "channels must be in 1..255");
    if (stride == 0)
        return fail(SELA_HIP_EINVAL, "stride must not be 0");
    if ((uint64_t)n_frames * channels >= (1ull << 31))
        return fail(SELA_HIP_EINVAL, "n_frames * channels must stay below 2^31");
    if (!sela::envelope_bucket_ok(bucket))
        return fail(SELA_HIP_EINVAL, "bucket must be one of 32, 64, 128, 256, 512, 1024, 2048");
    if ((uint64_t)sela::envelope_slots(stride, bucket) * channels > 0xFFFFFFFFull) // (the chunk loop counts a frame's records in 32 bits)
        return fail(SELA_HIP_EINVAL, "ceil(stride / bucket) * channels must fit 32 bits");
    if (!frame_offsets || (n_frames && (!frames || !env)))
        return fail(SELA_HIP_EINVAL, "null pointer");
    if (n_frames == 0)
        return SELA_HIP_OK;
    return sela::generic_envelope(frames, frame_offsets, n_frames, channels, stride, bucket, env, g_recurrence_form);
}

// ---- levels of 24- and 32-bit streams ------------------------------------------------------------------------
// ---- digest (5.28) ------------------------------------------------------------------------------------------------------------------
size_t sela_hip_digest_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride)
{
    return sela::digest_workspace_bytes(max_frames, channels, stride);
}

int sela_hip_digest_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride,
    struct sela_hip_digest* d_digests, uint64_t* d_track, uint64_t* d_sample_offsets, uint32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream)
{
    return digest_call(FramesForm{ d_frames, d_frame_offsets, n_frames }, channels, stride, d_digests, d_track, d_sample_offsets, d_status, d_workspace, workspace_bytes,
        stream);
}

int sela_hip_digest_payload_device(const uint8_t* d_payload, size_t payload_bytes, uint32_t max_frames, uint32_t channels, uint32_t stride,
    struct sela_hip_digest* d_digests, uint64_t* d_track, uint64_t* d_sample_offsets, uint64_t* d_frame_offsets, uint32_t* d_n_frames, uint32_t* d_status,
    void* d_workspace, size_t workspace_bytes, void* stream)
{
    return digest_call(PayloadForm{ d_payload, payload_bytes, max_frames, d_frame_offsets, d_n_frames }, channels, stride, d_digests, d_track, d_sample_offsets, d_status,
        d_workspace, workspace_bytes, stream);
}

// Host pointers, synchronous: where sela_hip_levels runs (generic_digest); no frames need no device.
int sela_hip_digest(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, struct sela_hip_digest* digests, uint32_t* track_crc32,
    uint64_t* track_bytes)
{
    if (track_crc32)
        *track_crc32 = 0;
    if (track_bytes)
        *track_bytes = 0;
    if (channels == 0 || channels > 255)
        return fail(SELA_HIP_EINVAL, "channels must be in 1..255");
    if ((uint64_t)n_frames * channels >= (1ull << 31))
        return fail(SELA_HIP_EINVAL, "n_frames * channels must stay below 2^31");
    if (!frame_offsets || (n_frames && !frames))
        return fail(SELA_HIP_EINVAL, "null pointer");
    if (n_frames == 0)
        return SELA_HIP_OK;
    return sela::generic_digest(frames, frame_offsets, n_frames, channels, digests, track_crc32, track_bytes, g_recurrence_form);
}

uint32_t sela_hip_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) { return sela::crc_combine(crc_a, crc_b, len_b); }

size_t sela_hip_crc32_workspace_bytes(uint64_t n_bytes) { return sela::crc32_workspace_bytes(n_bytes); }

int sela_hip_crc32_device(const void* d_bytes, uint64_t n_bytes, uint64_t* d_out, void* d_workspace, size_t workspace_bytes, void* stream)
{
    if (!d_out || !d_workspace || (n_bytes && !d_bytes))
        return fail(SELA_HIP_EINVAL, "null device pointer");
    if ((uintptr_t)d_out & 7)
        return fail(SELA_HIP_EINVAL, "d_out must be 8-byte aligned");
    if (workspace_bytes < sela::crc32_workspace_bytes(n_bytes))
        return fail(SELA_HIP_ECAPACITY, "workspace smaller than sela_hip_crc32_workspace_bytes()");
    return launched(sela::launch_crc32_device(d_bytes, n_bytes, d_out, d_workspace, static_cast<hipStream_t>(stream)), "crc32 launch");
}

// ---- digest of 24- and 32-bit streams (5.29) -----------------------------------------------------------------------------------------
size_t sela_hip_digest_pcm_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride)
{
    return sela::digest_pcm_workspace_bytes(max_frames, channels, stride);
}

int sela_hip_digest_pcm_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride,
    uint32_t bytes_per_sample, struct sela_hip_digest* d_digests, uint64_t* d_track, uint64_t* d_sample_offsets, uint32_t* d_status, void* d_workspace,
    size_t workspace_bytes, void* stream)
{
    return digest_pcm_call(FramesForm{ d_frames, d_frame_offsets, n_frames }, channels, stride, bytes_per_sample, d_digests, d_track, d_sample_offsets, d_status,
        d_workspace, workspace_bytes, stream);
}

int sela_hip_digest_payload_pcm_device(const uint8_t* d_payload, size_t payload_bytes, uint32_t max_frames, uint32_t channels, uint32_t stride,
    uint32_t bytes_per_sample, struct sela_hip_digest* d_digests, uint64_t* d_track, uint64_t* d_sample_offsets, uint64_t* d_frame_offsets, uint32_t* d_n_frames,
    uint32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream)
{
    return digest_pcm_call(PayloadForm{ d_payload, payload_bytes, max_frames, d_frame_offsets, d_n_frames }, channels, stride, bytes_per_sample, d_digests, d_track,
        d_sample_offsets, d_status, d_workspace, workspace_bytes, stream);
}

// Host pointers, synchronous: sela_hip_levels_i32's checks and walk, then chunks of frames where that call runs (generic_digest_pcm);
// no frames need no device.
int sela_hip_digest_pcm(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t bytes_per_sample,
    struct sela_hip_digest* digests, uint32_t* track_crc32, uint64_t* track_bytes, uint32_t* wide_samples)
{
    if (track_crc32)
        *track_crc32 = 0;
    if (track_bytes)
        *track_bytes = 0;
    if (wide_samples)
        *wide_samples = 0;
    if (channels == 0 || channels > 255)
        return fail(SELA_HIP_EINVAL, "channels must be in 1..255");
    if ((uint64_t)n_frames * channels >= (1ull << 31))
        return fail(SELA_HIP_EINVAL, "n_frames * channels must stay below 2^31");
    if (!frame_offsets || (n_frames && !frames))
        return fail(SELA_HIP_EINVAL, "null pointer");
    if (bytes_per_sample != 3 && bytes_per_sample != 4)
        return fail(SELA_HIP_EINVAL, "bytes_per_sample must be 3 or 4 (16-bit samples: sela_hip_digest)");
    if (n_frames == 0)
        return SELA_HIP_OK;
    if (sela::check_frame_offsets(frame_offsets, n_frames) != SELA_HIP_OK)
        return SELA_HIP_EFORMAT;
    const uint32_t largest = sela::generic_index_samples(frames, frame_offsets, n_frames, channels, nullptr, nullptr);
    if (largest == 0)
        return fail(SELA_HIP_EFORMAT, "malformed frame stream (the header walk breaks, or no subframe says a length)");
    return sela::generic_digest_pcm(frames, frame_offsets, n_frames, channels, largest, bytes_per_sample, digests, track_crc32, track_bytes, wide_samples);
}

size_t sela_hip_levels_i32_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride)
{
    return sela::levels_i32_workspace_bytes(max_frames, channels, stride);
}

int sela_hip_levels_i32_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride,
    sela_hip_level32* d_levels, uint64_t* d_sample_offsets, uint32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream)
{
    return levels_i32_call(FramesForm{ d_frames, d_frame_offsets, n_frames }, channels, stride, d_levels, d_sample_offsets, d_status, d_workspace, workspace_bytes, stream);
}

int sela_hip_levels_payload_i32_device(const uint8_t* d_payload, size_t payload_bytes, uint32_t max_frames, uint32_t channels, uint32_t stride,
    sela_hip_level32* d_levels, uint64_t* d_sample_offsets, uint64_t* d_frame_offsets, uint32_t* d_n_frames, uint32_t* d_status, void* d_workspace,
    size_t workspace_bytes, void* stream)
{
    return levels_i32_call(PayloadForm{ d_payload, payload_bytes, max_frames, d_frame_offsets, d_n_frames }, channels, stride, d_levels, d_sample_offsets, d_status,
        d_workspace, workspace_bytes, stream);
}

size_t sela_hip_levels_samples_i32_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride)
{
    return sela::levels_samples_i32_workspace_bytes(max_frames, channels, stride);
}

// levels_call's checks in its order, with the samples where the frames are
int sela_hip_levels_samples_i32_device(const int32_t* d_samples, const uint32_t* d_counts, uint32_t n_frames, uint32_t channels, uint32_t stride,
    sela_hip_level32* d_levels, uint32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream)
{
    int rc = check_frames_shape(n_frames, channels, stride);
    if (rc == SELA_HIP_OK)
        rc = need_pointers(d_status && d_workspace && (!n_frames || d_levels));
    if (rc == SELA_HIP_OK && ((uintptr_t)d_levels & 7))
        rc = fail(SELA_HIP_EINVAL, "d_levels must be 8-byte aligned");
    if (rc != SELA_HIP_OK)
        return rc;
    if (n_frames && !d_samples)
        return fail(SELA_HIP_EINVAL, "null device pointer");
    if (((uintptr_t)d_samples & 3) || ((uintptr_t)d_counts & 3))
        return fail(SELA_HIP_EINVAL, "d_samples and d_counts must be 4-byte aligned");
    const size_t need = sela::levels_samples_i32_workspace_bytes(n_frames, channels, stride);
    if (need == SIZE_MAX || workspace_bytes < need)
        return fail(SELA_HIP_ECAPACITY, "workspace smaller than sela_hip_levels_samples_i32_workspace_bytes()");
    return launched(sela::launch_levels_samples_i32_device(d_samples, d_counts, n_frames, channels, stride, d_levels, d_status, d_workspace, static_cast<hipStream_t>(stream)),
        "levels_samples_i32 launch");
}

// Host pointers, synchronous: sela_hip_verify_i32's walk, then chunks of frames where that call runs (generic_levels_i32); no
// frames need no device.
int sela_hip_levels_i32(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, sela_hip_level32* levels)
{
    if (channels == 0 || channels > 255)
        return fail(SELA_HIP_EINVAL, "channels must be in 1..255");
    if ((uint64_t)n_frames * channels >= (1ull << 31))
        return fail(SELA_HIP_EINVAL, "n_frames * channels must stay below 2^31");
    if (!frame_offsets || (n_frames && (!frames || !levels)))
        return fail(SELA_HIP_EINVAL, "null pointer");
    if (n_frames == 0)
        return SELA_HIP_OK;
    if (sela::check_frame_offsets(frame_offsets, n_frames) != SELA_HIP_OK)
        return SELA_HIP_EFORMAT;
    const uint32_t largest = sela::generic_index_samples(frames, frame_offsets, n_frames, channels, nullptr, nullptr);
    if (largest == 0)
        return fail(SELA_HIP_EFORMAT, "malformed frame stream (the header walk breaks, or no subframe says a length)");
    return sela::generic_levels_i32(frames, frame_offsets, n_frames, channels, largest, levels);
}

// Test hooks (include/sela_hip_debug.h), one per call of the int32 family: the frames the last call on this workspace left to the
// fallback, the first of the call's control words.  Waits for the device.
static long long fallback_frames(size_t (*workspace_bytes)(uint32_t, uint32_t, uint32_t), const uint32_t* (*control_words)(const void*, uint32_t, uint32_t, uint32_t),
    const void* d_workspace, uint32_t max_frames, uint32_t channels, uint32_t stride)
{
    if (!d_workspace || workspace_bytes(max_frames, channels, stride) == SIZE_MAX)
        return -1;
    uint32_t left = 0;
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(&left, control_words(d_workspace, max_frames, channels, stride), sizeof(left), hipMemcpyDeviceToHost) != hipSuccess)
        return -1;
    return (long long)left;
}

long long sela_hip_debug_levels_i32_fallback_frames(const void* d_workspace, uint32_t max_frames, uint32_t channels, uint32_t stride)
{
    return fallback_frames(sela::levels_i32_workspace_bytes, sela::levels_i32_control_words, d_workspace, max_frames, channels, stride);
}

// ---- envelope of 24- and 32-bit streams -----------------------------------------------------------------------
size_t sela_hip_envelope_i32_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride)
{
    return sela::envelope_i32_workspace_bytes(max_frames, channels, stride);
}

int sela_hip_envelope_i32_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride, uint32_t bucket,
    struct sela_hip_envelope32* d_env, uint64_t* d_sample_offsets, uint32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream)
{
    return envelope_i32_call(FramesForm{ d_frames, d_frame_offsets, n_frames }, channels, stride, bucket, d_env, d_sample_offsets, d_status, d_workspace, workspace_bytes,
        stream);
}

int sela_hip_envelope_payload_i32_device(const uint8_t* d_payload, size_t payload_bytes, uint32_t max_frames, uint32_t channels, uint32_t stride, uint32_t bucket,
    struct sela_hip_envelope32* d_env, uint64_t* d_sample_offsets, uint64_t* d_frame_offsets, uint32_t* d_n_frames, uint32_t* d_status, void* d_workspace,
    size_t workspace_bytes, void* stream)
{
    return envelope_i32_call(PayloadForm{ d_payload, payload_bytes, max_frames, d_frame_offsets, d_n_frames }, channels, stride, bucket, d_env, d_sample_offsets, d_status,
        d_workspace, workspace_bytes, stream);
}

size_t sela_hip_envelope_samples_i32_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride)
{
    return sela::envelope_samples_i32_workspace_bytes(max_frames, channels, stride);
}

// envelope_i32_call's checks in its order, with the samples where the frames are
int sela_hip_envelope_samples_i32_device(const int32_t* d_samples, const uint32_t* d_counts, uint32_t n_frames, uint32_t channels, uint32_t stride, uint32_t bucket,
    struct sela_hip_envelope32* d_env, uint32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream)
{
    int rc = check_frames_shape(n_frames, channels, stride);
    if (rc == SELA_HIP_OK && !sela::envelope_bucket_ok(bucket))
        rc = fail(SELA_HIP_EINVAL, "bucket must be one of 32, 64, 128, 256, 512, 1024, 2048");
    if (rc == SELA_HIP_OK)
        rc = need_pointers(d_status && d_workspace && (!n_frames || d_env));
    if (rc == SELA_HIP_OK && ((uintptr_t)d_env & 7))
        rc = fail(SELA_HIP_EINVAL, "d_env must be 8-byte aligned");
    if (rc != SELA_HIP_OK)
        return rc;
    if (n_frames && !d_samples)
        return fail(SELA_HIP_EINVAL, "null device pointer");
    if (((uintptr_t)d_samples & 3) || ((uintptr_t)d_counts & 3))
        return fail(SELA_HIP_EINVAL, "d_samples and d_counts must be 4-byte aligned");
    const size_t need = sela::envelope_samples_i32_workspace_bytes(n_frames, channels, stride);
    if (need == SIZE_MAX || workspace_bytes < need)
        return fail(SELA_HIP_ECAPACITY, "workspace smaller than sela_hip_envelope_samples_i32_workspace_bytes()");
    return launched(sela::launch_envelope_samples_i32_device(d_samples, d_counts, n_frames, channels, stride, bucket, d_env, d_status, static_cast<hipStream_t>(stream)),
        "envelope_samples_i32 launch");
}

// Host pointers, synchronous: sela_hip_levels_i32's walk, then chunks of frames where that call runs (generic_envelope_i32), at the
// caller's stride; no frames need no device.
int sela_hip_envelope_i32(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride, uint32_t bucket,
    struct sela_hip_envelope32* env)
{
    if (channels == 0 || channels > 255)
        return fail(SELA_HIP_EINVAL, "channels must be in 1..255");
    if (stride == 0)
        return fail(SELA_HIP_EINVAL, "stride must not be 0");
    if ((uint64_t)n_frames * channels >= (1ull << 31))
        return fail(SELA_HIP_EINVAL, "n_frames * channels must stay below 2^31");
    if (!sela::envelope_bucket_ok(bucket))
        return fail(SELA_HIP_EINVAL, "bucket must be one of 32, 64, 128, 256, 512, 1024, 2048");
    if ((uint64_t)sela::envelope_slots(stride, bucket) * channels > 0xFFFFFFFFull) // (the chunk loop counts a frame's records in 32 bits)
        return fail(SELA_HIP_EINVAL, "ceil(stride / bucket) * channels must fit 32 bits");
    if (!frame_offsets || (n_frames && (!frames || !env)))
        return fail(SELA_HIP_EINVAL, "null pointer");
    if (n_frames == 0)
        return SELA_HIP_OK;
    if (sela::check_frame_offsets(frame_offsets, n_frames) != SELA_HIP_OK)
        return SELA_HIP_EFORMAT;
    if (sela::generic_index_samples(frames, frame_offsets, n_frames, channels, nullptr, nullptr) == 0)
        return fail(SELA_HIP_EFORMAT, "malformed frame stream (the header walk breaks, or no subframe says a length)");
    return sela::generic_envelope_i32(frames, frame_offsets, n_frames, channels, stride, bucket, env);
}

long long sela_hip_debug_envelope_i32_fallback_frames(const void* d_workspace, uint32_t max_frames, uint32_t channels, uint32_t stride)
{
    return fallback_frames(sela::envelope_i32_workspace_bytes, sela::envelope_i32_control_words, d_workspace, max_frames, channels, stride);
}

size_t sela_hip_decode_windows_workspace_bytes(uint32_t n_windows, uint32_t window_samples, uint32_t channels)
{
    return sela::window_workspace_bytes(n_windows, window_samples, channels);
}

int sela_hip_decode_windows_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames_total, uint32_t channels,
    const sela_hip_window* d_windows, uint32_t n_windows, uint32_t window_samples, uint32_t format, void* d_out, uint32_t* d_window_flags, uint32_t* d_status,
    void* d_workspace, size_t workspace_bytes, void* stream)
{
    return windows_call(FramesForm{ d_frames, d_frame_offsets, n_frames_total }, channels, d_windows, n_windows, window_samples, format, d_out, d_window_flags, d_status,
        d_workspace, workspace_bytes, stream, false);
}

// The same call for whole-track streams (5.20): a last frame of 1 .. 4095 samples is decoded by the any-length kernels.
size_t sela_hip_decode_windows_whole_workspace_bytes(uint32_t n_windows, uint32_t window_samples, uint32_t channels)
{
    return sela::window_whole_workspace_bytes(n_windows, window_samples, channels);
}

int sela_hip_decode_windows_whole_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames_total, uint32_t channels,
    const sela_hip_window* d_windows, uint32_t n_windows, uint32_t window_samples, uint32_t format, void* d_out, uint32_t* d_window_flags, uint32_t* d_status,
    void* d_workspace, size_t workspace_bytes, void* stream)
{
    return windows_call(FramesForm{ d_frames, d_frame_offsets, n_frames_total }, channels, d_windows, n_windows, window_samples, format, d_out, d_window_flags, d_status,
        d_workspace, workspace_bytes, stream, true);
}

// Host pointers, synchronous: the device call's shape checks (check_windows_shape), then generic_decode_windows
// (sela_capi_generic.hip) on the any-length route's leased context and stream, past the coalescer; an open streaming job of the
// thread is left alone.
static int windows_host_call(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames_total, uint32_t channels, const sela_hip_window* windows,
    uint32_t n_windows, uint32_t window_samples, uint32_t format, void* out, uint32_t* window_flags, bool whole)
{
    sela::windows_staged_bytes_reset(); // a call that is refused, or has no windows, staged nothing
    const int rc = check_windows_shape(channels, n_windows, window_samples, format, "sela_hip_decode");
    if (rc != SELA_HIP_OK)
        return rc;
    if ((n_windows && (!windows || !out)) || !frame_offsets || (n_frames_total && !frames))
        return fail(SELA_HIP_EINVAL, "null pointer");
    if (n_windows == 0)
        return SELA_HIP_OK;
    return sela::generic_decode_windows(frames, frame_offsets, n_frames_total, channels, windows, n_windows, window_samples, format, out, window_flags,
        g_recurrence_form, whole);
}

int sela_hip_decode_windows(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames_total, uint32_t channels, const sela_hip_window* windows,
    uint32_t n_windows, uint32_t window_samples, uint32_t format, void* out, uint32_t* window_flags)
{
    return windows_host_call(frames, frame_offsets, n_frames_total, channels, windows, n_windows, window_samples, format, out, window_flags, false);
}

int sela_hip_decode_windows_whole(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames_total, uint32_t channels, const sela_hip_window* windows,
    uint32_t n_windows, uint32_t window_samples, uint32_t format, void* out, uint32_t* window_flags)
{
    return windows_host_call(frames, frame_offsets, n_frames_total, channels, windows, n_windows, window_samples, format, out, window_flags, true);
}

// Sample windows of 24- and 32-bit streams (5.23).
size_t sela_hip_decode_windows_i32_workspace_bytes(uint32_t n_windows, uint32_t window_samples, uint32_t channels)
{
    return sela::window32_workspace_bytes(n_windows, window_samples, channels);
}

int sela_hip_decode_windows_i32_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames_total, uint32_t channels,
    const sela_hip_window* d_windows, uint32_t n_windows, uint32_t window_samples, uint32_t format, uint32_t sample_bits, void* d_out, uint32_t* d_window_flags,
    uint32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream)
{
    return windows_i32_call(FramesForm{ d_frames, d_frame_offsets, n_frames_total }, channels, d_windows, n_windows, window_samples, format, sample_bits, d_out,
        d_window_flags, d_status, d_workspace, workspace_bytes, stream, false);
}

// The same call for whole-track streams (5.25): a last frame of 1 .. 4095 samples is decoded by k_tailwin_decode and stored by
// k_tail32_store (sela_window32_whole.hip).
size_t sela_hip_decode_windows_i32_whole_workspace_bytes(uint32_t n_windows, uint32_t window_samples, uint32_t channels)
{
    return sela::window32_whole_workspace_bytes(n_windows, window_samples, channels);
}

int sela_hip_decode_windows_i32_whole_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames_total, uint32_t channels,
    const sela_hip_window* d_windows, uint32_t n_windows, uint32_t window_samples, uint32_t format, uint32_t sample_bits, void* d_out, uint32_t* d_window_flags,
    uint32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream)
{
    return windows_i32_call(FramesForm{ d_frames, d_frame_offsets, n_frames_total }, channels, d_windows, n_windows, window_samples, format, sample_bits, d_out,
        d_window_flags, d_status, d_workspace, workspace_bytes, stream, true);
}

// Host pointers, synchronous: the device call's shape checks (check_windows_i32_shape), then generic_decode_windows on the
// any-length route's leased context and stream, as sela_hip_decode_windows runs.
static int windows_i32_host_call(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames_total, uint32_t channels, const sela_hip_window* windows,
    uint32_t n_windows, uint32_t window_samples, uint32_t format, uint32_t sample_bits, void* out, uint32_t* window_flags, bool whole)
{
    sela::windows_staged_bytes_reset(); // a call that is refused, or has no windows, staged nothing
    const int rc = check_windows_i32_shape(channels, n_windows, window_samples, format, sample_bits);
    if (rc != SELA_HIP_OK)
        return rc;
    if ((n_windows && (!windows || !out)) || !frame_offsets || (n_frames_total && !frames))
        return fail(SELA_HIP_EINVAL, "null pointer");
    if (n_windows == 0)
        return SELA_HIP_OK;
    return sela::generic_decode_windows(frames, frame_offsets, n_frames_total, channels, windows, n_windows, window_samples, format, out, window_flags,
        g_recurrence_form, whole, true, sample_bits);
}

int sela_hip_decode_windows_i32(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames_total, uint32_t channels, const sela_hip_window* windows,
    uint32_t n_windows, uint32_t window_samples, uint32_t format, uint32_t sample_bits, void* out, uint32_t* window_flags)
{
    return windows_i32_host_call(frames, frame_offsets, n_frames_total, channels, windows, n_windows, window_samples, format, sample_bits, out, window_flags, false);
}

int sela_hip_decode_windows_i32_whole(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames_total, uint32_t channels, const sela_hip_window* windows,
    uint32_t n_windows, uint32_t window_samples, uint32_t format, uint32_t sample_bits, void* out, uint32_t* window_flags)
{
    return windows_i32_host_call(frames, frame_offsets, n_frames_total, channels, windows, n_windows, window_samples, format, sample_bits, out, window_flags, true);
}

size_t sela_hip_verify_i32_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride)
{
    return sela::verify_i32_workspace_bytes(max_frames, channels, stride);
}

int sela_hip_verify_i32_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride,
    const int32_t* d_samples, const uint32_t* d_lengths, uint32_t* d_diff_counts, uint32_t* d_first_diff, uint64_t* d_sample_offsets, uint32_t* d_status,
    void* d_workspace, size_t workspace_bytes, void* stream)
{
    return verify_i32_call(FramesForm{ d_frames, d_frame_offsets, n_frames }, channels, stride, d_samples, d_lengths, d_diff_counts, d_first_diff, d_sample_offsets,
        d_status, d_workspace, workspace_bytes, stream);
}

int sela_hip_verify_payload_i32_device(const uint8_t* d_payload, size_t payload_bytes, uint32_t max_frames, uint32_t channels, uint32_t stride,
    const int32_t* d_samples, const uint32_t* d_lengths, uint32_t* d_diff_counts, uint32_t* d_first_diff, uint64_t* d_sample_offsets, uint64_t* d_frame_offsets,
    uint32_t* d_n_frames, uint32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream)
{
    return verify_i32_call(PayloadForm{ d_payload, payload_bytes, max_frames, d_frame_offsets, d_n_frames }, channels, stride, d_samples, d_lengths, d_diff_counts,
        d_first_diff, d_sample_offsets, d_status, d_workspace, workspace_bytes, stream);
}

// Host pointers, synchronous: sela_hip_decode_i32's checks in its order, then chunks of frames on the any-length route's leased
// context and stream (generic_verify_i32), past the coalescer; an open streaming job of the thread is left alone.
int sela_hip_verify_i32(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride, const int32_t* samples,
    const uint32_t* lengths, uint32_t* diff_counts, uint32_t* first_diff, uint32_t* lossy_frames)
{
    if (lossy_frames)
        *lossy_frames = 0;
    if (channels == 0 || channels > 255 || stride == 0 || (n_frames && (!frames || !frame_offsets || !samples || !diff_counts || !first_diff)))
        return fail(SELA_HIP_EINVAL, "bad argument");
    if ((uint64_t)n_frames * channels >= (1ull << 31))
        return fail(SELA_HIP_EINVAL, "n_frames * channels must stay below 2^31");
    if (n_frames == 0)
        return SELA_HIP_OK;
    if (sela::check_frame_offsets(frame_offsets, n_frames) != SELA_HIP_OK)
        return SELA_HIP_EFORMAT;
    const uint32_t largest = sela::generic_index_samples(frames, frame_offsets, n_frames, channels, nullptr, nullptr);
    if (largest > stride)
        return fail(SELA_HIP_ECAPACITY, "stride is smaller than the largest samplesPerChannel of the stream (see sela_hip_index_samples)");
    return sela::generic_verify_i32(frames, frame_offsets, n_frames, channels, stride, samples, lengths, diff_counts, first_diff, lossy_frames);
}

long long sela_hip_debug_verify_i32_fallback_frames(const void* d_workspace, uint32_t max_frames, uint32_t channels, uint32_t stride)
{
    return fallback_frames(sela::verify_i32_workspace_bytes, sela::verify_i32_control_words, d_workspace, max_frames, channels, stride);
}

// ---- verification against packed PCM -----------------------------------------------------------------------
size_t sela_hip_verify_pcm_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride)
{
    return sela::verify_pcm_workspace_bytes(max_frames, channels, stride);
}

int sela_hip_verify_pcm_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride, const void* d_pcm,
    uint32_t bytes_per_sample, uint64_t pcm_samples, uint32_t* d_diff_counts, uint32_t* d_first_diff, uint64_t* d_sample_offsets, uint32_t* d_status,
    void* d_workspace, size_t workspace_bytes, void* stream)
{
    return verify_pcm_call(FramesForm{ d_frames, d_frame_offsets, n_frames }, channels, stride, d_pcm, bytes_per_sample, pcm_samples, d_diff_counts, d_first_diff,
        d_sample_offsets, d_status, d_workspace, workspace_bytes, stream);
}

int sela_hip_verify_payload_pcm_device(const uint8_t* d_payload, size_t payload_bytes, uint32_t max_frames, uint32_t channels, uint32_t stride, const void* d_pcm,
    uint32_t bytes_per_sample, uint64_t pcm_samples, uint32_t* d_diff_counts, uint32_t* d_first_diff, uint64_t* d_sample_offsets, uint64_t* d_frame_offsets,
    uint32_t* d_n_frames, uint32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream)
{
    return verify_pcm_call(PayloadForm{ d_payload, payload_bytes, max_frames, d_frame_offsets, d_n_frames }, channels, stride, d_pcm, bytes_per_sample, pcm_samples,
        d_diff_counts, d_first_diff, d_sample_offsets, d_status, d_workspace, workspace_bytes, stream);
}

// Host pointers, synchronous: sela_hip_decode_i32's checks in its order (the stride is the stream's own largest frame), then chunks
// of whole frames on the any-length route's leased context and stream (generic_verify_pcm), past the coalescer; an open streaming
// job of the thread is left alone.
int sela_hip_verify_pcm(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t bytes_per_sample, const void* pcm,
    uint64_t pcm_samples, uint32_t* diff_counts, uint32_t* first_diff, uint32_t* lossy_frames)
{
    if (lossy_frames)
        *lossy_frames = 0;
    if (channels == 0 || channels > 255 || (n_frames && (!frames || !frame_offsets || !diff_counts || !first_diff)) || (n_frames && pcm_samples && !pcm))
        return fail(SELA_HIP_EINVAL, "bad argument");
    if ((uint64_t)n_frames * channels >= (1ull << 31))
        return fail(SELA_HIP_EINVAL, "n_frames * channels must stay below 2^31");
    if (bytes_per_sample != 3 && bytes_per_sample != 4)
        return fail(SELA_HIP_EINVAL, "bytes_per_sample must be 3 or 4 (16-bit samples: sela_hip_verify)");
    if (n_frames == 0)
        return SELA_HIP_OK;
    if (sela::check_frame_offsets(frame_offsets, n_frames) != SELA_HIP_OK)
        return SELA_HIP_EFORMAT;
    return sela::generic_verify_pcm(frames, frame_offsets, n_frames, channels, bytes_per_sample, static_cast<const uint8_t*>(pcm), pcm_samples, diff_counts, first_diff,
        lossy_frames);
}

long long sela_hip_debug_verify_pcm_fallback_frames(const void* d_workspace, uint32_t max_frames, uint32_t channels, uint32_t stride)
{
    return fallback_frames(sela::verify_pcm_workspace_bytes, sela::verify_pcm_control_words, d_workspace, max_frames, channels, stride);
}

long long sela_hip_debug_digest_pcm_fallback_frames(const void* d_workspace, uint32_t max_frames, uint32_t channels, uint32_t stride)
{
    return fallback_frames(sela::digest_pcm_workspace_bytes, sela::digest_pcm_control_words, d_workspace, max_frames, channels, stride);
}

// Test hook (include/sela_hip_debug.h): the pieces of a call's workspace, from the description its launch runs.  No device.
int sela_hip_debug_workspace_pieces(int call, uint64_t a, uint32_t b, uint32_t c, uint64_t* offset_bytes_pairs, int capacity)
{
    sela::CarvePieces pieces = { offset_bytes_pairs, offset_bytes_pairs && capacity > 0 ? capacity : 0, 0 };
    sela::Carve at(&pieces);
    const uint32_t a32 = (uint32_t)a;
    size_t bytes = SIZE_MAX;
    if (call != SELA_HIP_WORKSPACE_INDEX && call != SELA_HIP_WORKSPACE_SALVAGE && call != SELA_HIP_WORKSPACE_ENCODE_WHOLE && call != SELA_HIP_WORKSPACE_ENCODE_WHOLE_PCM && a > 0xFFFFFFFFull)
        return -1;
    switch (call) {
    case SELA_HIP_WORKSPACE_ENCODE: bytes = sela::encode_workspace_bytes(a32, b, &at); break;
    case SELA_HIP_WORKSPACE_DECODE: bytes = sela::decode_workspace_bytes(a32, b, &at); break;
    case SELA_HIP_WORKSPACE_INDEX: bytes = sela::index_workspace_bytes(a, &at); break;
    case SELA_HIP_WORKSPACE_DECODE_I32: bytes = sela::decode_i32_workspace_bytes(a32, b, c, &at); break;
    case SELA_HIP_WORKSPACE_DECODE_N: bytes = sela::decode_n_workspace_bytes(a32, b, c, &at); break;
    case SELA_HIP_WORKSPACE_VERIFY: bytes = sela::verify_workspace_bytes(a32, b, c, &at); break;
    case SELA_HIP_WORKSPACE_VERIFY_I32: bytes = sela::verify_i32_workspace_bytes(a32, b, c, &at); break;
    case SELA_HIP_WORKSPACE_ENCODE_I32: bytes = sela::encode_i32_device_workspace_bytes(a32, b, c, false, &at); break;
    case SELA_HIP_WORKSPACE_ENCODE_PAIRED: bytes = sela::encode_i32_device_workspace_bytes(a32, b, c, true, &at); break;
    case SELA_HIP_WORKSPACE_WINDOWS: bytes = sela::window_workspace_bytes(a32, b, c, &at); break;
    case SELA_HIP_WORKSPACE_WINDOWS_WHOLE: bytes = sela::window_whole_workspace_bytes(a32, b, c, &at); break;
    case SELA_HIP_WORKSPACE_ENCODE_WHOLE: bytes = sela::whole_workspace_bytes(a, b, &at); break;
    case SELA_HIP_WORKSPACE_ENCODE_SPLIT:
        if (c == 0 || c >= a32)
            return -1;
        bytes = carve_encode_split(at, c, a32 - c, b).end;
        break;
    case SELA_HIP_WORKSPACE_DECODE_WHOLE: bytes = sela::decode_whole_workspace_bytes(a32, b, &at); break;
    case SELA_HIP_WORKSPACE_WINDOWS_I32: bytes = sela::window32_workspace_bytes(a32, b, c, &at); break;
    case SELA_HIP_WORKSPACE_WINDOWS_I32_WHOLE: bytes = sela::window32_whole_workspace_bytes(a32, b, c, &at); break;
    case SELA_HIP_WORKSPACE_ENCODE_WHOLE_PCM: bytes = sela::whole_pcm_workspace_bytes(a, b, &at); break;
    case SELA_HIP_WORKSPACE_SALVAGE: bytes = sela::salvage_workspace_bytes(a, b, &at); break;
    default: return -1;
    }
    return bytes == SIZE_MAX ? -1 : pieces.count;
}

// ---- streaming jobs (host pointers) ----------------------------------------------------------------------------
int sela_hip_encode_begin(sela_hip_job** job, uint32_t channels, uint32_t total_frames, uint8_t* frames_out, size_t frames_cap,
    uint64_t* frame_offsets_out)
{
    if (!frame_offsets_out || (total_frames && !frames_out))
        return fail(SELA_HIP_EINVAL, "bad argument");
    int rc = job_begin(job, true, channels, total_frames);
    if (rc != SELA_HIP_OK)
        return rc;
    sela_hip_job* j = *job;
    j->frames_out = frames_out;
    j->frames_cap = frames_cap;
    j->offsets_out = frame_offsets_out;
    frame_offsets_out[0] = 0;
    // the kernels store the stream where the device can reach it: the caller's buffer if it is page-locked,
    // otherwise a page-locked bounce buffer (no larger than the job can need)
    j->out_host = frames_out;
    j->out_mapped = static_cast<uint8_t*>(device_view(frames_out));
    if (total_frames && !j->out_mapped) {
        j->frames_cap = std::min(frames_cap, sela_hip_encode_bound_bytes(total_frames, channels));
        j->out_host = static_cast<uint8_t*>(pool().take(j->frames_cap ? j->frames_cap : 1));
        j->out_bounce = true;
        j->out_mapped = j->out_host ? static_cast<uint8_t*>(device_view(j->out_host)) : nullptr;
        if (!j->out_mapped) {
            (void)job_end(j, nullptr, nullptr);
            *job = nullptr;
            return fail(SELA_HIP_ENOMEM, "page-locked bounce buffer");
        }
    }
    return SELA_HIP_OK;
}

int sela_hip_encode_begin_opt(sela_hip_job** job, uint32_t channels, uint32_t total_frames, uint8_t* frames_out, size_t frames_cap,
    uint64_t* frame_offsets_out, uint32_t options)
{
    bool lossless = false;
    int rc = encode_options(options, &lossless);
    if (rc != SELA_HIP_OK)
        return rc;
    rc = sela_hip_encode_begin(job, channels, total_frames, frames_out, frames_cap, frame_offsets_out);
    if (rc == SELA_HIP_OK)
        (*job)->lossless = lossless; // (nothing is launched before the first feed)
    return rc;
}

int sela_hip_encode_feed(sela_hip_job* job, const int16_t* pcm, uint32_t n_frames, uint32_t* frames_final, uint64_t* bytes_final)
{
    if (!job || !job->encode || (n_frames && !pcm) || (uint64_t)job->fed + n_frames > job->total_frames)
        return fail(SELA_HIP_EINVAL, "bad argument");
    if (job->error != SELA_HIP_OK)
        return job->error;
    int rc = job_feed_encode(job, pcm, n_frames);
    if (rc != SELA_HIP_OK)
        return rc;
    rc = job_drain_ready(job);
    if (rc != SELA_HIP_OK)
        return rc;
    job_progress(job, frames_final, bytes_final);
    return SELA_HIP_OK;
}

int sela_hip_encode_end(sela_hip_job* job, uint32_t* frames_final, uint64_t* bytes_final)
{
    if (!job || !job->encode)
        return fail(SELA_HIP_EINVAL, "bad argument");
    return job_end(job, frames_final, bytes_final);
}

int sela_hip_decode_begin(sela_hip_job** job, uint32_t channels, uint32_t total_frames, int16_t* pcm_out)
{
    if (total_frames && !pcm_out)
        return fail(SELA_HIP_EINVAL, "bad argument");
    int rc = job_begin(job, false, channels, total_frames);
    if (rc != SELA_HIP_OK)
        return rc;
    sela_hip_job* j = *job;
    j->pcm_out = j->pcm_caller = pcm_out;
    if (total_frames && !device_view(pcm_out)) { // ordinary memory: the copy-outs land in a page-locked buffer first
        const size_t bytes = (size_t)total_frames * sela::kBlock * channels * sizeof(int16_t);
        j->pcm_out = static_cast<int16_t*>(pool().take(bytes));
        j->pcm_bounce = true;
        if (!j->pcm_out) {
            (void)job_end(j, nullptr, nullptr);
            *job = nullptr;
            return fail(SELA_HIP_ENOMEM, "page-locked bounce buffer");
        }
    }
    return SELA_HIP_OK;
}

int sela_hip_decode_feed(sela_hip_job* job, const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t* frames_final)
{
    if (!job || job->encode || (n_frames && (!frames || !frame_offsets)) || (uint64_t)job->fed + n_frames > job->total_frames)
        return fail(SELA_HIP_EINVAL, "bad argument");
    if (job->error != SELA_HIP_OK)
        return job->error;
    for (uint32_t f = 0; f < n_frames; f++)
        if (frame_offsets[f + 1] < frame_offsets[f] || (frame_offsets[f] & 3))
            return job_fail(job, fail(SELA_HIP_EFORMAT, "frame offsets must be ascending multiples of 4"));
    int rc = job_feed_decode(job, frames, frame_offsets, n_frames);
    if (rc != SELA_HIP_OK)
        return rc;
    rc = job_drain_ready(job);
    if (rc != SELA_HIP_OK)
        return rc;
    job_progress(job, frames_final, nullptr);
    return SELA_HIP_OK;
}

int sela_hip_decode_end(sela_hip_job* job, uint32_t* frames_final)
{
    if (!job || job->encode)
        return fail(SELA_HIP_EINVAL, "bad argument");
    return job_end(job, frames_final, nullptr);
}

// ---- one-shot host-pointer API -----------------------------------------------------------------------------------
namespace {

// One call, as it is: a job of one feed.
int encode_now(const int16_t* pcm, uint32_t n_frames, uint32_t channels, uint8_t* frames_out, size_t frames_cap, uint64_t* frame_offsets_out, uint32_t options = 0)
{
    sela_hip_job* job = nullptr;
    int rc = sela_hip_encode_begin_opt(&job, channels, n_frames, frames_out, frames_cap, frame_offsets_out, options);
    if (rc != SELA_HIP_OK)
        return rc;
    rc = sela_hip_encode_feed(job, pcm, n_frames, nullptr, nullptr);
    const std::string msg = rc != SELA_HIP_OK ? sela_hip_last_error() : "";
    const int rc_end = sela_hip_encode_end(job, nullptr, nullptr);
    if (rc != SELA_HIP_OK)
        return fail(rc, msg);
    return rc_end;
}

int decode_now(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, int16_t* pcm_out)
{
    sela_hip_job* job = nullptr;
    int rc = sela_hip_decode_begin(&job, channels, n_frames, pcm_out);
    if (rc != SELA_HIP_OK)
        return rc;
    rc = sela_hip_decode_feed(job, frames, frame_offsets, n_frames, nullptr);
    const std::string msg = rc != SELA_HIP_OK ? sela_hip_last_error() : "";
    const int rc_end = sela_hip_decode_end(job, nullptr);
    if (rc != SELA_HIP_OK)
        return fail(rc, msg);
    return rc_end;
}

// ---- small calls from many threads are coalesced: sela_coalescer.h, on this backend ---------------------------------------
struct HipBackend {
    static int encode_now(const int16_t* pcm, uint32_t n_frames, uint32_t channels, uint8_t* frames_out, size_t frames_cap, uint64_t* offsets_out)
    {
        return ::encode_now(pcm, n_frames, channels, frames_out, frames_cap, offsets_out);
    }
    static int decode_now(const uint8_t* frames, const uint64_t* offsets, uint32_t n_frames, uint32_t channels, int16_t* pcm_out)
    {
        return ::decode_now(frames, offsets, n_frames, channels, pcm_out);
    }
    static int decode_i32_now(const uint8_t* frames, const uint64_t* offsets, uint32_t n_frames, uint32_t channels, int32_t* samples_out, uint32_t stride,
        uint32_t* counts_out)
    {
        return sela::generic_decode(frames, offsets, n_frames, channels, samples_out, stride, counts_out, nullptr, nullptr);
    }
    static int encode_i32_now(const int32_t* samples, uint32_t n_frames, uint32_t channels, uint32_t n, uint8_t* frames_out, size_t frames_cap, uint64_t* offsets_out)
    {
        return sela::generic_encode(samples, false, n_frames, channels, n, frames_out, frames_cap, offsets_out);
    }
    static size_t encode_bound_bytes(uint32_t n_frames, uint32_t channels) { return sela_hip_encode_bound_bytes(n_frames, channels); }
    static size_t encode_i32_bound_bytes(uint32_t n_frames, uint32_t channels, uint32_t n) { return sela::generic_encode_bound_bytes(n_frames, channels, n); }
    static void* take(size_t bytes) { return pool().take(bytes); }
    static void give(void* p) { pool().give(p); }
    static std::string last_error() { return sela_hip_last_error(); }
    static void after_batch() // (both routes' leases: whoever leads next takes them over instead of creating a set of its own)
    {
        sela_hip_thread_release();
    }
};
using sela::kCoalesceFrames;
using sela::SmallCall;
typedef sela::CallCoalescer<HipBackend> Coalescer;

// One coalescer per device and direction: calls for different GPUs (one thread per GPU, each coding frame by frame) can never
// share a batch, so they do not wait for each other's leaders either.
std::mutex g_coalescers_mu;
Coalescer* g_coalescers[4][64] = {};

Coalescer* coalescer(Coalescer::Kind kind, int device)
{
    const int d = device >= 0 && device < 64 ? device : 0;
    std::lock_guard<std::mutex> lock(g_coalescers_mu);
    Coalescer*& c = g_coalescers[(int)kind][d];
    if (!c)
        c = new Coalescer(kind, kind == Coalescer::kDecode || kind == Coalescer::kDecode32 ? sela::kCoalesceLeadersDecode : sela::kCoalesceLeaders); // (never destroyed: calls may outlive the statics)
    return c;
}

int submit_small(Coalescer::Kind kind, SmallCall& call)
{
    const int rc = coalescer(kind, call.device)->submit(call);
    return rc == SELA_HIP_OK ? SELA_HIP_OK : fail(rc, call.error);
}
} // namespace

void sela_hip_debug_coalesced(int kind, long long* batches, long long* retried)
{
    long long b = 0, r = 0;
    if (kind >= 0 && kind < 4) {
        std::lock_guard<std::mutex> lock(g_coalescers_mu);
        for (Coalescer* c : g_coalescers[kind]) {
            long long cb = 0, cr = 0;
            if (c)
                c->counts(&cb, &cr);
            b += cb, r += cr;
        }
    }
    if (batches)
        *batches = b;
    if (retried)
        *retried = r;
}

int sela_hip_encode(const int16_t* pcm, uint32_t n_frames, uint32_t channels, uint32_t samples_per_channel, uint8_t* frames_out,
    size_t frames_cap, uint64_t* frame_offsets_out)
{
    if (samples_per_channel == 0 || samples_per_channel > 65535)
        return fail(SELA_HIP_EINVAL, "samples_per_channel must be 1 .. 65535 (the subframe's field is 16 bits wide)");
    if (channels == 0 || channels > 255 || !frame_offsets_out || (n_frames && (!pcm || !frames_out)))
        return fail(SELA_HIP_EINVAL, "bad argument");
    if (samples_per_channel != SELA_HIP_SAMPLES_PER_FRAME) // not the shape the fast kernels are built for: the any-length route
        return sela::generic_encode(pcm, true, n_frames, channels, samples_per_channel, frames_out, frames_cap, frame_offsets_out);
    if (n_frames == 0 || n_frames > kCoalesceFrames || (g_lease.held && g_lease.held->job_open)) // (a thread in the middle of a job of its own hears about that itself)
        return encode_now(pcm, n_frames, channels, frames_out, frames_cap, frame_offsets_out);
    SmallCall call;
    if (hipGetDevice(&call.device) != hipSuccess)
        return encode_now(pcm, n_frames, channels, frames_out, frames_cap, frame_offsets_out); // (reports the missing device)
    call.channels = channels, call.n_frames = n_frames;
    call.pcm = pcm, call.frames_out = frames_out, call.frames_cap = frames_cap, call.offsets_out = frame_offsets_out;
    return submit_small(Coalescer::kEncode, call);
}

// options != 0: past the coalescer (its batches are the plain call's).  2048-sample frames go to the fast kernels as a job of one
// feed -- unless the thread has a job open, which is left alone: then, and for every other length, the any-length route.
int sela_hip_encode_opt(const int16_t* pcm, uint32_t n_frames, uint32_t channels, uint32_t samples_per_channel, uint8_t* frames_out,
    size_t frames_cap, uint64_t* frame_offsets_out, uint32_t options)
{
    bool lossless = false;
    const int rc = encode_options(options, &lossless);
    if (rc != SELA_HIP_OK)
        return rc;
    if (!lossless)
        return sela_hip_encode(pcm, n_frames, channels, samples_per_channel, frames_out, frames_cap, frame_offsets_out);
    if (samples_per_channel == 0 || samples_per_channel > 65535)
        return fail(SELA_HIP_EINVAL, "samples_per_channel must be 1 .. 65535 (the subframe's field is 16 bits wide)");
    if (channels == 0 || channels > 255 || !frame_offsets_out || (n_frames && (!pcm || !frames_out)))
        return fail(SELA_HIP_EINVAL, "bad argument");
    if (samples_per_channel != SELA_HIP_SAMPLES_PER_FRAME || (g_lease.held && g_lease.held->job_open))
        return sela::generic_encode(pcm, true, n_frames, channels, samples_per_channel, frames_out, frames_cap, frame_offsets_out, true);
    return encode_now(pcm, n_frames, channels, frames_out, frames_cap, frame_offsets_out, options);
}

// ---- a whole track with its tail (the rule, the workspace and the splice: sela_whole.hip) -------------------------
namespace {
int whole_arguments(uint64_t n_samples, uint32_t channels, const void* pcm, const void* frames, const void* frame_offsets)
{
    if (channels == 0 || channels > 255)
        return fail(SELA_HIP_EINVAL, "channels must be in 1..255");
    if (sela_hip_whole_frames(n_samples) * sela_hip_signals_per_frame(channels) >= (1ull << 31))
        return fail(SELA_HIP_EINVAL, "frames * signals per frame must stay below 2^31");
    if (!frame_offsets || (n_samples && (!pcm || !frames)))
        return fail(SELA_HIP_EINVAL, "null pointer");
    return SELA_HIP_OK;
}

// what both whole-track device encoders (this one and 5.25's, from packed PCM) ask behind their own argument checks
int whole_device_arguments(const void* d_pcm, const void* d_frames, const void* d_status, const void* d_workspace, size_t workspace_bytes, size_t need, const char* sized_by)
{
    if (!d_status || !d_workspace)
        return fail(SELA_HIP_EINVAL, "null pointer");
    if (((uintptr_t)d_pcm & 3) || ((uintptr_t)d_frames & 3))
        return fail(SELA_HIP_EINVAL, "d_pcm and d_frames must be 4-byte aligned");
    if (workspace_bytes < need)
        return fail(SELA_HIP_ECAPACITY, std::string("workspace smaller than ") + sized_by + "()");
    return SELA_HIP_OK;
}

// The cases of a whole track, for both device encoders.  `code(main_pieces, first, count, length, out, cap, offsets, status, on)`
// codes frames [first, first + count) of `length` samples each, with the workspace's pieces for the 2048-sample frames or with the
// last frame's, into these outputs on that stream.  A track with front frames and a long last frame takes the fork (fork_join):
// the last frame coded into the workspace (`coded`) on the side stream, the front frames beside it, the splice behind the join.
extern "C++" template <typename Code>
int encode_whole_frames(const char* name, uint64_t n_samples, uint32_t channels, const sela::WholeLastWs& coded, uint8_t* d_frames, size_t frames_cap,
    uint64_t* d_frame_offsets, uint32_t* d_status, hipStream_t st, Code code)
{
    const uint32_t frames = (uint32_t)sela_hip_whole_frames(n_samples), tail = (uint32_t)(n_samples % SELA_HIP_SAMPLES_PER_FRAME);
    if (frames == 0) // nothing: offsets[0] = 0 and zero status words, as the any-length call leaves them
        return code(false, 0u, 0u, 1u, d_frames, frames_cap, d_frame_offsets, d_status, st);
    if (tail == 0) // whole frames only: the plain call, its bytes and offsets
        return code(true, 0u, frames, (uint32_t)SELA_HIP_SAMPLES_PER_FRAME, d_frames, frames_cap, d_frame_offsets, d_status, st);
    const uint32_t last = frames - 1, last_samples = (uint32_t)(n_samples - (uint64_t)last * SELA_HIP_SAMPLES_PER_FRAME);
    if (last == 0) // one frame, of up to 4095 samples: the any-length call as it stands
        return code(false, 0u, 1u, last_samples, d_frames, frames_cap, d_frame_offsets, d_status, st);
    const int rc = fork_join(
        whole_lane(), st, name,
        [&](hipStream_t side) { return code(false, last, 1u, last_samples, coded.frame, coded.cap, coded.offsets, coded.status, side); },
        [&] { return code(true, 0u, last, (uint32_t)SELA_HIP_SAMPLES_PER_FRAME, d_frames, frames_cap, d_frame_offsets, d_status, st); });
    if (rc != SELA_HIP_OK)
        return rc;
    return launched(sela::launch_whole_splice(coded, channels, d_frames, frames_cap, d_frame_offsets, last, d_status, st), (std::string(name) + " splice").c_str());
}

// The tail of both host-pointer encoders: `encode_last(out, cap, offsets)` codes the last frame, which starts behind `whole`
// frames, as a stream of its own -- offsets {0, bytes} -- at frame_offsets_out[whole]; frame_offsets_out[whole + 1] is patched.
extern "C++" template <typename EncodeLast>
int encode_whole_last(uint32_t whole, uint8_t* frames_out, size_t frames_cap, uint64_t* frame_offsets_out, EncodeLast encode_last)
{
    const uint64_t before = frame_offsets_out[whole];
    uint64_t last_offsets[2] = { 0, 0 };
    const int rc = encode_last(frames_out + before, frames_cap - (size_t)before, last_offsets);
    frame_offsets_out[whole + 1] = before + last_offsets[1];
    return rc;
}
} // namespace

int sela_hip_encode_whole_device(const int16_t* d_pcm, uint64_t n_samples, uint32_t channels, uint8_t* d_frames, size_t frames_cap, uint64_t* d_frame_offsets,
    uint32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream, uint32_t options)
{
    bool lossless = false;
    int rc = encode_options(options, &lossless);
    if (rc == SELA_HIP_OK)
        rc = whole_arguments(n_samples, channels, d_pcm, d_frames, d_frame_offsets);
    if (rc == SELA_HIP_OK)
        rc = whole_device_arguments(d_pcm, d_frames, d_status, d_workspace, workspace_bytes, sela::whole_workspace_bytes(n_samples, channels), "sela_hip_encode_whole_workspace_bytes");
    if (rc != SELA_HIP_OK)
        return rc;
    if (lossless && g_phase_cycles)
        return fail(SELA_HIP_EINVAL, "SELA_HIP_ENCODE_LOSSLESS while sela_hip_debug_phase_buffer is set: the phase counts are the plain kernels'");
    sela::Carve carve(d_workspace);
    const sela::WholeWs w = sela::carve_whole(carve, n_samples, channels);
    // the samples read in place: 2048-sample frames through the plain call's launches, every other length through the any-length call's
    return encode_whole_frames("encode_whole", n_samples, channels, w.last, d_frames, frames_cap, d_frame_offsets, d_status, static_cast<hipStream_t>(stream),
        [&](bool main_pieces, uint32_t first, uint32_t count, uint32_t length, uint8_t* out, size_t cap, uint64_t* offsets, uint32_t* status, hipStream_t on) {
            const int16_t* const from = d_pcm + (size_t)first * SELA_HIP_SAMPLES_PER_FRAME * channels;
            return main_pieces ? encode_device_call(from, count, channels, out, cap, offsets, status, w.main_workspace, w.main_bytes, nullptr, on, lossless)
                               : encode_i32_device_call(from, true, count, channels, length, out, cap, offsets, status, w.last_workspace, w.last_bytes, on, lossless);
        });
}

// Host pointers: the 2048-sample frames through sela_hip_encode_opt's route, the last frame through the any-length route -- which
// leases a context of its own and never meets the coalescer -- and, for a thread with a streaming job open, everything there.
int sela_hip_encode_whole(const int16_t* pcm, uint64_t n_samples, uint32_t channels, uint8_t* frames_out, size_t frames_cap, uint64_t* frame_offsets_out,
    uint32_t options)
{
    bool lossless = false;
    int rc = encode_options(options, &lossless);
    if (rc == SELA_HIP_OK)
        rc = whole_arguments(n_samples, channels, pcm, frames_out, frame_offsets_out);
    if (rc != SELA_HIP_OK)
        return rc;
    const uint32_t frames = (uint32_t)sela_hip_whole_frames(n_samples), tail = (uint32_t)(n_samples % SELA_HIP_SAMPLES_PER_FRAME);
    frame_offsets_out[0] = 0;
    if (frames == 0)
        return SELA_HIP_OK;
    const uint32_t whole = tail ? frames - 1 : frames; // frames of 2048 samples
    if (whole) {
        const bool job_open = g_lease.held && g_lease.held->job_open;
        rc = job_open ? sela::generic_encode(pcm, true, whole, channels, SELA_HIP_SAMPLES_PER_FRAME, frames_out, frames_cap, frame_offsets_out, lossless)
                      : sela_hip_encode_opt(pcm, whole, channels, SELA_HIP_SAMPLES_PER_FRAME, frames_out, frames_cap, frame_offsets_out, options);
        if (rc != SELA_HIP_OK || !tail)
            return rc;
    }
    return encode_whole_last(whole, frames_out, frames_cap, frame_offsets_out, [&](uint8_t* out, size_t cap, uint64_t* last_offsets) {
        return sela::generic_encode(pcm + (size_t)whole * SELA_HIP_SAMPLES_PER_FRAME * channels, true, 1, channels,
            (uint32_t)(n_samples - (uint64_t)whole * SELA_HIP_SAMPLES_PER_FRAME), out, cap, last_offsets, lossless);
    });
}

// ---- the same track from packed 3- or 4-byte PCM (the workspace: sela_whole.hip) ------------------------------------
namespace {
// sela_hip_encode_pcm_device's checks of the shape and the options in its order, on sela_hip_encode_whole_device's frames
int whole_pcm_arguments(uint32_t bytes_per_sample, uint64_t n_samples, uint32_t channels, uint32_t options, bool* lossless, const void* pcm, const void* frames,
    const void* frame_offsets)
{
    if (bytes_per_sample != 3 && bytes_per_sample != 4)
        return fail(SELA_HIP_EINVAL, "bytes_per_sample must be 3 or 4 (16-bit samples: sela_hip_encode_whole_device and sela_hip_encode_whole)");
    if (channels == 0 || channels > 255)
        return fail(SELA_HIP_EINVAL, "channels must be in 1..255");
    if (sela_hip_whole_frames(n_samples) * sela::generic_signals(channels, false) >= (1ull << 31))
        return fail(SELA_HIP_EINVAL, "frames * signals per frame must stay below 2^31");
    const int rc = encode_options(options, lossless);
    if (rc != SELA_HIP_OK)
        return rc;
    if (!frame_offsets || (n_samples && (!pcm || !frames)))
        return fail(SELA_HIP_EINVAL, "null pointer");
    return SELA_HIP_OK;
}
} // namespace

// The launches: k_pcm_unpack and the any-length encoder's three on frames 0 .. F - 2, on `stream`; the last frame's own unpack and
// three launches on the side stream, forked before the main launches and joined behind them (encode_whole_frames); the splice.
// The last frame's packed bytes start at byte (F - 1) * 2048 * channels * bytes_per_sample: a multiple of 4, as the unpack asks.
int sela_hip_encode_whole_pcm_device(const void* d_pcm, uint32_t bytes_per_sample, uint64_t n_samples, uint32_t channels, uint32_t options, uint8_t* d_frames,
    size_t frames_cap, uint64_t* d_frame_offsets, uint32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream)
{
    bool lossless = false;
    int rc = whole_pcm_arguments(bytes_per_sample, n_samples, channels, options, &lossless, d_pcm, d_frames, d_frame_offsets);
    if (rc == SELA_HIP_OK)
        rc = whole_device_arguments(d_pcm, d_frames, d_status, d_workspace, workspace_bytes, sela::whole_pcm_workspace_bytes(n_samples, channels),
            "sela_hip_encode_whole_pcm_workspace_bytes");
    if (rc != SELA_HIP_OK)
        return rc;
    sela::Carve carve(d_workspace);
    const sela::WholePcmWs w = sela::carve_whole_pcm(carve, n_samples, channels);
    // the frames unpacked into the workspace's samples and coded by the any-length encoder's launches
    return encode_whole_frames("encode_whole_pcm", n_samples, channels, w.last, d_frames, frames_cap, d_frame_offsets, d_status, static_cast<hipStream_t>(stream),
        [&](bool main_pieces, uint32_t first, uint32_t count, uint32_t length, uint8_t* out, size_t cap, uint64_t* offsets, uint32_t* status, hipStream_t on) {
            const uint8_t* const from = static_cast<const uint8_t*>(d_pcm) + (size_t)first * SELA_HIP_SAMPLES_PER_FRAME * channels * bytes_per_sample;
            int32_t* const samples = main_pieces ? w.main_samples : w.last_samples;
            hipError_t e = sela::launch_pcm_unpack(from, bytes_per_sample, count, channels, length, samples, on);
            if (e == hipSuccess)
                e = sela::launch_encode_i32_device(samples, false, count, channels, length, out, cap, offsets, status, main_pieces ? w.main_workspace : w.last_workspace, on,
                    lossless);
            return launched(e, "encode_whole_pcm launch");
        });
}

// Host pointers: frames 0 .. F - 2 in sela_hip_encode_pcm's chunks, the last frame as one more chunk of its own length, on the
// calling thread's leased context, past the coalescer; an open streaming job is left alone.
int sela_hip_encode_whole_pcm(const void* pcm, uint32_t bytes_per_sample, uint64_t n_samples, uint32_t channels, uint32_t options, uint8_t* frames_out,
    size_t frames_cap, uint64_t* frame_offsets_out)
{
    bool lossless = false;
    int rc = whole_pcm_arguments(bytes_per_sample, n_samples, channels, options, &lossless, pcm, frames_out, frame_offsets_out);
    if (rc != SELA_HIP_OK)
        return rc;
    const uint32_t frames = (uint32_t)sela_hip_whole_frames(n_samples);
    frame_offsets_out[0] = 0;
    if (frames == 0)
        return SELA_HIP_OK;
    const uint32_t whole = frames - 1; // the frames of 2048 samples in front of the last one
    const uint8_t* const bytes = static_cast<const uint8_t*>(pcm);
    if (whole) {
        rc = sela::generic_encode_pcm(bytes, bytes_per_sample, whole, channels, SELA_HIP_SAMPLES_PER_FRAME, lossless, frames_out, frames_cap, frame_offsets_out);
        if (rc != SELA_HIP_OK)
            return rc;
    }
    return encode_whole_last(whole, frames_out, frames_cap, frame_offsets_out, [&](uint8_t* out, size_t cap, uint64_t* last_offsets) {
        return sela::generic_encode_pcm(bytes + (size_t)whole * SELA_HIP_SAMPLES_PER_FRAME * channels * bytes_per_sample, bytes_per_sample, 1, channels,
            (uint32_t)(n_samples - (uint64_t)whole * SELA_HIP_SAMPLES_PER_FRAME), lossless, out, cap, last_offsets);
    });
}

namespace {
// the fast route: 2048 samples per channel and frame
int decode_standard(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, int16_t* pcm_out)
{
    if (n_frames == 0 || n_frames > kCoalesceFrames || (g_lease.held && g_lease.held->job_open))
        return decode_now(frames, frame_offsets, n_frames, channels, pcm_out);
    for (uint32_t f = 0; f < n_frames; f++) // (what the job would refuse is refused by the job, for this caller alone)
        if (frame_offsets[f + 1] < frame_offsets[f] || (frame_offsets[f] & 3))
            return decode_now(frames, frame_offsets, n_frames, channels, pcm_out);
    SmallCall call;
    if (hipGetDevice(&call.device) != hipSuccess)
        return decode_now(frames, frame_offsets, n_frames, channels, pcm_out);
    call.channels = channels, call.n_frames = n_frames;
    call.frames = frames, call.offsets_in = frame_offsets, call.pcm_out = pcm_out;
    return submit_small(Coalescer::kDecode, call);
}
} // namespace

int sela_hip_decode(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, int16_t* pcm_out)
{
    if (channels == 0 || channels > 255 || (n_frames && (!frames || !frame_offsets || !pcm_out)))
        return fail(SELA_HIP_EINVAL, "bad argument");
    // The fast kernels first, unasked: a stream of 2048-sample frames -- every stream an encoder writes -- pays nothing for the
    // other kind (a walk over the headers in host memory is a cache miss or two per frame: 0.1 ms and more for a 3-minute
    // track, a tenth of the whole call).  They refuse a subframe that does not say 2048 (SELA_HIP_EFORMAT, nothing written
    // beyond [n_frames][2048][channels], which is why pcm_out must hold that much, sela_hip.h); only then are the headers
    // walked, and a stream that turns out to be of the other kind goes, whole, down the any-length route.
    // (One look is free: the first subframe of the first frame.  A stream that says another length there is not offered to
    // the fast kernels at all -- they would write 2048-sample frames of silence into a pcm_out its caller sized from
    // sela_hip_index_samples().  A stream that turns odd LATER still needs the room the header asks for.)
    bool first_is_standard = true;
    if (n_frames && frame_offsets[1] >= frame_offsets[0]) {
        SelaSubframeHeader h;
        h.n = SELA_HIP_SAMPLES_PER_FRAME; // (stays so when the header itself is not in the frame)
        sela_subframe_read_bytes(frames + frame_offsets[0], frame_offsets[1] - frame_offsets[0], 4, &h);
        first_is_standard = h.n == SELA_HIP_SAMPLES_PER_FRAME;
    }
    const int rc = first_is_standard ? decode_standard(frames, frame_offsets, n_frames, channels, pcm_out) : SELA_HIP_EFORMAT;
    if (rc != SELA_HIP_EFORMAT || n_frames == 0)
        return rc;
    const std::string first_error = first_is_standard ? std::string(sela_hip_last_error()) : std::string("malformed frame stream");
    if (sela::check_frame_offsets(frame_offsets, n_frames) != SELA_HIP_OK)
        return SELA_HIP_EFORMAT;
    bool standard = true;
    std::vector<uint64_t> sample_offsets((size_t)n_frames + 1);
    const uint32_t largest = sela::generic_index_samples(frames, frame_offsets, n_frames, channels, sample_offsets.data(), &standard);
    if (standard || largest == 0)
        return fail(rc, first_error); // (malformed in the ordinary sense)
    return sela::generic_decode(frames, frame_offsets, n_frames, channels, nullptr, largest, nullptr, pcm_out, sample_offsets.data());
}

// ---- a full decode of a whole-track stream (the plan: sela_decode_whole_plan.h, the kernels: sela_window_whole.hip) ----
size_t sela_hip_decode_whole_workspace_bytes(uint32_t max_frames, uint32_t channels) { return sela::decode_whole_workspace_bytes(max_frames, channels); }

extern "C++" {
namespace {
// sela_hip_decode_whole_device / sela_hip_decode_whole_payload_device: the forms of the any-length calls (FramesForm, PayloadForm),
// the window calls' channels.  The launch: the plan on `stream`; the last frame's two kernels on the whole-track lane's side
// stream, forked behind the plan; the 2048-sample decoder on `stream` beside them, on the plan's count; the join (fork_join).
template <typename Form>
int decode_whole_call(const Form& form, uint32_t channels, int16_t* d_pcm_out, uint64_t pcm_capacity, uint64_t* d_n_samples, uint32_t* d_status, void* d_workspace,
    size_t workspace_bytes, void* stream)
{
    const auto formula = [](uint32_t max_frames, uint32_t ch, uint32_t) { return sela::decode_whole_workspace_bytes(max_frames, ch); };
    const DeviceCallOf<decltype(formula)> c = { "decode_whole", formula, channels, 0, d_workspace, workspace_bytes, static_cast<hipStream_t>(stream) };
    return form(
        c,
        [&](uint32_t n_frames) {
            if (channels == 0 || channels > 8)
                return fail(SELA_HIP_EINVAL, "channels must be in 1..8: the last frame is decoded by the window calls' kernels (more channels: sela_hip_decode_n_device)");
            int rc = need_pointers(d_status && d_n_samples && d_workspace && (!n_frames || d_pcm_out));
            if (rc == SELA_HIP_OK && (((uintptr_t)d_pcm_out & 1) || ((uintptr_t)d_n_samples & 7) || ((uintptr_t)d_status & 3)))
                rc = fail(SELA_HIP_EINVAL, "d_pcm_out must be 2-byte aligned, d_n_samples 8-byte aligned and d_status 4-byte aligned");
            return rc;
        },
        [&](const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t max_frames, const uint32_t* d_n_found, void* d_ws) {
            sela::Carve carve(d_ws);
            const sela::DecodeWholeWs w = sela::carve_decode_whole(carve, max_frames, channels);
            const hipStream_t st = c.stream;
            int rc = launched(sela::launch_decode_whole_plan(d_frames, d_frame_offsets, max_frames, d_n_found, pcm_capacity, w, d_n_samples, d_status, st), "decode_whole plan");
            if (rc != SELA_HIP_OK || max_frames == 0)
                return rc;
            int dev = -1;
            rc = fork_join(
                whole_lane(), st, "decode_whole",
                // the last frame on the side stream: memory disjoint from what the 2048-sample decoder writes ...
                [&](hipStream_t side) { return launched(sela::launch_decode_whole_tail(d_frames, d_frame_offsets, channels, w, d_pcm_out, d_status, side), "decode_whole tail"); },
                // ... beside it frames 0 .. n - 2 (or all n), on the plan's count; the status words are the plan's, so they are not zeroed
                // (no priorities: the launch does not have the device to itself)
                [&] {
                    return launched(sela::launch_decode(d_frames, d_frame_offsets, max_frames, channels, d_pcm_out, d_status, w.fast_workspace, st, nullptr, nullptr, nullptr,
                                        g_recurrence_form, 0, w.fast_frames, false),
                        "decode_whole launch");
                },
                &dev);
            if (rc == SELA_HIP_OK && !stream_is_capturing(st))
                flights().note(dev, st);
            return rc;
        });
}

// the codes of two halves of one stream, in sela_hip_decode_whole_status_error's order
int first_in_order(int a, int b)
{
    for (const int code : { SELA_HIP_ECAPACITY, SELA_HIP_EFORMAT, SELA_HIP_ERANGE, SELA_HIP_ENODEV })
        if (a == code || b == code)
            return code;
    return a != SELA_HIP_OK ? a : b;
}
} // namespace
} // extern "C++"

int sela_hip_decode_whole_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames, uint32_t channels, int16_t* d_pcm_out, uint64_t pcm_capacity,
    uint64_t* d_n_samples, uint32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream)
{
    return decode_whole_call(FramesForm{ d_frames, d_frame_offsets, n_frames }, channels, d_pcm_out, pcm_capacity, d_n_samples, d_status, d_workspace, workspace_bytes, stream);
}

int sela_hip_decode_whole_payload_device(const uint8_t* d_payload, size_t payload_bytes, uint32_t max_frames, uint32_t channels, int16_t* d_pcm_out, uint64_t pcm_capacity,
    uint64_t* d_n_samples, uint64_t* d_frame_offsets, uint32_t* d_n_frames, uint32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream)
{
    return decode_whole_call(PayloadForm{ d_payload, payload_bytes, max_frames, d_frame_offsets, d_n_frames }, channels, d_pcm_out, pcm_capacity, d_n_samples, d_status,
        d_workspace, workspace_bytes, stream);
}

// The order is the header's: capacity, format (a malformed frame or a dry Rice stream), range, internal.  The flags alone: status[1]
// counts a last frame that was declined for its coefficients too, which is a matter of range.
int sela_hip_decode_whole_status_error(const uint32_t* status)
{
    if (!status)
        return fail(SELA_HIP_EINVAL, "null pointer");
    return sela::judge_decode(status[0], SELA_HIP_FLAG_STRIDE | sela::kJudgeJob | SELA_HIP_FLAG_INTERNAL, status[3] == sela::kWholeRouteTail ? sela::kRouteDevice32 : sela::kRouteFast,
        "decode_whole");
}

// Host pointers, synchronous: the plan on the caller's bytes; frames 0 .. n - 2 where sela_hip_decode sends 2048-sample frames, the
// last frame through the any-length route's one-shot decode on its own leased context, past the coalescer.  A thread with a
// streaming job open gets both from that route, which leaves the job alone.
int sela_hip_decode_whole(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, int16_t* pcm_out, uint64_t pcm_capacity,
    uint64_t* n_samples)
{
    if (channels == 0 || channels > 8)
        return fail(SELA_HIP_EINVAL, "channels must be in 1..8 (more channels: sela_hip_decode)");
    if (!n_samples || (n_frames && (!frames || !frame_offsets || !pcm_out)))
        return fail(SELA_HIP_EINVAL, "null pointer");
    *n_samples = 0;
    if (n_frames == 0)
        return SELA_HIP_OK;
    if (sela::check_frame_offsets(frame_offsets, n_frames) != SELA_HIP_OK)
        return SELA_HIP_EFORMAT;
    const sela::DecodeWholePlan plan = sela::plan_decode_whole(frames, frame_offsets, n_frames, pcm_capacity);
    *n_samples = plan.samples;
    if (plan.flags & SELA_HIP_FLAG_STRIDE)
        return fail(SELA_HIP_ECAPACITY, "pcm_capacity is smaller than the stream's samples per channel (*n_samples)");
    int rc_front = SELA_HIP_OK;
    if (plan.fast_frames) {
        if (g_lease.held && g_lease.held->job_open) {
            std::vector<uint64_t> sample_offsets((size_t)plan.fast_frames + 1);
            for (uint32_t f = 0; f <= plan.fast_frames; f++)
                sample_offsets[f] = (uint64_t)SELA_HIP_SAMPLES_PER_FRAME * f;
            rc_front = sela::generic_decode(frames, frame_offsets, plan.fast_frames, channels, nullptr, SELA_HIP_SAMPLES_PER_FRAME, nullptr, pcm_out, sample_offsets.data());
        } else {
            rc_front = decode_standard(frames, frame_offsets, plan.fast_frames, channels, pcm_out);
        }
    }
    if (plan.route != sela::kWholeRouteTail)
        return rc_front;
    const std::string front_error = rc_front != SELA_HIP_OK ? std::string(sela_hip_last_error()) : std::string();
    const uint64_t at = frame_offsets[plan.tail.frame];
    const uint64_t last_offsets[2] = { 0, frame_offsets[plan.tail.frame + 1] - at }, last_samples[2] = { 0, plan.tail.n };
    // (the stride is the longest subframe's, as sela_hip_decode finds it: a frame whose channels disagree is the combine's to refuse)
    const uint32_t largest = sela::generic_index_samples(frames + at, last_offsets, 1, channels, nullptr, nullptr);
    const int rc_last = largest == 0 ? fail(SELA_HIP_EFORMAT, "malformed frame stream (the last frame's header walk breaks)")
                                     : sela::generic_decode(frames + at, last_offsets, 1, channels, nullptr, largest, nullptr,
                                           pcm_out + (size_t)SELA_HIP_SAMPLES_PER_FRAME * plan.tail.frame * channels, last_samples);
    const int rc = first_in_order(rc_front, rc_last);
    if (rc != SELA_HIP_OK && rc == rc_front && rc != rc_last)
        return fail(rc, front_error);
    return rc;
}

size_t sela_hip_encode_bound_bytes_n(uint32_t n_frames, uint32_t channels, uint32_t samples_per_channel)
{
    if (samples_per_channel == SELA_HIP_SAMPLES_PER_FRAME)
        return sela_hip_encode_bound_bytes(n_frames, channels);
    return sela::generic_encode_bound_bytes(n_frames, channels, samples_per_channel);
}

uint32_t sela_hip_index_samples(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, uint64_t* sample_offsets)
{
    if (!frames || !frame_offsets || channels == 0) {
        if (sample_offsets)
            for (uint32_t f = 0; f <= n_frames; f++)
                sample_offsets[f] = 0;
        return 0;
    }
    if (!sela::frame_offsets_ascend(frame_offsets, n_frames))
        return 0;
    return sela::generic_index_samples(frames, frame_offsets, n_frames, channels, sample_offsets, nullptr);
}

int sela_hip_encode_i32(const int32_t* samples, uint32_t n_frames, uint32_t channels, uint32_t samples_per_channel, uint8_t* frames_out, size_t frames_cap,
    uint64_t* frame_offsets_out)
{
    if (samples_per_channel == 0 || samples_per_channel > 65535)
        return fail(SELA_HIP_EINVAL, "samples_per_channel must be 1 .. 65535 (the subframe's field is 16 bits wide)");
    if (channels == 0 || channels > 255 || !frame_offsets_out || (n_frames && (!samples || !frames_out)))
        return fail(SELA_HIP_EINVAL, "bad argument");
    // Small calls from many threads -- the reference's thread loop over frame::FrameEncoder (src/sela/encoder.cpp:58-73) on frames
    // that are not the CLI's shape -- go to the device together, like the one-shot calls of the fast path (sela_coalescer.h):
    // calls of one shape (channels, samples per channel) share a job, every call gets its own bytes and its own error.  Not for a
    // thread with a job open: a batch's leader gives its contexts back when the batch is through (HipBackend::after_batch), the
    // job's with them; the any-length route leases a context of its own, so the call itself goes straight there.
    SmallCall call;
    if (n_frames == 0 || n_frames > kCoalesceFrames || (size_t)n_frames * channels * samples_per_channel > ((size_t)1 << 20) || (g_lease.held && g_lease.held->job_open)
        || hipGetDevice(&call.device) != hipSuccess)
        return sela::generic_encode(samples, false, n_frames, channels, samples_per_channel, frames_out, frames_cap, frame_offsets_out);
    call.channels = channels, call.n_frames = n_frames, call.shape = samples_per_channel;
    call.samples = samples, call.frames_out = frames_out, call.frames_cap = frames_cap, call.offsets_out = frame_offsets_out;
    return submit_small(Coalescer::kEncode32, call);
}

// options != 0: straight to the any-length route (past the coalescer, whose batches are the plain call's)
int sela_hip_encode_i32_opt(const int32_t* samples, uint32_t n_frames, uint32_t channels, uint32_t samples_per_channel, uint8_t* frames_out, size_t frames_cap,
    uint64_t* frame_offsets_out, uint32_t options)
{
    bool lossless = false;
    const int rc = encode_options(options, &lossless);
    if (rc != SELA_HIP_OK)
        return rc;
    if (!lossless)
        return sela_hip_encode_i32(samples, n_frames, channels, samples_per_channel, frames_out, frames_cap, frame_offsets_out);
    if (samples_per_channel == 0 || samples_per_channel > 65535)
        return fail(SELA_HIP_EINVAL, "samples_per_channel must be 1 .. 65535 (the subframe's field is 16 bits wide)");
    if (channels == 0 || channels > 255 || !frame_offsets_out || (n_frames && (!samples || !frames_out)))
        return fail(SELA_HIP_EINVAL, "bad argument");
    return sela::generic_encode(samples, false, n_frames, channels, samples_per_channel, frames_out, frames_cap, frame_offsets_out, true);
}

// The paired one-shot calls: where the lossless one-shot calls run -- the any-length route, in its chunks of
// frames, past the coalescer (whose batches are the plain call's); an open streaming job of the thread is left alone.
namespace {
int encode_paired_host(const void* input, bool in16, uint32_t n_frames, uint32_t channels, uint32_t samples_per_channel, uint8_t* frames_out, size_t frames_cap,
    uint64_t* frame_offsets_out, uint32_t options)
{
    bool lossless = false;
    const int rc = paired_options(options, &lossless);
    if (rc != SELA_HIP_OK)
        return rc;
    if (samples_per_channel == 0 || samples_per_channel > 65535)
        return fail(SELA_HIP_EINVAL, "samples_per_channel must be 1 .. 65535 (the subframe's field is 16 bits wide)");
    if (channels == 0 || channels > 255 || !frame_offsets_out || (n_frames && (!input || !frames_out)))
        return fail(SELA_HIP_EINVAL, "bad argument");
    return sela::generic_encode(input, in16, n_frames, channels, samples_per_channel, frames_out, frames_cap, frame_offsets_out, lossless, true);
}
} // namespace

int sela_hip_encode_paired_i32(const int32_t* samples, uint32_t n_frames, uint32_t channels, uint32_t samples_per_channel, uint8_t* frames_out, size_t frames_cap,
    uint64_t* frame_offsets_out, uint32_t options)
{
    return encode_paired_host(samples, false, n_frames, channels, samples_per_channel, frames_out, frames_cap, frame_offsets_out, options);
}

int sela_hip_encode_paired(const int16_t* pcm, uint32_t n_frames, uint32_t channels, uint32_t samples_per_channel, uint8_t* frames_out, size_t frames_cap,
    uint64_t* frame_offsets_out, uint32_t options)
{
    return encode_paired_host(pcm, true, n_frames, channels, samples_per_channel, frames_out, frames_cap, frame_offsets_out, options);
}

namespace {
// One frame whose channels differ in length (src/frame/frame_encoder.cpp:11-102): every channel is a block of its own -- coded
// as a one-channel frame of its own length by the any-length kernels -- and the frame is their subframes, renamed, behind one
// sync word; the second channel of an exactly-stereo frame against the difference channel 0 - channel 1 over its own length.
int encode_ragged_call(const int32_t* samples, const uint32_t* lengths, uint32_t channels, uint8_t* frame_out, size_t frame_cap, size_t* frame_bytes, bool lossless)
{
    if (channels == 0 || channels > 255 || !samples || !lengths || !frame_out || !frame_bytes)
        return fail(SELA_HIP_EINVAL, "bad argument");
    for (uint32_t c = 0; c < channels; c++)
        if (lengths[c] == 0 || lengths[c] > 65535)
            return fail(SELA_HIP_EINVAL, "every channel holds 1 .. 65535 samples (the subframe's field is 16 bits wide)");
    if (channels == 2 && lengths[0] < lengths[1])
        return fail(SELA_HIP_EINVAL, "an exactly-stereo frame whose first channel is the shorter one: the reference's difference signal reads it past its end (src/frame/frame_encoder.cpp:22-24)");
    if (frame_cap < 4)
        return fail(SELA_HIP_ECAPACITY, "frame_out too small");
    // a one-channel frame: sync word (4) | channel, type, parent | k, words (u16), order | words | k, words (u16), n (u16) | words
    auto mono = [&](const int32_t* x, uint32_t n, std::vector<uint8_t>& bytes, uint32_t& words) -> int {
        bytes.resize(sela::generic_encode_bound_bytes(1, 1, n));
        uint64_t offs[2] = { 0, 0 };
        const int rc = sela::generic_encode(x, false, 1, 1, n, bytes.data(), bytes.size(), offs, lossless);
        if (rc != SELA_HIP_OK)
            return rc;
        bytes.resize((size_t)offs[1]);
        const uint32_t cw = bytes[8] | ((uint32_t)bytes[9] << 8);
        const size_t p2 = 4 + 7 + 4 * (size_t)cw;
        words = cw + (bytes[p2 + 1] | ((uint32_t)bytes[p2 + 2] << 8));
        return SELA_HIP_OK;
    };
    const uint32_t sync = SELA_SYNC_WORD;
    std::memcpy(frame_out, &sync, 4);
    size_t at = 4;
    const int32_t* cur = samples;
    std::vector<uint8_t> own, dif;
    std::vector<int32_t> d;
    for (uint32_t c = 0; c < channels; c++) {
        const uint32_t n = lengths[c];
        uint32_t own_words = 0, dif_words = 0;
        int rc = mono(cur, n, own, own_words);
        if (rc != SELA_HIP_OK)
            return rc;
        const std::vector<uint8_t>* take = &own;
        uint8_t type = 0, parent = (uint8_t)c;
        if (channels == 2 && c == 1) { // :18-72
            d.resize(n);
            for (uint32_t j = 0; j < n; j++)
                d[j] = (int32_t)((uint32_t)samples[j] - (uint32_t)cur[j]);
            rc = mono(d.data(), n, dif, dif_words);
            if (rc != SELA_HIP_OK)
                return rc;
            if (dif_words < own_words) // :64-66: strictly fewer words
                take = &dif, type = 1, parent = 0;
        }
        const size_t sub = take->size() - 4;
        if (at + sub > frame_cap)
            return fail(SELA_HIP_ECAPACITY, "frame_out too small (4 + the sum over the channels of sela_hip_encode_bound_bytes_n(1, 1, lengths[c]) holds any frame of 17-bit samples)");
        std::memcpy(frame_out + at, take->data() + 4, sub);
        frame_out[at] = (uint8_t)c, frame_out[at + 1] = type, frame_out[at + 2] = parent;
        at += sub;
        cur += n;
    }
    *frame_bytes = at;
    return SELA_HIP_OK;
}
} // namespace

int sela_hip_encode_ragged_i32(const int32_t* samples, const uint32_t* lengths, uint32_t channels, uint8_t* frame_out, size_t frame_cap, size_t* frame_bytes)
{
    return encode_ragged_call(samples, lengths, channels, frame_out, frame_cap, frame_bytes, false);
}

int sela_hip_encode_ragged_i32_opt(const int32_t* samples, const uint32_t* lengths, uint32_t channels, uint8_t* frame_out, size_t frame_cap, size_t* frame_bytes,
    uint32_t options)
{
    bool lossless = false;
    const int rc = encode_options(options, &lossless);
    return rc != SELA_HIP_OK ? rc : encode_ragged_call(samples, lengths, channels, frame_out, frame_cap, frame_bytes, lossless);
}

int sela_hip_decode_i32(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, int32_t* samples_out, uint32_t stride,
    uint32_t* counts_out)
{
    if (channels == 0 || channels > 255 || (n_frames && (!frames || !frame_offsets || !samples_out || !counts_out)))
        return fail(SELA_HIP_EINVAL, "bad argument");
    if (n_frames == 0)
        return SELA_HIP_OK;
    if (sela::check_frame_offsets(frame_offsets, n_frames) != SELA_HIP_OK)
        return SELA_HIP_EFORMAT;
    const uint32_t largest = sela::generic_index_samples(frames, frame_offsets, n_frames, channels, nullptr, nullptr);
    if (largest > stride)
        return fail(SELA_HIP_ECAPACITY, "stride is smaller than the largest samplesPerChannel of the stream (see sela_hip_index_samples)");
    // (a stream the host walk cannot follow reports 0: the kernels find and report the malformed frame)
    // Small calls from many threads -- the reference's thread loop over frame::FrameDecoder -- go to the device together, like
    // the one-shot calls of the fast path (sela_coalescer.h): every call its own rows, its own error.
    SmallCall call;
    if (n_frames > kCoalesceFrames || (g_lease.held && g_lease.held->job_open) || hipGetDevice(&call.device) != hipSuccess) // (a thread with a job open: as in sela_hip_encode_i32)
        return sela::generic_decode(frames, frame_offsets, n_frames, channels, samples_out, stride, counts_out, nullptr, nullptr);
    call.channels = channels, call.n_frames = n_frames;
    call.frames = frames, call.offsets_in = frame_offsets, call.samples_out = samples_out, call.stride = stride, call.counts_out = counts_out;
    return submit_small(Coalescer::kDecode32, call);
}

int sela_hip_lpc_encode_n(const int32_t* samples, uint32_t n_blocks, uint32_t samples_per_block, int32_t* order_out, int32_t* q_out, int32_t* residues_out)
{
    if (n_blocks && (!samples || !order_out || !q_out || !residues_out))
        return fail(SELA_HIP_EINVAL, "null pointer");
    if (samples_per_block == 0 || samples_per_block > (1u << 24))
        return fail(SELA_HIP_EINVAL, "samples_per_block must be 1 .. 2^24");
    if (n_blocks == 0)
        return sela::device_ready();
    return sela::generic_lpc_encode(samples, n_blocks, samples_per_block, order_out, q_out, residues_out);
}

int sela_hip_lpc_decode_n(const int32_t* order, const int32_t* q, const int32_t* residues, uint32_t n_blocks, uint32_t samples_per_block, int32_t* samples_out,
    int64_t* coefs_out)
{
    if (n_blocks && (!order || !q || (samples_out && !residues) || (!samples_out && !coefs_out)))
        return fail(SELA_HIP_EINVAL, "null pointer");
    if (samples_per_block == 0 || samples_per_block > (1u << 24))
        return fail(SELA_HIP_EINVAL, "samples_per_block must be 1 .. 2^24");
    if (n_blocks == 0)
        return sela::device_ready();
    return sela::generic_lpc_decode(order, q, residues, n_blocks, samples_per_block, samples_out, coefs_out);
}

int sela_hip_lpc_encode(const int32_t* samples, uint32_t n_blocks, int32_t* order_out, int32_t* q_out, int32_t* residues_out)
{
    if (n_blocks && (!samples || !order_out || !q_out || !residues_out))
        return fail(SELA_HIP_EINVAL, "null pointer");
    if (sela::device_ready() != SELA_HIP_OK)
        return SELA_HIP_ENODEV;
    if (n_blocks == 0)
        return SELA_HIP_OK;
    // A block is analysed as the DIFFERENCE signal of a stereo frame (left - right = the block's samples): that is how 17-bit
    // samples reach the kernels, whose input is the 16-bit PCM of a WAV file.  The trace build of k_encode_blocks leaves the
    // order and the quantised coefficients of every signal in its trace, and here the residues too.
    constexpr size_t kBlk = SELA_HIP_SAMPLES_PER_FRAME;
    std::vector<int16_t> pcm((size_t)n_blocks * kBlk * 2);
    for (size_t i = 0; i < (size_t)n_blocks * kBlk; i++) {
        const int32_t s = samples[i];
        if (s < -65535 || s > 65535) // beyond 16-bit channels and their difference: not the fast kernels' input
            return sela::generic_lpc_encode(samples, n_blocks, SELA_HIP_SAMPLES_PER_FRAME, order_out, q_out, residues_out);
        const int32_t left = s > 32767 ? 32767 : (s < -32768 ? -32768 : s);
        pcm[2 * i] = (int16_t)left;
        pcm[2 * i + 1] = (int16_t)(left - s);
    }
    hipError_t e = hipSuccess;
    Scratch mem;
    const size_t ws = sela::encode_workspace_bytes(n_blocks, 2), cap = sela_hip_encode_bound_bytes(n_blocks, 2);
    int16_t* d_pcm = mem.upload(pcm.data(), pcm.size(), e);
    uint8_t* d_frames = mem.take<uint8_t>(cap, e);
    uint64_t* d_offsets = mem.take<uint64_t>((size_t)n_blocks + 1, e);
    uint32_t* d_status = mem.take<uint32_t>(4, e);
    uint8_t* d_ws = mem.take<uint8_t>(ws, e);
    sela_hip_trace* d_trace = mem.take<sela_hip_trace>((size_t)n_blocks * 3, e);
    int32_t* d_res = mem.take<int32_t>((size_t)n_blocks * 3 * kBlk, e);
    if (e == hipSuccess)
        e = sela::launch_encode(d_pcm, n_blocks, 2, d_frames, cap, d_offsets, d_status, d_ws, d_trace, nullptr, nullptr, nullptr, nullptr, 0, -1, 0, d_res);
    if (e == hipSuccess)
        e = hipDeviceSynchronize();
    std::vector<sela_hip_trace> trace((size_t)n_blocks * 3);
    if (e == hipSuccess)
        e = hipMemcpy(trace.data(), d_trace, trace.size() * sizeof(sela_hip_trace), hipMemcpyDeviceToHost);
    for (uint32_t b = 0; b < n_blocks && e == hipSuccess; b++) // signal 2 of frame b
        e = hipMemcpy(residues_out + (size_t)b * kBlk, d_res + ((size_t)b * 3 + 2) * kBlk, kBlk * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess)
        return fail_hip(e, "lpc_encode");
    uint32_t flags = 0;
    for (uint32_t b = 0; b < n_blocks; b++) {
        const sela_hip_trace& t = trace[(size_t)b * 3 + 2];
        order_out[b] = t.order;
        for (int i = 0; i < SELA_MAX_LPC_ORDER; i++)
            q_out[(size_t)b * SELA_MAX_LPC_ORDER + i] = i < t.order ? t.q[i] : 0;
        flags |= t.flags;
    }
    if (flags & (SELA_HIP_FLAG_RICE_RANGE | SELA_HIP_FLAG_COEF_OVERFLOW))
        return fail(SELA_HIP_ERANGE, "lpc_encode: a block left the range the format can carry");
    return SELA_HIP_OK;
}

int sela_hip_lpc_decode(const int32_t* order, const int32_t* q, const int32_t* residues, uint32_t n_blocks, int32_t* samples_out, int64_t* coefs_out)
{
    if (n_blocks && (!order || !q || (samples_out && !residues) || (!samples_out && !coefs_out)))
        return fail(SELA_HIP_EINVAL, "null pointer");
    if (sela::device_ready() != SELA_HIP_OK)
        return SELA_HIP_ENODEV;
    if (n_blocks == 0)
        return SELA_HIP_OK;
    constexpr size_t kBlk = SELA_HIP_SAMPLES_PER_FRAME, kCoefs = SELA_MAX_LPC_ORDER + 1;
    hipError_t e = hipSuccess;
    Scratch mem;
    int32_t* d_order = mem.upload(order, n_blocks, e);
    int32_t* d_q = mem.upload(q, (size_t)n_blocks * SELA_MAX_LPC_ORDER, e);
    int32_t* d_res = samples_out ? mem.upload(residues, (size_t)n_blocks * kBlk, e) : nullptr;
    int32_t* d_out = samples_out ? mem.take<int32_t>((size_t)n_blocks * kBlk, e) : nullptr;
    int64_t* d_coefs = coefs_out ? mem.take<int64_t>((size_t)n_blocks * kCoefs, e) : nullptr;
    uint32_t* d_status = mem.take<uint32_t>(4, e);
    if (e == hipSuccess)
        e = hipMemset(d_status, 0, 16);
    if (e == hipSuccess && d_coefs)
        e = hipMemset(d_coefs, 0, (size_t)n_blocks * kCoefs * sizeof(int64_t));
    if (e == hipSuccess)
        e = sela::launch_stage_lpc_decode(d_order, d_q, d_res, n_blocks, d_out, d_coefs, d_status, nullptr);
    uint32_t status[4] = {};
    if (e == hipSuccess)
        e = hipMemcpy(status, d_status, 16, hipMemcpyDeviceToHost); // (synchronises)
    if (e == hipSuccess && samples_out)
        e = hipMemcpy(samples_out, d_out, (size_t)n_blocks * kBlk * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess && coefs_out)
        e = hipMemcpy(coefs_out, d_coefs, (size_t)n_blocks * kCoefs * sizeof(int64_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess)
        return fail_hip(e, "lpc_decode");
    return sela::judge_decode(status[0], sela::kJudgeLpc, sela::kRouteLpc, "lpc_decode"); // (the fast kernels' blocks are 2048 samples: never SHORT_BLOCK)
}

int sela_hip_rice_encode(const int32_t* values, const uint64_t* value_offsets, uint32_t n_streams, uint32_t* k_out, uint32_t* word_counts_out,
    uint32_t* words_out, const uint64_t* word_offsets)
{
    if (n_streams && (!value_offsets || !k_out || !word_counts_out || !word_offsets))
        return fail(SELA_HIP_EINVAL, "null pointer");
    if (sela::device_ready() != SELA_HIP_OK)
        return SELA_HIP_ENODEV;
    if (n_streams == 0)
        return SELA_HIP_OK;
    for (uint32_t i = 0; i < n_streams; i++)
        if (value_offsets[i + 1] < value_offsets[i] || word_offsets[i + 1] < word_offsets[i])
            return fail(SELA_HIP_EINVAL, "offsets must not decrease");
    const size_t n_values = (size_t)value_offsets[n_streams], n_words = (size_t)word_offsets[n_streams];
    if ((n_values && !values) || (n_words && !words_out))
        return fail(SELA_HIP_EINVAL, "null pointer");
    hipError_t e = hipSuccess;
    Scratch mem;
    int32_t* d_values = mem.upload(values, n_values, e);
    uint64_t* d_voff = mem.upload(value_offsets, (size_t)n_streams + 1, e);
    uint64_t* d_woff = mem.upload(word_offsets, (size_t)n_streams + 1, e);
    uint32_t* d_k = mem.take<uint32_t>(n_streams, e);
    uint32_t* d_counts = mem.take<uint32_t>(n_streams, e);
    uint32_t* d_words = mem.take<uint32_t>(n_words, e);
    uint32_t* d_status = mem.take<uint32_t>(4, e);
    if (e == hipSuccess)
        e = hipMemset(d_status, 0, 16);
    if (e == hipSuccess && n_words)
        e = hipMemset(d_words, 0, n_words * sizeof(uint32_t));
    if (e == hipSuccess)
        e = sela::launch_stage_rice_encode(d_values, d_voff, n_streams, d_k, d_counts, d_words, d_woff, d_status, nullptr);
    uint32_t status[4] = {};
    if (e == hipSuccess)
        e = hipMemcpy(status, d_status, 16, hipMemcpyDeviceToHost);
    if (e == hipSuccess)
        e = hipMemcpy(k_out, d_k, n_streams * sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess)
        e = hipMemcpy(word_counts_out, d_counts, n_streams * sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess && n_words)
        e = hipMemcpy(words_out, d_words, n_words * sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess)
        return fail_hip(e, "rice_encode");
    if (status[0] & SELA_HIP_FLAG_RICE_RANGE)
        return fail(SELA_HIP_ERANGE, "rice_encode: a value is beyond the reference's int32 zig-zag (|value| >= 2^30)");
    if (status[0] & SELA_HIP_FLAG_WORDS_CAP)
        return fail(SELA_HIP_ECAPACITY, "rice_encode: a stream needs more words than its range of words_out (see word_counts_out)");
    return SELA_HIP_OK;
}

int sela_hip_rice_decode(const uint32_t* words, const uint64_t* word_offsets, const uint32_t* k, const uint64_t* value_offsets, uint32_t n_streams,
    int32_t* values_out)
{
    if (n_streams && (!word_offsets || !k || !value_offsets))
        return fail(SELA_HIP_EINVAL, "null pointer");
    if (sela::device_ready() != SELA_HIP_OK)
        return SELA_HIP_ENODEV;
    if (n_streams == 0)
        return SELA_HIP_OK;
    for (uint32_t i = 0; i < n_streams; i++)
        if (value_offsets[i + 1] < value_offsets[i] || word_offsets[i + 1] < word_offsets[i] || k[i] >= 32)
            return fail(SELA_HIP_EINVAL, "offsets must not decrease; Rice parameters are below 32");
    const size_t n_values = (size_t)value_offsets[n_streams], n_words = (size_t)word_offsets[n_streams];
    if ((n_values && !values_out) || (n_words && !words))
        return fail(SELA_HIP_EINVAL, "null pointer");
    hipError_t e = hipSuccess;
    Scratch mem;
    uint32_t* d_words = mem.upload(words, n_words, e);
    uint64_t* d_woff = mem.upload(word_offsets, (size_t)n_streams + 1, e);
    uint64_t* d_voff = mem.upload(value_offsets, (size_t)n_streams + 1, e);
    uint32_t* d_k = mem.upload(k, n_streams, e);
    int32_t* d_values = mem.take<int32_t>(n_values, e);
    uint32_t* d_status = mem.take<uint32_t>(4, e);
    if (e == hipSuccess)
        e = hipMemset(d_status, 0, 16);
    if (e == hipSuccess)
        e = sela::launch_stage_rice_decode(d_words, d_woff, d_k, d_voff, n_streams, d_values, d_status, nullptr);
    uint32_t status[4] = {};
    if (e == hipSuccess)
        e = hipMemcpy(status, d_status, 16, hipMemcpyDeviceToHost);
    if (e == hipSuccess && n_values)
        e = hipMemcpy(values_out, d_values, n_values * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess)
        return fail_hip(e, "rice_decode");
    if (status[0] & (SELA_HIP_FLAG_RICE_OVERRUN | SELA_HIP_FLAG_BAD_FRAME))
        return fail(SELA_HIP_EFORMAT, "rice_decode: a stream ended before all its values were read");
    return SELA_HIP_OK;
}

uint32_t sela_hip_index_frames(const uint8_t* frames, size_t frames_bytes, uint32_t n_frames, uint32_t channels, uint64_t* frame_offsets)
{
    size_t off = 0;
    uint32_t f = 0;
    for (; f < n_frames; f++) {
        frame_offsets[f] = off;
        if (off + 4 > frames_bytes)
            break;
        uint32_t sync;
        std::memcpy(&sync, frames + off, 4);
        if (sync != SELA_SYNC_WORD) // src/file/sela_file.cpp:54-56: stop silently
            break;
        uint64_t p = off + 4;
        for (uint32_t c = 0; c < channels && p; c++) {
            SelaSubframeHeader h;
            p = sela_subframe_read_bytes(frames, frames_bytes, p, &h);
        }
        if (!p)
            break;
        off = p;
    }
    frame_offsets[f] = off;
    return f;
}

} // extern "C"
