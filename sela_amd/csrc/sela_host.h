// sela_host.h -- every host function of libsela_hip.so that one translation unit defines and another calls, declared once.
// Included by the file that defines a function and by every file that calls it, so a changed parameter is a compile error;
// default arguments appear here and nowhere else.  (The any-length route's launches and records: sela_generic.h, included.)
#ifndef SELA_HOST_H_
#define SELA_HOST_H_

#include <string>

#include "sela_device.h"
#include "sela_generic.h"

namespace sela {

// ---- sela_encode.hip -----------------------------------------------------------------------------------------------------------
// (every *_workspace_bytes: the call's one description of its workspace, measured -- `at` as in sela_generic.h)
size_t encode_workspace_bytes(uint32_t n_frames, uint32_t channels, Carve* at = nullptr);
const BlockMeta* encode_block_records(const void* d_workspace, uint32_t n_frames, uint32_t channels); // what opens a launch's workspace (device)
int encode_team_lanes(uint32_t n_frames, uint32_t channels, int forced);
uint32_t encode_split_frames(uint32_t n_frames, uint32_t channels, int permille);
void set_keep_both_candidates(int on);
void set_encode_hashes(int on);
hipError_t launch_encode(const int16_t* d_pcm, uint32_t n_frames, uint32_t channels, uint8_t* d_frames, size_t frames_cap,
    uint64_t* d_frame_offsets, uint32_t* d_status, void* d_workspace, sela_hip_trace* d_trace, hipStream_t stream,
    hipEvent_t* ev, uint64_t* d_phase_cycles, const EncodeHostLink* link, int force_plain_fir, int self_blocks_override, int team_lanes,
    int32_t* d_trace_residues = nullptr, uint32_t priorities = 0, int phase = 0, const uint64_t* plan_base = nullptr, bool plan_accumulate = false,
    bool lossless = false);
hipError_t launch_stage_rice_encode(const int32_t* d_values, const uint64_t* d_value_offsets, uint32_t n_streams, uint32_t* d_k, uint32_t* d_word_counts,
    uint32_t* d_words, const uint64_t* d_word_offsets, uint32_t* d_status, hipStream_t stream);

// ---- sela_decode.hip, sela_index.inc (decode_waves: sela_device.h) ----------------------------------------------------------------
int32_t* carve_decode(Carve& c, uint32_t n_frames, uint32_t channels); // launch_decode's and launch_verify_frames' one piece
size_t decode_workspace_bytes(uint32_t n_frames, uint32_t channels, Carve* at = nullptr);
uint32_t decode_max_channels();
hipError_t launch_decode(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames, uint32_t channels,
    int16_t* d_pcm_out, uint32_t* d_status, void* d_workspace, hipStream_t stream, hipEvent_t* ev, uint64_t* d_phase_cycles,
    uint8_t* frame_flags, int recurrence_form, uint32_t synth_priorities = 0, const uint32_t* d_n_found = nullptr, bool zero_status = true);
hipError_t launch_stage_lpc_decode(const int32_t* d_order, const int32_t* d_q, const int32_t* d_residues, uint32_t n_blocks, int32_t* d_samples,
    int64_t* d_coefs, uint32_t* d_status, hipStream_t stream);
hipError_t launch_stage_rice_decode(const uint32_t* d_words, const uint64_t* d_word_offsets, const uint32_t* d_k, const uint64_t* d_value_offsets,
    uint32_t n_streams, int32_t* d_values, uint32_t* d_status, hipStream_t stream);
size_t index_workspace_bytes(uint64_t payload_bytes, Carve* at = nullptr);
hipError_t launch_index(const uint8_t* d_payload, uint64_t payload_bytes, uint32_t max_frames, uint32_t channels, uint64_t* d_frame_offsets,
    uint32_t* d_n_frames, void* d_workspace, hipStream_t stream);
// What sela_salvage.hip shares with the index (sela_index.inc): its "none", the shape of its candidates kernel, its workspace,
// and its first three launches.
constexpr uint32_t kIndexNone = 0xFFFFFFFFu;
constexpr int kIndexThreads = 256;
constexpr int kIndexWordsPerThread = 16;
constexpr uint32_t kIndexChunkWords = (uint32_t)kIndexThreads * kIndexWordsPerThread; // words one candidates workgroup covers
struct IndexWs {
    uint32_t* stage_pos;  // [words] per workgroup, then jump array A
    uint32_t* stage_next; // [words] per workgroup, then jump array B
    uint32_t* pos;        // [n_cand] word index of candidate i (increasing)
    uint32_t* next;       // [n_cand] word index of the end of candidate i's frame (<= words)
    uint32_t* rank;       // [n_cand] frame index of a reached candidate, kIndexNone otherwise
    uint32_t* map;        // [words]  map[pos[i]] = i
    uint32_t* counts;     // [blocks + 1] candidates per workgroup, then their exclusive scan
    uint32_t* n_cand;     // [1]
};
// The workspace (sela_workspace.h), for a payload of `words` 32-bit words (every word may be a candidate): six arrays of one
// uint32 per word, the scan's counts and the candidate count.
inline IndexWs carve_index(Carve& c, uint64_t words)
{
    const uint64_t blocks = (words + kIndexChunkWords - 1) / kIndexChunkWords;
    IndexWs ws;
    ws.stage_pos = c.take<uint32_t>(words);
    ws.stage_next = c.take<uint32_t>(words);
    ws.pos = c.take<uint32_t>(words);
    ws.next = c.take<uint32_t>(words);
    ws.rank = c.take<uint32_t>(words);
    ws.map = c.take<uint32_t>(words);
    ws.counts = c.take<uint32_t>(blocks + 1);
    ws.n_cand = c.take<uint32_t>(1);
    return ws;
}
// k_index_candidates, k_index_scan and k_index_compact alone (words > 0): pos[], next[], map[] and *n_cand of `ws` filled.
// k_index_scan also sets the outputs it is given to "no frame found": d_frame_offsets[0] = 0, *d_n_frames = 0.
hipError_t launch_index_candidates(const uint8_t* d_payload, uint64_t payload_bytes, uint32_t channels, const IndexWs& ws, uint64_t* d_frame_offsets,
    uint32_t* d_n_frames, hipStream_t stream);
// k_index_scan alone: counts[0 .. blocks) of `ws` -> their exclusive scan, counts[blocks] = *n_cand = the total; the outputs as above.
hipError_t launch_index_scan(const IndexWs& ws, uint32_t blocks, uint64_t* d_frame_offsets, uint32_t* d_n_frames, hipStream_t stream);

// ---- sela_salvage.hip: the frames of a damaged payload -----------------------------------------------------------
size_t salvage_workspace_bytes(uint64_t payload_bytes, uint32_t max_frames, Carve* at = nullptr);
// d_out null: the walk alone (d_frame_offsets may then be null too); d_records may be null.  The caller has checked the arguments.
hipError_t launch_salvage(const uint8_t* d_payload, uint64_t payload_bytes, uint32_t max_frames, uint32_t channels, sela_hip_salvaged* d_records,
    uint64_t* d_totals, uint8_t* d_out, uint64_t out_cap, uint64_t* d_frame_offsets, void* d_workspace, hipStream_t stream);

// ---- sela_salvage_unaligned.hip: the frames of a damaged payload at any byte ------------------------------------
size_t salvage_unaligned_workspace_bytes(uint64_t payload_bytes, uint32_t max_frames, Carve* at = nullptr);
// As launch_salvage; payload_bytes below 2^32.
hipError_t launch_salvage_unaligned(const uint8_t* d_payload, uint64_t payload_bytes, uint32_t max_frames, uint32_t channels, sela_hip_salvaged* d_records,
    uint64_t* d_totals, uint8_t* d_out, uint64_t out_cap, uint64_t* d_frame_offsets, void* d_workspace, hipStream_t stream);

// ---- sela_window.hip: sample windows of a stream ---------------------------------------------------------------
uint32_t window_cover(uint32_t window_samples); // the most frames a window of that length touches: the grid's second extent
size_t window_workspace_bytes(uint32_t n_windows, uint32_t window_samples, uint32_t channels, Carve* at = nullptr);
hipError_t launch_window_frames(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames_total, uint32_t channels, const sela_hip_window* d_windows,
    uint32_t n_windows, uint32_t window_samples, uint32_t format, void* d_out, uint32_t* d_window_flags, uint32_t* d_status, void* d_workspace, hipStream_t stream,
    int recurrence_form, uint32_t synth_priorities);
struct WindowWs { // launch_window_frames' pieces; launch_window_whole's workspace opens with them
    int32_t* residues;   // generic mode's, one block per (workgroup, channel)
    uint32_t* flag_words; // a word per window, for a call that passes no d_window_flags
};
WindowWs carve_windows(Carve& c, uint32_t n_windows, uint32_t window_samples, uint32_t channels);

hipError_t launch_window_clear(uint32_t* d_status, uint32_t* d_window_flags /* or null */, uint32_t n_windows, hipStream_t stream); // k_window_clear alone

// ---- sela_window32.hip: sample windows of 24- and 32-bit streams -------------------------------------------------
size_t window32_workspace_bytes(uint32_t n_windows, uint32_t window_samples, uint32_t channels, Carve* at = nullptr);
hipError_t launch_window32(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames_total, uint32_t channels, const sela_hip_window* d_windows,
    uint32_t n_windows, uint32_t window_samples, uint32_t format, uint32_t sample_bits, void* d_out, uint32_t* d_window_flags, uint32_t* d_status, void* d_workspace,
    bool standard_path /* false: every subframe by segments (sela_hip_debug_standard_first(2)) */, hipStream_t stream);
struct TailSub;
struct Window32Ws { // launch_window32's pieces; launch_window32_whole's workspace opens with them
    TailSub* subs;        // a record per (window, covering frame, subframe position) ...
    int32_t* dec;         // ... and its 2048 decoded 32-bit samples
    uint32_t* flag_words; // a word per window, for a call that passes no d_window_flags
};
Window32Ws carve_window32(Carve& c, uint32_t n_windows, uint32_t window_samples, uint32_t channels);

// ---- sela_window_whole.hip: windows that reach a whole-track stream's long last frame --------------------------
size_t window_whole_workspace_bytes(uint32_t n_windows, uint32_t window_samples, uint32_t channels, Carve* at = nullptr);
hipError_t launch_window_whole(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames_total, uint32_t channels, const sela_hip_window* d_windows,
    uint32_t n_windows, uint32_t window_samples, uint32_t format, void* d_out, uint32_t* d_window_flags, uint32_t* d_status, void* d_workspace, hipStream_t stream,
    int recurrence_form, uint32_t synth_priorities);
// k_tailwin_plan and k_tailwin_decode alone, for the window calls of other files (sela_window32_whole.hip): d_subs is TailSub
// [n_windows][channels], d_dec int32 [n_windows][channels][kTailStride]
struct WindowTail;
hipError_t launch_tailwin_plan(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames_total, const sela_hip_window* d_windows, uint32_t n_windows,
    uint32_t window_samples, sela_hip_window* d_copies, WindowTail* d_tails, hipStream_t stream);
hipError_t launch_tailwin_decode(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t channels, const WindowTail* d_tails, uint32_t n_windows, int32_t* d_dec,
    void* d_subs, hipStream_t stream);

// ---- sela_window32_whole.hip: 32-bit windows that reach a whole-track stream's long last frame ------------------
size_t window32_whole_workspace_bytes(uint32_t n_windows, uint32_t window_samples, uint32_t channels, Carve* at = nullptr);
hipError_t launch_window32_whole(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames_total, uint32_t channels, const sela_hip_window* d_windows,
    uint32_t n_windows, uint32_t window_samples, uint32_t format, uint32_t sample_bits, void* d_out, uint32_t* d_window_flags, uint32_t* d_status, void* d_workspace,
    bool standard_path, hipStream_t stream);

// ---- sela_window_whole.hip: a full decode of a whole-track stream ------------------------------------------------
struct WindowTail;
struct DecodeWholeWs { // the workspace of sela_hip_decode_whole_device
    void* fast_workspace;   // launch_decode's (decode_workspace_bytes)
    WindowTail* tail;       // the long last frame as k_tailwin_decode is told of it, or an empty record
    uint32_t* fast_frames;  // launch_decode's count of frames
    void* subs;             // a record per subframe of the last frame ...
    int32_t* dec;           // ... and its 4096 decoded 32-bit samples
};
DecodeWholeWs carve_decode_whole(Carve& c, uint32_t max_frames, uint32_t channels);
size_t decode_whole_workspace_bytes(uint32_t max_frames, uint32_t channels, Carve* at = nullptr);
hipError_t launch_decode_whole_plan(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t max_frames, const uint32_t* d_n_found, uint64_t pcm_capacity,
    const DecodeWholeWs& w, uint64_t* d_n_samples, uint32_t* d_status, hipStream_t stream);
hipError_t launch_decode_whole_tail(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t channels, const DecodeWholeWs& w, int16_t* d_pcm_out,
    uint32_t* d_status, hipStream_t stream);

// ---- sela_whole.hip: a whole track with its tail ---------------------------------------------------------------
struct WholeLastWs { // the end of both whole-track encoders' workspaces: the last frame as coded, for the splice
    uint8_t* frame;    // its bytes, and their room
    size_t cap;
    uint64_t* offsets; // its two offsets ...
    uint32_t* status;  // ... and its four status words
};
struct WholeWs { // the workspace of sela_hip_encode_whole_device
    void* main_workspace;   // the 2048-sample frames' workspace (encode_workspace_bytes), and its bytes
    void* last_workspace;   // the last frame's any-length workspace (encode_i32_device_workspace_bytes), and its bytes
    size_t main_bytes, last_bytes;
    WholeLastWs last;
};
WholeWs carve_whole(Carve& c, uint64_t max_samples, uint32_t channels); // (arguments that whole_workspace_bytes does not refuse)
size_t whole_workspace_bytes(uint64_t max_samples, uint32_t channels, Carve* at = nullptr); // SIZE_MAX for what the call refuses
struct WholePcmWs { // the workspace of sela_hip_encode_whole_pcm_device
    int32_t* main_samples;  // the 2048-sample frames unpacked, and sela_hip_encode_i32_device's workspace for them
    void* main_workspace;
    int32_t* last_samples;  // the last frame unpacked, and its any-length workspace
    void* last_workspace;
    WholeLastWs last;
};
WholePcmWs carve_whole_pcm(Carve& c, uint64_t max_samples, uint32_t channels); // (arguments that whole_pcm_workspace_bytes does not refuse)
size_t whole_pcm_workspace_bytes(uint64_t max_samples, uint32_t channels, Carve* at = nullptr); // SIZE_MAX for what the call refuses
hipError_t launch_whole_splice(const WholeLastWs& coded, uint32_t channels, uint8_t* d_frames, uint64_t frames_cap, uint64_t* d_frame_offsets, uint32_t last,
    uint32_t* d_status, hipStream_t stream);

// ---- sela_capi.hip: what the any-length route's host side shares with the boundary --------------------------------------------
int report_error(int code, const std::string& what);   // sets the thread's last error, returns code
int report_hip_error(hipError_t e, const char* where); // (ENOMEM for an allocation failure, ENODEV otherwise)
int device_ready();                                    // SELA_HIP_OK, or ENODEV reported: there is no CPU fallback
inline bool frame_offsets_ascend(const uint64_t* frame_offsets, uint32_t n_frames)
{
    for (uint32_t f = 0; f < n_frames; f++)
        if (frame_offsets[f + 1] < frame_offsets[f])
            return false;
    return true;
}
int check_frame_offsets(const uint64_t* frame_offsets, uint32_t n_frames); // SELA_HIP_OK, or EFORMAT reported: "frame offsets must not decrease"
struct CurrentDevice { // how a leased context (sela_lease.h) asks for the calling thread's device
    static int current_device()
    {
        int dev = -1;
        return hipGetDevice(&dev) == hipSuccess ? dev : -1;
    }
    static void set_device(int dev) { (void)hipSetDevice(dev); }
};

// The verdicts on what the kernels report: ONE policy per direction, an ordered table of (flag, code, text) each.  A call
// names the conditions it judges (`judged`) and opens the texts that name their caller (`who`: "decode", "lpc_decode",
// "encode", "lpc_encode"); the first row that is set and judged is reported, else SELA_HIP_OK.
enum DecodeRoute { // whose frames they were: a malformed one reads differently by the route that met it
    kRouteDevice32, // sela_hip_decode_i32_device, the any-length route of sela_hip_decode_n_device (status[3] == 2)
    kRouteHost32,   // generic_decode: decreasing offsets were refused before the device saw them
    kRouteFast,     // the 2048-sample kernels: the streaming jobs, status[3] == 1
    kRouteWalk,     // sela_hip_decode_n_device when the header walk broke (status[3] == 0)
    kRouteLpc,      // the LPC stage on its own: blocks, and an order that is an argument (EINVAL)
};
constexpr uint32_t kJudgeJob = SELA_HIP_FLAG_BAD_FRAME | SELA_HIP_FLAG_RICE_OVERRUN | SELA_HIP_FLAG_COEF_OVERFLOW | SELA_HIP_FLAG_Q_RANGE; // the jobs' verdict: not SHORT_BLOCK, not INTERNAL
constexpr uint32_t kJudgeLpc = SELA_HIP_FLAG_BAD_FRAME | SELA_HIP_FLAG_COEF_OVERFLOW | SELA_HIP_FLAG_Q_RANGE;
constexpr uint32_t kJudgeEncode = SELA_HIP_FLAG_SHORT_BLOCK | SELA_HIP_FLAG_RICE_RANGE | SELA_HIP_FLAG_COEF_OVERFLOW | SELA_HIP_FLAG_WORDS_CAP;
int judge_decode(uint32_t flags, uint32_t judged, DecodeRoute route, const char* who);
int judge_encode(uint32_t flags, uint32_t judged, const char* who);

// ---- sela_capi_generic.hip: the any-length / 32-bit route on host pointers ---------------------------------------------------
void generic_release();
void generic_shutdown();
int generic_standard_first_mode();
size_t generic_encode_bound_bytes(uint32_t n_frames, uint32_t channels, uint32_t n);
int generic_encode(const void* input, bool in16, uint32_t n_frames, uint32_t channels, uint32_t n, uint8_t* frames_out, size_t frames_cap, uint64_t* frame_offsets_out,
    bool lossless = false, bool paired = false);
uint32_t generic_index_samples(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, uint64_t* sample_offsets, bool* all_standard);
int generic_decode(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, int32_t* samples_out, uint32_t stride,
    uint32_t* counts_out, int16_t* pcm_out, const uint64_t* sample_offsets);
int generic_verify(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, const int16_t* pcm, uint32_t* diff_counts,
    uint32_t* first_diff, uint32_t* lossy_frames, int recurrence_form);
int generic_verify_i32(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride, const int32_t* samples,
    const uint32_t* lengths, uint32_t* diff_counts, uint32_t* first_diff, uint32_t* lossy_frames);
// sela_hip_levels: generic_verify's walk and chunks, the records coming back where its two arrays do
int generic_levels(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, sela_hip_level* levels, int recurrence_form);
// sela_hip_envelope: generic_levels' walk and chunks at the caller's stride, ceil(stride / bucket) * channels records a frame
int generic_envelope(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride, uint32_t bucket,
    struct sela_hip_envelope* env, int recurrence_form);
// sela_hip_digest: generic_levels' walk and chunks, the chunks' track words folded on the host (any of the three outputs may be null)
int generic_digest(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, struct sela_hip_digest* digests, uint32_t* track_crc32,
    uint64_t* track_bytes, int recurrence_form);
int generic_levels_i32(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride, sela_hip_level32* levels);
// sela_hip_envelope_i32: generic_levels_i32's chunks at the caller's stride, ceil(stride / bucket) * channels records a frame
int generic_envelope_i32(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride, uint32_t bucket,
    struct sela_hip_envelope32* env);
// sela_hip_digest_pcm: generic_levels_i32's chunks, the chunks' track words and wide-sample counts folded on the host (any output may be null)
int generic_digest_pcm(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride, uint32_t bytes_per_sample,
    struct sela_hip_digest* digests, uint32_t* track_crc32, uint64_t* track_bytes, uint32_t* wide_samples);
// sela_hip_verify_pcm: the stride is the stream's largest samplesPerChannel (the host's walk); each chunk's packed bytes are staged
// from the chunk's first frame, so the device's base is aligned and the chunk's own sample offsets start at 0.
int generic_verify_pcm(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t bytes_per_sample, const uint8_t* pcm,
    uint64_t pcm_samples, uint32_t* diff_counts, uint32_t* first_diff, uint32_t* lossy_frames);
int generic_decode_windows(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames_total, uint32_t channels, const sela_hip_window* windows,
    uint32_t n_windows, uint32_t window_samples, uint32_t format, void* out, uint32_t* window_flags, int recurrence_form,
    bool whole = false /* plan_windows_whole and launch_window_whole */,
    bool wide = false /* launch_window32 and its formats */, uint32_t sample_bits = 0);
void windows_staged_bytes_reset(); // sela_hip_debug_windows_staged_bytes of the calling thread back to 0: the entry point's first act
int generic_lpc_encode(const int32_t* samples, uint32_t n_blocks, uint32_t n, int32_t* order_out, int32_t* q_out, int32_t* residues_out);
int generic_lpc_decode(const int32_t* order, const int32_t* q, const int32_t* residues, uint32_t n_blocks, uint32_t n, int32_t* samples_out, int64_t* coefs_out);

} // namespace sela
#endif
