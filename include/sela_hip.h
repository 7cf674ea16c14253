/*
 * sela_hip.h -- C ABI of the MI355X-native SELA frame encode/decode path (libsela_hip.so).
 *
 * This is the drop-in boundary for the hot path.  The reference (sahaRatul/sela v2.0.2) has no
 * FFI of its own; the work these entry points replace is the worker fan-out plus everything
 * below it:
 *
 *   sela_hip_encode*  replaces  sela::Encoder::processFrames        src/sela/encoder.cpp:40-92
 *                     i.e. per frame frame::FrameEncoder::process   src/frame/frame_encoder.cpp:11-102
 *                          -> lpc::ResidueGenerator::process        src/lpc/residue_generator.cpp:121-134
 *                          -> rice::RiceEncoder::process            src/rice/rice_encoder.cpp:73-81
 *                     and the per-frame serialisation of            src/file/sela_file.cpp:115-135
 *   sela_hip_decode*  replaces  sela::Decoder::processFrames        src/sela/decoder.cpp:41-92
 *                     i.e. per frame frame::FrameDecoder::process   src/frame/frame_decoder.cpp:11-72
 *                          -> rice::RiceDecoder::process            src/rice/rice_decoder.cpp:54-61
 *                          -> lpc::SampleGenerator::process         src/lpc/sample_generator.cpp:32-39
 *                     and the interleave of                         src/file/wav_file.cpp:244-257
 *
 * Data formats at the boundary are the reference's own on-disk formats, so no conversion is
 * needed on either side:
 *   PCM     : interleaved little-endian int16, [n_frames][2048][channels] -- the WAV data chunk
 *             (src/file/wav_file.cpp:193-199), whole 2048-sample frames only (tail dropped by the
 *             caller exactly as src/file/wav_file.cpp:184,203 does).
 *   frames  : the byte stream that follows the 15-byte .sela file header: per frame the sync word
 *             0xAA55FF00 and `channels` subframes (src/file/sela_file.cpp:115-135), frames
 *             back to back.  frame_offsets[f] is the byte offset of frame f in that stream,
 *             frame_offsets[n_frames] its total size.  Every frame size is a multiple of 4.
 *
 * The plain encode calls write the reference's stream bit for bit -- which a few frames in ten thousand do not decode back to
 * their PCM.  The *_opt calls with SELA_HIP_ENCODE_LOSSLESS write a stream every decoder of the format reads back
 * exactly (see "encode options" below); the verify calls tell the two apart frame by frame.
 *
 * All functions return 0 on success or a negative SELA_HIP_E* code; they never throw and never
 * fall back to a CPU implementation.  sela_hip_last_error() gives a thread-local message.
 *
 * Two flavours:
 *   *_device : pointers are DEVICE pointers on the current HIP device, work is enqueued on
 *              `stream` (a hipStream_t passed as void*; NULL = the default stream) and the call
 *              returns without synchronising unless stated.  This is what bench.py times
 *              (inputs resident in HBM).
 *   host     : pointers are HOST pointers; the library stages through its own device buffers
 *              (H2D, kernels, D2H) and returns when the result is in host memory.  This is what
 *              the C++ host (host/) calls from sela::Encoder/Decoder and frame::Frame{En,De}coder.
 *              One-shot calls (whole batch in memory) and streaming jobs (begin / feed / end: the
 *              caller keeps reading its file while earlier pieces are already on the device).
 *              Buffers from sela_hip_host_alloc() are page-locked: copies from and to them are truly
 *              asynchronous; ordinary (pageable) memory works too, only slower.
 */
#ifndef SELA_HIP_H_
#define SELA_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SELA_HIP_OK 0
#define SELA_HIP_ENODEV (-1)   /* no usable HIP device / HIP runtime error (see last_error) */
#define SELA_HIP_EINVAL (-2)   /* bad argument (channels == 0, samples_per_channel == 0 or > 65535, ...) */
#define SELA_HIP_ENOMEM (-3)   /* device or host allocation failed */
#define SELA_HIP_ECAPACITY (-4) /* caller-provided output or workspace too small */
#define SELA_HIP_EFORMAT (-5)  /* malformed frame stream (bad sync word, inconsistent sizes) */
#define SELA_HIP_ERANGE (-6)   /* a block left the range the format can carry (SURVEY.md App. E "(G)") */

#define SELA_HIP_SAMPLES_PER_FRAME 2048u

/* Per-(frame, signal) analysis record, optional debug output of the encoder (FP64 intermediates
 * that the reference keeps private).  signal 0..channels-1 are the channels, signal `channels`
 * is the difference channel0-channel1 of an exactly-stereo frame. */
typedef struct sela_hip_trace {
    double mean;
    double ac[101];
    double k[100];
    int64_t a[101];
    int32_t q[100];
    int32_t order;
    uint32_t coef_k, coef_words, res_k, res_words, flags;
} sela_hip_trace;

/* ---- lifetime ------------------------------------------------------------------------------ */
/* Select/initialise `device` (>= 0) for the calling thread, or -1 to keep the current device. */
int sela_hip_init(int device);
/* The host-pointer API keeps staging buffers, streams and events per calling thread; creating them costs the runtime
 * about 10 ms.  sela_hip_thread_release() PARKS the calling thread's set for the next thread that uses the same device
 * (a thread that simply ends parks it too), so short-lived worker threads start warm.  sela_hip_shutdown() frees the
 * calling thread's set and every parked one, and returns the idle page-locked blocks to the system. */
void sela_hip_thread_release(void);
void sela_hip_shutdown(void);
const char* sela_hip_last_error(void);
int sela_hip_device_count(void);
/* Page-locked host memory for the buffers handed to the host-pointer API (PCM in, frames out, ...).
 * Freed blocks are pooled and handed out again (pinning is slow); sela_hip_shutdown() returns them to the
 * system.  Without a usable HIP device these fall back to ordinary aligned memory, so container code
 * (WAV / .sela parsing) that holds its data in such buffers still runs on a CPU-only box. */
void* sela_hip_host_alloc(size_t bytes);
void sela_hip_host_free(void* p);

/* ---- sizing ------------------------------------------------------------------------------------ */
/* Number of signals analysed per frame: channels, +1 for exactly-stereo input. */
uint32_t sela_hip_signals_per_frame(uint32_t channels);
/* Bytes of device workspace the *_device calls need for a batch of n_frames.  The workspace needs no
 * initialisation and may be reused by later calls; one call at a time may use it. */
size_t sela_hip_encode_workspace_bytes(uint32_t n_frames, uint32_t channels);
/* (The decoder keeps positions and samples on chip; the workspace is only written for subframes that take the
 * kernels' generic mode -- Rice streams beyond what 16-bit audio produces.) */
size_t sela_hip_decode_workspace_bytes(uint32_t n_frames, uint32_t channels);
/* Most channels the decoder takes: 255, what the 8-bit channel field of the .sela header can say (up to eight channels
 * take one wave per subframe, more take the same waves in rounds; src/frame/frame_decoder.cpp:11-72). */
uint32_t sela_hip_decode_max_channels(void);
/* Upper bound of the frame byte stream produced by encoding n_frames (what `frames_cap` must be
 * to be certain never to get SELA_HIP_ECAPACITY). */
size_t sela_hip_encode_bound_bytes(uint32_t n_frames, uint32_t channels);

/* ---- device-pointer API (asynchronous on `stream`) --------------------------------------------- */
/*
 * Encode n_frames frames.  d_pcm: int16 [n_frames][2048][channels].  Outputs: d_frames (byte stream,
 * capacity frames_cap bytes, 4-byte aligned), d_frame_offsets (uint64 [n_frames + 1]),
 * d_status (uint32[4]: [0] = OR of per-block flag bits, [1] = number of frames that did not fit
 * frames_cap, [2..3] reserved; zeroed by the call).  d_trace may be NULL.
 * Launches 3 kernels on `stream` and returns immediately.
 */
int sela_hip_encode_device(const int16_t* d_pcm, uint32_t n_frames, uint32_t channels,
    uint8_t* d_frames, size_t frames_cap, uint64_t* d_frame_offsets, uint32_t* d_status,
    void* d_workspace, size_t workspace_bytes, sela_hip_trace* d_trace, void* stream);

/*
 * Decode n_frames frames.  d_frames / d_frame_offsets as produced above (or by parsing a .sela
 * file).  d_pcm_out: int16 [n_frames][2048][channels].  d_status: uint32[4], [0] = OR of flag
 * bits, [1] = number of malformed frames (zeroed by the call).  channels <= sela_hip_decode_max_channels().
 * One kernel on `stream` (one workgroup per frame, one wave per subframe); d_workspace as sized by
 * sela_hip_decode_workspace_bytes().  Returns immediately.
 */
int sela_hip_decode_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames,
    uint32_t channels, int16_t* d_pcm_out, uint32_t* d_status, void* d_workspace, size_t workspace_bytes,
    void* stream);

/*
 * Find the frames of a payload -- the byte stream that follows the 15-byte .sela file header -- on the device: the
 * device-side sela_hip_index_frames().  d_frame_offsets (uint64 [max_frames + 1]) and *d_n_frames (uint32) receive exactly
 * what sela_hip_index_frames(payload, payload_bytes, max_frames, channels, ...) returns for the same bytes, for every input:
 * entries [0 .. *d_n_frames], the last of them where the walk stopped (a bad sync word, a header or stream running past
 * payload_bytes, or the max_frames cap); entries beyond are not written.  d_payload must be 4-byte aligned.
 * Asynchronous on `stream`, no allocation, no host synchronisation (a stream being captured into a graph may take it):
 * 4 kernel launches up to max_frames = 4096, 5 + ceil(log2(max_frames)) above.
 * d_workspace: sela_hip_index_workspace_bytes(payload_bytes, max_frames) bytes, no initialisation: 6 bytes per payload
 * byte (six uint32 per 4-byte word: every word may start a frame), 1 byte per 4 KiB and at most 2.5 KiB more; the same for
 * every max_frames.
 * SELA_HIP_EINVAL: channels outside 1..255, a null pointer, a misaligned d_payload, a payload of 16 GiB or more;
 * SELA_HIP_ECAPACITY: a smaller workspace.
 */
size_t sela_hip_index_workspace_bytes(size_t payload_bytes, uint32_t max_frames);
int sela_hip_index_frames_device(const uint8_t* d_payload, size_t payload_bytes, uint32_t max_frames, uint32_t channels,
    uint64_t* d_frame_offsets /* [max_frames + 1] */, uint32_t* d_n_frames /* [1] */, void* d_workspace, size_t workspace_bytes,
    void* stream);
/*
 * sela_hip_index_frames_device() and then sela_hip_decode_device() on the frames it found, on one stream: the frame count
 * never leaves the device.  d_pcm_out: int16 [max_frames][2048][channels], frames from *d_n_frames on are not decoded and
 * their PCM is not written.  d_status as sela_hip_decode_device()'s (frames that do not say 2048 samples are
 * SELA_HIP_FLAG_BAD_FRAME there too).  d_workspace: sela_hip_index_workspace_bytes(payload_bytes, max_frames) +
 * sela_hip_decode_workspace_bytes(max_frames, channels) bytes.  channels <= sela_hip_decode_max_channels(); errors as the
 * two calls'.  Returns immediately.
 */
int sela_hip_decode_payload_device(const uint8_t* d_payload, size_t payload_bytes, uint32_t max_frames, uint32_t channels,
    int16_t* d_pcm_out, uint64_t* d_frame_offsets, uint32_t* d_n_frames, uint32_t* d_status, void* d_workspace,
    size_t workspace_bytes, void* stream);

/* ---- host-pointer API (synchronous) -------------------------------------------------------------- */
/* frames_out must hold sela_hip_encode_bound_bytes() or the call may return SELA_HIP_ECAPACITY.
 * These are begin + feed(everything) + end of the streaming jobs below, on library-owned streams: an encode is ONE
 * kernel launch per feed (it fetches the PCM from page-locked memory itself and stores the finished frames into
 * frames_out), a decode a pipeline of 1024-frame chunks (copy in / kernel / copy out overlapped).  Results are
 * identical to one device-pointer call on the whole batch.
 * Calls of at most 32 frames made from several threads at once -- a binding that keeps the reference's per-frame thread
 * loop (src/sela/encoder.cpp:58-73) -- are coalesced: calls that arrive while another one is on the device go there
 * together, as one job, when it returns.  Every call still gets exactly its own result and its own error (a buffer that
 * is too small, a malformed frame, a coefficient outside the tables); a lone caller is not delayed.  The same holds for
 * sela_hip_encode_i32 / sela_hip_decode_i32 below. */
int sela_hip_encode(const int16_t* pcm, uint32_t n_frames, uint32_t channels, uint32_t samples_per_channel,
    uint8_t* frames_out, size_t frames_cap, uint64_t* frame_offsets_out /* [n_frames+1] */);
int sela_hip_decode(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels,
    int16_t* pcm_out);
/* Blocks of any length.  The reference's frame path does not know the number 2048: lpc::ResidueGenerator loops over
 * samples.size() (src/lpc/residue_generator.cpp:12-45,98-119) and a subframe carries its own samplesPerChannel, a u16
 * (src/include/data/sela_sub_frame.hpp:27, src/frame/frame_decoder.cpp:24-25,48-49); only its WAV reader cuts 2048-sample
 * frames.  So:
 *   sela_hip_encode() takes any samples_per_channel in 1 .. 65535 (pcm = [n_frames][samples_per_channel][channels]); other
 *     than 2048 goes through the any-length kernels (sela_generic.hip: the same arithmetic with a run-time length, one wave
 *     per block).  frames_out needs sela_hip_encode_bound_bytes_n().  A block that is not longer than the
 *     predictor order its own analysis picks makes the reference read past its vector (residue_generator.cpp:104-110):
 *     SELA_HIP_ERANGE.
 *   sela_hip_decode() takes a stream whose frames say anything in 0 .. 65535: when one says something other than 2048 the
 *     whole call goes through the any-length kernels, frame f's samples land at pcm_out + sample_offsets[f] * channels with
 *     sample_offsets[] as sela_hip_index_samples() reports them (for 2048 everywhere that is f * 2048, the layout above), and
 *     a frame whose channels disagree about the length is malformed (SELA_HIP_EFORMAT; the reference's WAV writer indexes
 *     past the shorter ones, src/file/wav_file.cpp:248-262).  The fast kernels are tried first, unasked (a stream of
 *     2048-sample frames pays nothing for the other kind) -- unless the stream's FIRST frame already says another length --
 *     and they may write up to [n_frames][2048][channels] before they find an odd frame further on: pcm_out must hold
 *     max(n_frames * 2048, sample_offsets[n_frames]) * channels samples.
 * The streaming jobs and the 2048-sample int16 device-pointer calls (sela_hip_decode_device, sela_hip_decode_payload_device)
 * stay what they are: the fast path for what the reference's CLI writes (2048 everywhere); a stream with another length gets
 * SELA_HIP_EFORMAT from them, and the caller comes here -- or, with the stream in device memory, to sela_hip_decode_n_device
 * (this call's output on device pointers) or sela_hip_decode_i32_device below. */
size_t sela_hip_encode_bound_bytes_n(uint32_t n_frames, uint32_t channels, uint32_t samples_per_channel);
/* sample_offsets[f] = samples per channel before frame f (its first subframe's samplesPerChannel counts for the frame),
 * [n_frames + 1] entries; returns the largest samplesPerChannel any subframe of the stream names (0 for a stream the walk
 * cannot follow: the decode calls report that as SELA_HIP_EFORMAT). */
uint32_t sela_hip_index_samples(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels,
    uint64_t* sample_offsets);

/* ---- the frame classes' own value types: 32-bit samples, any length ---------------------------------------------------------
 * frame::FrameEncoder(const data::WavFrame&).process() and frame::FrameDecoder(const data::SelaFrame&).process()
 * (src/include/frame.hpp:8-24) on what they really take and return: data::WavFrame = int32 samples per channel
 * (src/include/data/wav_frame.hpp:8-16), nothing narrowed (src/frame/frame_decoder.cpp:64-71; only file::WavFile::writeToFile
 * truncates to 16 bits).  The encoder always runs the any-length kernels (sela_generic.hip: the fast kernels' loops with a
 * run-time length); the decoder runs the fast decoder's lane-parallel parse and tuned synthesis with 32-bit samples and a
 * run-time length (k_decode_subframes32: one piece for subframes of at most 2048 samples that fit the parser's plan, segments for
 * everything else) and leaves to a serial kernel only the streams it will not judge (frames that are not whole words, malformed
 * headers, Rice streams that run dry, coefficients outside the tables).  Results identical to the calls above wherever both apply.
 *   samples      [n_frames][channels][samples_per_channel] (planar per frame: WavFrame.samples[c][i]), 1 .. 65535 per channel.
 *   samples_out  [n_frames][channels][stride]: channel c of frame f at ((f * channels) + c) * stride, counts_out[f * channels + c]
 *                of them valid (0 for a channel no subframe of the frame names; what lies behind a channel's count is not
 *                defined); stride >= the largest samplesPerChannel in the stream (sela_hip_index_samples() returns it) or
 *                SELA_HIP_ECAPACITY.  The calls run on a stream of the calling thread's own (leased, not the default stream)
 *                and return when the result is in host memory; after an error the outputs' contents are not defined.
 * Errors as above; values whose int32 zig-zag overflows in the reference (|residue| >= 2^30) and Rice streams beyond the u16
 * word count of a subframe are SELA_HIP_ERANGE.
 * These calls, sela_hip_encode_ragged_i32 and the any-length route of sela_hip_encode / sela_hip_decode also work while the
 * calling thread has a streaming job open (below) and leave that job alone; the one-shot calls on 2048-sample frames refuse
 * with SELA_HIP_EINVAL then. */
int sela_hip_encode_i32(const int32_t* samples, uint32_t n_frames, uint32_t channels, uint32_t samples_per_channel,
    uint8_t* frames_out, size_t frames_cap, uint64_t* frame_offsets_out /* [n_frames+1] */);
int sela_hip_decode_i32(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels,
    int32_t* samples_out, uint32_t stride, uint32_t* counts_out /* [n_frames * channels] */);
/* ONE frame whose channels differ in length, as frame::FrameEncoder::process codes it (src/frame/frame_encoder.cpp:11-102):
 * every channel is analysed at its own samples[i].size() (:73-98) and its subframe carries that as samplesPerChannel
 * (src/include/data/sela_sub_frame.hpp:41); the second channel of an exactly-stereo frame is also tried as the difference
 * channel 0 - channel 1 over ITS OWN length (:20-24), so channel 0 must be at least as long -- where it is shorter the
 * reference indexes past its vector, and this call returns SELA_HIP_EINVAL.  The decoder has always taken such frames
 * (sela_hip_decode_i32).
 *   samples      the channels back to back: lengths[0] samples of channel 0, then lengths[1] of channel 1, ...
 *   lengths      [channels], each 1 .. 65535
 *   frame_out    the frame's bytes (sync word + subframes); 4 + the sum over the channels of
 *                sela_hip_encode_bound_bytes_n(1, 1, lengths[c]) holds any frame of samples within 17 bits (SELA_HIP_ECAPACITY
 *                when a frame does not fit); *frame_bytes receives the size.
 * Errors as sela_hip_encode_i32. */
int sela_hip_encode_ragged_i32(const int32_t* samples, const uint32_t* lengths, uint32_t channels, uint8_t* frame_out, size_t frame_cap,
    size_t* frame_bytes);
/* sela_hip_decode_i32 on DEVICE pointers -- the whole domain the reference decodes (any samplesPerChannel in 0 .. 65535, 32-bit
 * samples, channels of different lengths), asynchronous on `stream`: no allocation, no host synchronisation, no host-side read of
 * device data, so a stream being captured into a HIP graph may take either call.
 *   d_samples_out [n_frames][channels][stride] and d_counts_out [n_frames * channels]: exactly the layouts of sela_hip_decode_i32;
 *                 what lies behind a channel's count is not defined.
 *   d_sample_offsets [n_frames + 1] (or NULL): what sela_hip_index_samples() returns for the same frames (for decreasing
 *                 offsets, where that function writes none, their contents are not defined).
 *   d_status uint32[4], written by the call (needs no initialisation):
 *     [0] the OR of the flag bits, [1] the number of malformed frames,
 *     [2] the largest samplesPerChannel any subframe names, or 0 where sela_hip_index_samples() returns 0 (a caller whose
 *         stride was too small can resize from it without walking the stream on the host),
 *     [3] reserved, zeroed.
 *   SELA_HIP_FLAG_STRIDE is set exactly where sela_hip_decode_i32 returns SELA_HIP_ECAPACITY: the offsets never decrease, the
 *     whole header walk succeeds and [2] > stride.  Decreasing frame offsets are malformed frames here.
 *   sela_hip_decode_status_error() turns a host copy of the status words into the code sela_hip_decode_i32 returns for the same
 *     input (for a stream the host call decodes in one chunk of frames -- its chunks hold 768 MiB of device scratch -- since that
 *     call stops at the first chunk in trouble).
 * d_frames: 4-byte aligned, holding every frame the offsets name.  d_workspace: sela_hip_decode_i32_workspace_bytes(n_frames,
 * channels, stride) bytes, no initialisation (the payload call: sela_hip_index_workspace_bytes(payload_bytes, max_frames) more);
 * one call at a time may use it.  channels * n_frames below 2^31.
 * sela_hip_debug_standard_first (include/sela_hip_debug.h) routes these calls as it routes the host call (0: the serial kernel
 * alone, 2: every subframe by segments).
 * SELA_HIP_EINVAL: a null pointer (d_sample_offsets may be NULL), channels outside 1..255, stride 0, a misaligned d_frames /
 * d_payload; SELA_HIP_ECAPACITY: a smaller workspace. */
size_t sela_hip_decode_i32_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride);
int sela_hip_decode_i32_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames, uint32_t channels,
    uint32_t stride, int32_t* d_samples_out /* [n_frames][channels][stride] */, uint32_t* d_counts_out /* [n_frames * channels] */,
    uint64_t* d_sample_offsets /* [n_frames + 1] or NULL */, uint32_t* d_status /* [4] */, void* d_workspace, size_t workspace_bytes,
    void* stream);
/* sela_hip_index_frames_device() and then the call above on the frames it found, on one stream: the count never leaves the device.
 * Frames from *d_n_frames on are not decoded: their samples and counts are not written; d_sample_offsets[0 .. *d_n_frames] is. */
int sela_hip_decode_payload_i32_device(const uint8_t* d_payload, size_t payload_bytes, uint32_t max_frames, uint32_t channels,
    uint32_t stride, int32_t* d_samples_out, uint32_t* d_counts_out, uint64_t* d_sample_offsets, uint64_t* d_frame_offsets,
    uint32_t* d_n_frames, uint32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream);
/* Host only, no GPU: the code sela_hip_decode_i32 returns for the input whose device status words (a host copy) these are,
 * in the host call's order -- SELA_HIP_FLAG_STRIDE: SELA_HIP_ECAPACITY; a malformed frame (decreasing offsets among them) or a
 * Rice stream that runs dry: SELA_HIP_EFORMAT; a coefficient beyond int64 or outside the tables, a subframe not longer than its
 * order: SELA_HIP_ERANGE; SELA_HIP_FLAG_INTERNAL: SELA_HIP_ENODEV; else 0.  A null pointer: SELA_HIP_EINVAL. */
int sela_hip_decode_status_error(const uint32_t* status /* [4], host copy */);
/* sela_hip_encode_i32 -- and sela_hip_encode of any samples_per_channel -- on DEVICE pointers, asynchronous on `stream`: no
 * allocation, no host synchronisation, no host-side read of device data, so a stream being captured into a HIP graph may take
 * either call.  Neither touches the calling thread's scratch or an open streaming job.
 *   d_samples int32 [n_frames][channels][samples_per_channel] (planar, as sela_hip_encode_i32), 4-byte aligned;
 *   d_pcm int16 [n_frames][samples_per_channel][channels] (interleaved, as sela_hip_encode), 2-byte aligned.
 *   samples_per_channel: 1 .. 65535 (2048 included).
 *   d_frames (4-byte aligned) receives exactly the bytes of the host call on the same input, d_frame_offsets[0 .. n_frames] its
 *     offsets -- always written in full, also when frames do not fit: a caller whose buffer was too small resizes from
 *     d_frame_offsets[n_frames].  A frame that ends beyond frames_cap is not written; nothing at or past frames_cap is.
 *   d_status uint32[4], written by the call (needs no initialisation): [0] the OR of the flag bits (both stereo candidates'),
 *     [1] the number of frames not written for capacity, [2] and [3] zero.
 * d_workspace: sela_hip_encode_i32_workspace_bytes(n_frames, channels, samples_per_channel) bytes (it does not depend on the
 * data), no initialisation; one call at a time may use it.  sela_hip_debug_generic_wrap_taps applies as to the host call.
 * n_frames = 0 writes d_frame_offsets[0] = 0 and zero status words.
 * SELA_HIP_EINVAL: a null pointer, channels outside 1..255, samples_per_channel outside 1..65535, n_frames x signals per frame
 * at 2^31 or more, a misaligned d_frames or input; SELA_HIP_ECAPACITY: a smaller workspace.  Nothing is enqueued then. */
size_t sela_hip_encode_i32_workspace_bytes(uint32_t n_frames, uint32_t channels, uint32_t samples_per_channel);
int sela_hip_encode_i32_device(const int32_t* d_samples, uint32_t n_frames, uint32_t channels, uint32_t samples_per_channel,
    uint8_t* d_frames, size_t frames_cap, uint64_t* d_frame_offsets /* [n_frames + 1] */, uint32_t* d_status /* [4] */,
    void* d_workspace, size_t workspace_bytes, void* stream);
int sela_hip_encode_n_device(const int16_t* d_pcm, uint32_t n_frames, uint32_t channels, uint32_t samples_per_channel,
    uint8_t* d_frames, size_t frames_cap, uint64_t* d_frame_offsets /* [n_frames + 1] */, uint32_t* d_status /* [4] */,
    void* d_workspace, size_t workspace_bytes, void* stream);
/* Host only, no GPU: the code the host call returns for the input whose device status words (a host copy) these are, in its
 * order -- SELA_HIP_FLAG_SHORT_BLOCK, _RICE_RANGE, _COEF_OVERFLOW or _WORDS_CAP: SELA_HIP_ERANGE; then [1] > 0:
 * SELA_HIP_ECAPACITY; else 0 (SELA_HIP_FLAG_Q_RANGE alone included).  A null pointer: SELA_HIP_EINVAL. */
int sela_hip_encode_status_error(const uint32_t* status /* [4], host copy */);

/* sela_hip_decode on DEVICE pointers -- any samplesPerChannel in 0 .. 65535, samples wider than 16 bits narrowed as that call
 * narrows them -- asynchronous on `stream`: no allocation, no host synchronisation, no host-side read of device data, so a
 * stream being captured into a HIP graph may take either call.  Neither touches the calling thread's scratch, its open streaming
 * job or the coalescer.  The route the host call takes is taken on the device, before anything is decoded: the 2048-sample
 * decoder (k_decode_frames / _wide) where every subframe says 2048, the header walk is whole and stride >= 2048; else the
 * any-length kernels where the walk gives a largest samplesPerChannel that fits stride and the offsets never decrease; else none.
 *   d_pcm_out int16, room for n_frames * stride * channels samples: where sela_hip_decode on the same frames returns 0, exactly
 *                 the bytes it writes (frame f at d_pcm_out + sample_offsets[f] * channels).  Nothing at or past
 *                 n_frames * stride * channels is written, on any input; on success nothing at or past
 *                 sample_offsets[n_frames] * channels either.
 *   d_sample_offsets [n_frames + 1] (or NULL): what sela_hip_index_samples() returns for the same frames (for decreasing
 *                 offsets their contents are not defined).
 *   d_status uint32[4], written by the call (needs no initialisation):
 *     [0] the OR of the flag bits, [1] the number of malformed frames, [2] the largest samplesPerChannel (as the i32 call),
 *     [3] the route taken: 0 nothing decoded, 1 the 2048-sample decoder, 2 the any-length kernels.
 *   SELA_HIP_FLAG_STRIDE: the offsets never decrease, the walk is whole and [2] > stride (a 2048 stream with stride < 2048
 *     included); nothing is decoded then.
 *   sela_hip_decode_n_status_error() turns a host copy of the status words into the code sela_hip_decode returns for the same
 *     input, SELA_HIP_FLAG_STRIDE aside (SELA_HIP_ECAPACITY, which that call never needs).
 * d_frames: 4-byte aligned, holding every frame the offsets name.  d_workspace: sela_hip_decode_n_workspace_bytes(n_frames,
 * channels, stride) bytes, no initialisation (the payload call: sela_hip_index_workspace_bytes(payload_bytes, max_frames) more);
 * one call at a time may use it.  channels * n_frames below 2^31.  sela_hip_debug_standard_first routes the any-length kernels
 * as it routes the i32 call.
 * SELA_HIP_EINVAL: a null pointer (d_sample_offsets may be NULL), channels outside 1..255, stride 0, a misaligned d_frames /
 * d_payload; SELA_HIP_ECAPACITY: a smaller workspace.  Nothing is enqueued then. */
size_t sela_hip_decode_n_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride);
int sela_hip_decode_n_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride,
    int16_t* d_pcm_out /* [n_frames * stride][channels] */, uint64_t* d_sample_offsets /* [n_frames + 1] or NULL */, uint32_t* d_status /* [4] */,
    void* d_workspace, size_t workspace_bytes, void* stream);
/* sela_hip_index_frames_device() and then the call above on the frames it found, on one stream: the count never leaves the device.
 * Frames from *d_n_frames on are not decoded; d_sample_offsets[0 .. *d_n_frames] is written. */
int sela_hip_decode_payload_n_device(const uint8_t* d_payload, size_t payload_bytes, uint32_t max_frames, uint32_t channels, uint32_t stride,
    int16_t* d_pcm_out, uint64_t* d_sample_offsets, uint64_t* d_frame_offsets, uint32_t* d_n_frames, uint32_t* d_status, void* d_workspace,
    size_t workspace_bytes, void* stream);
/* Host only, no GPU: the code sela_hip_decode returns for the input whose device status words (a host copy) these are --
 * SELA_HIP_FLAG_STRIDE: SELA_HIP_ECAPACITY; then by the route ([3]):
 *   1 (the streaming job's mapping): a malformed frame or a Rice stream that runs dry: SELA_HIP_EFORMAT; a coefficient beyond
 *     int64 or outside the tables: SELA_HIP_ERANGE; else 0;
 *   2: sela_hip_decode_status_error()'s order (generic_decode's);
 *   0: SELA_HIP_FLAG_BAD_FRAME (the walk breaks, offsets decrease, or the largest length is 0): SELA_HIP_EFORMAT; else 0 (no frames).
 * A null pointer: SELA_HIP_EINVAL. */
int sela_hip_decode_n_status_error(const uint32_t* status /* [4], host copy */);

/* ---- verification: a stream against its PCM, frame by frame ----------------------------------------------
 * The codec reproduces the reference bit for bit, and the reference is not lossless on every frame.  These calls
 * say which frames of a stream come back different from the PCM they were made from, and where (a caller avoids the loss with
 * SELA_HIP_ENCODE_LOSSLESS, "encode options" below): what sela_hip_decode_n_device
 * does, with a compare where it stores -- on the 2048-sample route (up to eight channels) in one kernel that writes no PCM at all.
 *   d_pcm          int16, the layout sela_hip_decode writes: frame f at d_pcm + sample_offsets[f] * channels.  Read only.
 *   d_diff_counts  [n_frames]: the (sample, channel) values of frame f that sela_hip_decode_n_device would have written
 *                  differently from d_pcm.
 *   d_first_diff   [n_frames]: the smallest such index relative to the frame's start (i * channels + c), or 0xFFFFFFFF.
 *   d_status uint32[4], written by the call: [0], [1] and [3] exactly as sela_hip_decode_n_device leaves them for the same frames;
 *                  [2] the number of frames whose count is not 0 (the largest samplesPerChannel is not reported here:
 *                  sela_hip_index_samples() or d_sample_offsets say it).
 *   sela_hip_decode_n_status_error() applies to [0], [1] and [3] unchanged; where it gives non-zero, or SELA_HIP_FLAG_STRIDE is
 *   set, the two arrays are not defined.  n_frames = 0 writes zero status words.
 * Arguments, alignment (d_diff_counts and d_first_diff: 4 bytes), errors, capture and the one-call-at-a-time rule of the workspace
 * (sela_hip_verify_workspace_bytes; the payload call: sela_hip_index_workspace_bytes more) are sela_hip_decode_n_device's.  Apart
 * from the outputs named here and the workspace nothing is written.  sela_hip_debug_standard_first routes the any-length kernels
 * as it does for the decode call. */
size_t sela_hip_verify_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride);
int sela_hip_verify_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride,
    const int16_t* d_pcm, uint32_t* d_diff_counts /* [n_frames] */, uint32_t* d_first_diff /* [n_frames] */,
    uint64_t* d_sample_offsets /* [n_frames + 1] or NULL */, uint32_t* d_status /* [4] */, void* d_workspace, size_t workspace_bytes, void* stream);
/* sela_hip_index_frames_device() and then the call above on the frames it found, on one stream: the count stays on the device.
 * Frames from *d_n_frames on are left alone (their entries in the two arrays are not written). */
int sela_hip_verify_payload_device(const uint8_t* d_payload, size_t payload_bytes, uint32_t max_frames, uint32_t channels, uint32_t stride,
    const int16_t* d_pcm, uint32_t* d_diff_counts, uint32_t* d_first_diff, uint64_t* d_sample_offsets, uint64_t* d_frame_offsets,
    uint32_t* d_n_frames, uint32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream);
/* Host pointers, synchronous, in chunks of frames: returns what sela_hip_decode returns for the stream (0: the arrays are
 * valid).  *lossy_frames (or NULL): the frames with a difference.  Runs on the calling thread's any-length context and its own
 * stream, past the coalescer; an open streaming job of the thread is left alone. */
int sela_hip_verify(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, const int16_t* pcm,
    uint32_t* diff_counts /* [n_frames] */, uint32_t* first_diff /* [n_frames] */, uint32_t* lossy_frames /* or NULL */);

/* ---- verification of 32-bit and ragged streams: a stream against its int32 samples ------------------------
 * The calls above on the whole domain of sela_hip_decode_i32_device: samples of up to 32 bits, planar frames, channels of
 * different lengths, every subframe layout that call takes.  What sela_hip_decode_i32_device does, with a compare where it
 * stores: for every layout this library's encoders write (each channel named by one subframe, a difference subframe's parent an
 * independent one at least as long) no decoded sample is written to the caller's memory or moved by channel at all.
 *   d_samples      int32 [n_frames][channels][stride], the layout sela_hip_decode_i32_device writes (channel c of frame f at
 *                  ((f * channels) + c) * stride; with stride == samples_per_channel also what sela_hip_encode_i32_device
 *                  reads).  Read only.
 *   d_lengths      [n_frames * channels], the original's length of every channel, or NULL: every channel is stride long.  No
 *                  sample at or beyond stride is read; a length above stride counts as stride.
 *   With m the count sela_hip_decode_i32_device would report for (f, c) and L the original's length:
 *   d_diff_counts  [n_frames]: the sum over the channels of #{ i < min(m, L) : decoded[i] != original[i] } + |m - L| (a sample
 *                  that is missing or extra is a difference).
 *   d_first_diff   [n_frames]: the smallest c * stride + i over the channels, i the first differing index of channel c -- where
 *                  no value differs but the lengths do, min(m, L) -- or 0xFFFFFFFF when nothing differs.
 *   d_status uint32[4], written by the call (needs no initialisation): [0] and [1] exactly as sela_hip_decode_i32_device leaves
 *                  them for the same frames (SELA_HIP_FLAG_STRIDE included: nothing is compared then); [2] the number of frames
 *                  whose count is not 0; [3] zero.
 *   sela_hip_decode_status_error() applies unchanged; where it gives non-zero the two arrays are not defined.  n_frames = 0
 *   writes zero status words.
 * Asynchronous on `stream`: no allocation, no host synchronisation, no host-side read of device data, so a stream being captured
 * into a HIP graph may take either device call.  Apart from the outputs named here and the workspace nothing is written; the two
 * arrays need no initialisation; the results are deterministic.  sela_hip_debug_standard_first routes the decode kernels as it
 * does for the decode call.
 * d_workspace: sela_hip_verify_i32_workspace_bytes(n_frames, channels, stride) bytes, no initialisation (the payload call:
 * sela_hip_index_workspace_bytes(payload_bytes, max_frames) more); one call at a time may use it.  With up(b) = b rounded up to
 * a multiple of 256 it is
 *     sela_hip_decode_i32_workspace_bytes(max_frames, channels, stride)      the subframes as decoded, their records, the index
 *   + up(max_frames * channels * stride * 4)                                 the samples by channel, for frames of any other layout
 *   + up(max_frames * channels * 4)                                          ... and their counts
 *   + up(max(max_frames, 1) * 4)                                             a mark per frame: which way it went
 *   + up(max(max_frames * ceil(stride / 4096), 1) * 8)                       two words per (frame, slice of 4096 samples)
 *   + 256                                                                    the two control words
 * and SIZE_MAX where sela_hip_decode_i32_workspace_bytes() is, or where max_frames * channels reaches 2^31.
 * Errors and alignment as sela_hip_decode_i32_device; also SELA_HIP_EINVAL for a null d_samples, d_diff_counts or d_first_diff
 * (n_frames > 0) or one of them, or d_lengths, not 4-byte aligned.  Nothing is enqueued then; an argument error is found before a
 * device is asked for. */
size_t sela_hip_verify_i32_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride);
int sela_hip_verify_i32_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride,
    const int32_t* d_samples /* [n_frames][channels][stride] */, const uint32_t* d_lengths /* [n_frames * channels] or NULL */,
    uint32_t* d_diff_counts /* [n_frames] */, uint32_t* d_first_diff /* [n_frames] */, uint64_t* d_sample_offsets /* [n_frames + 1] or NULL */,
    uint32_t* d_status /* [4] */, void* d_workspace, size_t workspace_bytes, void* stream);
/* sela_hip_index_frames_device() and then the call above on the frames it found, on one stream: the count stays on the device.
 * Frames from *d_n_frames on are left alone (their entries in the two arrays are not written). */
int sela_hip_verify_payload_i32_device(const uint8_t* d_payload, size_t payload_bytes, uint32_t max_frames, uint32_t channels, uint32_t stride,
    const int32_t* d_samples, const uint32_t* d_lengths, uint32_t* d_diff_counts, uint32_t* d_first_diff, uint64_t* d_sample_offsets,
    uint64_t* d_frame_offsets, uint32_t* d_n_frames, uint32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream);
/* Host pointers, synchronous, in chunks of frames: returns what sela_hip_decode_i32 returns for the stream and this stride (0: the
 * arrays are valid).  *lossy_frames (or NULL): the frames with a difference.  Runs on the calling thread's any-length context and
 * its own stream, past the coalescer; an open streaming job of the thread is left alone. */
int sela_hip_verify_i32(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride,
    const int32_t* samples /* [n_frames][channels][stride] */, const uint32_t* lengths /* [n_frames * channels] or NULL */,
    uint32_t* diff_counts /* [n_frames] */, uint32_t* first_diff /* [n_frames] */, uint32_t* lossy_frames /* or NULL */);

/* ---- sample windows of a stream: only the frames they touch are decoded --------------------------------------
 * Every frame decodes on its own, so one second out of a three-minute track -- a player's seek, a batch of random crops from
 * compressed tracks that lie in device memory -- costs the nine or ten frames it overlaps.  A window names a STREAM, a run of
 * consecutive frames of the caller's frame table (one file among many concatenated into one table, or the whole table), and a
 * start inside it; all windows of a call have one length, window_samples.
 *   Output sample i of window w (i < window_samples): where start + i < 2048 * n_frames it is exactly the value
 *   sela_hip_decode_device writes for sample (start + i) % 2048 of table frame first_frame + (start + i) / 2048 -- for every input,
 *   malformed frames included (a silent channel, a refused parent, a frame that does not say 2048 samples: zeros and
 *   SELA_HIP_FLAG_BAD_FRAME, as from that call) -- and zero otherwise.  A stream that runs past the table
 *   (first_frame + n_frames > n_frames_total) is cut at the table's end: nothing outside the table is read.  start may be any
 *   uint64.  Windows may overlap, repeat and come in any order.
 *   format         SELA_HIP_WINDOW_I16_INTERLEAVED: d_out is int16 [n_windows][window_samples][channels];
 *                  SELA_HIP_WINDOW_F32_PLANAR: d_out is float [n_windows][channels][window_samples] holding value / 32768 (exact
 *                  in binary32).  Every element of d_out is written, by one launch: it needs no initialisation.
 *   d_window_flags uint32 [n_windows] or NULL, written by the call: the OR of the flag bits of the frames that window touched (a
 *                  loader drops one bad crop and keeps the batch).
 *   d_status uint32[4], written by the call: [0] the OR of the flag bits over every frame decoded; [1] the number of (window,
 *                  frame) decodes that met a malformed frame; [2] the number of windows with a non-zero flag word; [3] zero.
 *                  n_windows = 0 writes zero status words and nothing else.
 * Scope: frames of 2048 samples, 1 .. 8 channels, 16-bit samples.  More than 8 channels is SELA_HIP_EINVAL (decode the frames
 * with sela_hip_decode_device and crop); frames of other lengths are SELA_HIP_FLAG_BAD_FRAME, as from sela_hip_decode_device; samples
 * of more than 16 bits: sela_hip_decode_windows_i32_device, below; streams of any other frame length have no window call (random
 * access there needs a search of sample_offsets).
 * The device call is asynchronous on `stream`: no allocation, no host synchronisation, no host-side read of device data (the
 * descriptors stay on the device; the launch is shaped by window_samples alone), so a stream being captured into a HIP graph may
 * take it, and a replay reads whatever d_windows holds then.  d_workspace: sela_hip_decode_windows_workspace_bytes() bytes, no
 * initialisation, one call at a time.  Apart from d_out, d_window_flags, d_status and the workspace nothing is written.
 * Errors, found before a device is asked for (nothing is enqueued then) -- SELA_HIP_EINVAL: a null pointer (d_frames and
 * d_frame_offsets only where n_frames_total > 0, everything but d_status only where n_windows > 0), channels outside 1 .. 8,
 * window_samples 0 or above 2^24, another format, d_frames not 4-byte aligned, d_windows not 8-byte aligned, d_out not aligned to
 * its element (2 or 4 bytes), d_window_flags or d_status not 4-byte aligned, or n_windows * cover at or above 2^31, where
 * cover = (window_samples + 2046) / 2048 + 1 is the most frames a window touches; SELA_HIP_ECAPACITY: a smaller workspace. */
typedef struct sela_hip_window {
    uint64_t start;       /* first sample per channel, relative to the stream's first sample */
    uint32_t first_frame; /* the stream: frames [first_frame, first_frame + n_frames) of the table */
    uint32_t n_frames;
} sela_hip_window;        /* 16 bytes; lives in DEVICE memory for the device call */
#define SELA_HIP_WINDOW_I16_INTERLEAVED 0u
#define SELA_HIP_WINDOW_F32_PLANAR 1u
size_t sela_hip_decode_windows_workspace_bytes(uint32_t n_windows, uint32_t window_samples, uint32_t channels);
int sela_hip_decode_windows_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets /* [n_frames_total + 1] */, uint32_t n_frames_total,
    uint32_t channels, const sela_hip_window* d_windows, uint32_t n_windows, uint32_t window_samples, uint32_t format, void* d_out,
    uint32_t* d_window_flags /* [n_windows] or NULL */, uint32_t* d_status /* [4] */, void* d_workspace, size_t workspace_bytes, void* stream);
/* Host pointers, synchronous: the call above on the calling thread's any-length context and its own stream, past the coalescer;
 * an open streaming job of the thread is left alone (where sela_hip_verify runs).  Only the frames the windows touch are copied
 * to the device: the distinct covering frames are staged back to back and the descriptors put on that compacted table.
 * Returns, after the argument errors above (host pointers need no alignment) and SELA_HIP_EFORMAT for frame offsets that
 * decrease, what the fast route of sela_hip_decode_n_status_error() makes of the status words: a malformed frame or a dry Rice
 * stream: SELA_HIP_EFORMAT; a coefficient outside the tables or beyond int64: SELA_HIP_ERANGE.  UNLIKE the sibling host calls,
 * `out` and `window_flags` are filled in both of these cases: one bad crop must not cost a loader its batch, and window_flags says
 * which crop it was. */
int sela_hip_decode_windows(const uint8_t* frames, const uint64_t* frame_offsets /* [n_frames_total + 1] */, uint32_t n_frames_total,
    uint32_t channels, const sela_hip_window* windows, uint32_t n_windows, uint32_t window_samples, uint32_t format, void* out,
    uint32_t* window_flags /* [n_windows] or NULL */);

/* ---- sample windows of whole-track streams: the long last frame too ---------------------------------------------
 * sela_hip_encode_whole (5.19) writes streams of 2048-sample frames and ONE last frame of 1 .. 4095 samples, which the calls above
 * refuse.  These take the same arguments and the same descriptor, make the same argument checks in the same order with the same
 * codes (nothing is enqueued on a refusal), and read a window's stream as a WHOLE-TRACK stream: let n be the stream's frames
 * inside the table, L the last of them and n_L what L says its length is by sela_hip_index_samples' rule (its first subframe's
 * samplesPerChannel).  Where n_L is in 1 .. 4095 and not 2048 the stream holds S = 2048 (n - 1) + n_L samples per channel, and output
 * sample i of window w is
 *   start + i < 2048 (n - 1):   what sela_hip_decode_windows_device writes, for every input, malformed frames included;
 *   2048 (n - 1) <= start + i < S:   exactly the int16 sela_hip_decode_n_device writes for sample start + i - 2048 (n - 1) of frame L
 *                  decoded alone, where its any-length kernel takes the frame (that call's narrowing, its combine rules for
 *                  difference channels); SELA_HIP_WINDOW_F32_PLANAR holds that value / 32768;
 *   otherwise:     zero.
 * A frame L that kernel declines -- not at a word-aligned place, a header the walk refuses, a subframe longer than 4095 samples or
 * not longer than its order, channels that disagree about the length or a layout the combine refuses, a Rice stream that runs
 * dry, a coefficient outside the tables -- leaves its share zero and raises a flag in the window's word and in d_status[0]:
 * SELA_HIP_FLAG_RICE_OVERRUN, _Q_RANGE or _COEF_OVERFLOW where one was met, SELA_HIP_FLAG_BAD_FRAME otherwise.  Nothing outside
 * the frame's bytes is read.  The combine writes L's independent subframes first, then its differences in subframe order, as the
 * reference does: a difference under a difference that stands in front of it in the stream (a chain in stream order) is decoded,
 * its parent being final by then; one whose parent is a difference behind it is a layout the combine refuses (BAD_FRAME).
 * Where n_L is 2048, 0 or above 4095 every word written (d_out, d_window_flags, d_status) is what
 * sela_hip_decode_windows_device writes; so is everything for a frame in front of L that does not say 2048.
 * d_status[1] also counts the (window, L) decodes that raised SELA_HIP_FLAG_BAD_FRAME; d_status[2] counts each window with a
 * non-zero flag word once.  The device call is asynchronous and capturable as the one above: its launches are shaped by
 * window_samples, n_windows and channels alone.  Scope: 1 .. 8 channels, 16-bit output, a last frame of at most 4095 samples.
 *   workspace = sela_hip_decode_windows_workspace_bytes(n_windows, window_samples, channels)
 *             + n_windows * (48 + channels * (16 + 4 * 4096)) + 1024
 * (a copy of each descriptor and a record of its share of L; per channel a record and 4096 decoded 32-bit samples; alignment).
 * The host call stages the covering frames only, L among them for every window that starts at or behind 2048 (n - 1), and returns
 * what sela_hip_decode_windows returns, `out` and `window_flags` filled in the SELA_HIP_EFORMAT and SELA_HIP_ERANGE cases too. */
size_t sela_hip_decode_windows_whole_workspace_bytes(uint32_t n_windows, uint32_t window_samples, uint32_t channels);
int sela_hip_decode_windows_whole_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets /* [n_frames_total + 1] */, uint32_t n_frames_total,
    uint32_t channels, const sela_hip_window* d_windows, uint32_t n_windows, uint32_t window_samples, uint32_t format, void* d_out,
    uint32_t* d_window_flags /* [n_windows] or NULL */, uint32_t* d_status /* [4] */, void* d_workspace, size_t workspace_bytes, void* stream);
int sela_hip_decode_windows_whole(const uint8_t* frames, const uint64_t* frame_offsets /* [n_frames_total + 1] */, uint32_t n_frames_total,
    uint32_t channels, const sela_hip_window* windows, uint32_t n_windows, uint32_t window_samples, uint32_t format, void* out,
    uint32_t* window_flags /* [n_windows] or NULL */);

/* ---- sample windows of 24- and 32-bit streams -------------------------------------------------------------------
 * The window calls above hand out 16-bit samples.  These take the same descriptor (in device memory for the device call) and the
 * same table and stream semantics -- a stream is cut at the table's end, start may be any uint64, windows may overlap, repeat and
 * come in any order -- and hand out samples of up to 32 bits:
 *   format         SELA_HIP_WINDOW_I32_PLANAR: d_out is int32 [n_windows][channels][window_samples];
 *                  SELA_HIP_WINDOW_PCM24_INTERLEAVED: 3-byte little-endian [n_windows][window_samples][channels], each sample's low
 *                  three bytes -- window w starts at byte w * window_samples * channels * 3, at any byte phase;
 *                  SELA_HIP_WINDOW_PCM32_INTERLEAVED: int32 little-endian [n_windows][window_samples][channels];
 *                  SELA_HIP_WINDOW_F32_PLANAR: float [n_windows][channels][window_samples] holding (float)value * 2^-(sample_bits - 1),
 *                  the conversion rounding to nearest-even (exact for 24-bit audio); sample_bits in 1 .. 32.
 *                  SELA_HIP_WINDOW_I16_INTERLEAVED is SELA_HIP_EINVAL here (the calls above).  sample_bits is ignored for the
 *                  other formats.
 * Output sample i of window w refers to table frame f = first_frame + (start + i) / 2048 where that lies inside the window's
 * stream.  Frame f is TAKEN when it sits at a 4-byte-aligned offset, the header walk accepts all `channels` subframes, each says
 * 2048 samples, is longer than its order and is sela_subframe_decodable, no Rice stream runs dry, no coefficient leaves the tables
 * or int64, and the layout passes the combine's rules (channel and parent exist, the parent is written before and is long enough,
 * every channel ends at 2048).  For a taken frame the value is exactly what sela_hip_decode_i32_device writes for
 * (f, channel, (start + i) % 2048) at stride 2048.  For any other frame the whole share of that frame is zero and its flags are
 * SELA_HIP_FLAG_RICE_OVERRUN, _Q_RANGE or _COEF_OVERFLOW where one was met, SELA_HIP_FLAG_BAD_FRAME otherwise (a frame that does
 * not say 2048 among them).  Samples behind the stream's end are zero, without a flag.
 *   d_window_flags uint32 [n_windows] or NULL: the OR over the frames that window touched.
 *   d_status uint32[4]: [0] the OR over all (window, frame) decodes; [1] the number of (window, frame) decodes that raised
 *                  SELA_HIP_FLAG_BAD_FRAME; [2] the number of windows with a non-zero flag word; [3] PCM24 only: the number of
 *                  output samples outside [-2^23, 2^23), whose low three bytes are written all the same; 0 for the other formats.
 *                  n_windows = 0 writes zero status words and nothing else.
 * Every byte of d_out is written exactly once by the call's launches (there is no pre-clear), and no other byte: a PCM24 share
 * goes out as aligned dwords with single bytes only at its two ragged ends.  Scope: frames of 2048 samples, 1 .. 8 channels.
 * The device call is asynchronous and capturable as sela_hip_decode_windows_device is: one serial chain on `stream`, launches
 * shaped by n_windows, window_samples and channels alone, no allocation, no host wait, no host read of device data.
 *   workspace = n_windows * cover * channels * (16 + 4 * 2048) + 4 * n_windows + 1024,   cover = (window_samples + 2046) / 2048 + 1
 * (per window, covering frame and channel a record and 2048 decoded 32-bit samples; a flag word per window for a call that
 * passes no d_window_flags; alignment).  It does not depend on the data.
 * Errors, found before a device is asked for (nothing is enqueued then): those of sela_hip_decode_windows_device in its order
 * and with its codes, where "another format" is anything but the four above or sample_bits outside 1 .. 32 with F32, the product
 * refused at 2^31 is n_windows * cover * channels, n_windows at or above 2^24 is refused behind it (a launch holds fewer than 2^32
 * work-items per dimension), and d_out must be 4-byte aligned in every format; SELA_HIP_ECAPACITY: a smaller workspace.
 * The host call stages only the distinct covering frames, runs where sela_hip_decode_windows runs and returns what it returns:
 * SELA_HIP_EFORMAT for a malformed or dry frame, SELA_HIP_ERANGE for coefficient trouble, `out` and `window_flags` filled in both
 * cases.  It has no status words: the PCM24 count of d_status[3] is the device call's alone.  ALIGNMENT IN THE HOST CALL: the
 * covering frames are staged back to back, so the rule "at a 4-byte-aligned offset" is applied to a frame's offset in the STAGED
 * table, not in the caller's.  Every frame the library's encoders write is whole words, and a table of such frames behaves alike
 * in both calls; a frame of whole words that the caller's table holds at an offset of 4k + 1 .. 3 (behind a frame that is not whole
 * words) is refused by the device call always, and by the host call only when the frames staged in front of it leave it at such an
 * offset again -- alone in its batch it lands on offset 0 and is decoded. */
#define SELA_HIP_WINDOW_I32_PLANAR 2u
#define SELA_HIP_WINDOW_PCM24_INTERLEAVED 3u
#define SELA_HIP_WINDOW_PCM32_INTERLEAVED 4u
size_t sela_hip_decode_windows_i32_workspace_bytes(uint32_t n_windows, uint32_t window_samples, uint32_t channels);
int sela_hip_decode_windows_i32_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets /* [n_frames_total + 1] */, uint32_t n_frames_total,
    uint32_t channels, const sela_hip_window* d_windows, uint32_t n_windows, uint32_t window_samples, uint32_t format, uint32_t sample_bits, void* d_out,
    uint32_t* d_window_flags /* [n_windows] or NULL */, uint32_t* d_status /* [4] */, void* d_workspace, size_t workspace_bytes, void* stream);
int sela_hip_decode_windows_i32(const uint8_t* frames, const uint64_t* frame_offsets /* [n_frames_total + 1] */, uint32_t n_frames_total,
    uint32_t channels, const sela_hip_window* windows, uint32_t n_windows, uint32_t window_samples, uint32_t format, uint32_t sample_bits, void* out,
    uint32_t* window_flags /* [n_windows] or NULL */);

/* ---- sample windows of 24- and 32-bit whole-track streams: the long last frame too ------------------------------
 * These are to sela_hip_decode_windows_i32* what sela_hip_decode_windows_whole* are to sela_hip_decode_windows*: the same
 * arguments and descriptor, the same argument checks in the same order with the same codes (nothing is enqueued on a refusal), the
 * same four formats, and a window's stream read as a WHOLE-TRACK stream.  Let n be the stream's frames inside the table, L the
 * last of them and n_L what L says its length is by sela_hip_index_samples' rule.  Where n_L is in 1 .. 4095 and not 2048 the
 * stream holds S = 2048 (n - 1) + n_L samples per channel, and output sample i of window w is
 *   start + i < 2048 (n - 1):   what sela_hip_decode_windows_i32_device writes, for every input, malformed frames included;
 *   2048 (n - 1) <= start + i < S:   exactly the value sela_hip_decode_i32_device writes for sample start + i - 2048 (n - 1) of frame L
 *                  decoded alone at stride 4095, where the last frame's kernel takes the frame and the combine's rules accept
 *                  its layout -- in the call's format: int32 planar, (float)value * 2^-(sample_bits - 1), interleaved int32, or
 *                  the low three bytes;
 *   otherwise:     zero.
 * A frame L that is declined -- the cases sela_hip_decode_windows_whole_device lists -- leaves its share zero and raises the flags
 * that call lists, in the window's word and in d_status[0..2], by the same counting.  SELA_HIP_WINDOW_PCM24_INTERLEAVED adds the
 * tail share's samples outside [-2^23, 2^23) to d_status[3].  Where n_L is 2048, 0 or above 4095 every word written (d_out,
 * d_window_flags, d_status) is what sela_hip_decode_windows_i32_device writes; so is everything for a frame in front of L that does
 * not say 2048.  Scope: 1 .. 8 channels, a last frame of at most 4095 samples.
 * The device call is one serial chain on `stream`, asynchronous and capturable as the plain call is.  The plain call's launches
 * write every byte of d_out, the share of L as the zeros of a stream that has ended there; one more store launch then writes
 * every byte of a taken share and NO byte outside it (a PCM24 share as aligned dwords with single bytes only at its two ragged
 * ends).  So where the plain call promises "exactly once", here the bytes of a taken share of L are written TWICE by the call, by
 * two launches in series; every other byte of d_out once; no other byte.
 *   workspace = sela_hip_decode_windows_i32_workspace_bytes(n_windows, window_samples, channels)
 *             + n_windows * (48 + channels * (16 + 4 * 4096)) + 1024
 * (a copy of each descriptor and a record of its share of L; per channel a record and 4096 decoded 32-bit samples; alignment).
 * It does not depend on the data or the device.
 * The host call stages the covering frames only, L among them for every window that reaches 2048 (n - 1), and returns what
 * sela_hip_decode_windows_i32 returns, `out` and `window_flags` filled in the SELA_HIP_EFORMAT and SELA_HIP_ERANGE cases too. */
size_t sela_hip_decode_windows_i32_whole_workspace_bytes(uint32_t n_windows, uint32_t window_samples, uint32_t channels);
int sela_hip_decode_windows_i32_whole_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets /* [n_frames_total + 1] */, uint32_t n_frames_total,
    uint32_t channels, const sela_hip_window* d_windows, uint32_t n_windows, uint32_t window_samples, uint32_t format, uint32_t sample_bits, void* d_out,
    uint32_t* d_window_flags /* [n_windows] or NULL */, uint32_t* d_status /* [4] */, void* d_workspace, size_t workspace_bytes, void* stream);
int sela_hip_decode_windows_i32_whole(const uint8_t* frames, const uint64_t* frame_offsets /* [n_frames_total + 1] */, uint32_t n_frames_total,
    uint32_t channels, const sela_hip_window* windows, uint32_t n_windows, uint32_t window_samples, uint32_t format, uint32_t sample_bits, void* out,
    uint32_t* window_flags /* [n_windows] or NULL */);

/* ---- encode options: the lossless mode ----------------------------------------------------------------------
 * The reference's encoder predicts with (2^34 + sum) >> 35 and its decoder with -((2^34 - sum) >> 35): where 2^34 + sum is a
 * multiple of 2^35 the two differ by one, and the frame does not come back as it went in.  With SELA_HIP_ENCODE_LOSSLESS the
 * residues are taken against the DECODER's prediction, so that every decoder of the format -- the reference's included --
 * rebuilds every sample exactly.  Order, coefficients, Rice coding, the stereo rule and the frame layout are what they are; the
 * stream differs from the plain call's only in frames that hold such a tie (one residue by 1, and what follows from it).
 *
 * Every *_opt call takes exactly the arguments of its namesake and a trailing `options` word:
 *   options == 0                an alias of the namesake (it calls it).
 *   a bit not defined here      SELA_HIP_EINVAL.
 *   SELA_HIP_ENCODE_LOSSLESS with d_trace != NULL: SELA_HIP_EINVAL (the trace is the reference's arithmetic).
 * In both error cases nothing is enqueued.  Workspace sizes, bounds, alignment, status words, errors and graph capture are the
 * namesake's, and so is the choice of kernels.  The host-pointer one-shot calls with options != 0 do not go through the
 * coalescer; a thread with a streaming job open gets them from the any-length route, which leaves that job alone.  For a
 * streaming job the option belongs to the job: feed / end are sela_hip_encode_feed / sela_hip_encode_end.
 * The stage calls (sela_hip_lpc_encode*) have no option: their residues stay the reference's class's. */
#define SELA_HIP_ENCODE_LOSSLESS 1u
int sela_hip_encode_device_opt(const int16_t* d_pcm, uint32_t n_frames, uint32_t channels, uint8_t* d_frames, size_t frames_cap,
    uint64_t* d_frame_offsets, uint32_t* d_status, void* d_workspace, size_t workspace_bytes, sela_hip_trace* d_trace, void* stream,
    uint32_t options);
int sela_hip_encode_n_device_opt(const int16_t* d_pcm, uint32_t n_frames, uint32_t channels, uint32_t samples_per_channel,
    uint8_t* d_frames, size_t frames_cap, uint64_t* d_frame_offsets, uint32_t* d_status, void* d_workspace, size_t workspace_bytes,
    void* stream, uint32_t options);
int sela_hip_encode_i32_device_opt(const int32_t* d_samples, uint32_t n_frames, uint32_t channels, uint32_t samples_per_channel,
    uint8_t* d_frames, size_t frames_cap, uint64_t* d_frame_offsets, uint32_t* d_status, void* d_workspace, size_t workspace_bytes,
    void* stream, uint32_t options);
int sela_hip_encode_opt(const int16_t* pcm, uint32_t n_frames, uint32_t channels, uint32_t samples_per_channel, uint8_t* frames_out,
    size_t frames_cap, uint64_t* frame_offsets_out, uint32_t options);
int sela_hip_encode_i32_opt(const int32_t* samples, uint32_t n_frames, uint32_t channels, uint32_t samples_per_channel,
    uint8_t* frames_out, size_t frames_cap, uint64_t* frame_offsets_out, uint32_t options);
int sela_hip_encode_ragged_i32_opt(const int32_t* samples, const uint32_t* lengths, uint32_t channels, uint8_t* frame_out,
    size_t frame_cap, size_t* frame_bytes, uint32_t options);

/* ---- channel pairs: difference coding for any number of channels ----------------------------------------------
 * The format lets any subframe be stored as a difference against a parent channel (type 1, parentChannelNumber), and every
 * decoder rebuilds parent - difference (src/frame/frame_decoder.cpp:39-69).  The plain calls use that, as the reference does,
 * for the second channel of an exactly-stereo frame only.  The paired calls use it for every pair of adjacent channels.
 * The rule, for a frame of C channels of n samples each:
 *   Channels are paired (2p, 2p + 1), p = 0 .. C / 2 - 1; an odd last channel is alone.
 *   Channel 2p is always an independent subframe (type 0, parent 2p).
 *   Channel 2p + 1 has two candidates: its own signal, and d[j] = ch[2p][j] - ch[2p + 1][j] (int32 wrap-around, as the stereo
 *     frame's difference).  The difference is stored (type 1, parent 2p) iff its coef_words + res_words is STRICTLY FEWER
 *     (src/frame/frame_encoder.cpp:64-72).  A candidate flagged SELA_HIP_FLAG_WORDS_CAP / _RICE_RANGE is treated as the plain
 *     call treats it in a stereo frame.
 *   Subframes appear in channel order.  There are C + C / 2 signals per frame: 0 .. C - 1 the channels, C + p pair p's
 *     difference (sela_hip_paired_signals_per_frame).  d_status[0] is the OR over all candidates of all pairs.
 * The frame equals, byte for byte, the sync word followed by the two subframes of the reference's stereo frame of
 * (ch[2p], ch[2p + 1]) for every pair, then the reference's mono subframe of an odd last channel -- each with its channel byte
 * renumbered, and its parent byte where type == 1.  For C = 1 and C = 2 the bytes are the plain call's.  With
 * SELA_HIP_ENCODE_LOSSLESS every candidate's residues are the lossless mode's.  A parent is always an independent channel of the
 * same length: nothing a decoder of the format could refuse is produced.
 * options: 0 or SELA_HIP_ENCODE_LOSSLESS; anything else is SELA_HIP_EINVAL, reported before the call's other checks.
 * The device calls are sela_hip_encode_i32_device / sela_hip_encode_n_device in everything else: layouts, alignment, asynchronous
 * on `stream` with no allocation, no host wait and no host read of device data (graph capture), d_frame_offsets always written in
 * full, frames beyond frames_cap counted in d_status[1] and not written, n_frames = 0, sela_hip_encode_status_error, and
 * SELA_HIP_EINVAL where n_frames x signals per frame reaches 2^31.  The workspace, sela_hip_encode_paired_workspace_bytes()
 * bytes, does not depend on the data.  They run on the any-length kernels for every shape, 2048 x int16 included.
 * The host calls run where the lossless one-shot calls run: the any-length route in its chunks of frames, past the coalescer; an
 * open streaming job of the thread is left alone.
 * sela_hip_encode_bound_bytes_n() bounds a paired stream as it stands: it allows every subframe one candidate's slot (12 header
 * bytes, 32 coefficient words, the residue words of the worst Rice parameter), and a stored subframe is still one candidate --
 * a difference whose residues leave the zig-zag's range is SELA_HIP_ERANGE as the stereo frame's is. */
uint32_t sela_hip_paired_signals_per_frame(uint32_t channels); /* channels + channels / 2 */
size_t sela_hip_encode_paired_workspace_bytes(uint32_t n_frames, uint32_t channels, uint32_t samples_per_channel);
int sela_hip_encode_paired_i32_device(const int32_t* d_samples, uint32_t n_frames, uint32_t channels, uint32_t samples_per_channel,
    uint8_t* d_frames, size_t frames_cap, uint64_t* d_frame_offsets /* [n_frames + 1] */, uint32_t* d_status /* [4] */,
    void* d_workspace, size_t workspace_bytes, void* stream, uint32_t options);
int sela_hip_encode_paired_n_device(const int16_t* d_pcm, uint32_t n_frames, uint32_t channels, uint32_t samples_per_channel,
    uint8_t* d_frames, size_t frames_cap, uint64_t* d_frame_offsets /* [n_frames + 1] */, uint32_t* d_status /* [4] */,
    void* d_workspace, size_t workspace_bytes, void* stream, uint32_t options);
int sela_hip_encode_paired_i32(const int32_t* samples, uint32_t n_frames, uint32_t channels, uint32_t samples_per_channel,
    uint8_t* frames_out, size_t frames_cap, uint64_t* frame_offsets_out /* [n_frames + 1] */, uint32_t options);
int sela_hip_encode_paired(const int16_t* pcm, uint32_t n_frames, uint32_t channels, uint32_t samples_per_channel, uint8_t* frames_out,
    size_t frames_cap, uint64_t* frame_offsets_out /* [n_frames + 1] */, uint32_t options);

/* ---- a whole track: the tail kept in a long last frame ---------------------------------------------------------
 * The reference's WAV reader cuts 2048-sample frames and drops what is left over; the format does not ask for that (a frame says
 * its own samplesPerChannel).  These calls code all N = n_samples samples per channel of a track.  The rule, with F = N / 2048 and
 * t = N % 2048:
 *   N == 0            no frame.
 *   t == 0            F frames of 2048 samples: the bytes and offsets of sela_hip_encode_device(_opt) on them.
 *   F >= 1, t > 0     F frames: frames 0 .. F - 2 of 2048 samples, frame F - 1 of 2048 + t (2049 .. 4095) -- the tail is folded into
 *                     the last whole frame, never a frame of its own (a block of up to a hundred samples is routinely no longer
 *                     than the order its own analysis picks: SELA_HIP_FLAG_SHORT_BLOCK).
 *   F == 0, N > 0     one frame of N samples; a short one may be SELA_HIP_FLAG_SHORT_BLOCK / SELA_HIP_ERANGE, exactly as from
 *                     sela_hip_encode on the same frame.
 * Frame f starts at sample 2048 * f for every f.  Frames 0 .. F - 2 are byte for byte the plain call's; the last frame is byte for
 * byte frame::FrameEncoder's for a WavFrame of its length (the stereo decision included), i.e. sela_hip_encode_n_device's.
 * Host only, no GPU:
 *   sela_hip_whole_frames(N)                 the number of frames;
 *   sela_hip_whole_frame(N, f, &first, &len) frame f's first sample and length (SELA_HIP_EINVAL: no such frame, a null pointer);
 *   sela_hip_encode_whole_bound_bytes        what frames_cap must be to be certain the stream fits (SIZE_MAX beyond size_t);
 *   sela_hip_encode_whole_workspace_bytes    the device call's workspace for every track of at most max_samples samples per channel:
 *                                            it does not depend on the data or the device, and grows with max_samples.  The plain
 *                                            call's workspace for the track's frames, then the any-length call's for one frame of
 *                                            min(max_samples, 4095) samples, that frame's bound, and 512 bytes.  SIZE_MAX for what
 *                                            the call refuses.
 * sela_hip_encode_whole_device: d_pcm int16 [N][channels] interleaved, 4-byte aligned; d_frames 4-byte aligned; d_frame_offsets
 *   [frames + 1]; d_status uint32[4]; options: 0 or SELA_HIP_ENCODE_LOSSLESS.  Asynchronous on `stream`: no allocation, no host wait,
 *   no host read of device data, so a stream being captured into a HIP graph may take it.  The contract is sela_hip_encode_n_device's:
 *   the offsets are always written in full; a frame that ends beyond frames_cap is not written and nothing at or past frames_cap is;
 *   d_status[0] is the OR of the flag bits of all frames, d_status[1] the number of frames not written, [2] and [3] zero;
 *   sela_hip_encode_status_error() applies unchanged; N == 0 writes d_frame_offsets[0] = 0 and zero status words.
 *   Launches: the plain call's three on frames 0 .. F - 2, the any-length call's three on the last frame -- read in place, coded into
 *   the workspace, on a stream of the library's own between two events (forked from `stream` before the plain launches, joined
 *   behind them; inside a capture the side stream joins the capture and leaves it at the join) -- and one small kernel on `stream`
 *   that copies the last frame behind the others, writes d_frame_offsets[F] and folds the two status words together.  With t == 0,
 *   or a single frame, only the one call it is, on `stream`.
 *   SELA_HIP_EINVAL: an option bit not defined, channels outside 1..255, frames x signals per frame at 2^31 or more, a null pointer
 *   (d_pcm and d_frames only where N > 0), a misaligned d_pcm or d_frames; SELA_HIP_ECAPACITY: a smaller workspace.  Nothing is
 *   enqueued then.
 * sela_hip_encode_whole: the same stream from HOST pointers, synchronous, on the calling thread's contexts: frames 0 .. F - 2 where
 *   sela_hip_encode_opt codes them, the last frame on the any-length route, past the coalescer.  A thread with a streaming job open is
 *   served by the any-length route alone, which leaves that job alone.  Errors are sela_hip_encode_opt's (SELA_HIP_ECAPACITY: frames_out
 *   too small; frame_offsets_out is not defined then). */
uint64_t sela_hip_whole_frames(uint64_t n_samples);
int sela_hip_whole_frame(uint64_t n_samples, uint64_t frame, uint64_t* first_sample, uint32_t* length);
size_t sela_hip_encode_whole_bound_bytes(uint64_t n_samples, uint32_t channels);
size_t sela_hip_encode_whole_workspace_bytes(uint64_t max_samples, uint32_t channels);
int sela_hip_encode_whole_device(const int16_t* d_pcm, uint64_t n_samples, uint32_t channels, uint8_t* d_frames, size_t frames_cap,
    uint64_t* d_frame_offsets /* [frames + 1] */, uint32_t* d_status /* [4] */, void* d_workspace, size_t workspace_bytes, void* stream,
    uint32_t options);
int sela_hip_encode_whole(const int16_t* pcm, uint64_t n_samples, uint32_t channels, uint8_t* frames_out, size_t frames_cap,
    uint64_t* frame_offsets_out /* [frames + 1] */, uint32_t options);

/* ---- a full decode of a whole-track stream: the 2048-sample decoder with the last frame beside it ----------------
 * sela_hip_decode_n_device and sela_hip_decode take a stream with ONE frame that does not say 2048 down the any-length route,
 * every frame of it.  These calls read the stream as the window calls above do (5.20).  Let n be the frame count (the payload
 * form's is found on the device and stays there), L = n - 1 and n_L what L says its length is by sela_hip_index_samples' rule.
 *   n_L in 1 .. 4095 and not 2048:   S = 2048 (n - 1) + n_L samples per channel.  Samples [0, 2048 (n - 1)) are word for word what
 *                  sela_hip_decode_device writes for frames 0 .. n - 2, malformed ones included (zeros, SELA_HIP_FLAG_BAD_FRAME);
 *                  samples [2048 (n - 1), S) are the int16 sela_hip_decode_n_device writes for frame L decoded alone, interleaved at
 *                  d_pcm_out + 2048 (n - 1) * channels.  A frame L the any-length kernel declines or whose layout the combine rules
 *                  refuse raises its flag as the window calls list them, and nothing at or past 2048 (n - 1) * channels is written.
 *                  d_status[3] = 3.
 *   any other n_L: S = 2048 n, every word written is sela_hip_decode_device's on all n frames, d_status[3] = 1.
 *   n == 0:        zero status words, *d_n_samples = 0, nothing else written.
 * *d_n_samples = S always.  Where S > pcm_capacity (samples per channel): SELA_HIP_FLAG_STRIDE, d_status[3] = 0, nothing is decoded
 * or written.  Nothing at or past min(S, pcm_capacity) * channels is written on any input.  d_status[0] is the OR of the flags,
 * d_status[1] the number of malformed frames among 0 .. n - 2 (sela_hip_decode_device's count) plus one for a frame L that is not
 * decoded, whatever its flag, d_status[2] zero.
 * sela_hip_decode_whole_status_error (host only, no GPU) maps a host copy of the status words, in this order:
 *   1. SELA_HIP_FLAG_STRIDE                                                 -> SELA_HIP_ECAPACITY
 *   2. a malformed frame (SELA_HIP_FLAG_BAD_FRAME) or a dry Rice stream (SELA_HIP_FLAG_RICE_OVERRUN)  -> SELA_HIP_EFORMAT
 *   3. SELA_HIP_FLAG_COEF_OVERFLOW, SELA_HIP_FLAG_Q_RANGE                   -> SELA_HIP_ERANGE
 *   4. SELA_HIP_FLAG_INTERNAL                                               -> SELA_HIP_ENODEV
 *   5. otherwise 0.
 * Scope: 1 .. 8 channels (more: SELA_HIP_EINVAL, as for the window calls), 16-bit output, a last frame of at most 4095 samples.
 * SELA_HIP_EINVAL also for a null pointer (d_frames and d_pcm_out only where there are frames) and a d_frames that is not 4-byte
 * aligned, SELA_HIP_ECAPACITY for a smaller workspace, as sela_hip_decode_n_device; the payload form adds
 * sela_hip_index_frames_device's checks.  Errors are found before a device is asked for, and nothing is enqueued.
 * Asynchronous on `stream`: no allocation, no host wait, no host read of device data; the launches are shaped by n_frames /
 * max_frames and channels alone, so a stream being captured into a HIP graph may take the call.  Launches: a plan kernel of one
 * thread; the 2048-sample decoder on `stream`, on the plan's count; the last frame's decode and store on a stream of the library's
 * own between two events, forked behind the plan and joined at the end (inside a capture the side stream joins and leaves it).
 *   workspace = sela_hip_decode_workspace_bytes(max_frames, channels) + channels * (16 + 4 * 4096) + 1024
 * (the 2048-sample decoder's; per channel of the last frame a record and 4096 decoded 32-bit samples; the plan's record of L, its
 * count of frames and alignment); the payload form needs sela_hip_index_workspace_bytes(payload_bytes, max_frames) more.
 * sela_hip_decode_whole: the same reading of HOST bytes, synchronous.  Frames 0 .. n - 2 go where sela_hip_decode sends a stream of
 * 2048-sample frames, the last frame through the any-length route's one-shot decode on a context of its own, past the coalescer; a
 * thread with a streaming job open is served by that route alone, and the job is left alone.  *n_samples = S (0 after an argument
 * error).  For a whole-track stream -- frames of 2048 samples, with or without a long last one -- it returns 0 where sela_hip_decode
 * returns 0, with the same bytes in [0, S * channels); otherwise the first code in the order above (SELA_HIP_ECAPACITY: pcm_capacity
 * < S, nothing written).  A stream with another odd frame is malformed here (SELA_HIP_EFORMAT) and sela_hip_decode's to decode. */
size_t sela_hip_decode_whole_workspace_bytes(uint32_t max_frames, uint32_t channels);
int sela_hip_decode_whole_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets /* [n_frames + 1] */, uint32_t n_frames, uint32_t channels,
    int16_t* d_pcm_out, uint64_t pcm_capacity /* samples per channel */, uint64_t* d_n_samples /* [1] */, uint32_t* d_status /* [4] */, void* d_workspace,
    size_t workspace_bytes, void* stream);
int sela_hip_decode_whole_payload_device(const uint8_t* d_payload, size_t payload_bytes, uint32_t max_frames, uint32_t channels, int16_t* d_pcm_out,
    uint64_t pcm_capacity /* samples per channel */, uint64_t* d_n_samples /* [1] */, uint64_t* d_frame_offsets /* [max_frames + 1] */, uint32_t* d_n_frames /* [1] */,
    uint32_t* d_status /* [4] */, void* d_workspace, size_t workspace_bytes, void* stream);
int sela_hip_decode_whole_status_error(const uint32_t* status /* [4], host copy */);
int sela_hip_decode_whole(const uint8_t* frames, const uint64_t* frame_offsets /* [n_frames + 1] */, uint32_t n_frames, uint32_t channels, int16_t* pcm_out,
    uint64_t pcm_capacity /* samples per channel */, uint64_t* n_samples);

/* ---- 24- and 32-bit PCM: packed interleaved samples to and from .sela on the device ---------------------------
 * What a WAV file's data chunk or a capture buffer holds: little-endian interleaved samples of bytes_per_sample = 3 or 4 bytes,
 * [n_frames][samples_per_channel][channels].  (2-byte samples have had their calls all along: sela_hip_encode_n_device,
 * sela_hip_decode_n_device and the int16 host calls.)  Two kernels convert between that and the planar int32 of the i32 calls:
 *   sela_hip_pcm_unpack_device   packed -> d_samples int32 [n_frames][channels][samples_per_channel], sign-extended: what
 *     sela_hip_encode_i32_device, the paired calls and sela_hip_verify_i32_device take.
 *   sela_hip_pcm_pack_device     what sela_hip_decode_i32_device writes -- d_samples [n_frames][channels][stride], d_counts
 *     [n_frames * channels], d_sample_offsets [n_frames + 1] -- -> frame f interleaved at byte d_sample_offsets[f] * channels *
 *     bytes_per_sample of d_pcm_out, each sample its low bytes_per_sample bytes (the reference's writer, src/file/wav_file.cpp:262).
 *     A frame whose channels disagree about its length (a count other than d_sample_offsets[f + 1] - d_sample_offsets[f]), or
 *     that would end behind n_frames * stride samples, is not written: SELA_HIP_FLAG_BAD_FRAME into d_status[0] and one more in
 *     d_status[1].  With 3 bytes d_status[3] grows by the number of samples outside [-2^23, 2^23).  d_status[0] is read first:
 *     with SELA_HIP_FLAG_STRIDE in it nothing is written.  The call only ORs and adds: zero the words, or let a decode write them.
 * Every base pointer is 4-byte aligned (a 3-byte frame may still start at any byte of its buffer: frames are packed back to
 * back).  The kernels read only aligned dwords that hold at least one byte of their input -- never a byte beyond the page the
 * input ends in -- and write each byte of their output once and no other byte.
 *
 * The composed calls, asynchronous on `stream` like every device-pointer call (no allocation, no host synchronisation, no
 * host-side read of device data: a stream being captured into a HIP graph may take them):
 *   sela_hip_encode_pcm_device   the unpack into the workspace, then sela_hip_encode_i32_device_opt's launches on it: d_frames,
 *     d_frame_offsets and d_status are exactly that call's on the unpacked samples, sela_hip_encode_status_error() judges them.
 *     options: 0 or SELA_HIP_ENCODE_LOSSLESS.  d_workspace: sela_hip_encode_pcm_workspace_bytes(n_frames, channels,
 *     samples_per_channel) bytes -- the i32 call's and the samples'.
 *   sela_hip_decode_pcm_device   sela_hip_decode_i32_device's launches into the workspace, then the pack: the contract of
 *     sela_hip_decode_n_device's any-length route with a 3- or 4-byte container.  d_pcm_out has room for n_frames * stride * channels
 *     * bytes_per_sample bytes; nothing at or past that is written on any input, on success nothing at or past d_sample_offsets
 *     [n_frames] * channels * bytes_per_sample.  d_status [0..2] as sela_hip_decode_i32_device writes them -- SELA_HIP_FLAG_STRIDE
 *     exactly where that call raises it, and nothing is written then -- with the frames the pack refuses added; [3] the samples
 *     that did not fit a 3-byte container (their low bytes are written; 0 for 4 bytes).  d_workspace:
 *     sela_hip_decode_pcm_workspace_bytes(n_frames, channels, stride).
 *   sela_hip_decode_pcm_status_error   host only: sela_hip_decode_status_error()'s verdict on [0..2]; [3] is informational.
 *
 * sela_hip_encode_pcm_bound_bytes: room for every frame of such samples that the encoder does not refuse.  Nothing about a frame's
 * size follows from the container -- a residue is a sample minus a prediction, and a predictor of order up to 100 on quantised
 * coefficients may predict anything -- so the bound is the format's: the encoder refuses (SELA_HIP_ERANGE) a residue whose
 * zig-zag value u reaches 2^31 and a subframe of more than 65535 Rice words, and its Rice parameter is the minimum of bits(k),
 * convex in k = 0 .. 19, so never worse than k = 19: (u >> 19) + 20 <= 4115 bits a sample.  Per subframe that is the 12-byte
 * header, 32 coefficient words and min(65535, ceil(samples_per_channel * 4115 / 32)) residue words; per frame 4 bytes more.
 * (sela_hip_encode_bound_bytes_n promises 17-bit samples only; this is never smaller, and grows with each argument.)
 *
 * sela_hip_encode_pcm / sela_hip_decode_pcm: host pointers, synchronous.  The packed bytes travel -- 3 per sample of a 24-bit
 * container over the link, not 4 -- in chunks of whole frames that keep the device scratch bounded (as sela_hip_encode_i32's), on
 * the calling thread's leased context, past the coalescer; an open streaming job is left alone.  sela_hip_decode_pcm walks the
 * stream as sela_hip_decode does (sela_hip_index_samples); pcm_out holds pcm_cap bytes, of which sample_offsets[n_frames] *
 * channels * bytes_per_sample are written (fewer: SELA_HIP_ECAPACITY); *wide_samples (or NULL) receives status[3] of all chunks.
 *
 * SELA_HIP_EINVAL: a null pointer (d_sample_offsets of the decode may be NULL), bytes_per_sample other than 3 or 4, channels
 * outside 1..255, samples_per_channel outside 1..65535, stride 0, a base pointer that is not 4-byte aligned, n_frames x signals
 * per frame at 2^31 or more, an unknown option; SELA_HIP_ECAPACITY: a smaller workspace.  Nothing is enqueued then. */
size_t sela_hip_encode_pcm_workspace_bytes(uint32_t n_frames, uint32_t channels, uint32_t samples_per_channel);
size_t sela_hip_encode_pcm_bound_bytes(uint32_t n_frames, uint32_t channels, uint32_t samples_per_channel, uint32_t bytes_per_sample);
size_t sela_hip_decode_pcm_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride);
int sela_hip_pcm_unpack_device(const void* d_pcm, uint32_t bytes_per_sample, uint32_t n_frames, uint32_t channels, uint32_t samples_per_channel,
    int32_t* d_samples /* [n_frames][channels][samples_per_channel] */, void* stream);
int sela_hip_pcm_pack_device(const int32_t* d_samples /* [n_frames][channels][stride] */, const uint32_t* d_counts /* [n_frames * channels] */,
    const uint64_t* d_sample_offsets /* [n_frames + 1] */, uint32_t n_frames, uint32_t channels, uint32_t stride, uint32_t bytes_per_sample, void* d_pcm_out,
    uint32_t* d_status /* [4] */, void* stream);
int sela_hip_encode_pcm_device(const void* d_pcm, uint32_t bytes_per_sample, uint32_t n_frames, uint32_t channels, uint32_t samples_per_channel, uint32_t options,
    uint8_t* d_frames, size_t frames_cap, uint64_t* d_frame_offsets /* [n_frames + 1] */, uint32_t* d_status /* [4] */, void* d_workspace, size_t workspace_bytes,
    void* stream);
int sela_hip_decode_pcm_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride,
    uint32_t bytes_per_sample, void* d_pcm_out, uint64_t* d_sample_offsets /* [n_frames + 1] or NULL */, uint32_t* d_status /* [4] */, void* d_workspace,
    size_t workspace_bytes, void* stream);
int sela_hip_decode_pcm_status_error(const uint32_t* status /* [4], host copy */);
int sela_hip_encode_pcm(const void* pcm, uint32_t bytes_per_sample, uint32_t n_frames, uint32_t channels, uint32_t samples_per_channel, uint32_t options,
    uint8_t* frames_out, size_t frames_cap, uint64_t* frame_offsets_out /* [n_frames + 1] */);
int sela_hip_decode_pcm(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t bytes_per_sample, void* pcm_out,
    size_t pcm_cap /* bytes */, uint32_t* wide_samples /* or NULL */);

/* ---- verification against packed PCM: a 24- or 32-bit stream against the WAV's own bytes ---------------------------
 * sela_hip_verify_i32_device with the original read where a WAV or a capture buffer has it: little-endian interleaved samples of
 * bytes_per_sample = 3 or 4, the layout sela_hip_decode_pcm_device writes.  One compare kernel takes the packed bytes through
 * LDS; no unpacked copy of the original is made, and frames of different lengths (a whole-track tail, any-length frames) are
 * taken as they come.
 *   d_pcm          pcm_samples samples per channel; frame f starts at byte so[f] * channels * bytes_per_sample, so being
 *                  sela_hip_index_samples' sample offsets (a frame's first subframe says how long the frame is).  The base is
 *                  4-byte aligned; a frame may start at any byte phase.  Read only, and only as aligned dwords that hold at least
 *                  one byte of [0, pcm_samples * channels * bytes_per_sample) -- whatever the stream says: n_f is clamped to
 *                  stride and so[f] to pcm_samples before anything is addressed.
 *   With n_f = so[f + 1] - so[f], L_f = min(n_f, max(pcm_samples - so[f], 0)), m_c the count sela_hip_decode_i32_device reports
 *   for (f, c) and dec its samples:
 *   d_diff_counts  [n_frames]: the sum over the channels of #{ i < min(m_c, L_f) : dec[c][i] != the sign-extended original }
 *                  + |m_c - L_f|.  A decoded value outside 24 bits never equals a 3-byte original, even if its low bytes do.
 *   d_first_diff   [n_frames]: the smallest i * channels + c -- interleaved order relative to the frame, as
 *                  sela_hip_verify_device counts -- i being channel c's first differing index, or min(m_c, L_f) where only the
 *                  lengths differ; 0xFFFFFFFF where nothing differs.
 *   (Apart from the order of d_first_diff: sela_hip_verify_i32_device on the unpacked samples with d_lengths[f][c] = L_f.)
 *   d_sample_offsets [n_frames + 1] or NULL: the sample offsets, as sela_hip_decode_pcm_device leaves them.
 *   d_status uint32[4]: [0] and [1] exactly sela_hip_decode_i32_device's (SELA_HIP_FLAG_STRIDE included: nothing is compared
 *                  then); [2] the number of frames whose count is not 0; [3] zero.  sela_hip_decode_status_error() applies
 *                  unchanged; n_frames = 0 writes zero status words.
 * Asynchronous on `stream`: no allocation, no host synchronisation, no host-side read of device data -- capturable into a HIP
 * graph.  Nothing but the outputs named here and the workspace is written.
 * d_workspace: sela_hip_verify_pcm_workspace_bytes(n_frames, channels, stride) bytes, no initialisation (the payload call:
 * sela_hip_index_workspace_bytes(payload_bytes, max_frames) more).  With up(b) = b rounded up to a multiple of 256 and
 * tile = max((4096 / channels) & ~3, 4) samples it is
 *     sela_hip_decode_i32_workspace_bytes(max_frames, channels, stride)      the subframes as decoded, their records, the index
 *   + up(max_frames * channels * stride * 4)                                 the samples by channel, for frames of any other layout
 *   + up(max_frames * channels * 4)                                          ... and their counts
 *   + up(max(max_frames, 1) * 4)                                             a mark per frame: which way it went
 *   + up(max(max_frames * ceil(stride / tile), 1) * 8)                       two words per (frame, tile)
 *   + 256                                                                    the two control words
 *   + up((max_frames + 1) * 8)                                               the sample offsets of a caller that passes none
 * and SIZE_MAX where sela_hip_verify_i32_workspace_bytes() is, or for channels = 0.
 * Errors: sela_hip_verify_i32_device's, in its order; then SELA_HIP_EINVAL for bytes_per_sample other than 3 or 4, then for a
 * d_pcm that is not 4-byte aligned (d_sample_offsets: 8-byte).  Nothing is enqueued then; an argument error is found before a
 * device is asked for. */
size_t sela_hip_verify_pcm_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride);
int sela_hip_verify_pcm_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride,
    const void* d_pcm, uint32_t bytes_per_sample, uint64_t pcm_samples, uint32_t* d_diff_counts /* [n_frames] */, uint32_t* d_first_diff /* [n_frames] */,
    uint64_t* d_sample_offsets /* [n_frames + 1] or NULL */, uint32_t* d_status /* [4] */, void* d_workspace, size_t workspace_bytes, void* stream);
/* sela_hip_index_frames_device() and then the call above on the frames it found, on one stream: the count stays on the device.
 * Frames from *d_n_frames on are left alone (their entries in the two arrays are not written). */
int sela_hip_verify_payload_pcm_device(const uint8_t* d_payload, size_t payload_bytes, uint32_t max_frames, uint32_t channels, uint32_t stride,
    const void* d_pcm, uint32_t bytes_per_sample, uint64_t pcm_samples, uint32_t* d_diff_counts, uint32_t* d_first_diff, uint64_t* d_sample_offsets,
    uint64_t* d_frame_offsets, uint32_t* d_n_frames, uint32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream);
/* Host pointers, synchronous, in chunks of whole frames (3 bytes a sample travel for a 3-byte original): sela_hip_decode_i32's
 * checks in its order, the stride being the stream's own largest frame; 0: the arrays are valid.  *lossy_frames (or NULL): the
 * frames with a difference.  pcm needs no alignment.  Runs where sela_hip_verify_i32 runs: the calling thread's any-length context
 * and its own stream, past the coalescer; an open streaming job of the thread is left alone. */
int sela_hip_verify_pcm(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t bytes_per_sample,
    const void* pcm, uint64_t pcm_samples, uint32_t* diff_counts /* [n_frames] */, uint32_t* first_diff /* [n_frames] */, uint32_t* lossy_frames /* or NULL */);

/* ---- levels: how loud a stream is, per frame and channel -------------------------------------------------------
 * A track's peak, RMS and DC offset, and which of its frames are digital silence, without decoding it into memory: what
 * sela_hip_decode_n_device does, with a reduction where it stores -- on the 2048-sample route (up to eight channels) in one kernel
 * that writes no PCM at all.  Record [f][c] is taken over exactly the int16 values v that sela_hip_decode_n_device writes for
 * (frame f, channel c) with the same d_frames, d_frame_offsets, n_frames, channels and stride: its narrowing of wider samples, its
 * combine of difference subframes, its route, its zeros for a channel that ends early.  All four fields are integers and exact,
 * whatever the order of the additions: peak <= 32768 (|-32768|), |sum| <= 65535 * 32768 < 2^31, sum_squares <= 65535 * 2^30 < 2^46.
 * Scope: the domain of sela_hip_decode_n_device (16-bit output, frames of 0 .. 65535 samples, 1 .. 255 channels, the long last frame
 * of a whole-track stream included).  Samples of more than 16 bits are measured as that call narrows them, not as they are.
 *   d_levels       [n_frames][channels], 8-byte aligned.
 *   d_status uint32[4], written by the call: [0], [1] and [3] exactly as sela_hip_decode_n_device leaves them for the same frames;
 *                  [2] the number of frames in which some channel has peak != 0 (the largest samplesPerChannel is not reported
 *                  here: sela_hip_index_samples() or d_sample_offsets say it).
 *   sela_hip_decode_n_status_error() applies to [0], [1] and [3] unchanged; where it gives non-zero, or SELA_HIP_FLAG_STRIDE is
 *   set, d_levels is not defined.  n_frames = 0 writes zero status words (and d_sample_offsets[0] = 0 where given) and nothing else.
 * d_workspace: sela_hip_levels_workspace_bytes(n_frames, channels, stride) bytes, no initialisation (the payload call:
 * sela_hip_index_workspace_bytes(payload_bytes, max_frames) more); one call at a time may use it.  With up(b) = b rounded up to a
 * multiple of 256 the size is
 *     sela_hip_decode_n_workspace_bytes(max_frames, channels, stride)       the decode call's pieces, its alignment included
 *   + up(2 * max_frames * channels * stride)                                the int16 PCM of the routes that are not fused
 * and SIZE_MAX where sela_hip_verify_workspace_bytes() is, or for channels = 0.
 * Arguments, errors and their order are sela_hip_verify_device's (SELA_HIP_EINVAL: channels outside 1..255, stride 0, n_frames *
 * channels at 2^31 or more, a null pointer -- d_sample_offsets may be NULL, d_levels only where there are frames -- a d_levels
 * that is not 8-byte aligned, a null or misaligned d_frames / d_payload; SELA_HIP_ECAPACITY: a smaller workspace), found before any
 * device is asked for: nothing is enqueued then.  Asynchronous on `stream`, one serial chain: no allocation, no host wait, no
 * host read of device data, so a stream being captured into a HIP graph may take either call.  Apart from d_levels,
 * d_sample_offsets, d_status and the workspace (the payload call: its two index outputs too) nothing is written.
 * sela_hip_debug_standard_first routes the any-length kernels as it does for the decode call. */
typedef struct sela_hip_level { /* 24 bytes, 8-byte aligned */
    uint32_t peak;        /* max |v| over the frame's samples of this channel: 0 .. 32768 */
    uint32_t samples;     /* samples per channel of the frame: sample_offsets[f + 1] - sample_offsets[f] */
    int64_t sum;          /* sum of v */
    uint64_t sum_squares; /* sum of v * v */
} sela_hip_level;
size_t sela_hip_levels_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride);
int sela_hip_levels_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride,
    sela_hip_level* d_levels /* [n_frames][channels] */, uint64_t* d_sample_offsets /* [n_frames + 1] or NULL */, uint32_t* d_status /* [4] */,
    void* d_workspace, size_t workspace_bytes, void* stream);
/* sela_hip_index_frames_device() and then the call above on the frames it found, on one stream: the count stays on the device.
 * Frames from *d_n_frames on are left alone (their records are not written). */
int sela_hip_levels_payload_device(const uint8_t* d_payload, size_t payload_bytes, uint32_t max_frames, uint32_t channels, uint32_t stride,
    sela_hip_level* d_levels, uint64_t* d_sample_offsets, uint64_t* d_frame_offsets, uint32_t* d_n_frames, uint32_t* d_status, void* d_workspace,
    size_t workspace_bytes, void* stream);
/* Host pointers, synchronous, in chunks of frames: returns what sela_hip_decode returns for the stream (0: the records are
 * valid).  Runs where sela_hip_verify runs: the calling thread's any-length context and its own stream, past the coalescer; an
 * open streaming job of the thread is left alone.  n_frames = 0 returns 0 and asks for no device. */
int sela_hip_levels(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, sela_hip_level* levels /* [n_frames][channels] */);

/* ---- levels of 24- and 32-bit streams --------------------------------------------------------------------------
 * The calls above on the whole domain of sela_hip_decode_i32_device: samples of up to 32 bits, channels of different lengths,
 * every subframe layout that call takes.  What sela_hip_decode_i32_device does, with a reduction where it stores: record [f][c] is
 * taken over exactly samples_out[f][c][0 .. counts_out[f * channels + c]) as that call writes them for the same d_frames,
 * d_frame_offsets, n_frames, channels and stride -- difference subframes combined mod 2^32, a channel that no subframe names with a
 * count of 0 and so an all-zero record, a malformed frame with whatever counts that call writes.  Frames of the layouts this
 * project's encoders write are reduced from the subframes as decoded and no sample is stored; any other frame goes through the
 * decode call's combine into the workspace first.  All five fields are integers and exact, whatever the launch's shape:
 * peak <= 2^31 (|INT32_MIN|), |sum| <= 65535 * 2^31 < 2^47, sum of squares <= 65535 * 2^62 < 2^78, hence two words.
 *   d_levels       [n_frames][channels], 8-byte aligned.
 *   d_status uint32[4], written by the call: [0], [1] and [3] exactly as sela_hip_decode_i32_device leaves them for the same
 *                  frames; [2] the number of frames in which some channel has peak != 0 (the largest samplesPerChannel is not
 *                  reported here: sela_hip_index_samples() or d_sample_offsets say it).
 *   sela_hip_decode_status_error() applies to [0], [1] and [3] unchanged; with SELA_HIP_FLAG_STRIDE set d_levels is not defined.
 *   n_frames = 0 writes the status words (and d_sample_offsets[0] = 0 where given) and nothing else.
 * d_workspace: sela_hip_levels_i32_workspace_bytes(n_frames, channels, stride) bytes, no initialisation (the payload call:
 * sela_hip_index_workspace_bytes(payload_bytes, max_frames) more); one call at a time may use it.  The size is
 * sela_hip_verify_i32_workspace_bytes()'s with 32 bytes per (frame, slice of 4096 samples, channel) where that call has 8 bytes per
 * (frame, slice); it does not depend on the data, and is SIZE_MAX where sela_hip_verify_i32_workspace_bytes() is, or for channels = 0.
 * Arguments, errors and their order are sela_hip_levels_device's (SELA_HIP_EINVAL: channels outside 1..255, stride 0, n_frames *
 * channels at 2^31 or more, a null pointer -- d_sample_offsets may be NULL, d_levels only where there are frames -- a d_levels
 * that is not 8-byte aligned, a null or misaligned d_frames / d_payload; SELA_HIP_ECAPACITY: a smaller workspace), found before any
 * device is asked for: nothing is enqueued then.  Asynchronous on `stream`, one serial chain: no allocation, no host wait, no
 * host read of device data, so a stream being captured into a HIP graph may take any of these calls.  Apart from d_levels,
 * d_sample_offsets, d_status and the workspace (the payload call: its two index outputs too) nothing is written, and no byte of
 * d_levels beyond [n_frames][channels]. */
typedef struct sela_hip_level32 { /* 32 bytes, 8-byte aligned */
    uint32_t peak;           /* max |v| over the channel's samples of the frame: 0 .. 2^31 */
    uint32_t samples;        /* the channel's samples in the frame: counts_out[f * channels + c] */
    int64_t sum;             /* sum of v */
    uint64_t sum_squares_lo; /* sum of v * v, bits 0 .. 63 */
    uint64_t sum_squares_hi; /* sum of v * v, bits 64 .. 127 */
} sela_hip_level32;
size_t sela_hip_levels_i32_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride);
int sela_hip_levels_i32_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride,
    sela_hip_level32* d_levels /* [n_frames][channels] */, uint64_t* d_sample_offsets /* [n_frames + 1] or NULL */, uint32_t* d_status /* [4] */,
    void* d_workspace, size_t workspace_bytes, void* stream);
/* sela_hip_index_frames_device() and then the call above on the frames it found, on one stream: the count stays on the device.
 * Frames from *d_n_frames on are left alone (their records are not written). */
int sela_hip_levels_payload_i32_device(const uint8_t* d_payload, size_t payload_bytes, uint32_t max_frames, uint32_t channels, uint32_t stride,
    sela_hip_level32* d_levels, uint64_t* d_sample_offsets, uint64_t* d_frame_offsets, uint32_t* d_n_frames, uint32_t* d_status, void* d_workspace,
    size_t workspace_bytes, void* stream);
/* The same records from planar int32 samples that already lie in device memory -- sela_hip_pcm_unpack_device's output ahead of an
 * encode, or a decode's output: record [f][c] over d_samples[f][c][0 .. min(d_counts[f * channels + c], stride)), d_counts NULL:
 * stride samples each.  d_samples and d_counts 4-byte aligned (rows at multiples of 16 bytes are read 16 bytes at a time).
 * d_status: [2] as above, the other words zeroed.  d_workspace: sela_hip_levels_samples_i32_workspace_bytes(n_frames, channels,
 * stride) bytes (the partial records alone).  Errors as above, without a stream of frames. */
size_t sela_hip_levels_samples_i32_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride);
int sela_hip_levels_samples_i32_device(const int32_t* d_samples /* [n_frames][channels][stride] */, const uint32_t* d_counts /* [n_frames * channels] or NULL */,
    uint32_t n_frames, uint32_t channels, uint32_t stride, sela_hip_level32* d_levels, uint32_t* d_status /* [4] */, void* d_workspace, size_t workspace_bytes,
    void* stream);
/* Host pointers, synchronous, in chunks of frames with the stream's largest samplesPerChannel for a stride: returns what
 * sela_hip_decode_i32 returns for the stream (0: the records are valid).  Runs where sela_hip_verify_i32 runs: the calling thread's
 * any-length context and its own stream, past the coalescer; an open streaming job of the thread is left alone.  n_frames = 0
 * returns 0 and asks for no device. */
int sela_hip_levels_i32(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, sela_hip_level32* levels /* [n_frames][channels] */);

/* ---- digest: the CRC-32 of the PCM a stream decodes to ------------------------------------------------------------
 * "Does this stream still decode to that audio?", asked without holding the audio: the CRC-32 everybody computes (IEEE 802.3,
 * reflected polynomial 0xEDB88320, initial value and final XOR 0xFFFFFFFF: zlib.crc32, `crc32`, `cksum -a crc32`) of the bytes
 * sela_hip_decode_n_device writes, without writing them -- on the 2048-sample route (up to eight channels) in one kernel that
 * stores no PCM at all.  Scope: the domain of sela_hip_decode_n_device (16-bit interleaved output, frames of 0 .. 65535 samples,
 * 1 .. 255 channels, the long last frame of a whole-track stream included).
 *   d_digests[f]   .crc32: the CRC-32 of exactly the samples * channels * 2 bytes sela_hip_decode_n_device writes for frame f with
 *                  the same d_frames, d_frame_offsets, n_frames, channels and stride (little-endian int16, interleaved: its
 *                  narrowing of wider samples, its combine of difference subframes, its route, its zeros for a channel that ends
 *                  early); .samples: sample_offsets[f + 1] - sample_offsets[f].  A frame of 0 samples has crc32 0.  8-byte aligned.
 *   d_track        uint64[2], 8-byte aligned, not NULL: [0] (its low 32 bits; the high ones 0) the CRC-32 of all frames' bytes in
 *                  order, [1] their number.  For a stream of whole frames [0] is zlib.crc32 of the WAV data chunk a decode of the
 *                  file writes; for a whole-track (keep-tail) file that of the whole original data chunk, where the file decodes
 *                  losslessly.  Written on the device from the records: crc(A | B) = crc(A) * x^(8 |B|) ^ crc(B) in GF(2)[x] mod P.
 *   d_status uint32[4], written by the call: [0], [1] and [3] exactly as sela_hip_decode_n_device leaves them for the same frames;
 *                  [2] is 0.  sela_hip_decode_n_status_error() applies unchanged; where it gives non-zero, or SELA_HIP_FLAG_STRIDE
 *                  is set, the records and d_track are not defined.  n_frames = 0 writes the status words, d_track = {0, 0} (and
 *                  d_sample_offsets[0] = 0 where given) and nothing else.
 * d_workspace: sela_hip_digest_workspace_bytes(n_frames, channels, stride) bytes, no initialisation (the payload call:
 * sela_hip_index_workspace_bytes(payload_bytes, max_frames) more); one call at a time may use it.  With up(b) = b rounded up to a
 * multiple of 256 the size is
 *     sela_hip_levels_workspace_bytes(max_frames, channels, stride)                        the levels call's two pieces, its alignment included
 *   + up(4 * max(max_frames * ceil(2 * channels * stride / 32768), 1))                     a word per (frame, slice of 32 KiB of its PCM)
 *   + up(4 * min(max(ceil(max_frames / 256), 1), 256))                                     the track fold's word per workgroup
 * and SIZE_MAX where sela_hip_levels_workspace_bytes() is.
 * Arguments, errors and their order are sela_hip_levels_device's (SELA_HIP_EINVAL: channels outside 1..255, stride 0, n_frames *
 * channels at 2^31 or more, a null pointer -- d_sample_offsets may be NULL, d_digests only where there are frames, d_track never
 * -- a d_digests or d_track that is not 8-byte aligned, a null or misaligned d_frames / d_payload; SELA_HIP_ECAPACITY: a smaller
 * workspace), found before any device is asked for: nothing is enqueued then.  Asynchronous on `stream`, one serial chain: no
 * allocation, no host wait, no host read of device data, so a stream being captured into a HIP graph may take either call.
 * Apart from d_digests[0 .. n_frames), d_track, d_sample_offsets, d_status and the workspace (the payload call: its two index
 * outputs too) nothing is written.  The 24- and 32-bit family (sela_hip_decode_pcm_device's bytes): sela_hip_digest_pcm_device, below.
 * (The record's struct tag and the host call share a name, so C++ code says `struct sela_hip_digest`; sela_hip_digest_record
 * names the type in both languages.) */
struct sela_hip_digest { /* 8 bytes */
    uint32_t crc32;   /* CRC-32 of the frame's interleaved int16 bytes */
    uint32_t samples; /* samples per channel of the frame */
};
typedef struct sela_hip_digest sela_hip_digest_record;
size_t sela_hip_digest_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride);
int sela_hip_digest_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride,
    struct sela_hip_digest* d_digests /* [n_frames] */, uint64_t* d_track /* [2] */, uint64_t* d_sample_offsets /* [n_frames + 1] or NULL */,
    uint32_t* d_status /* [4] */, void* d_workspace, size_t workspace_bytes, void* stream);
/* sela_hip_index_frames_device() and then the call above on the frames it found, on one stream: the count stays on the device.
 * Frames from *d_n_frames on are left alone (their records are not written); d_track covers the frames found. */
int sela_hip_digest_payload_device(const uint8_t* d_payload, size_t payload_bytes, uint32_t max_frames, uint32_t channels, uint32_t stride,
    struct sela_hip_digest* d_digests, uint64_t* d_track, uint64_t* d_sample_offsets, uint64_t* d_frame_offsets, uint32_t* d_n_frames, uint32_t* d_status,
    void* d_workspace, size_t workspace_bytes, void* stream);
/* Host pointers, synchronous, in chunks of frames whose track words are folded on the host with sela_hip_crc32_combine(): returns
 * what sela_hip_decode returns for the stream (0: the records and the two track figures are valid; digests, track_crc32 and
 * track_bytes may each be NULL).  Runs where sela_hip_levels runs: the calling thread's any-length context and its own stream, past
 * the coalescer; an open streaming job of the thread is left alone.  n_frames = 0 gives 0 / 0 and asks for no device. */
int sela_hip_digest(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, struct sela_hip_digest* digests /* [n_frames] or NULL */,
    uint32_t* track_crc32, uint64_t* track_bytes);
/* crc32(A | B) from crc32(A), crc32(B) and the length of B in bytes, any length: zlib's crc32_combine.  Pure host arithmetic. */
uint32_t sela_hip_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);
/* The same lanes, waves and folds on bytes that already lie in device memory -- a capture buffer, a WAV's data chunk, a decode's
 * output: d_out[0] = the CRC-32 of d_bytes[0 .. n_bytes), d_out[1] = n_bytes; any length, any alignment of d_bytes (d_out: 8-byte).
 * d_workspace: sela_hip_crc32_workspace_bytes(n_bytes) bytes (a word per slice of max(32 KiB, n_bytes / 4096), so at most 17 KiB).
 * SELA_HIP_EINVAL: d_out or d_workspace NULL, d_bytes NULL with n_bytes != 0, a misaligned d_out; SELA_HIP_ECAPACITY: a smaller
 * workspace.  Asynchronous on `stream`, two launches, capturable; only d_out and the workspace are written. */
size_t sela_hip_crc32_workspace_bytes(uint64_t n_bytes);
int sela_hip_crc32_device(const void* d_bytes, uint64_t n_bytes, uint64_t* d_out /* [2] */, void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- digest of 24- and 32-bit streams: the CRC-32 of the packed PCM they decode to ---------------------------------
 * The digest above on the domain of sela_hip_decode_pcm_device: samples of up to 32 bits in a container of bytes_per_sample = 3 or
 * 4 bytes, frames of any length, every subframe layout that call takes.  What sela_hip_decode_pcm_device does, with a CRC where it
 * stores: frames of the layouts this project's encoders write are taken from the subframes as decoded, packed in LDS and digested
 * there -- no decoded byte reaches memory; any other frame goes through the decode call's combine into the workspace first.
 *   d_digests[f]   .crc32: the CRC-32 of exactly the samples * channels * bytes_per_sample bytes sela_hip_decode_pcm_device writes
 *                  for frame f with the same d_frames, d_frame_offsets, n_frames, channels, stride and bytes_per_sample (little-
 *                  endian, interleaved, each sample's low bytes_per_sample bytes, difference subframes combined mod 2^32);
 *                  .samples: sample_offsets[f + 1] - sample_offsets[f].  A frame of 0 samples has crc32 0.  8-byte aligned; the
 *                  record is the one above.
 *   d_track        uint64[2], 8-byte aligned, not NULL: [0] (its low 32 bits; the high ones 0) the CRC-32 of all frames' bytes in
 *                  order, [1] their number, sample_offsets[n_frames] * channels * bytes_per_sample.  For a lossless file that is
 *                  zlib.crc32 of the WAV data chunk it was made from (cut to whole frames unless the tail was kept).
 *   d_status uint32[4], written by the call: exactly what sela_hip_decode_pcm_device leaves for the same frames -- [0] and [1] with
 *                  SELA_HIP_FLAG_STRIDE, SELA_HIP_FLAG_BAD_FRAME and the frames its pack refuses (channels that disagree about
 *                  the frame's length) as there, [2] the largest samplesPerChannel, [3] the samples of digested frames outside
 *                  [-2^23, 2^23) with a 3-byte container (their low three bytes are digested), 0 with 4 bytes.
 *                  sela_hip_decode_pcm_status_error() applies unchanged; where it gives non-zero, or SELA_HIP_FLAG_STRIDE is set,
 *                  the records and d_track are not defined.  n_frames = 0 writes the status words, d_track = {0, 0} (and
 *                  d_sample_offsets[0] = 0 where given) and nothing else.
 * d_workspace: sela_hip_digest_pcm_workspace_bytes(n_frames, channels, stride) bytes, no initialisation (the payload call:
 * sela_hip_index_workspace_bytes(payload_bytes, max_frames) more); one call at a time may use it.  With up(b) = b rounded up to a
 * multiple of 256 and tile = max((4096 / channels) & ~3, 4) samples it is
 *     sela_hip_decode_i32_workspace_bytes(max_frames, channels, stride)      the subframes as decoded, their records, the index
 *   + up(max_frames * channels * stride * 4)                                 the samples by channel, for frames of any other layout
 *   + up(max_frames * channels * 4)                                          ... and their counts
 *   + up(max(max_frames, 1) * 4)                                             a mark per frame: which way it went
 *   + up(max(max_frames * ceil(stride / tile), 1) * 8)                       the raw CRC per (frame, tile): a word of the verify call's two
 *   + 256                                                                    the two control words
 *   + up((max_frames + 1) * 8)                                               the sample offsets of a caller that passes none
 *   + up(4 * min(max(ceil(max_frames / 256), 1), 256))                       the track fold's word per workgroup
 * -- sela_hip_verify_pcm_workspace_bytes() and the last line -- and SIZE_MAX where sela_hip_verify_pcm_workspace_bytes() is.
 * Arguments, errors and their order are sela_hip_digest_device's (SELA_HIP_EINVAL: channels outside 1..255, stride 0, n_frames *
 * channels at 2^31 or more, a null pointer -- d_sample_offsets may be NULL, d_digests only where there are frames, d_track never
 * -- a d_digests or d_track that is not 8-byte aligned); then SELA_HIP_EINVAL for bytes_per_sample other than 3 or 4 and for a
 * d_sample_offsets that is not 8-byte aligned, then for a null or misaligned d_frames / d_payload; SELA_HIP_ECAPACITY: a smaller
 * workspace.  All are found before any device is asked for: nothing is enqueued then.  Asynchronous on `stream`, one serial chain:
 * no allocation, no host wait, no host read of device data, so a stream being captured into a HIP graph may take either call.
 * Apart from d_digests[0 .. n_frames), d_track, d_sample_offsets, d_status and the workspace (the payload call: its two index
 * outputs too) nothing is written. */
size_t sela_hip_digest_pcm_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride);
int sela_hip_digest_pcm_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride,
    uint32_t bytes_per_sample, struct sela_hip_digest* d_digests /* [n_frames] */, uint64_t* d_track /* [2] */,
    uint64_t* d_sample_offsets /* [n_frames + 1] or NULL */, uint32_t* d_status /* [4] */, void* d_workspace, size_t workspace_bytes, void* stream);
/* sela_hip_index_frames_device() and then the call above on the frames it found, on one stream: the count stays on the device.
 * Frames from *d_n_frames on are left alone (their records are not written); d_track covers the frames found. */
int sela_hip_digest_payload_pcm_device(const uint8_t* d_payload, size_t payload_bytes, uint32_t max_frames, uint32_t channels, uint32_t stride,
    uint32_t bytes_per_sample, struct sela_hip_digest* d_digests, uint64_t* d_track, uint64_t* d_sample_offsets, uint64_t* d_frame_offsets, uint32_t* d_n_frames,
    uint32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream);
/* Host pointers, synchronous, in chunks of frames with the stream's largest samplesPerChannel for a stride; each chunk's track words
 * and status[3] come back with its status and are folded on the host (sela_hip_crc32_combine): returns what sela_hip_decode_pcm
 * returns for the stream (0: the records and the three figures are valid; digests, track_crc32, track_bytes and wide_samples may
 * each be NULL).  Runs where sela_hip_levels_i32 runs: the calling thread's any-length context and its own stream, past the
 * coalescer; an open streaming job of the thread is left alone.  n_frames = 0 gives 0 / 0 / 0 and asks for no device. */
int sela_hip_digest_pcm(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t bytes_per_sample,
    struct sela_hip_digest* digests /* [n_frames] or NULL */, uint32_t* track_crc32, uint64_t* track_bytes, uint32_t* wide_samples);

/* ---- a whole track from packed 3- or 4-byte PCM: the tail of a 24- or 32-bit file kept ----------------------------
 * sela_hip_encode_whole* ("a whole track", above) for the containers of sela_hip_encode_pcm*: d_pcm is little-endian interleaved
 * [N][channels] samples of bytes_per_sample = 3 or 4 bytes.  The layout rule is the one sela_hip_whole_frames / sela_hip_whole_frame
 * define.  With F = N / 2048 and t = N % 2048: frames 0 .. F - 2 are byte for byte what sela_hip_encode_pcm_device writes for them at
 * samples_per_channel = 2048 with the same options; the last frame is byte for byte what that call writes for one frame of 2048 + t
 * samples (frame::FrameEncoder's for a frame of that length, the per-frame stereo decision included); N < 2048 gives one frame of
 * N samples; t == 0 the plain call's stream; N == 0 writes d_frame_offsets[0] = 0 and zero status words.
 *   sela_hip_encode_whole_pcm_bound_bytes      (F - 1) * sela_hip_encode_pcm_bound_bytes(1, channels, 2048, bytes_per_sample)
 *                                              + sela_hip_encode_pcm_bound_bytes(1, channels, the last frame's length,
 *                                              bytes_per_sample); SIZE_MAX beyond size_t, 0 for what the call refuses or N == 0.
 *   sela_hip_encode_whole_pcm_workspace_bytes  the device call's workspace for every track of at most max_samples samples per
 *                                              channel; it does not depend on the data or the device.  With F = the frames of
 *                                              max_samples, last = min(max(max_samples, 1), 4095) and up(b) = b rounded up to a
 *                                              multiple of 256 it is
 *                                                up(4 * F * 2048 * channels) + sela_hip_encode_i32_workspace_bytes(F, channels, 2048)
 *                                              + up(4 * last * channels) + sela_hip_encode_i32_workspace_bytes(1, channels, last)
 *                                              + up(sela_hip_encode_pcm_bound_bytes(1, channels, last, 4)) + 256 + 256
 *                                              (the 2048-sample frames unpacked and their encoder's workspace, the same for the
 *                                              last frame, that frame as coded, its offsets and status words, alignment);
 *                                              SIZE_MAX for what the call refuses.
 * sela_hip_encode_whole_pcm_device: d_pcm and d_frames 4-byte aligned; d_frame_offsets [frames + 1]; d_status uint32[4]; options: 0
 *   or SELA_HIP_ENCODE_LOSSLESS.  Offsets, status words and the capacity rule are sela_hip_encode_whole_device's: the offsets are
 *   always written in full; a frame that ends beyond frames_cap is counted in d_status[1] and not written, and nothing at or past
 *   frames_cap is; sela_hip_encode_status_error() judges the status words.  Asynchronous on `stream` and capturable: no allocation,
 *   no host wait, no host read of device data.  Launches: the unpack and the any-length encoder's three on frames 0 .. F - 2, into
 *   and out of the workspace, on `stream`; the last frame's own unpack -- its packed bytes start at byte (F - 1) * 2048 * channels *
 *   bytes_per_sample, a multiple of 4 -- and three encode launches on a stream of the library's own between two events (forked from
 *   `stream` before the main launches, joined behind them; inside a capture the side stream joins the capture and leaves it at the
 *   join), coded into the workspace; then the splice of sela_hip_encode_whole_device on `stream`.  With t == 0, or a single frame,
 *   only the one call it is, on `stream`.
 *   SELA_HIP_EINVAL, in this order: bytes_per_sample other than 3 or 4, channels outside 1..255, frames x signals per frame at 2^31
 *   or more, an unknown option, a null pointer (d_pcm and d_frames only where N > 0), a misaligned d_pcm or d_frames;
 *   SELA_HIP_ECAPACITY: a smaller workspace.  They are found before a device is asked for, and nothing is enqueued.
 * sela_hip_encode_whole_pcm: the same stream from HOST pointers, synchronous.  Frames 0 .. F - 2 go where sela_hip_encode_pcm codes
 *   them, in chunks of whole frames with the packed bytes travelling; the last frame is one more chunk of its own length on the
 *   same leased context.  Errors are sela_hip_encode_pcm's (SELA_HIP_ECAPACITY: frames_out too small; frame_offsets_out is not
 *   defined then).  A thread's open streaming job is left alone. */
size_t sela_hip_encode_whole_pcm_bound_bytes(uint64_t n_samples, uint32_t channels, uint32_t bytes_per_sample);
size_t sela_hip_encode_whole_pcm_workspace_bytes(uint64_t max_samples, uint32_t channels);
int sela_hip_encode_whole_pcm_device(const void* d_pcm, uint32_t bytes_per_sample, uint64_t n_samples, uint32_t channels, uint32_t options,
    uint8_t* d_frames, size_t frames_cap, uint64_t* d_frame_offsets /* [frames + 1] */, uint32_t* d_status /* [4] */,
    void* d_workspace, size_t workspace_bytes, void* stream);
int sela_hip_encode_whole_pcm(const void* pcm, uint32_t bytes_per_sample, uint64_t n_samples, uint32_t channels, uint32_t options,
    uint8_t* frames_out, size_t frames_cap, uint64_t* frame_offsets_out /* [frames + 1] */);

/* ---- streaming jobs (host pointers) -------------------------------------------------------------------
 * For callers that produce their input piece by piece (a file being read): feed() enqueues a piece and
 * returns at once -- from page-locked buffers nothing in it waits for the device (an encode feed is one kernel
 * launch; a decode feed waits when one of its eight chunk buffer sets comes round again) -- so the caller's next
 * read runs beside the device work.  A piece's buffer must stay valid and unchanged until the job reports its
 * frames final (or ends).  Pieces -- and a decode job's pcm_out -- in ordinary (pageable) memory go through page-locked
 * bounce buffers of the library (one more host copy: slower, same results).  One open job per calling thread; a job is
 * used from the thread that began it.
 * An encode feed normally has its PCM fetched by a staging kernel beside the encode launch.  If the device is so busy
 * with other work that the two cannot run side by side within the launch's bounded wait (or another thread's job on
 * this device is using that path), the feed -- and any queued behind it -- is issued again with the copy engine in
 * place of the staging kernel: a busy device costs time, never the result.
 *
 * encode: the job appends to frames_out (capacity frames_cap) and fills frame_offsets_out[0 .. total_frames];
 * *frames_final / *bytes_final (optional) report how much of both is complete in host memory, so a writer can
 * drain finished bytes to disk while later pieces are still being encoded (src/file/sela_file.cpp:105-137 is
 * what it replaces).  end() waits for everything, reports the totals, and frees the job -- also after an error.
 * decode: pieces are whole frames (frame_offsets[0 .. n_frames] index into `frames`); pcm_out fills in order.
 * Errors are those of the one-shot calls. */
typedef struct sela_hip_job sela_hip_job;
int sela_hip_encode_begin(sela_hip_job** job, uint32_t channels, uint32_t total_frames, uint8_t* frames_out, size_t frames_cap,
    uint64_t* frame_offsets_out /* [total_frames + 1] */);
/* (options: see "encode options" above; they hold for every feed of the job) */
int sela_hip_encode_begin_opt(sela_hip_job** job, uint32_t channels, uint32_t total_frames, uint8_t* frames_out, size_t frames_cap,
    uint64_t* frame_offsets_out /* [total_frames + 1] */, uint32_t options);
int sela_hip_encode_feed(sela_hip_job* job, const int16_t* pcm, uint32_t n_frames, uint32_t* frames_final, uint64_t* bytes_final);
int sela_hip_encode_end(sela_hip_job* job, uint32_t* frames_final, uint64_t* bytes_final);
int sela_hip_decode_begin(sela_hip_job** job, uint32_t channels, uint32_t total_frames, int16_t* pcm_out);
int sela_hip_decode_feed(sela_hip_job* job, const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t* frames_final);
int sela_hip_decode_end(sela_hip_job* job, uint32_t* frames_final);

/* Walk a frame byte stream on the host and fill frame_offsets[0..n_frames]; stops at the first bad
 * sync word like src/file/sela_file.cpp:54-56.  Returns the number of frames found (<= n_frames). */
uint32_t sela_hip_index_frames(const uint8_t* frames, size_t frames_bytes, uint32_t n_frames, uint32_t channels,
    uint64_t* frame_offsets);

/* ---- salvage: the frames of a damaged payload ------------------------------------------------
 * sela_hip_index_frames() and its device form stop silently at the first position that fails their test; every call that
 * reads a payload decodes only what that walk found.  The salvage walk goes on past such a position.  For a payload of B
 * bytes let W = B / 4 (integer division) and C = channels:
 *   candidate   a word index w < W whose word is the sync word and whose C subframe headers, read with sela_format.h's
 *               reader and bound B, all fit: sela_hip_index_frames()'s test of a position.  end(w) is the byte where that frame
 *               would end, always a multiple of 4;
 *   confirmed   a candidate with end(w) == 4 W, or with end(w) / 4 itself a candidate: a true frame followed by an intact
 *               frame or by the end of the payload is one, a sync word met by chance in Rice data or in garbage almost never;
 *   the walk    starts at p = 0 with no frame taken.  While fewer than max_frames frames are taken: if p / 4 is a candidate, it
 *               is taken (the position is trusted: offset 0, or the end of a taken frame); otherwise the smallest confirmed
 *               candidate q with 4 q >= p is taken with skipped_before = 4 q - p, and if there is none the walk ends.
 *               Then p = end(taken).
 * Per taken frame one record; totals[0] = frames taken, [1] = records with skipped_before > 0, [2] = sum of bytes,
 * [3] = offset + bytes of the last record (0 without one): B - totals[3] bytes lie behind the last frame.
 * What follows from the rule:
 *   - where sela_hip_index_frames() finds n frames, the first n records are those frames with skipped_before == 0: on an
 *     intact payload the salvage is the index;
 *   - offsets strictly increase and frames never overlap;
 *   - the taken frames written back to back form a payload on which sela_hip_index_frames() finds exactly those frames and
 *     ends at its last byte; salvaging that payload again takes the same frames with no gap.
 * Its limits, as they are:
 *   - only word positions relative to the payload are looked at (as in sela_hip_index_frames_device): damage that inserts
 *     or deletes a number of bytes that is not a multiple of 4 loses everything behind it;
 *   - an intact frame whose predecessor was not taken AND whose successor's header is damaged is neither trusted nor
 *     confirmed, and is not recovered;
 *   - a trusted frame whose damaged length fields still pass the bounds sends the walk to the wrong place; it
 *     resynchronises from there;
 *   - a chance sync word whose headers fit and whose end lands on a candidate is confirmed, and is taken when the walk is
 *     searching at or before it.
 * Whether a taken frame's CONTENTS are sound is not judged here: that is the decoders' flags', sela_hip_verify*'s and
 * sela_hip_digest*'s business. */
typedef struct sela_hip_salvaged { /* 24 bytes, 8-byte aligned */
    uint64_t offset;         /* of the frame in the payload, a multiple of 4 (any byte from the *_unaligned calls) */
    uint64_t skipped_before; /* bytes between the end of the frame before (or offset 0) and this one */
    uint32_t bytes;          /* the frame's length, a multiple of 4 */
    uint32_t reserved;       /* 0 */
} sela_hip_salvaged;
/* The walk on the host: pure CPU, no device needed, any alignment of `payload`.  records: [max_frames], entries
 * [0 .. the count) are written (NULL: none); totals: uint64 [4] (or NULL).  channels outside 1..255: no frame.  Returns
 * the number of frames taken. */
uint32_t sela_hip_salvage_frames(const uint8_t* payload, size_t payload_bytes, uint32_t max_frames, uint32_t channels,
    sela_hip_salvaged* records, uint64_t* totals);
/*
 * The same walk on the device: d_records and d_totals receive exactly what sela_hip_salvage_frames() writes for the same
 * bytes, for every input; entries beyond totals[0] are not written.  d_payload must be 4-byte aligned.  Asynchronous on
 * `stream`, no allocation, no host synchronisation, no host read of device data; the launches are shaped by payload_bytes
 * and max_frames alone (a stream being captured into a graph may take it): 8 + ceil(log2(max_frames)) kernel launches;
 * one for a payload without a word or a max_frames of 0.
 * d_workspace: sela_hip_salvage_workspace_bytes(payload_bytes, max_frames) bytes, no initialisation.  With W =
 * payload_bytes / 4, K = ceil(W / 4096), F = min(max_frames, W) and up(b) = b rounded up to a multiple of 256 it is
 *   9 up(4 W) + 2 up(4 (K + 1)) + 3 up(4 F) + 5 * 256 + 256
 * bytes: the index's six arrays of one uint32 per payload word, three more, a word per 4096 candidates twice, three uint32
 * per frame, five single words, and the base's alignment.
 * SELA_HIP_EINVAL: channels outside 1..255, a null pointer, a misaligned d_payload, a payload of 16 GiB or more;
 * SELA_HIP_ECAPACITY: a smaller workspace -- sela_hip_index_frames_device()'s cases and codes, found before anything is
 * enqueued.
 */
size_t sela_hip_salvage_workspace_bytes(size_t payload_bytes, uint32_t max_frames);
int sela_hip_salvage_frames_device(const uint8_t* d_payload, size_t payload_bytes, uint32_t max_frames, uint32_t channels,
    sela_hip_salvaged* d_records /* [max_frames] */, uint64_t* d_totals /* [4] */, void* d_workspace, size_t workspace_bytes,
    void* stream);
/*
 * The walk, then the taken frames copied back to back into d_out (one more launch): d_frame_offsets[0 .. totals[0]] are
 * their offsets there, ready for every *_device call that takes frames with their offsets.  d_records may be NULL.
 * A frame that ends beyond out_cap is counted and given its offsets but not written, and neither is any frame behind it:
 * no byte of d_out at or behind the first such frame's offset is written.  The caller reads the room needed from
 * d_frame_offsets[totals[0]] (== totals[2]), as with the encoders.  d_out is 4-byte aligned and does not overlap the
 * payload (SELA_HIP_EINVAL).  Workspace, asynchrony and the other errors: as the call above.
 */
int sela_hip_salvage_payload_device(const uint8_t* d_payload, size_t payload_bytes, uint32_t max_frames, uint32_t channels,
    uint8_t* d_out, size_t out_cap, uint64_t* d_frame_offsets /* [max_frames + 1] */, sela_hip_salvaged* d_records /* [max_frames] or NULL */,
    uint64_t* d_totals /* [4] */, void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- salvage at any byte: frames behind inserted or deleted bytes -------------------------------------------------
 * The salvage above looks at word positions only.  These calls are its rule with "word" replaced by "byte": a frame is still a
 * multiple of 4 bytes long, but it may start at any byte of the payload.  For a payload of B bytes and C = channels:
 *   candidate   a byte offset b with b + 4 <= B whose four bytes are the sync word (little endian) and whose C subframe
 *               headers, read with sela_format.h's byte reader and bound B, all fit.  end(b) is the byte where that frame would
 *               end: b plus a multiple of 4;
 *   confirmed   a candidate with B - end(b) < 4, or with end(b) itself a candidate.  (Where end(b) is a multiple of 4 the first
 *               is the word rule's "end(w) == 4 W".);
 *   the walk    starts at p = 0 with no frame taken.  While fewer than max_frames frames are taken: if p is a candidate, it is
 *               taken as it stands (the position is trusted: offset 0, or the end of a taken frame; skipped_before = 0);
 *               otherwise the smallest confirmed candidate b >= p is taken with skipped_before = b - p, and if there is none
 *               the walk ends.  Then p = end(taken).
 * Records and totals are the salvage's above; `offset` and `skipped_before` are any byte count, `bytes` a multiple of 4.
 * What follows from the rule:
 *   - where sela_hip_index_frames() finds n frames, the first n records are those frames with skipped_before == 0;
 *   - offsets strictly increase and frames never overlap;
 *   - the taken frames written back to back form a payload that sela_hip_index_frames() reads to its last byte, and that
 *     both salvages take whole with no gap;
 *   - on a payload of intact frames with garbage that holds no sync word, of any byte length, put between frames, every frame
 *     is taken; the frames may sit at different phases.
 * Its limits, as they are:
 *   - a trusted frame whose length fields are wrong still sends the walk to the wrong place: where bytes were deleted INSIDE a
 *     frame, that frame is taken with its neighbour's head in it, and the neighbour is lost;
 *   - an intact frame whose predecessor was not taken AND whose successor's header is damaged is still missed;
 *   - a chance sync word, at any byte now, whose headers fit and whose end lands on a candidate is confirmed, and is taken when
 *     the walk is searching at or before it.
 * The host walk: pure CPU, any alignment of `payload`; arguments and result as sela_hip_salvage_frames(). */
uint32_t sela_hip_salvage_frames_unaligned(const uint8_t* payload, size_t payload_bytes, uint32_t max_frames, uint32_t channels,
    sela_hip_salvaged* records, uint64_t* totals);
/*
 * The same walk on the device, and the walk with the copy: arguments, outputs, out_cap, asynchrony, launch count, argument checks,
 * their order and their codes are sela_hip_salvage_frames_device()'s and sela_hip_salvage_payload_device()'s, with two differences.
 * Positions are uint32 BYTE offsets here, so a payload_bytes of 2^32 or more is SELA_HIP_EINVAL.  And no byte at or behind
 * d_payload + payload_bytes is read although the last bytes of a payload whose length is no multiple of 4 matter (a frame may
 * end there): they are read as bytes, never as a word that reaches past the end.  d_payload and d_out stay 4-byte aligned and
 * apart; the compacted payload in d_out is made of whole frames, so every *_device call reads it as it stands.
 * d_workspace: sela_hip_salvage_unaligned_workspace_bytes(payload_bytes, max_frames) bytes, no initialisation.  The sync word
 * cannot overlap itself, so at most one candidate starts inside any aligned word and the workspace stays one entry per WORD: with
 * W = payload_bytes / 4, K = ceil(W / 4096), F = min(max_frames, W) and up(b) = b rounded up to a multiple of 256 it is
 *   9 up(4 W) + 2 up(4 (K + 1)) + 3 up(4 F) + 5 * 256 + 256
 * bytes, sela_hip_salvage_workspace_bytes()'s formula.
 */
size_t sela_hip_salvage_unaligned_workspace_bytes(size_t payload_bytes, uint32_t max_frames);
int sela_hip_salvage_frames_unaligned_device(const uint8_t* d_payload, size_t payload_bytes, uint32_t max_frames, uint32_t channels,
    sela_hip_salvaged* d_records /* [max_frames] */, uint64_t* d_totals /* [4] */, void* d_workspace, size_t workspace_bytes,
    void* stream);
int sela_hip_salvage_payload_unaligned_device(const uint8_t* d_payload, size_t payload_bytes, uint32_t max_frames, uint32_t channels,
    uint8_t* d_out, size_t out_cap, uint64_t* d_frame_offsets /* [max_frames + 1] */, sela_hip_salvaged* d_records /* [max_frames] or NULL */,
    uint64_t* d_totals /* [4] */, void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- envelope: min, max, sum and energy per bucket of samples ---------------------------------------------------
 * The level record of 5.26 on a finer grid and with the signed extremes: what a waveform overview, the sample-accurate ends of
 * silence, clip positions and onset candidates need, without decoding the track into memory.  `bucket` is a power of two from 32
 * to 2048 samples; a frame has slots = sela_hip_envelope_slots(stride, bucket) = ceil(stride / bucket) records per channel.
 * Record [f][b][c] is taken over exactly the int16 values v that sela_hip_decode_n_device writes for frame f, channel c, samples
 * [b * bucket, min((b + 1) * bucket, n_f)) with the same d_frames, d_frame_offsets, n_frames, channels and stride (n_f: the
 * frame's samples per channel): its narrowing of wider samples, its combine of difference subframes, its route, its zeros for a
 * channel that ends early.  A last partial bucket is taken over the samples it has; a slot at or beyond n_f is the all-zero
 * record.  Every record of every frame that ran is written exactly once: nothing is cleared first and nothing else is written.
 * All fields are integers and exact, whatever the launch shape: |sum| <= 2048 * 32768 = 2^26, sum_squares <= 2048 * 2^30 = 2^41.
 * Frames of 2048 samples, and the long last frame of a whole-track stream, start at a multiple of 2048, which every bucket
 * divides: the frames' buckets are the track's absolute grid, and with stride = 2048 the array is [track bucket][channel].
 * Scope: the domain of sela_hip_decode_n_device (16-bit output); samples of more than 16 bits are measured as that call narrows
 * them, not as they are.
 *   d_env          [n_frames][slots][channels], 8-byte aligned.
 *   d_status uint32[4], written by the call: [0], [1] and [3] exactly as sela_hip_decode_n_device leaves them for the same frames;
 *                  [2] is 0.  sela_hip_decode_n_status_error() applies unchanged; where it gives non-zero, or SELA_HIP_FLAG_STRIDE
 *                  is set, d_env is not defined.  n_frames = 0 writes zero status words (and d_sample_offsets[0] = 0 where given)
 *                  and nothing else.
 * d_workspace: sela_hip_envelope_workspace_bytes(n_frames, channels, stride) bytes -- sela_hip_levels_workspace_bytes() of the
 * same arguments, byte for byte, SIZE_MAX where that is -- no initialisation (the payload call: sela_hip_index_workspace_bytes
 * (payload_bytes, max_frames) more); one call at a time may use it.
 * Arguments, errors and their order are sela_hip_levels_device's, with two more: SELA_HIP_EINVAL for a bucket outside
 * {32, 64, ..., 2048}, checked with the shape, and for a d_env that is not 8-byte aligned; SELA_HIP_ECAPACITY: a smaller
 * workspace.  All found before any device is asked for: nothing is enqueued then.  Asynchronous on `stream`, one serial chain: no
 * allocation, no host wait, so a stream being captured into a HIP graph may take either call. */
struct sela_hip_envelope { /* 16 bytes, 8-byte aligned */
    int16_t min;          /* smallest v of the bucket (0 for an empty bucket) */
    int16_t max;          /* largest v */
    int32_t sum;          /* sum of v */
    uint64_t sum_squares; /* sum of v * v */
};
typedef struct sela_hip_envelope sela_hip_envelope_record; /* (sela_hip_envelope itself names the host call below, as with the digest) */
uint32_t sela_hip_envelope_slots(uint32_t stride, uint32_t bucket); /* ceil(stride / bucket); 0 for an invalid bucket or stride 0 */
size_t sela_hip_envelope_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride);
int sela_hip_envelope_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride, uint32_t bucket,
    struct sela_hip_envelope* d_env /* [n_frames][slots][channels] */, uint64_t* d_sample_offsets /* [n_frames + 1] or NULL */, uint32_t* d_status /* [4] */,
    void* d_workspace, size_t workspace_bytes, void* stream);
/* sela_hip_index_frames_device() and then the call above on the frames it found, on one stream: the count stays on the device.
 * Frames from *d_n_frames on are left alone (their records are not written). */
int sela_hip_envelope_payload_device(const uint8_t* d_payload, size_t payload_bytes, uint32_t max_frames, uint32_t channels, uint32_t stride, uint32_t bucket,
    struct sela_hip_envelope* d_env, uint64_t* d_sample_offsets, uint64_t* d_frame_offsets, uint32_t* d_n_frames, uint32_t* d_status, void* d_workspace,
    size_t workspace_bytes, void* stream);
/* Host pointers, synchronous, in chunks of frames: returns what sela_hip_decode returns for the stream (0: the records are
 * valid; a frame longer than `stride` is SELA_HIP_ECAPACITY, as the status judge says it).  Runs where sela_hip_levels runs; an open
 * streaming job of the thread is left alone.  n_frames = 0 returns 0 and asks for no device.  SELA_HIP_EINVAL: the level call's
 * cases, stride 0, a bucket outside the set, and ceil(stride / bucket) * channels beyond 32 bits. */
int sela_hip_envelope(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride, uint32_t bucket,
    struct sela_hip_envelope* env /* [n_frames][slots][channels] */);

/* ---- envelope of 24- and 32-bit streams: wide records per bucket ------------------------------------------------
 * The envelope above on the whole domain of sela_hip_decode_i32_device: samples of up to 32 bits as they are, channels of
 * different lengths, every subframe layout.  `bucket` is the same set (a power of two from 32 to 2048), slots =
 * sela_hip_envelope_slots(stride, bucket) the same function.  Record [f][b][c] is taken over exactly
 * samples_out[f][c][b * bucket .. min((b + 1) * bucket, counts_out[f * channels + c])) as sela_hip_decode_i32_device writes them
 * for the same d_frames, d_frame_offsets, n_frames, channels and stride: difference subframes combined mod 2^32, every channel
 * ending at its own count, a channel no subframe names all zero records, a malformed frame measured with whatever counts that
 * call gives it.  A last partial bucket is taken over the samples it has -- a sample that is not there is not a 0 --; a slot at
 * or beyond the channel's count is the all-zero record.  Every record of every frame that ran is written exactly once: nothing is
 * cleared first and nothing else is written.
 * Bounds: a bucket holds at most 2048 samples, so |sum| <= 2048 * 2^31 = 2^42 and sum_squares <= 2048 * 2^62 = 2^73 -- four
 * full-scale samples already reach 2^64, hence the two energy words.  All fields are integers and exact, whatever the launch
 * shape.
 *   d_env          [n_frames][slots][channels], 8-byte aligned.
 *   d_status uint32[4], written by the call: [0], [1] and [3] exactly as sela_hip_decode_i32_device leaves them for the same
 *                  frames; [2] is 0.  Where SELA_HIP_FLAG_STRIDE is set, d_env is not defined (nothing outside it is written).
 * d_workspace: sela_hip_envelope_i32_workspace_bytes(n_frames, channels, stride) bytes -- sela_hip_verify_i32_workspace_bytes() of
 * the same arguments, byte for byte, SIZE_MAX where that is: a slice of 4096 samples holds whole buckets, so no partial record
 * lies in it -- no initialisation (the payload call: sela_hip_index_workspace_bytes(payload_bytes, max_frames) more); one call at
 * a time may use it.
 * Arguments, errors and their order are sela_hip_levels_i32_device's, with two more: SELA_HIP_EINVAL for a bucket outside
 * {32, 64, ..., 2048}, checked with the shape, and for a d_env that is not 8-byte aligned; SELA_HIP_ECAPACITY: a smaller
 * workspace.  All found before any device is asked for: nothing is enqueued then.  Asynchronous on `stream`, one serial chain: no
 * allocation, no host wait, no host read, so a stream being captured into a HIP graph may take any of the three device calls. */
struct sela_hip_envelope32 { /* 32 bytes, 8-byte aligned */
    int32_t min, max;        /* smallest / largest v of the bucket (0, 0 for an empty bucket) */
    int64_t sum;             /* sum of v */
    uint64_t sum_squares_lo; /* sum of v * v, bits 0 .. 63 */
    uint64_t sum_squares_hi; /* ... and bits 64 .. 127 */
};
typedef struct sela_hip_envelope32 sela_hip_envelope32_record;
size_t sela_hip_envelope_i32_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride);
int sela_hip_envelope_i32_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride, uint32_t bucket,
    struct sela_hip_envelope32* d_env /* [n_frames][slots][channels] */, uint64_t* d_sample_offsets /* [n_frames + 1] or NULL */, uint32_t* d_status /* [4] */,
    void* d_workspace, size_t workspace_bytes, void* stream);
/* sela_hip_index_frames_device() and then the call above on the frames it found, on one stream: the count stays on the device.
 * Frames from *d_n_frames on are left alone (their records are not written). */
int sela_hip_envelope_payload_i32_device(const uint8_t* d_payload, size_t payload_bytes, uint32_t max_frames, uint32_t channels, uint32_t stride, uint32_t bucket,
    struct sela_hip_envelope32* d_env, uint64_t* d_sample_offsets, uint64_t* d_frame_offsets, uint32_t* d_n_frames, uint32_t* d_status, void* d_workspace,
    size_t workspace_bytes, void* stream);
/* The same records from planar int32 samples that already lie in device memory (an unpack's output ahead of an encode, a
 * decode's output), as sela_hip_levels_samples_i32_device: channel c of frame f holds min(d_counts[f * channels + c], stride)
 * samples (d_counts NULL: stride).  d_samples and d_counts 4-byte aligned.  d_status: all four words zeroed.  d_workspace:
 * sela_hip_envelope_samples_i32_workspace_bytes() bytes -- a token, nothing is kept in it. */
size_t sela_hip_envelope_samples_i32_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride);
int sela_hip_envelope_samples_i32_device(const int32_t* d_samples /* [n_frames][channels][stride] */, const uint32_t* d_counts /* [n_frames * channels] or NULL */,
    uint32_t n_frames, uint32_t channels, uint32_t stride, uint32_t bucket, struct sela_hip_envelope32* d_env, uint32_t* d_status /* [4] */, void* d_workspace,
    size_t workspace_bytes, void* stream);
/* Host pointers, synchronous, in chunks of frames: returns what sela_hip_decode_i32 returns for the stream (0: the records are
 * valid; a frame longer than `stride` is SELA_HIP_ECAPACITY, as the status judge says it).  Runs where sela_hip_levels_i32 runs;
 * an open streaming job of the thread is left alone.  n_frames = 0 returns 0 and asks for no device.  SELA_HIP_EINVAL: the level
 * call's cases, stride 0, a bucket outside the set, and ceil(stride / bucket) * channels beyond 32 bits. */
int sela_hip_envelope_i32(const uint8_t* frames, const uint64_t* frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride, uint32_t bucket,
    struct sela_hip_envelope32* env /* [n_frames][slots][channels] */);

/* ---- the stages on their own -------------------------------------------------------------------------------
 * The reference's public L1 classes (src/include/lpc.hpp:73-117, src/include/rice.hpp:9-43; its tests call them directly:
 * test/lpctests.cpp:10-32, test/ricetests.cpp:7-25), batched, on HOST pointers.  Not the fast path -- a frame goes through
 * all of them inside one kernel (sela_hip_encode / sela_hip_decode) -- but the same device code, for callers and tests of
 * a stage by itself.  Every call synchronises.
 *
 * lpc::ResidueGenerator::process (src/lpc/residue_generator.cpp:121-134): n_blocks blocks of 2048 samples (int32) -> per block the order, the quantised reflection
 * coefficients (q_out[block][0 .. order), the rest zeroed) and 2048 residues.  Samples beyond 17 bits are taken too (through the
 * any-length kernels, like sela_hip_lpc_encode_n).  A Rice stream too long for a frame's slot is not this stage's business:
 * the residues are returned whatever their size. */
int sela_hip_lpc_encode(const int32_t* samples, uint32_t n_blocks, int32_t* order_out, int32_t* q_out /* [n_blocks][100] */, int32_t* residues_out);
/* The same for blocks of samples_per_block samples (1 .. 2^24) of any 32-bit value -- the class takes any vector
 * (src/lpc/residue_generator.cpp:6-10).  q_out[block][order .. 100) is zeroed.  A block not longer than the order its analysis
 * picks: SELA_HIP_ERANGE (the reference reads past its vector, residue_generator.cpp:104-110). */
int sela_hip_lpc_encode_n(const int32_t* samples, uint32_t n_blocks, uint32_t samples_per_block, int32_t* order_out, int32_t* q_out /* [n_blocks][100] */,
    int32_t* residues_out);
/* lpc::SampleGenerator::process (src/lpc/sample_generator.cpp:11-39): the inverse.  q[block][0 .. order[block]); samples_out
 * [n_blocks][2048] as the 32-bit values the reference returns.  coefs_out (or NULL): [n_blocks][101], the Q35 predictor
 * a[0 .. order] of lpc::LinearPredictor::generatelinearPredictionCoefficients (src/lpc/linear_predictor.cpp:30-61);
 * samples_out may be NULL when only the predictor is wanted. */
int sela_hip_lpc_decode(const int32_t* order, const int32_t* q /* [n_blocks][100] */, const int32_t* residues, uint32_t n_blocks, int32_t* samples_out,
    int64_t* coefs_out);
/* The same for blocks of samples_per_block residues (1 .. 2^24). */
int sela_hip_lpc_decode_n(const int32_t* order, const int32_t* q /* [n_blocks][100] */, const int32_t* residues, uint32_t n_blocks, uint32_t samples_per_block,
    int32_t* samples_out, int64_t* coefs_out);
/* rice::RiceEncoder::process (src/rice/rice_encoder.cpp:73-81): n_streams streams of int32 values, stream i =
 * values[value_offsets[i] .. value_offsets[i + 1]) -> its Rice parameter k_out[i] (the first minimum over 0..19), its
 * word count word_counts_out[i] (ceil((float)bits / 32) as the reference computes it) and its words at
 * words_out[word_offsets[i] ..] (word_offsets[i + 1] - word_offsets[i] words of room: SELA_HIP_ECAPACITY if a stream needs
 * more -- the counts are valid then).  |value| >= 2^30 (the reference's int32 zig-zag overflows there): SELA_HIP_ERANGE. */
int sela_hip_rice_encode(const int32_t* values, const uint64_t* value_offsets, uint32_t n_streams, uint32_t* k_out, uint32_t* word_counts_out,
    uint32_t* words_out, const uint64_t* word_offsets);
/* rice::RiceDecoder::process (src/rice/rice_decoder.cpp:54-61): stream i = words[word_offsets[i] .. word_offsets[i + 1]) with
 * parameter k[i] (< 32) -> value_offsets[i + 1] - value_offsets[i] values at values_out[value_offsets[i] ..].  A stream that
 * ends before its values do decodes the missing bits as zeros and the call returns SELA_HIP_EFORMAT. */
int sela_hip_rice_decode(const uint32_t* words, const uint64_t* word_offsets, const uint32_t* k, const uint64_t* value_offsets, uint32_t n_streams,
    int32_t* values_out);

/* ---- per-kernel timing (measurement hook used by bench.py) ------------------------------------------
 * When enabled, the *_device calls of the calling thread bracket each kernel launch with HIP events
 * recorded on the caller's stream.  sela_hip_kernel_times() waits for the events of the most recent
 * encode (3 kernels: blocks, plan, assemble) or decode (1 kernel) call and returns their durations
 * in milliseconds; it returns the number of kernels reported (0 if timing was off). */
void sela_hip_enable_kernel_timing(int enable);
int sela_hip_kernel_times(float* ms_out, int capacity);

/* ---- flag bits reported through d_status[0] / sela_hip_trace.flags --------------------------------- */
#define SELA_HIP_FLAG_Q_RANGE 1u       /* quantised reflection coefficient outside [-64,63] (clamped) */
#define SELA_HIP_FLAG_COEF_OVERFLOW 2u /* |2^35 * coefficient| >= 2^63 */
#define SELA_HIP_FLAG_RICE_RANGE 4u    /* zig-zag residue does not fit 32 bits */
#define SELA_HIP_FLAG_RICE_OVERRUN 8u  /* decoder ran past the end of a Rice stream */
#define SELA_HIP_FLAG_WORDS_CAP 16u    /* a Rice stream exceeded the per-block slot (encoder) */
#define SELA_HIP_FLAG_BAD_FRAME 32u    /* bad sync word / inconsistent subframe header (decoder) */
#define SELA_HIP_FLAG_INTERNAL 64u     /* a bounded wait inside a kernel ran out (never expected; reported as SELA_HIP_ENODEV) */
#define SELA_HIP_FLAG_SHORT_BLOCK 128u /* a block no longer than its own predictor order: the reference's warm-up loop reads past
                                        * its vector there (src/lpc/residue_generator.cpp:104-110); reported as SELA_HIP_ERANGE */
#define SELA_HIP_FLAG_STRIDE 256u     /* a subframe is longer than the caller's stride (sela_hip_decode_i32_device: what the host call reports
                                        * as SELA_HIP_ECAPACITY; nothing is written past [n_frames][channels][stride] all the same) */

#ifdef __cplusplus
}
#endif
#endif /* SELA_HIP_H_ */
