// sela_generic.h -- what sela_generic.hip (the any-length / 32-bit route) shares with the C ABI (sela_capi.hip).
#ifndef SELA_GENERIC_H_
#define SELA_GENERIC_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sela_hip.h"
#include "sela_workspace.h"

namespace sela {

struct GenericMeta { // one per (frame, signal), written by k_generic_analyse
    uint32_t order, coef_k, coef_words, res_k, res_words, flags;
    uint32_t form; // which form of the residue filter the block took: 0 FP64 taps (exact by its bound), 1 the 64-bit wrap-around taps
};
void set_generic_wrap_taps(int on); // tests: every block on the wrap-around taps
struct GenericSubInfo { // one per (frame, subframe position), written by k_generic_decode
    uint8_t channel, type, parent, ok;
    uint32_t n;
};

// Signals analysed per frame: the channels, and a difference per pair the plan may store in place of the pair's odd channel --
// the one pair of an exactly-stereo frame (src/frame/frame_encoder.cpp:18), or with `paired` every pair
// (2p, 2p + 1), signal channels + p being pair p's difference, in instantiations of k_generic_analyse and k_generic_plan of their own.
inline uint32_t generic_signals(uint32_t channels, bool paired) { return channels + (paired ? channels / 2 : channels == 2 ? 1u : 0u); }
size_t generic_encode_workspace_bytes(uint32_t n_frames, uint32_t channels, uint32_t n);
hipError_t launch_generic_analyse(const void* d_input, bool in16, uint32_t n_frames, uint32_t channels, uint32_t n_sig, uint32_t n, int32_t* d_sig,
    int32_t* d_res, int32_t* d_q, GenericMeta* d_meta, hipStream_t stream, bool lossless = false /* DESIGN.md 5.16 */,
    bool paired = false /* n_sig = generic_signals(channels, true) */);
hipError_t launch_generic_plan(const GenericMeta* d_meta, uint32_t n_frames, uint32_t channels, uint32_t n_sig, uint64_t base_bytes, uint64_t* d_frame_offsets,
    uint64_t* d_word_base, uint32_t* d_chosen, uint32_t* d_status, uint64_t* d_total_words, hipStream_t stream, bool paired = false);
hipError_t launch_generic_emit(const GenericMeta* d_meta, uint32_t n_frames, uint32_t channels, uint32_t n_sig, uint32_t n, const int32_t* d_res, const int32_t* d_q,
    const uint32_t* d_chosen, const uint64_t* d_word_base, uint32_t* d_words /* zeroed */, uint64_t words_cap /* a subframe whose words would reach beyond is left out */,
    const uint64_t* d_frame_offsets, uint64_t base_bytes, uint8_t* d_frames, uint64_t frames_cap, hipStream_t stream);
// fast_first: the subframes go to k_decode_subframes32 (sela_decode32.hip: the fast decoder's lane-parallel parse and tuned
// synthesis, any length) instead of k_generic_decode (the serial walk); d_status[2] then counts the subframes that kernel left
// alone -- not zero: run the launch again without fast_first -- and d_status[3] those it parsed by segments (standard_path:
// 2048-sample subframes that fit the parser's plan take the frame kernel's own one-piece parse; off only in tests).
hipError_t launch_generic_decode(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint64_t base_bytes, uint32_t n_frames, uint32_t channels, uint32_t stride,
    int32_t* d_dec, GenericSubInfo* d_info, int32_t* d_all, uint32_t* d_counts, const uint64_t* d_sample_offsets, int16_t* d_pcm_out, uint32_t* d_status,
    bool fast_first, bool standard_path, hipStream_t stream);
// d_n_found (or null): the device's own count of frames; frames from *d_n_found on are left alone (sela_hip_decode_payload_i32_device)
hipError_t launch_decode_subframes32(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint64_t base_bytes, uint32_t n_frames, uint32_t channels,
    uint32_t stride, int32_t* d_dec, GenericSubInfo* d_info, uint32_t* d_status, bool standard_path, hipStream_t stream, const uint32_t* d_n_found = nullptr);
// sela_hip_decode_i32_device / sela_hip_decode_payload_i32_device: the sample index, the fast kernel, the judge
// and the combine, all on `stream`, nothing waited for.  Arguments checked by the caller; mode as sela_hip_debug_standard_first.
// (Every *_workspace_bytes here measures its call's one description of the workspace, sela_workspace.h -- `at`: on that Carve,
// one that lists its pieces or a sub() range of another call's; null: on a fresh one.  SIZE_MAX: more than any device holds.  The
// four sized by (frames, channels, stride) are passed around as plain functions of those three: the overload without `at`.)
size_t decode_i32_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride, Carve* at);
inline size_t decode_i32_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride) { return decode_i32_workspace_bytes(max_frames, channels, stride, nullptr); }
// sela_hip_decode_n_device / sela_hip_decode_payload_n_device: the sample index, the route taken on the device,
// both routes' kernels gated by it, the int16 writer.  Arguments checked by the caller.
size_t decode_n_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride, Carve* at);
inline size_t decode_n_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride) { return decode_n_workspace_bytes(max_frames, channels, stride, nullptr); }
hipError_t launch_decode_n_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t max_frames, const uint32_t* d_n_found, uint32_t channels,
    uint32_t stride, int16_t* d_pcm_out, uint64_t* d_sample_offsets, uint32_t* d_status, void* d_workspace, int mode, int recurrence_form, uint32_t synth_priorities,
    hipStream_t stream);
hipError_t launch_decode_i32_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t max_frames, const uint32_t* d_n_found, uint32_t channels,
    uint32_t stride, int32_t* d_samples_out, uint32_t* d_counts_out, uint64_t* d_sample_offsets, uint32_t* d_status, void* d_workspace, int mode, hipStream_t stream);
// sela_hip_verify_device / sela_hip_verify_payload_device: launch_decode_n_device's shape with the decode's
// stores turned into a compare against d_pcm.  Up to kVerifyFusedChannels channels the 2048-sample route is one kernel
// (k_verify_frames, sela_verify.hip); every other route decodes into the workspace and k_verify_compare takes it from there.
constexpr uint32_t kVerifyFusedChannels = 8;    // = kDecMaxWaves (sela_decode_core.inc)
constexpr uint32_t kVerifySliceValues = 16384;  // interleaved int16 values one workgroup of k_verify_compare takes
uint32_t verify_slices(uint32_t channels, uint32_t stride);
hipError_t launch_verify_frames(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames, uint32_t channels, const int16_t* d_pcm,
    uint32_t* d_diff_counts, uint32_t* d_first_diff, uint32_t* d_status, void* d_workspace, hipStream_t stream, int recurrence_form, uint32_t synth_priorities,
    const uint32_t* d_n_found);
hipError_t launch_verify_compare(const int16_t* d_decoded, const int16_t* d_pcm, const uint64_t* d_sample_offsets, uint32_t max_frames, uint32_t channels,
    uint32_t stride, const uint32_t* d_n_a, const uint32_t* d_n_b /* or null */, void* d_parts /* [max_frames][verify_slices()] x 8 bytes */,
    uint32_t* d_diff_counts, uint32_t* d_first_diff, uint32_t* d_status, hipStream_t stream);
size_t verify_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride, Carve* at);
inline size_t verify_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride) { return verify_workspace_bytes(max_frames, channels, stride, nullptr); }
hipError_t launch_verify_n_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t max_frames, const uint32_t* d_n_found, uint32_t channels,
    uint32_t stride, const int16_t* d_pcm, uint32_t* d_diff_counts, uint32_t* d_first_diff, uint64_t* d_sample_offsets, uint32_t* d_status, void* d_workspace,
    int mode, int recurrence_form, uint32_t synth_priorities, hipStream_t stream);
// sela_hip_levels_device / sela_hip_levels_payload_device: launch_verify_n_device's shape with the compare
// turned into a reduction -- peak, sum and sum of squares per (frame, channel).  Up to kVerifyFusedChannels channels the
// 2048-sample route is one kernel (k_level_frames, sela_levels.hip); every other route decodes into the workspace and
// k_level_channels takes it from there.
hipError_t launch_level_frames(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames, uint32_t channels, sela_hip_level* d_levels,
    uint32_t* d_status, void* d_workspace, hipStream_t stream, int recurrence_form, uint32_t synth_priorities, const uint32_t* d_n_found);
hipError_t launch_level_channels(const int16_t* d_decoded, const uint64_t* d_sample_offsets, uint32_t max_frames, uint32_t channels, uint32_t stride,
    const uint32_t* d_n_a, const uint32_t* d_n_b /* or null */, sela_hip_level* d_levels, uint32_t* d_status, hipStream_t stream);
size_t levels_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride, Carve* at);
inline size_t levels_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride) { return levels_workspace_bytes(max_frames, channels, stride, nullptr); }
hipError_t launch_levels_n_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t max_frames, const uint32_t* d_n_found, uint32_t channels,
    uint32_t stride, sela_hip_level* d_levels, uint64_t* d_sample_offsets, uint32_t* d_status, void* d_workspace, int mode, int recurrence_form,
    uint32_t synth_priorities, hipStream_t stream);
// sela_hip_digest_device / sela_hip_digest_payload_device: launch_levels_n_device's shape with the reduction
// turned into a CRC-32 of the bytes, and the track's two words folded from the records behind it.  Up to kVerifyFusedChannels
// channels the 2048-sample route is one kernel (k_digest_frames, sela_digest.hip); every other route decodes into the workspace
// and k_digest_pcm / k_digest_slices take it from there; k_digest_fold / k_digest_track write d_track.
constexpr uint32_t kDigestSliceBytes = 32768;   // bytes of a frame's PCM one workgroup of k_digest_pcm takes
uint32_t digest_slices(uint32_t channels, uint32_t stride);
uint32_t digest_fold_blocks(uint32_t max_frames);
hipError_t launch_digest_frames(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames, uint32_t channels, struct sela_hip_digest* d_digests,
    uint32_t* d_status, void* d_workspace, hipStream_t stream, int recurrence_form, uint32_t synth_priorities, const uint32_t* d_n_found);
hipError_t launch_digest_pcm(const int16_t* d_decoded, const uint64_t* d_sample_offsets, uint32_t max_frames, uint32_t channels, uint32_t stride,
    const uint32_t* d_n_a, const uint32_t* d_n_b /* or null */, uint32_t* d_parts /* [max_frames][digest_slices()] */, struct sela_hip_digest* d_digests,
    hipStream_t stream);
// (the two folds take the bytes of a value: 2 here, 3 or 4 for the tiles of sela_digest_pcm.hip; d_n_a null: every frame of the call)
hipError_t launch_digest_slices(const uint32_t* d_parts, const uint64_t* d_sample_offsets, uint32_t max_frames, uint32_t channels, uint32_t stride,
    const uint32_t* d_n_a /* or null */, const uint32_t* d_n_b /* or null */, uint64_t slice_bytes, uint32_t slices, uint32_t value_bytes,
    struct sela_hip_digest* d_digests, hipStream_t stream);
hipError_t launch_digest_fold(const struct sela_hip_digest* d_digests, const uint64_t* d_sample_offsets, uint32_t max_frames, const uint32_t* d_n_found,
    uint32_t channels, uint32_t value_bytes, uint32_t* d_fold /* [digest_fold_blocks()] */, uint64_t* d_track, hipStream_t stream);
size_t digest_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride, Carve* at);
inline size_t digest_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride) { return digest_workspace_bytes(max_frames, channels, stride, nullptr); }
hipError_t launch_digest_n_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t max_frames, const uint32_t* d_n_found, uint32_t channels,
    uint32_t stride, struct sela_hip_digest* d_digests, uint64_t* d_track, uint64_t* d_sample_offsets, uint32_t* d_status, void* d_workspace, int mode,
    int recurrence_form, uint32_t synth_priorities, hipStream_t stream);
// sela_hip_envelope_device / sela_hip_envelope_payload_device: launch_levels_n_device's shape and workspace with
// the frame's total cut into buckets of 32 .. 2048 samples -- min, max, sum and sum of squares per (frame, bucket, channel).  Up to
// kVerifyFusedChannels channels the 2048-sample route is one kernel (k_envelope_frames, sela_envelope.hip); every other route
// decodes into the workspace and k_envelope_channels takes it from there.  status[2] stays 0.
constexpr uint32_t kEnvelopeMinBucket = 32, kEnvelopeMaxBucket = 2048;
inline bool envelope_bucket_ok(uint32_t bucket) { return bucket >= kEnvelopeMinBucket && bucket <= kEnvelopeMaxBucket && (bucket & (bucket - 1)) == 0; }
// records per frame and channel: ceil(stride / bucket); 0 for an invalid bucket or stride 0
inline uint32_t envelope_slots(uint32_t stride, uint32_t bucket) { return envelope_bucket_ok(bucket) ? (uint32_t)(((uint64_t)stride + bucket - 1) / bucket) : 0u; }
hipError_t launch_envelope_frames(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames, uint32_t channels, uint32_t stride, uint32_t bucket,
    struct sela_hip_envelope* d_env, uint32_t* d_status, void* d_workspace, hipStream_t stream, int recurrence_form, uint32_t synth_priorities, const uint32_t* d_n_found);
hipError_t launch_envelope_channels(const int16_t* d_decoded, const uint64_t* d_sample_offsets, uint32_t max_frames, uint32_t channels, uint32_t stride, uint32_t bucket,
    const uint32_t* d_n_a, const uint32_t* d_n_b /* or null */, struct sela_hip_envelope* d_env, hipStream_t stream);
hipError_t launch_envelope_n_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t max_frames, const uint32_t* d_n_found, uint32_t channels,
    uint32_t stride, uint32_t bucket, struct sela_hip_envelope* d_env, uint64_t* d_sample_offsets, uint32_t* d_status, void* d_workspace, int mode, int recurrence_form,
    uint32_t synth_priorities, hipStream_t stream);
// sela_hip_crc32_device: k_digest_pcm / k_digest_slices on bytes that lie in device memory already
size_t crc32_workspace_bytes(uint64_t n_bytes, Carve* at);
inline size_t crc32_workspace_bytes(uint64_t n_bytes) { return crc32_workspace_bytes(n_bytes, nullptr); }
hipError_t launch_crc32_device(const void* d_bytes, uint64_t n_bytes, uint64_t* d_out, void* d_workspace, hipStream_t stream);
// sela_hip_verify_i32_device / sela_hip_verify_payload_i32_device: launch_decode_i32_device's shape with the
// combine turned into a compare against d_samples ([frames][channels][stride] int32, d_lengths or null).  The kernels are
// sela_verify32.hip's: frames of a direct layout are compared from the subframes as decoded, nothing stored; any other frame goes
// through k_generic_combine<false> into the workspace first, the whole call's frames as soon as one frame needs it.
constexpr uint32_t kVerify32Slice = 4096;       // samples of every channel one workgroup of k_verify32_direct takes (= kCombineSlice)
uint32_t verify32_slices(uint32_t stride);
hipError_t launch_verify32_begin(uint32_t* d_status, uint32_t* d_ctl /* [2] */, hipStream_t stream);
hipError_t launch_verify32_direct(const int32_t* d_dec, const GenericSubInfo* d_info, uint32_t max_frames, const uint32_t* d_n_found, uint32_t channels,
    uint32_t stride, const int32_t* d_samples, const uint32_t* d_lengths, const uint32_t* d_status, uint32_t* d_ctl, uint32_t* d_marks /* [max_frames] */,
    void* d_parts /* [max_frames][verify32_slices()] x 8 bytes */, hipStream_t stream);
hipError_t launch_verify32_rest(const int32_t* d_all, const uint32_t* d_counts, uint32_t max_frames, const uint32_t* d_n_found, uint32_t channels, uint32_t stride,
    const int32_t* d_samples, const uint32_t* d_lengths, uint32_t* d_status, const uint32_t* d_ctl, const uint32_t* d_marks, void* d_parts,
    uint32_t* d_diff_counts, uint32_t* d_first_diff, hipStream_t stream);
// the gate (launched behind every direct kernel by the family's sequence, sela_generic.hip), and the sum alone for a compare
// whose rest kernel does not launch it (sela_verify_pcm.hip)
hipError_t launch_verify32_gate(uint32_t max_frames, const uint32_t* d_n_found, uint32_t* d_ctl, hipStream_t stream);
hipError_t launch_verify32_sum(const void* d_parts, uint32_t n_slices, uint32_t max_frames, const uint32_t* d_n_found, uint32_t* d_diff_counts, uint32_t* d_first_diff,
    uint32_t* d_status, hipStream_t stream);
size_t verify_i32_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride, Carve* at);
inline size_t verify_i32_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride) { return verify_i32_workspace_bytes(max_frames, channels, stride, nullptr); }
const uint32_t* verify_i32_control_words(const void* d_workspace, uint32_t max_frames, uint32_t channels, uint32_t stride); // the call's two control words (device)
hipError_t launch_verify_i32_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t max_frames, const uint32_t* d_n_found, uint32_t channels,
    uint32_t stride, const int32_t* d_samples, const uint32_t* d_lengths, uint32_t* d_diff_counts, uint32_t* d_first_diff, uint64_t* d_sample_offsets,
    uint32_t* d_status, void* d_workspace, int mode, hipStream_t stream);
// sela_hip_levels_i32_device / sela_hip_levels_payload_i32_device: launch_verify_i32_device's shape with the
// compare turned into a reduction -- peak, sum and the 128-bit sum of squares per (frame, channel).  The kernels are
// sela_levels32.hip's; between the slices a partial record per (frame, slice, channel) lies in the workspace.
hipError_t launch_level32_begin(uint32_t* d_status, uint32_t* d_ctl /* [2] or null */, bool whole /* every status word, not [2] alone */, hipStream_t stream);
hipError_t launch_level32_direct(const int32_t* d_dec, const GenericSubInfo* d_info, uint32_t max_frames, const uint32_t* d_n_found, uint32_t channels,
    uint32_t stride, const uint32_t* d_status, uint32_t* d_ctl, uint32_t* d_marks /* [max_frames] */,
    uint64_t* d_parts /* [max_frames][verify32_slices()][channels] x 32 bytes */, hipStream_t stream);
// d_ctl and d_marks null: every frame of d_all (the caller's samples; d_counts or null: stride); then the records and status[2]
hipError_t launch_level32_rest(const int32_t* d_all, const uint32_t* d_counts, uint32_t max_frames, const uint32_t* d_n_found, uint32_t channels, uint32_t stride,
    uint32_t* d_status, const uint32_t* d_ctl, const uint32_t* d_marks, uint64_t* d_parts, sela_hip_level32* d_levels, hipStream_t stream);
size_t levels_i32_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride, Carve* at);
inline size_t levels_i32_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride) { return levels_i32_workspace_bytes(max_frames, channels, stride, nullptr); }
const uint32_t* levels_i32_control_words(const void* d_workspace, uint32_t max_frames, uint32_t channels, uint32_t stride); // the call's two control words (device)
hipError_t launch_levels_i32_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t max_frames, const uint32_t* d_n_found, uint32_t channels,
    uint32_t stride, sela_hip_level32* d_levels, uint64_t* d_sample_offsets, uint32_t* d_status, void* d_workspace, int mode, hipStream_t stream);
// sela_hip_levels_samples_i32_device: the fallback's reduction on its own, over samples that already lie in device memory
size_t levels_samples_i32_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride, Carve* at);
inline size_t levels_samples_i32_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride) { return levels_samples_i32_workspace_bytes(max_frames, channels, stride, nullptr); }
hipError_t launch_levels_samples_i32_device(const int32_t* d_samples, const uint32_t* d_counts, uint32_t max_frames, uint32_t channels, uint32_t stride,
    sela_hip_level32* d_levels, uint32_t* d_status, void* d_workspace, hipStream_t stream);
// sela_hip_envelope_i32_device / sela_hip_envelope_payload_i32_device: launch_levels_i32_device's shape with the
// frame's total cut into buckets of 32 .. 2048 samples -- min, max, sum and the 128-bit sum of squares per (frame, bucket, channel).
// The kernels are sela_envelope32.hip's; a slice holds whole buckets, so they write the records themselves and the workspace is
// launch_verify_i32_device's, byte for byte.  The begin step is launch_level32_begin; status[2] stays 0.
hipError_t launch_envelope32_direct(const int32_t* d_dec, const GenericSubInfo* d_info, uint32_t max_frames, const uint32_t* d_n_found, uint32_t channels,
    uint32_t stride, uint32_t bucket, const uint32_t* d_status, uint32_t* d_ctl, uint32_t* d_marks /* [max_frames] */,
    struct sela_hip_envelope32* d_env /* [max_frames][envelope_slots()][channels] */, hipStream_t stream);
// d_ctl and d_marks null: every frame of d_all (the caller's samples; d_counts or null: stride)
hipError_t launch_envelope32_rest(const int32_t* d_all, const uint32_t* d_counts, uint32_t max_frames, uint32_t channels, uint32_t stride, uint32_t bucket,
    const uint32_t* d_status, const uint32_t* d_ctl, const uint32_t* d_marks, struct sela_hip_envelope32* d_env, hipStream_t stream);
size_t envelope_i32_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride, Carve* at);
inline size_t envelope_i32_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride) { return envelope_i32_workspace_bytes(max_frames, channels, stride, nullptr); }
const uint32_t* envelope_i32_control_words(const void* d_workspace, uint32_t max_frames, uint32_t channels, uint32_t stride); // the call's two control words (device)
hipError_t launch_envelope_i32_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t max_frames, const uint32_t* d_n_found, uint32_t channels,
    uint32_t stride, uint32_t bucket, struct sela_hip_envelope32* d_env, uint64_t* d_sample_offsets, uint32_t* d_status, void* d_workspace, int mode, hipStream_t stream);
// sela_hip_envelope_samples_i32_device: the rest kernel on its own, over samples that already lie in device memory; the workspace
// is a token (nothing lies between the kernels)
size_t envelope_samples_i32_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride, Carve* at);
inline size_t envelope_samples_i32_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride) { return envelope_samples_i32_workspace_bytes(max_frames, channels, stride, nullptr); }
hipError_t launch_envelope_samples_i32_device(const int32_t* d_samples, const uint32_t* d_counts, uint32_t max_frames, uint32_t channels, uint32_t stride, uint32_t bucket,
    struct sela_hip_envelope32* d_env, uint32_t* d_status, hipStream_t stream);
// sela_hip_verify_pcm_device / sela_hip_verify_payload_pcm_device: launch_verify_i32_device's shape with the
// original read as packed interleaved PCM of 3 or 4 bytes a sample, frame f at d_sample_offsets[f] (the caller's, or the
// workspace's copy) -- sela_verify_pcm.hip's kernels on the tiles of sela_pcm_layout.h, no unpacked copy.
uint32_t verify_pcm_tiles(uint32_t stride, uint32_t channels); // pcm_tiles(stride, channels)
hipError_t launch_verify_pcm_direct(const int32_t* d_dec, const GenericSubInfo* d_info, uint32_t max_frames, const uint32_t* d_n_found, uint32_t channels,
    uint32_t stride, const void* d_pcm, uint32_t bytes_per_sample, uint64_t pcm_samples, const uint64_t* d_sample_offsets, const uint32_t* d_status, uint32_t* d_ctl,
    uint32_t* d_marks /* [max_frames] */, void* d_parts /* [max_frames][verify_pcm_tiles()] x 8 bytes */, hipStream_t stream);
hipError_t launch_verify_pcm_rest(const int32_t* d_all, const uint32_t* d_counts, uint32_t max_frames, uint32_t channels, uint32_t stride, const void* d_pcm,
    uint32_t bytes_per_sample, uint64_t pcm_samples, const uint64_t* d_sample_offsets, const uint32_t* d_status, uint32_t* d_ctl, uint32_t* d_marks, void* d_parts,
    hipStream_t stream);
size_t verify_pcm_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride, Carve* at);
inline size_t verify_pcm_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride) { return verify_pcm_workspace_bytes(max_frames, channels, stride, nullptr); }
const uint32_t* verify_pcm_control_words(const void* d_workspace, uint32_t max_frames, uint32_t channels, uint32_t stride); // the call's two control words (device)
hipError_t launch_verify_pcm_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t max_frames, const uint32_t* d_n_found, uint32_t channels,
    uint32_t stride, const void* d_pcm, uint32_t bytes_per_sample, uint64_t pcm_samples, uint32_t* d_diff_counts, uint32_t* d_first_diff, uint64_t* d_sample_offsets,
    uint32_t* d_status, void* d_workspace, int mode, hipStream_t stream);
// sela_hip_digest_pcm_device / sela_hip_digest_payload_pcm_device: launch_verify_pcm_device's shape with the
// compare turned into the CRC-32 of the packed bytes sela_hip_decode_pcm_device would write -- sela_digest_pcm.hip's kernels on the
// tiles of sela_pcm_layout.h, one raw CRC per (frame, tile) -- and sela_digest.hip's folds behind it.
uint64_t digest_pcm_tile_bytes(uint32_t channels, uint32_t bytes_per_sample);
hipError_t launch_digest32_begin(uint32_t* d_ctl /* [2] */, hipStream_t stream);
hipError_t launch_digest32_direct(const int32_t* d_dec, const GenericSubInfo* d_info, uint32_t max_frames, const uint32_t* d_n_found, uint32_t channels, uint32_t stride,
    uint32_t bytes_per_sample, const uint64_t* d_sample_offsets, uint32_t* d_status, uint32_t* d_ctl, uint32_t* d_marks /* [max_frames] */,
    uint32_t* d_parts /* [max_frames][verify_pcm_tiles()] */, hipStream_t stream);
hipError_t launch_digest32_rest(const int32_t* d_all, const uint32_t* d_counts, uint32_t max_frames, uint32_t channels, uint32_t stride, uint32_t bytes_per_sample,
    const uint64_t* d_sample_offsets, uint32_t* d_status, uint32_t* d_ctl, uint32_t* d_marks, uint32_t* d_parts, hipStream_t stream);
size_t digest_pcm_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride, Carve* at);
inline size_t digest_pcm_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride) { return digest_pcm_workspace_bytes(max_frames, channels, stride, nullptr); }
const uint32_t* digest_pcm_control_words(const void* d_workspace, uint32_t max_frames, uint32_t channels, uint32_t stride); // the call's two control words (device)
hipError_t launch_digest_pcm_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t max_frames, const uint32_t* d_n_found, uint32_t channels,
    uint32_t stride, uint32_t bytes_per_sample, struct sela_hip_digest* d_digests, uint64_t* d_track, uint64_t* d_sample_offsets, uint32_t* d_status,
    void* d_workspace, int mode, hipStream_t stream);
// sela_hip_encode_i32_device / sela_hip_encode_n_device: k_generic_analyse, k_generic_plan<true> and
// k_generic_write on `stream`, nothing waited for.  input as launch_generic_analyse; arguments checked by the caller.
size_t encode_i32_device_workspace_bytes(uint32_t n_frames, uint32_t channels, uint32_t n, bool paired = false, Carve* at = nullptr);
hipError_t launch_encode_i32_device(const void* d_input, bool in16, uint32_t n_frames, uint32_t channels, uint32_t n, uint8_t* d_frames, uint64_t frames_cap,
    uint64_t* d_frame_offsets, uint32_t* d_status, void* d_workspace, hipStream_t stream, bool lossless = false, bool paired = false);
hipError_t launch_lpc_decode_any(const int32_t* d_order, const int32_t* d_q, const int32_t* d_residues, uint32_t n_blocks, uint32_t n, int32_t* d_samples,
    int64_t* d_coefs, uint32_t* d_status, hipStream_t stream);

} // namespace sela
#endif
