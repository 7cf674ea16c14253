// sela_decode.hip -- MI355X (gfx950) decoder kernel of the SELA frame path.
//
// ONE launch: k_decode_frames, one WORKGROUP per frame, one WAVE per subframe.  A wave takes its subframe
// from the frame bytes to finished samples without leaving the CU:
//
//   headers                                   layout of src/file/sela_file.cpp:58-91
//   rice::RiceDecoder x2                      src/rice/rice_decoder.cpp:11-61   (segment-parallel, below)
//   dequantise + step-up                      src/lpc/linear_predictor.cpp:16-61
//   lpc::SampleGenerator::generateSamples     src/lpc/sample_generator.cpp:11-30 (lane-ring recurrence, below)
//
// then, after a workgroup barrier, frame::FrameDecoder's second pass (out[ch] = parent - difference,
// src/frame/frame_decoder.cpp:40-69) and the int16 interleave of src/file/wav_file.cpp:244-257, stored
// coalesced.
//
// The synthesis recurrence is a dependent chain of ~90 cycles per sample, so the kernel lives on occupancy:
// what a subframe keeps in LDS is cut to 5.7 KB (28 waves per CU).  The Rice stream is NOT copied on chip --
// it is read where it lies through a bounds-checked buffer resource (reads past the subframe's words
// return zero) -- the parser leaves one 16-bit POSITION per codeword instead of a 32-bit value, the
// residues of a block of 64 samples are decoded from those positions just in time (the loads are in
// flight during the previous block's 64 steps), and the finished samples go over the positions as int16
// (the WAV writer truncates to 16 bits anyway, and (parent - difference) mod 2^16 only needs 16 bits).
//
// ---- Rice parsing across the lanes of a wave ------------------------------------------------------------
// A Golomb-Rice stream is a serial bit parse -- where codeword i+1 starts depends on codeword i -- but it
// RESYNCHRONISES: a parser dropped at an arbitrary bit is in step with the true parse after a few
// codewords (inside a unary run it is in step at the next terminator; inside a remainder field it has a
// chance of roughly E[quotient]/k per codeword).  So every lane gets a ZONE of the stream (whole words):
//
//   phase A  lane i parses from the first bit of its zone to the zone's end and sets one bit per codeword
//            start in a bitmap (only lane i writes its zone's words);
//   phase B  lane i keeps going through the following zones until it stands on a start that a later lane
//            marked: from there on the two trajectories are one.  m_i = that position (or "end of stream");
//   resolve  the true trajectory starts at the stream's first bit in its first lane; it follows that lane's
//            path to m, which lies in the zone of a later lane j AND on lane j's path, then lane j's path to
//            m_j, ... (a walk of <= 64 hops on the scalar unit).  Lanes the chain skips were never in step
//            and list nothing.  A lane on the chain counts its codewords from its true entry (popcount
//            of its bitmap words + what it parsed in phase B); an exclusive scan gives the index of its
//            first value;
//   pass 2   the lanes on the chain walk their codewords once more from their true entries, in parallel, and
//            write every start position to pos[] (over the bitmap, which is dead by then).
//
// All three walks take four codewords per memory round trip (a 160-bit window per lane) while every lane's
// codewords are short, and one at a time otherwise (unary runs longer than the window, k = 31).  The first
// kCoefLanes lanes do the same for the coefficient stream (<= 100 codewords, its own k), in the same loops:
// both streams are zones of ONE bit space, the subframe's aligned words.  tools/parse_model.py is an
// executable model of this algorithm; tests/test_host_logic.py runs it against the CPU oracle.
//
// A frame with a subframe that does not fit the LDS plan (a Rice stream longer than any 16-bit audio produces)
// takes the GENERIC mode of the same kernel: a plain serial parse into the workspace, then the same synthesis.
// Slow, complete, and never needed by files the encoder writes.  Frames of more than 8 channels (up to the 255 the
// header's field carries) are decoded by k_decode_frames_wide, eight subframes at a time.
#include <atomic>

#include "sela_host.h"

#include "sela_synth.h"

namespace sela {

#include "sela_decode_core.inc" // the parser, the synthesis, the header walk: shared with sela_decode32.hip

// kProf: also write per-phase cycle counts (debug hook sela_hip_debug_phase_buffer; 16 uint64 per subframe).
template <bool kProf>
__global__ __launch_bounds__(kDecMaxWaves * 64) __attribute__((amdgpu_waves_per_eu(7, 8))) void k_decode_frames(const uint8_t* __restrict__ frames,
    const uint64_t* __restrict__ frame_offsets, uint32_t n_frames, uint32_t channels, int16_t* __restrict__ pcm_out,
    uint32_t* __restrict__ status, int32_t* __restrict__ ws_residues, uint64_t* __restrict__ phase_cycles,
    uint8_t* __restrict__ frame_flags /* or null: one byte per (frame, wave), written only when not zero */,
    uint32_t vec_shift_from /* frames from this one on run the synthesis with the shift on the vector side (synth_steps) */,
    uint32_t synth_priorities /* s_setprio through the synthesis by the subframe's order class: byte 0 orders <= 48, 1 <= 60, 2 above; 0: none */,
    const uint32_t* __restrict__ n_frames_found /* or null: frames from *n_frames_found on are not decoded (sela_hip_decode_payload_device) */)
{
    long long stamp[10];
    for (int i = 0; i < 10; i++)
        stamp[i] = 0;
    uint32_t prof_sub = kNoSubframe;
    if (kProf)
        stamp[0] = clock64();
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    const int n_waves = blockDim.x / 64;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / 64)), lane = threadIdx.x % 64;
    const DecFrameLds l = carve_frame_lds(dyn, channels, n_waves);

    const uint32_t f = blockIdx.x;
    if (f >= n_frames || (n_frames_found && f >= *n_frames_found))
        return;
    const bool vec_shift = f >= vec_shift_from;
    const uint8_t* const fb = frames + frame_offsets[f];
    const uint64_t fbytes = frame_offsets[f + 1] - frame_offsets[f];
    uint32_t flags = 0;
    SubHeader hd;
    bool ok;
    const bool fast = frame_prologue(l, fb, fbytes, channels, n_waves, wave, lane, hd, ok);
    if (kProf)
        stamp[1] = clock64();

    for (uint32_t c = wave; c < channels; c += n_waves) {
        if (c != (uint32_t)wave) {
            hd = walk_headers(fb, fbytes, c);
            ok = block_header_ok(hd, channels);
        }
        if (!ok) {
            flags |= SELA_HIP_FLAG_BAD_FRAME;
            continue;
        }
        if (kProf)
            prof_sub = c;
        decode_subframe<kProf>(fb, fbytes, hd, fast, l.sub + c, l.scratch0 + wave, ws_residues, (size_t)f * channels + c, vec_shift, synth_priorities, lane, flags, stamp);
        if (lane == 0)
            l.sub_info[hd.channel] = sub_info_word(hd.type, hd.parent, c);
    }
    __syncthreads();

    // ---- second pass + interleave to int16, stored coalesced ------------------------------------------------------------
    if (channels == 2) {
        // stereo: four samples of both channels per thread, one 16-byte store
        const StereoPass sp = stereo_pass(l.sub, l.sub_info);
        uint4* out = reinterpret_cast<uint4*>(pcm_out + (size_t)f * kBlock * 2);
        for (uint32_t i4 = threadIdx.x; i4 < (uint32_t)kBlock / 4; i4 += blockDim.x)
            out[i4] = stereo_words(sp, i4);
    } else {
        for (uint32_t i = threadIdx.x; i < (uint32_t)kBlock; i += blockDim.x)
            for (uint32_t c = 0; c < channels; c++)
                pcm_out[((size_t)f * kBlock + i) * channels + c] = (int16_t)(uint16_t)channel_value16(l.sub, l.sub_info, c, i);
    }
    if (threadIdx.x == 0)
        flags |= layout_flags(l.sub_info, channels);
    flags = wave_or(flags);
    if (lane == 0 && flags) {
        if (frame_flags) // (the host pipeline: page-locked host memory, zeroed by the host; a plain store, no atomics over the link)
            frame_flags[(size_t)f * n_waves + wave] = (uint8_t)flags;
        else {
            atomicOr(&status[0], flags);
            if (wave == 0 && (flags & SELA_HIP_FLAG_BAD_FRAME))
                atomicAdd(&status[1], 1u);
        }
    }
    if (kProf && lane == 0 && prof_sub != kNoSubframe) { // (one subframe per wave is reported)
        stamp[9] = clock64();
        for (int i = 0; i < 9; i++)
            phase_cycles[((size_t)f * channels + prof_sub) * 16 + i] = (uint64_t)(stamp[i + 1] - stamp[i]);
    }
}


// ---- more than eight channels: k_decode_frames_wide ---------------------------------------------------------------
// frame::FrameDecoder::process takes any channel count the header's 8-bit field carries (src/frame/frame_decoder.cpp:
// 11-72).  k_decode_frames keeps every channel of a frame in LDS until the parent - difference pass, which bounds it
// (one wave and one 4.5 KB record per channel).  Here the eight waves of a workgroup take the frame's subframes in
// rounds, each wave with a record of its own: a subframe goes from the frame bytes to finished samples through the same
// decode_subframe (the segment-parallel parse when it fits the plan, the serial parse into the workspace otherwise --
// decided per SUBFRAME: no other wave depends on this one's record) and leaves its raw samples in the output, strided.  The
// second pass (src/frame/frame_decoder.cpp:40-69) then runs over the output: a difference-coded channel becomes parent -
// difference, where the parent's samples are the raw ones an independent subframe left there.  The reference's encoder
// writes difference subframes for exactly-stereo input only (src/frame/frame_encoder.cpp:18), so for these frames the
// pass has nothing to do -- but files are input, not promises.
__global__ __launch_bounds__(kDecMaxWaves * 64) void k_decode_frames_wide(const uint8_t* __restrict__ frames,
    const uint64_t* __restrict__ frame_offsets, uint32_t n_frames, uint32_t channels, int16_t* __restrict__ pcm_out,
    uint32_t* __restrict__ status, int32_t* __restrict__ ws_residues, uint8_t* __restrict__ frame_flags, uint32_t vec_shift_from,
    const uint32_t* __restrict__ n_frames_found /* or null, as in k_decode_frames */)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / 64)), lane = threadIdx.x % 64;
    DecSubframeLds* const sl = reinterpret_cast<DecSubframeLds*>(dyn) + wave;
    DecWaveScratch* const scratch = reinterpret_cast<DecWaveScratch*>(dyn + (size_t)kDecMaxWaves * sizeof(DecSubframeLds)) + wave;
    uint32_t* const sub_info = reinterpret_cast<uint32_t*>(dyn + (size_t)kDecMaxWaves * (sizeof(DecSubframeLds) + sizeof(DecWaveScratch)));
    const uint32_t f = blockIdx.x;
    if (f >= n_frames || (n_frames_found && f >= *n_frames_found))
        return;
    const bool vec_shift = f >= vec_shift_from;
    const uint8_t* const fb = frames + frame_offsets[f];
    const uint64_t fbytes = frame_offsets[f + 1] - frame_offsets[f];
    uint32_t flags = 0;
    for (uint32_t c = threadIdx.x; c < channels; c += blockDim.x)
        sub_info[c] = kNoSubframe;
    __syncthreads();
    HeaderCursor cur = frame_cursor(fb, fbytes);
    int16_t* const out_frame = pcm_out + (size_t)f * kBlock * channels;
    for (uint32_t c = wave; c < channels; c += kDecMaxWaves) {
        const SubHeader hd = walk_to(fb, fbytes, cur, c);
        if (!block_header_ok(hd, channels)) {
            flags |= SELA_HIP_FLAG_BAD_FRAME;
            continue;
        }
        // (hd.order <= 100 <= 2 waves' worth: checked by block_header_ok)
        decode_subframe<false>(fb, fbytes, hd, hd.cw + 2 + hd.rw <= (uint32_t)kStreamCap, sl, scratch, ws_residues, (size_t)f * channels + c, vec_shift, 0, lane, flags, nullptr);
        // the raw samples of this subframe, where its channel lies in the output (mod 2^16: src/file/wav_file.cpp:248-251)
        for (int i = lane; i < kBlock; i += kWave)
            out_frame[(size_t)i * channels + hd.channel] = sl->smp[i];
        wave_sync(); // (the record is reused by this wave's next subframe)
        if (lane == 0)
            sub_info[hd.channel] = sub_info_word(hd.type, hd.parent, 0);
    }
    // ---- second pass of frame::FrameDecoder, over the output -----------------------------------------------------------
    // Writers and readers are waves of ONE workgroup, i.e. of one CU behind one L2: the stores only have to have left the
    // CU (the wait is written out -- a fence's own wait is dropped when the compiler believes nothing is outstanding,
    // MI355X_MICROARCH.md "inter-workgroup visibility"), and nothing older may be served from its vector cache.  (A release
    // fence at agent scope would write back the whole L2 for nothing.)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    for (uint32_t c = 0; c < channels; c++) {
        const uint32_t info = sub_info[c]; // (wave-uniform)
        if (info == kNoSubframe) { // a channel that no valid subframe delivered decodes to silence
            for (uint32_t i = threadIdx.x; i < (uint32_t)kBlock; i += blockDim.x)
                out_frame[(size_t)i * channels + c] = 0;
            if (threadIdx.x == 0)
                flags |= SELA_HIP_FLAG_BAD_FRAME;
        } else if (sub_info_type(info) == 1) {
            const uint32_t parent = sub_info_parent(info);
            const uint32_t pinfo = sub_info[parent];
            if (threadIdx.x == 0 && parent_refused(pinfo)) // (flagged, and a dependent parent's raw samples taken)
                flags |= SELA_HIP_FLAG_BAD_FRAME;
            for (uint32_t i = threadIdx.x; i < (uint32_t)kBlock; i += blockDim.x) {
                const uint32_t pv = pinfo == kNoSubframe ? 0u : (uint32_t)(uint16_t)out_frame[(size_t)i * channels + parent];
                const uint32_t dv = (uint32_t)(uint16_t)out_frame[(size_t)i * channels + c];
                out_frame[(size_t)i * channels + c] = (int16_t)(uint16_t)(pv - dv);
            }
        }
    }
    flags = wave_or(flags);
    if (lane == 0 && flags) {
        if (frame_flags)
            frame_flags[(size_t)f * kDecMaxWaves + wave] = (uint8_t)flags;
        else {
            atomicOr(&status[0], flags);
            if (wave == 0 && (flags & SELA_HIP_FLAG_BAD_FRAME))
                atomicAdd(&status[1], 1u);
        }
    }
}

int decode_waves(uint32_t channels)
{
    return channels < (uint32_t)kDecMaxWaves ? (int)channels : kDecMaxWaves;
}

size_t decode_lds_bytes(uint32_t channels) { return decode_lds_bytes_for(channels, decode_waves(channels)); }

uint32_t decode_max_channels() { return (uint32_t)kDecMaxChannels; }

// Generic mode parks the residues of a subframe here (int32[2048]); the usual path never touches it.
int32_t* carve_decode(Carve& c, uint32_t n_frames, uint32_t channels) { return c.take<int32_t>((uint64_t)n_frames * channels * kBlock); }
size_t decode_workspace_bytes(uint32_t n_frames, uint32_t channels, Carve* at)
{
    return measured(at, [&](Carve& c) { carve_decode(c, n_frames, channels); });
}

// Which workgroups of a launch run their recurrence in the form for a wave that has its SIMD (nearly) to itself
// (synth_steps, kVecShift): all of them when the whole launch is at most kLonelyWaves waves, else those of the last, partial
// round of resident workgroups if that round is as small -- they start when the rounds before them are done.
struct DecodeResidency {
    std::atomic<uint32_t> frames[kResidencySlots][64][kDecMaxWaves + 1]; // [kernel slot][device][waves per workgroup]: workgroups the device holds at once, 0 = not asked yet
};
uint32_t resident_frames(const void* kernel, int n_waves, size_t lds, int slot)
{
    static DecodeResidency cache;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64 || slot < 0 || slot >= kResidencySlots || n_waves < 0 || n_waves > kDecMaxWaves)
        return 0;
    uint32_t have = cache.frames[slot][dev][n_waves].load(std::memory_order_relaxed);
    if (have == 0) {
        int per_cu = 0, cus = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, n_waves * 64, lds) != hipSuccess
            || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || per_cu <= 0 || cus <= 0)
            return 0;
        have = (uint32_t)per_cu * (uint32_t)cus;
        cache.frames[slot][dev][n_waves].store(have, std::memory_order_relaxed);
    }
    return have;
}
uint32_t vec_shift_from_for(uint32_t n_frames, int n_waves, uint32_t resident)
{
    if ((uint64_t)n_frames * (uint32_t)n_waves <= kLonelyWaves)
        return 0;
    if (resident == 0)
        return n_frames;
    const uint32_t last_round = n_frames / resident * resident; // first frame of the last, partial round
    return (uint64_t)(n_frames - last_round) * (uint32_t)n_waves <= kLonelyWaves ? last_round : n_frames;
}

// ---- the decoder's stages on their own (the reference's public L1 classes) -------------------------------------------------
// lpc::SampleGenerator (src/include/lpc.hpp:106-117, src/lpc/sample_generator.cpp:11-39): order + quantised reflection
// coefficients + 2048 residues -> 2048 samples, one wave per block, through the very dequantisation, step-up, table and
// recurrence the frame kernels run (the residues come from memory as in the generic mode; the samples go out as the 32-bit
// values the reference's class returns -- a difference signal needs 17 bits).
__global__ __launch_bounds__(64) void k_stage_lpc_decode(const int32_t* __restrict__ order_in, const int32_t* __restrict__ q_in,
    const int32_t* __restrict__ residues, uint32_t n_blocks, int32_t* __restrict__ samples_out, int64_t* __restrict__ coefs_out /* [block][101] or null */,
    uint32_t* __restrict__ status)
{
    __shared__ DecWaveScratch scratch;
    const uint32_t b = blockIdx.x;
    if (b >= n_blocks)
        return;
    const int lane = threadIdx.x;
    uint32_t flags = 0;
    const int32_t o = order_in[b];
    if (o < 0 || o > kMaxOrder) {
        if (lane == 0)
            atomicOr(&status[0], (uint32_t)SELA_HIP_FLAG_BAD_FRAME);
        return;
    }
    const uint32_t order = (uint32_t)o;
    const int32_t q_lo = (uint32_t)lane < order ? q_in[(size_t)b * kMaxOrder + lane] : 0;
    const int32_t q_hi = (uint32_t)lane + 64 < order ? q_in[(size_t)b * kMaxOrder + lane + 64] : 0;
    SynthTables* const tables = &scratch.t;
    step_up_from_q(order, q_lo, q_hi, tables->a, lane, flags);
    if (coefs_out) // lpc::LinearPredictor::linearPredictionCoefficients (src/lpc/linear_predictor.cpp:57-60)
        for (uint32_t i = lane; i <= order; i += kWave)
            coefs_out[(size_t)b * (kMaxOrder + 1) + i] = tables->a[i];
    if (samples_out) {
        const bool fits24 = build_synth_table(tables->a, tables->tab, (int)order, lane);
        SynthOut<true> out32;
        out32.samples = samples_out + (size_t)b * kBlock;
        out32.n = (uint32_t)kBlock;
        synthesize_by_order<false, true>(order, nullptr, 0, 0, nullptr, residues + (size_t)b * kBlock, tables->tab, fits24, lane, out32);
    }
    flags = wave_or(flags);
    if (lane == 0 && flags)
        atomicOr(&status[0], flags);
}

// rice::RiceDecoder (src/include/rice.hpp:29-43, src/rice/rice_decoder.cpp:11-61): one wave per stream, the serial parse of the
// generic mode -- count the ones up to the first zero, read k bits MSB first -- for any number of values.
__global__ __launch_bounds__(64) void k_stage_rice_decode(const uint32_t* __restrict__ words, const uint64_t* __restrict__ word_offsets,
    const uint32_t* __restrict__ k_in, const uint64_t* __restrict__ value_offsets, uint32_t n_streams, int32_t* __restrict__ values_out,
    uint32_t* __restrict__ status)
{
    const uint32_t s = blockIdx.x;
    if (s >= n_streams)
        return;
    const int lane = threadIdx.x;
    const uint64_t nw = word_offsets[s + 1] - word_offsets[s], count = value_offsets[s + 1] - value_offsets[s];
    const uint32_t k = k_in[s];
    uint32_t flags = 0;
    if (k >= 32 || nw >= (1ull << 26) || count >= (1ull << 31))
        flags = SELA_HIP_FLAG_BAD_FRAME;
    else
        flags = parse_stream_serial(words + word_offsets[s], 0, (uint32_t)(32 * nw), (uint32_t)nw, k, (uint32_t)count, values_out + value_offsets[s], lane);
    if (lane == 0 && flags)
        atomicOr(&status[0], flags);
}

hipError_t launch_stage_lpc_decode(const int32_t* d_order, const int32_t* d_q, const int32_t* d_residues, uint32_t n_blocks, int32_t* d_samples,
    int64_t* d_coefs, uint32_t* d_status, hipStream_t stream)
{
    if (n_blocks)
        hipLaunchKernelGGL(k_stage_lpc_decode, dim3(n_blocks), dim3(64), 0, stream, d_order, d_q, d_residues, n_blocks, d_samples, d_coefs, d_status);
    return hipGetLastError();
}

hipError_t launch_stage_rice_decode(const uint32_t* d_words, const uint64_t* d_word_offsets, const uint32_t* d_k, const uint64_t* d_value_offsets,
    uint32_t n_streams, int32_t* d_values, uint32_t* d_status, hipStream_t stream)
{
    if (n_streams)
        hipLaunchKernelGGL(k_stage_rice_decode, dim3(n_streams), dim3(64), 0, stream, d_words, d_word_offsets, d_k, d_value_offsets, n_streams, d_values, d_status);
    return hipGetLastError();
}

hipError_t launch_decode(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames, uint32_t channels,
    int16_t* d_pcm_out, uint32_t* d_status, void* d_workspace, hipStream_t stream, hipEvent_t* ev /* 2 events or nullptr */,
    uint64_t* d_phase_cycles, uint8_t* frame_flags /* null: flags go to d_status, which is zeroed here */,
    int recurrence_form /* -1: by launch size (vec_shift_from_for); 0 / 1: every frame in the scalar- / vector-shift form (tests) */,
    uint32_t synth_priorities /* s_setprio through the synthesis by order class (k_decode_frames); 0: none.  A launch that has the
                                 device to itself raises the subframes of orders above 60 -- two registers per lane, 1.6 x the
                                 synthesis work, 31 % of the bench track's subframes -- so that they do not finish last:
                                 k_decode_frames 0.247 -> 0.240 ms at 3875 frames, one lane +1.1 %; beside another stream's
                                 kernels the same costs 0.4 %, so the caller passes 0 there */,
    const uint32_t* d_n_found /* or null: the device's own count of frames to decode, at most n_frames (the grid and the
                                 choices above are made for n_frames) */,
    bool zero_status /* false: d_status keeps what it holds and the kernels add to it (sela_hip_decode_n_device: the sample index
                        wrote it) */)
{
    hipError_t err = frame_flags || !zero_status ? hipSuccess : hipMemsetAsync(d_status, 0, 4 * sizeof(uint32_t), stream);
    if (err != hipSuccess || n_frames == 0)
        return err;
    const int n_waves = decode_waves(channels);
    if (channels > (uint32_t)kDecMaxChannels)
        return hipErrorInvalidValue;
    Carve carve(d_workspace);
    int32_t* const ws = carve_decode(carve, n_frames, channels);
    if (channels > (uint32_t)kDecMaxWaves) { // more channels than a workgroup has waves: rounds (k_decode_frames_wide)
        if (d_phase_cycles)
            return hipErrorInvalidValue; // (the phase counts are the one-wave-per-subframe kernel's)
        const size_t lds = (size_t)kDecMaxWaves * (sizeof(DecSubframeLds) + sizeof(DecWaveScratch)) + (size_t)channels * 4;
        if (ev)
            (void)hipEventRecord(ev[0], stream);
        const uint32_t from = recurrence_form >= 0 ? (recurrence_form ? 0u : n_frames)
                                                   : vec_shift_from_for(n_frames, kDecMaxWaves, resident_frames(reinterpret_cast<const void*>(k_decode_frames_wide), kDecMaxWaves, lds));
        hipLaunchKernelGGL(k_decode_frames_wide, dim3(n_frames), dim3(kDecMaxWaves * 64), lds, stream, d_frames, d_frame_offsets, n_frames, channels,
            d_pcm_out, d_status, ws, frame_flags, from, d_n_found);
        if (ev)
            (void)hipEventRecord(ev[1], stream);
        return hipGetLastError();
    }
    const size_t need = decode_lds_bytes(channels);
    // (Capping the occupancy so that a batch fills whole rounds of resident workgroups was tried -- extra dynamic
    // LDS -- and lost at every batch size: the recurrence is latency-bound per wave, more waves always overlap more.)
    const size_t lds = need;
    if (lds > 64 * 1024) { // above the default dynamic-LDS limit (more than four channels); per device, so every time
        err = d_phase_cycles
            ? hipFuncSetAttribute(reinterpret_cast<const void*>(k_decode_frames<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)
            : hipFuncSetAttribute(reinterpret_cast<const void*>(k_decode_frames<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (err != hipSuccess)
            return err;
    }
    const uint32_t from = recurrence_form >= 0 ? (recurrence_form ? 0u : n_frames)
                                                : vec_shift_from_for(n_frames, n_waves, resident_frames(reinterpret_cast<const void*>(k_decode_frames<false>), n_waves, lds));
    const uint32_t synth_prio = synth_priorities;
    if (ev)
        (void)hipEventRecord(ev[0], stream);
    if (d_phase_cycles)
        hipLaunchKernelGGL(k_decode_frames<true>, dim3(n_frames), dim3(n_waves * 64), lds, stream, d_frames, d_frame_offsets, n_frames, channels,
            d_pcm_out, d_status, ws, d_phase_cycles, frame_flags, from, synth_prio, d_n_found);
    else
        hipLaunchKernelGGL(k_decode_frames<false>, dim3(n_frames), dim3(n_waves * 64), lds, stream, d_frames, d_frame_offsets, n_frames, channels,
            d_pcm_out, d_status, ws, d_phase_cycles, frame_flags, from, synth_prio, d_n_found);
    if (ev)
        (void)hipEventRecord(ev[1], stream);
    return hipGetLastError();
}

// ---- the frames of a payload found on the device ------------------------------------------------------------------------
#include "sela_index.inc"

} // namespace sela
