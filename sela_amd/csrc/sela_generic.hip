// sela_generic.hip -- the frame path for ANY block length and 32-bit samples (gfx950).
//
// The reference's frame API is length-agnostic and 32-bit: data::WavFrame carries int32 samples per channel
// (src/include/data/wav_frame.hpp:8-16), lpc::ResidueGenerator loops over samples.size() (src/lpc/residue_generator.cpp:12-45,
// 98-119), a subframe brings its own samplesPerChannel (src/include/data/sela_sub_frame.hpp:27,
// src/frame/frame_decoder.cpp:24-25,48-49) and frame::FrameDecoder returns untruncated int32 (frame_decoder.cpp:64-71).
// The fast kernels (sela_encode.hip, sela_decode.hip) are built around the one shape the reference's CLI produces --
// 2048 samples of 16-bit PCM -- and everything else comes here: the same arithmetic, bit for bit, with the length a run-time
// value (1 .. 65535: the u16 field) and nothing assumed about the samples.  One wave per block / subframe: the fast kernels'
// loops with a run-time length (round 6), global-memory scratch between the kernels; the route for callers of the frame classes
// with other shapes, not the one bench.py's headline times.
//
// Encode: k_generic_analyse (samples -> order, q[], residues, the two Rice plans) -> k_generic_plan (stereo decision, frame
// sizes, offsets) -> k_generic_pack (the chosen candidates' Rice streams) -> k_generic_assemble (on-disk bytes).
// Decode: k_decode_subframes32 (sela_decode32.hip: the fast decoder's lane-parallel parse and tuned synthesis, any length, 32-bit)
// or, for what that kernel will not judge, k_generic_decode (one wave per subframe: headers, a serial Rice walk, synthesis)
// -> k_generic_combine (independent subframes first, then dependent ones in subframe order: src/frame/frame_decoder.cpp:17-69).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>

#include "sela_host.h"

namespace sela {

namespace {

__device__ __forceinline__ uint64_t wave_sum_wrap(uint64_t v) // sum over the 64 lanes mod 2^64 (wave-uniform result)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m, 64);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m, 64);
        v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}

// (int32)double as the x86 build of the reference converts (cvttsd2si: INT32_MIN for anything outside)
__device__ __forceinline__ int32_t trunc_to_i32(double v)
{
    if (!(v > -2147483649.0 && v < 2147483648.0))
        return INT32_MIN;
    return (int32_t)v;
}

// OR the low `nbits` (1..32) of v into a zeroed word buffer (global memory or LDS) at bit position pos
__device__ __forceinline__ void or_bits(uint32_t* buf, uint64_t pos, uint32_t v, uint32_t nbits)
{
    const uint64_t w = pos >> 5;
    const uint32_t sh = (uint32_t)pos & 31;
    atomicOr(&buf[w], v << sh);
    if (sh + nbits > 32)
        atomicOr(&buf[w + 1], v >> (32 - sh));
}

// one Golomb-Rice codeword (src/rice/rice_encoder.cpp:41-53): u >> k ones, a zero, the low k bits MSB first
__device__ inline void put_codeword(uint32_t* buf, uint64_t pos, uint32_t u, uint32_t k)
{
    uint32_t ones = u >> k;
    const uint32_t rem = k ? __brev(u << (32 - k)) : 0u;
    while (ones >= 32) {
        or_bits(buf, pos, 0xFFFFFFFFu, 32);
        pos += 32;
        ones -= 32;
    }
    or_bits(buf, pos, (1u << ones) - 1u, ones + 1); // the ones and their terminator (a zero: nothing to OR)
    pos += ones + 1;
    if (k)
        or_bits(buf, pos, rem, k);
}

// pack the stream v[0..n) with parameter k into zeroed words (src/rice/rice_encoder.cpp:35-71).
// Round 6: 1024 values at a time, lane L owning 16 CONSECUTIVE values (staged through LDS so that the loads are coalesced and the
// lanes' reads fall on different banks) -- ONE scan of the lanes' bit counts per stretch, every codeword of at most 32 bits OR-ed
// into the LDS window without a branch -- and the window leaves as whole words: plain stores, but for the stretch's first and
// last word, which its neighbours share (an atomic OR each).  A stretch whose quotients are long (a lane's bits beyond 2^26) or
// whose bits do not fit the window goes 64 codewords at a time as the first version did for every round (rice_pack_round).
constexpr uint32_t kPackPerLane = 16;                         // consecutive values a lane owns in a stretch
constexpr uint32_t kPackStretch = 64 * kPackPerLane;         // 1024 values
constexpr uint32_t kPackWindow = 1152;  // words: 36,864 bits for 1024 codewords (36 bits each), and room for the 1024 staged values
                                        // (1088 words: one pad word per 16).  4.6 KB per wave: eight waves per SIMD (a stretch of 2048
                                        // values in a window of 9.2 KB, four waves per SIMD: 110 us for 7750 subframes of 2048 samples)

// 64 codewords at bit position `base` of the stream: lane = codeword
__device__ inline uint64_t rice_pack_round(uint32_t u, bool valid, uint32_t k, uint32_t* out, uint64_t base, int lane, uint32_t* win)
{
    const uint64_t len = valid ? (uint64_t)(u >> k) + 1 + k : 0;
    uint64_t incl = len;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)incl, d, 64);
        const uint32_t hi = (uint32_t)__shfl_up((int)(uint32_t)(incl >> 32), d, 64);
        if (lane >= d)
            incl += ((uint64_t)hi << 32) | lo;
    }
    const uint32_t tlo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)incl, 63);
    const uint32_t thi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(incl >> 32), 63);
    const uint64_t total = ((uint64_t)thi << 32) | tlo; // the round's bits (wave-uniform)
    const uint64_t first_word = base >> 5, span = ((base + total + 31) >> 5) - first_word;
    if (span <= kPackWindow) {
        for (uint32_t w = lane; w < (uint32_t)span; w += 64)
            win[w] = 0;
        wave_sync();
        if (valid)
            put_codeword(win, (base & 31) + incl - len, u, k);
        wave_sync();
        for (uint32_t w = lane; w < (uint32_t)span; w += 64) {
            const uint32_t x = win[w];
            if (x == 0)
                continue; // (the words are zeroed)
            if (w == 0 || w + 1 == (uint32_t)span)
                atomicOr(&out[first_word + w], x);
            else
                out[first_word + w] = x;
        }
        wave_sync();
    } else if (valid) {
        put_codeword(out, base + incl - len, u, k); // piece by piece, straight into memory
    }
    return total;
}

// (a stretch's values as they come from memory: lane L holds values L, L + 64, ..; beyond n: 0)
__device__ __forceinline__ void pack_fetch(const int32_t* v, uint32_t n, uint32_t i0, int lane, int32_t (&raw)[kPackPerLane])
{
#pragma unroll
    for (int t = 0; t < (int)kPackPerLane; t++) {
        const uint32_t i = i0 + (uint32_t)lane + 64u * (uint32_t)t;
        raw[t] = i < n ? v[i] : 0;
    }
}

// kFetched: the first stretch's values are in `raw` already.  A wave of k_generic_pack is a chain of trips to memory -- two thousand
// vector instructions in 27 us, SQ_WAIT_ANY 70 % of its cycles -- and every trip taken early is one less: the kernel asks for the
// block's record, its coefficients and its first 1024 residues together, and a stretch is asked for before the one in front of it is
// packed: 80 -> 60 us for 7750 subframes of 2048 (more waves per SIMD do not help it: its 160 registers are live values; forced to
// 128 it spills 9 and takes 57 us, to 96 it spills 735 and takes 444).
template <bool kFetched>
__device__ inline void rice_pack_stream(const int32_t* v, uint32_t n, uint32_t k, uint32_t* out, int lane, uint32_t* win, int32_t (&raw)[kPackPerLane])
{
    uint64_t base = 0;
    if (!kFetched)
        pack_fetch(v, n, 0, lane, raw);
    for (uint32_t i0 = 0; i0 < n; i0 += kPackStretch) {
        const uint32_t in_stretch = min(kPackStretch, n - i0);
        // stage: value i of the stretch at word i + i / 16
#pragma unroll
        for (int t = 0; t < (int)kPackPerLane; t++) {
            const uint32_t i = (uint32_t)lane + 64u * (uint32_t)t;
            if (i < in_stretch)
                win[i + (i >> 4)] = zigzag32(raw[t]);
        }
        if (i0 + kPackStretch < n)
            pack_fetch(v, n, i0 + kPackStretch, lane, raw);
        wave_sync();
        uint32_t u[kPackPerLane];
        const uint32_t mine = in_stretch > kPackPerLane * (uint32_t)lane ? min(kPackPerLane, in_stretch - kPackPerLane * (uint32_t)lane) : 0u;
        uint32_t bits = 0, longest = 0;
#pragma unroll
        for (int t = 0; t < (int)kPackPerLane; t++) {
            u[t] = (uint32_t)t < mine ? win[(kPackPerLane + 1) * lane + t] : 0u;
            const uint32_t q = u[t] >> k;
            longest = max(longest, q);
            bits += (uint32_t)t < mine ? q + 1 + k : 0u; // (may wrap when a quotient is long: then `longest` says so)
        }
        wave_sync(); // the staged values are in registers: the window is free
        const bool easy = !__any(longest >= (1u << 20)); // a lane's bits below 2^25, the stretch's below 2^32
        uint32_t at = 0, total = 0;
        if (easy) {
            at = wave_exclusive_scan(bits, lane);
            total = (uint32_t)__builtin_amdgcn_readlane((int)(at + bits), 63);
        }
        const uint64_t first_word = base >> 5;
        const uint32_t span = easy ? (uint32_t)((((base & 31) + total + 31) >> 5)) : 0u;
        if (easy && span + 1 <= kPackWindow) {
            for (uint32_t w = lane; w <= span; w += 64) // (one word to spare: or_bits_both touches the word behind a codeword's last)
                win[w] = 0;
            wave_sync();
            uint32_t pos = (uint32_t)(base & 31) + at;
#pragma unroll
            for (int t = 0; t < (int)kPackPerLane; t++) {
                if ((uint32_t)t < mine) {
                    const uint32_t ones = u[t] >> k, len = ones + 1 + k;
                    if (len <= 32) {
                        const uint32_t rem = __builtin_amdgcn_ubfe(__brev(u[t]), 32 - k, k); // the low k bits, the first one the most significant
                        const uint64_t wide = (uint64_t)(((1u << ones) - 1u) | (rem << ((ones + 1) & 31))) << (pos & 31);
                        atomicOr(&win[pos >> 5], (uint32_t)wide);
                        atomicOr(&win[(pos >> 5) + 1], (uint32_t)(wide >> 32));
                    } else {
                        put_codeword(win, pos, u[t], k);
                    }
                    pos += len;
                }
            }
            wave_sync();
            for (uint32_t w = lane; w < span; w += 64) {
                const uint32_t x = win[w];
                if (x == 0)
                    continue; // (the words are zeroed)
                if (w == 0 || w + 1 == span)
                    atomicOr(&out[first_word + w], x);
                else
                    out[first_word + w] = x;
            }
            wave_sync();
            base += total;
        } else { // long quotients, or more bits than the window holds: 64 codewords at a time, codeword i of the stretch in lane i % 64
            // (rice_pack_round uses the window too, so round by round from the registers)
            for (uint32_t r0 = 0; r0 < in_stretch; r0 += 64) {
                // codeword r0 + lane lives in lane (r0 + lane) / 16's register (r0 + lane) % 16
                const uint32_t src_lane = (r0 + (uint32_t)lane) / kPackPerLane;
                uint32_t mine_u = 0;
#pragma unroll
                for (int t = 0; t < (int)kPackPerLane; t++) {
                    const uint32_t got = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(4 * src_lane), (int)u[t]);
                    mine_u = (((r0 + (uint32_t)lane) % kPackPerLane) == (uint32_t)t) ? got : mine_u;
                }
                base += rice_pack_round(mine_u, r0 + lane < in_stretch, k, out, base, lane, win);
            }
        }
    }
}

} // namespace

// ---- analysis: one wave per (frame, signal) -------------------------------------------------------------------------------
// lpc::ResidueGenerator::process (src/lpc/residue_generator.cpp:121-134) as written, with samples.size() = n:
//   x[j] = s[j] / 32767 (:12-18);  mean = (sequential sum) / n (:27-30);  ac[lag] = sequential sum over j = lag .. n-1 of
//   (x[j] - mean) * (x[j - lag] - mean), lag = 0..100 (:33-38);  Schur (:47-68);  order (:70-78);  quantise (:80-96);
//   dequantise + step-up (linear_predictor.cpp:16-61);  residues (:98-119);  then both Rice plans (rice_encoder.cpp:20-33, 37).
//
// Round 6: the loops of the fast kernels (sela_encode.hip) with the length a run-time value -- the first version walked
// every chain through v_readlane and moved its windows by DPP, 45 k vector instructions for a block of 2048 samples.
//   mean            a chunk of 64 quotients goes to LDS and comes back by same-address reads: one v_add_f64 per sample.
//   autocorrelation lane L owns lags 2L and 2L + 1 (51 lanes): its two window values are c[j - 2L] and the one before, so a
//                   step needs ONE new value per lane -- from a ring of 256 centred samples in LDS (+ 64 mirrored behind its
//                   end: the 64 reads of a chunk have compile-time offsets) -- the wave-uniform c[j] by a same-address read of
//                   the same ring, two multiplies and two adds: every product rounded before it is added, every accumulator
//                   in ascending j.
//   Schur           in registers: lane L holds columns 2L, 2L + 1 of gen0 / gen1; gen1[j + 1] of the odd column is the next
//                   lane's register (one DPP move of 64 bits per stage).
//   residues        1024 samples at a time, lane L owning 16 CONSECUTIVE samples and sliding a statically addressed window of
//                   16 registers over its history (one new LDS word and 16 multiply-adds per tap) -- in FP64 (v_fma_f64, full
//                   rate) where that is exact: 2^34 + sum |a[j]| x max |s| < 2^53 bounds every partial sum of integers, in any
//                   order.  A block beyond that bound (21-bit noise with a long predictor; nothing 16-bit) takes the 64-bit
//                   wrap-around taps in a window that moves one lane per tap, as the first version did for every block.
//   Rice parameter  by convexity (rice_plan_convex), not by all twenty sums.
// Occupancy is what this kernel lives on -- its mean, its Schur stages and its accumulators are dependent chains -- and the residue
// filter's register window is what bounds it: 32 samples per lane (128 VGPRs of window and sums, 168 in all, 12 KB of LDS) allow three
// waves per SIMD, 16 per lane (125 / 7.9 KB) four or, with 16 registers spilled outside the loops, five: 763 / 667 / 655 us for 11,625
// blocks of 2048 samples.
#define SELA_GEN_WAVES 5
constexpr int kGenPad = 128;                                   // "no sample" / the samples before a stretch, in front of it
constexpr int kGenPerLane = 16;                                // consecutive samples a lane owns in a stretch of the residue filter
constexpr int kGenPadShift = kGenPerLane == 32 ? 5 : 4;        // index i stored at i + (i >> shift): the lanes' strides fall on different banks
constexpr int kGenStretch = kGenPerLane * kWave;               // samples per pass of the residue filter
constexpr int kGenSBufWords = (kGenPad + kGenStretch) + ((kGenPad + kGenStretch) >> kGenPadShift);
static_assert(kGenPerLane == 16 || kGenPerLane == 32, "the window is a power of two of registers");
constexpr int kGenRing = 256, kGenMirror = 64;

struct AnalyseLds {
    union {
        struct {
            alignas(16) double ring[kGenRing + kGenMirror];
            alignas(16) double chunk[64];
        } ac;
        int32_t st[kGenSBufWords];
    };
    double kk[104];   // reflection coefficients, then the dequantised ones
    int64_t a[104];   // Q35 predictor
    double af[104];   // the same as doubles (FP64 taps)
    int32_t q[128];
};

typedef const volatile __attribute__((address_space(3))) double* LdsDoubles; // (volatile: the reads stay ds_read_b64, 2 LDS cycles each)
// Two neighbours at once.  Lane L's window starts 2 L doubles below lane 0's, a stride of 16 bytes: as ds_read_b64 the two halves
// of a half-wave fall on the same banks (SQ_LDS_BANK_CONFLICT 23 % of SQ_LDS_IDX_ACTIVE), as ds_read_b128 the 64 lanes read 1 KB
// of consecutive LDS, four conflict-free passes for two steps' values.
typedef double __attribute__((ext_vector_type(2))) DoublePair;
typedef const volatile __attribute__((address_space(3))) DoublePair* LdsPairs;

// x = s / 32767 (src/lpc/residue_generator.cpp:12-18): q0 = s * RN(1/32767), one residual fma, one correction fma equal the
// correctly rounded quotient for every |s| <= 70000 (exhaustive check: tests/test_host_logic.py); anything larger divides.
__device__ __forceinline__ double scale_any(int32_t v, bool small /* wave-uniform: every lane's |v| <= 70000 */)
{
    if (small) {
        constexpr double r = 1.0 / SELA_SAMPLE_SCALE;
        const double x = (double)v;
        const double q0 = x * r;
        const double e = __builtin_fma(-SELA_SAMPLE_SCALE, q0, x);
        return __builtin_fma(e, r, q0);
    }
    return (double)v / SELA_SAMPLE_SCALE;
}

// Taps j0 + JJ + 1 .. j0 + kGenPerLane of the residue filter in FP64 (the window of sela_encode.hip's fir_taps_f64): tap j uses
// win[(t - j) mod kGenPerLane] = s[kGenPerLane lane + t - j] and loads the one new element s[kGenPerLane lane - j].
template <int JJ>
__device__ __forceinline__ void gen_taps_f64(int j0, int order, int lane, const int32_t* sT, const double* a_f, double (&win)[kGenPerLane], double (&acc)[kGenPerLane])
{
    const int j = j0 + JJ + 1;
    if (j > order)
        return;
    const double aj = read_first_lane(a_f[j]);
    const int e = kGenPad + kGenPerLane * lane - j;
    win[(kGenPerLane - JJ - 1) & (kGenPerLane - 1)] = (double)sT[e + (e >> kGenPadShift)];
#pragma unroll
    for (int t = 0; t < kGenPerLane; t++)
        acc[t] = __builtin_fma(aj, win[(t - JJ - 1) & (kGenPerLane - 1)], acc[t]);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (JJ < kGenPerLane - 1)
        gen_taps_f64<JJ + 1>(j0, order, lane, sT, a_f, win, acc);
}

// rice::RiceEncoder::calculateOptimumRiceParam (src/rice/rice_encoder.cpp:20-33) for the values load(0 .. n): the FIRST k in
// [0, 20) that minimises bits(k) = sum(u >> k) + n (1 + k).  The reference evaluates all 20 candidates; the same answer needs
// a few of them because bits() is convex in k (the argument of rice_plan, sela_encode.hip): the first minimum is the smallest
// k with T(k) - T(k + 1) <= n, found by walking from a guess near log2(mean u).  Exact 64-bit sums.  t0 = T(0) = sum of the
// zig-zagged values.
template <typename Load>
__device__ __forceinline__ void rice_plan_convex(Load load, uint32_t n, int lane, uint64_t t0, uint32_t& best_k, uint64_t& best_bits)
{
    constexpr uint32_t kLast = SELA_MAX_RICE_PARAM - 1;
    auto T = [&](uint32_t k) -> uint64_t {
        uint64_t part = 0;
        for (uint32_t i = lane; i < n; i += 64)
            part += zigzag32(load(i)) >> k;
        return wave_sum_wrap(part);
    };
    const uint64_t mean = n ? t0 / n : 0;
    uint32_t k = mean ? 63u - (uint32_t)__clzll(mean) : 0u;
    k = k > kLast - 1 ? kLast - 1 : k;
    uint64_t ta = k ? T(k) : t0;
    uint64_t tb = T(k + 1);
    if (ta - tb <= n) { // bits(k + 1) >= bits(k): the first minimum is at or below k
        while (k > 0) {
            const uint64_t tc = k != 1 ? T(k - 1) : t0;
            if (tc - ta > n)
                break;
            k--;
            tb = ta;
            ta = tc;
        }
    } else { // still descending: move up
        for (;;) {
            k++;
            ta = tb;
            if (k == kLast)
                break;
            tb = T(k + 1);
            if (ta - tb <= n)
                break;
        }
    }
    best_k = k;
    best_bits = ta + (uint64_t)n * (1 + k);
}

// kLossless: the residues are taken against the DECODER's prediction -(int32)((2^34 - sum) >> 35)
// (src/lpc/sample_generator.cpp:25-28) -- the encoder's, less one where 2^34 + sum is a multiple of 2^35.
template <bool kIn16, bool kLossless, bool kPaired>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(SELA_GEN_WAVES, SELA_GEN_WAVES))) void k_generic_analyse(const void* __restrict__ input, uint32_t n_frames, uint32_t channels,
    uint32_t n_sig, uint32_t n, int32_t* __restrict__ sig_ws, int32_t* __restrict__ res_ws, int32_t* __restrict__ q_ws, GenericMeta* __restrict__ meta, uint32_t force_wrap_taps /* tests: every block on the 64-bit wrap-around taps */)
{
    __shared__ __attribute__((aligned(16))) AnalyseLds lds;
    const uint32_t b = blockIdx.x;
    if (b >= n_frames * n_sig)
        return;
    const int lane = threadIdx.x;
    const uint32_t f = b / n_sig, sg = b % n_sig;
    int32_t* const s = sig_ws + (size_t)b * n;
    int32_t* const r = res_ws + (size_t)b * n;
    uint32_t flags = 0;

    // ---- the signal: a channel, or channel 0 - channel 1 of an exactly-stereo frame (src/frame/frame_encoder.cpp:18-24) -- with
    //      kPaired signal channels + p is channel 2p - channel 2p + 1 of any frame;
    //      x = s / 32767 and its sequential sum (:27-29) ---------------------------------------------------------------------
    // kPaired is an instantiation of its own, so that the plain calls keep the code they had: with the pair's channel computed for
    // every signal they were 1 % slower.
    const bool is_diff = sg >= channels;
    const uint32_t ca = kPaired && is_diff ? 2 * (sg - channels) : sg; // kPaired: the channel, or the pair's even one
    // int16, interleaved, an even number of channels: a pair's two samples are one 32-bit word, aligned where the input is
    const bool pair_word = kPaired && kIn16 && is_diff && !(channels & 1) && !((uintptr_t)input & 3);
    auto load_sample = [&](uint32_t j) -> int32_t {
        if constexpr (kPaired) {
            if (kIn16) {
                const int16_t* at = static_cast<const int16_t*>(input) + (size_t)f * n * channels + (size_t)j * channels + ca;
                if (!is_diff)
                    return (int32_t)at[0];
                if (pair_word) {
                    const uint32_t two = *reinterpret_cast<const uint32_t*>(at);
                    return (int32_t)(int16_t)two - (int32_t)(int16_t)(two >> 16);
                }
                return (int32_t)at[0] - (int32_t)at[1];
            }
            const int32_t* at = static_cast<const int32_t*>(input) + ((size_t)f * channels + ca) * n + j;
            return is_diff ? (int32_t)((uint32_t)at[0] - (uint32_t)at[n]) : at[0];
        } else {
            if (kIn16) {
                const int16_t* pcm = static_cast<const int16_t*>(input) + (size_t)f * n * channels;
                return sg < channels ? (int32_t)pcm[(size_t)j * channels + sg] : (int32_t)pcm[(size_t)j * channels] - (int32_t)pcm[(size_t)j * channels + 1];
            }
            const int32_t* pl = static_cast<const int32_t*>(input) + (size_t)f * channels * n;
            return sg < channels ? pl[(size_t)sg * n + j] : (int32_t)((uint32_t)pl[j] - (uint32_t)pl[(size_t)n + j]);
        }
    };
    double sum = 0.0;
    uint32_t mag_lane = 0; // the largest |sample| of this lane
    {
        int32_t v_next = (uint32_t)lane < n ? load_sample(lane) : 0;
        for (uint32_t j0 = 0; j0 < n; j0 += 64) {
            const uint32_t j = j0 + lane;
            const bool valid = j < n;
            const int32_t v = v_next;
            if (j0 + 64 < n)
                v_next = j + 64 < n ? load_sample(j + 64) : 0;
            if (valid)
                s[j] = v;
            const uint32_t mag = v < 0 ? 0u - (uint32_t)v : (uint32_t)v;
            mag_lane = max(mag_lane, mag);
            const double x = valid ? scale_any(v, !__any(mag > 70000u)) : 0.0;
            lds.ac.chunk[lane] = x;
            wave_sync();
            const LdsDoubles ch = (LdsDoubles)lds.ac.chunk;
            if (n - j0 >= 64u) {
                const LdsPairs cp = (LdsPairs)lds.ac.chunk;
#pragma unroll
                for (int l = 0; l < 32; l++) {
                    const DoublePair two = cp[l];
                    sum += two.x;
                    sum += two.y;
                }
            } else {
                const int cnt = (int)(n - j0);
                for (int l = 0; l < cnt; l++)
                    sum += ch[l];
            }
            wave_sync();
        }
    }
    const double mean = sum / (double)n;
    const uint32_t s_mag = wave_max_u32(mag_lane);
    const bool small_samples = s_mag <= 70000u;
    // the other lanes' s[] is read below: the stores have left the CU, nothing older is served from its vector cache
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");

    // ---- autocorrelation (:33-38): lags 2 lane and 2 lane + 1 ---------------------------------------------------------------
    double acc_e = 0.0, acc_o = 0.0;
    {
        for (int i = lane; i < kGenRing + kGenMirror; i += 64)
            lds.ac.ring[i] = 0.0; // c before the block: a product with it adds +-0, which leaves an accumulator as it is
        wave_sync();
        double B = 0.0; // c[j - 1 - 2 lane]
        int32_t v_next = (uint32_t)lane < n ? s[lane] : 0;
        for (uint32_t j0 = 0; j0 < n; j0 += 64) {
            const bool valid = j0 + lane < n;
            const int32_t v = v_next;
            if (j0 + 64 < n)
                v_next = j0 + 64 + lane < n ? s[j0 + 64 + lane] : 0;
            const double c_mine = valid ? scale_any(v, small_samples) - mean : 0.0;
            const uint32_t slab = (j0 >> 6) & 3u;
            lds.ac.ring[64 * slab + lane] = c_mine;
            if (slab == 0)
                lds.ac.ring[kGenRing + lane] = c_mine;
            wave_sync();
            const LdsDoubles rl = (LdsDoubles)lds.ac.ring + ((j0 - 2u * (uint32_t)lane) & (uint32_t)(kGenRing - 1)); // c[j0 - 2 lane]
            if (n - j0 >= 64u) {
                // (the window values are fetched kAcAhead pairs ahead of their use: an LDS read takes ~100 cycles to come back)
                constexpr int kAcAhead = 4;
                const LdsPairs rp = (LdsPairs)rl; // j0 and 2 lane are even and the ring is 16-byte aligned
                DoublePair ahead[kAcAhead];
#pragma unroll
                for (int u = 0; u < kAcAhead; u++)
                    ahead[u] = rp[u];
                // the wave-uniform multiplier c[j] comes by a same-address LDS read as well (two v_readlane of the register that holds the
                // chunk cost 4.1 k of the block's 23.3 k vector instructions: 0.775 -> 0.756 ms at 11,625 blocks)
                const LdsPairs cp = (LdsPairs)((LdsDoubles)lds.ac.ring + (j0 & (uint32_t)(kGenRing - 1)));
                DoublePair mult[kAcAhead];
#pragma unroll
                for (int u = 0; u < kAcAhead; u++)
                    mult[u] = cp[u];
#pragma unroll
                for (int u = 0; u < 32; u++) {
                    const DoublePair cj = mult[u % kAcAhead];
                    if (u + kAcAhead < 32)
                        mult[u % kAcAhead] = cp[u + kAcAhead];
                    const DoublePair A = ahead[u % kAcAhead];
                    if (u + kAcAhead < 32)
                        ahead[u % kAcAhead] = rp[u + kAcAhead];
                    {
                        const double pe = cj.x * A.x, po = cj.x * B; // step j0 + 2 u
                        acc_e += pe;
                        acc_o += po;
                    }
                    {
                        const double pe = cj.y * A.y, po = cj.y * A.x; // step j0 + 2 u + 1
                        acc_e += pe;
                        acc_o += po;
                    }
                    B = A.y;
                    __builtin_amdgcn_sched_barrier(0);
                }
            } else {
                const int cnt = (int)(n - j0);
                for (int t = 0; t < cnt; t++) {
                    const double cj = read_lane(c_mine, t);
                    const double A = rl[t];
                    const double pe = cj * A, po = cj * B;
                    acc_e += pe;
                    acc_o += po;
                    B = A;
                }
            }
            wave_sync();
        }
    }

    // ---- normalise (:41-44), Schur recursion (:47-68), always 100 stages ------------------------------------------------------
    // gen0 = gen1 = ac[1 .. 100]: lane L holds columns 2L (= ac[2L + 1], its own odd lag) and 2L + 1 (= ac[2L + 2], the next
    // lane's even lag).  A stage: gen1'[j] = gen1[j + 1] + k gen0[j]; gen0'[j] = gen1[j + 1] k + gen0[j] for the columns still
    // alive (what lies beyond them is never read by a live column).
    {
        const double ac0 = read_lane(acc_e, 0);
        const double n_e = acc_e / ac0, n_o = acc_o / ac0;
        double g1a = n_o, g1b = wave_shl1(0.0, n_e);
        double g0a = g1a, g0b = g1b;
        double err = 1.0;
        double g = read_lane(g1a, 0);
        double k = -g / err;
        err += g * k;
        if (lane == 0)
            lds.kk[0] = k;
#pragma unroll 1
        for (int i = 1; i < kMaxOrder; i++) {
            const double next = wave_shl1(0.0, g1a); // gen1[2L + 2]
            const double n1a = g1b + k * g0a, n0a = g1b * k + g0a;
            const double n1b = next + k * g0b, n0b = next * k + g0b;
            g1a = n1a, g0a = n0a, g1b = n1b, g0b = n0b;
            g = read_lane(g1a, 0);
            k = -g / err;
            err += g * k;
            if (lane == 0)
                lds.kk[i] = k;
        }
    }
    wave_sync();
    const double k_lo = lds.kk[lane];
    const double k_hi = lane + 64 < kMaxOrder ? lds.kk[lane + 64] : 0.0;
    wave_sync();

    // ---- order (:70-78), quantise (:80-96) ----------------------------------------------------------------------------------
    int order;
    {
        const unsigned long long b_lo = __ballot(fabs(k_lo) > SELA_ORDER_THRESHOLD);
        const unsigned long long b_hi = __ballot(lane + 64 < kMaxOrder && fabs(k_hi) > SELA_ORDER_THRESHOLD);
        order = b_hi ? 128 - __clzll(b_hi) : (b_lo ? 64 - __clzll(b_lo) : 1);
    }
    {
        const double sqrt2 = SELA_SQRT2;
        double v_lo;
        if (lane == 0)
            v_lo = floor(64 * (-1 + (sqrt2 * sqrt(k_lo + 1))));
        else if (lane == 1)
            v_lo = floor(64 * (-1 + (sqrt2 * sqrt(-k_lo + 1))));
        else
            v_lo = floor(64 * k_lo);
        const double v_hi = floor(64 * k_hi);
        const int32_t q_lo = isnan(v_lo) ? 0 : trunc_to_i32(v_lo);
        const int32_t q_hi = isnan(v_hi) ? 0 : trunc_to_i32(v_hi);
        if (lane < order) {
            lds.q[lane] = q_lo;
            lds.kk[lane] = order <= 1 ? 0.0 : dequant(lane, q_lo, flags);
        }
        if (lane + 64 < order) {
            lds.q[lane + 64] = q_hi;
            lds.kk[lane + 64] = dequant(lane + 64, q_hi, flags);
        }
    }
    wave_sync();
    step_up<false>(lds.kk, lds.a, order, lane, flags); // (registers: see step_up)
    for (int i = lane; i < kMaxOrder; i += 64)
        q_ws[(size_t)b * kMaxOrder + i] = i < order ? lds.q[i] : 0;

    // ---- residues (:98-119): r[0] = s[0]; r[i] = s[i] - (int32)((2^34 + sum_{j=1..min(i,order)} a[j] s[i-j]) >> 35) ----------
    if ((uint32_t)order >= n)
        flags |= SELA_HIP_FLAG_SHORT_BLOCK; // the reference's warm-up loop reads samples[1 .. order] (:104-110): past its vector
    // which form: FP64 taps are exact while 2^34 + sum |a[j]| x max |s| < 2^53
    bool fp64_taps;
    {
        bool modest = true; // every |a[j]| below 2^39: their sum fits 2^46 and each is two exact FP64 halves
        uint64_t a_abs = 0;
        for (int j = 1 + lane; j <= order; j += 64) {
            const int64_t aj = lds.a[j];
            const uint64_t mag = aj < 0 ? 0 - (uint64_t)aj : (uint64_t)aj;
            modest &= mag < ((uint64_t)1 << 39);
            a_abs += modest ? mag : 0u;
            const int64_t top = aj >> 20;
            lds.af[j] = ((double)(int32_t)(top >> 16) * 65536.0 + (double)(uint32_t)((uint64_t)top & 0xFFFFu)) * 1048576.0 + (double)(uint32_t)((uint64_t)aj & 0xFFFFFu);
        }
        const uint64_t a_sum = wave_sum_wrap(a_abs);
        const uint64_t room = ((uint64_t)1 << 53) - ((uint64_t)1 << (SELA_Q_SHIFT - 1));
        fp64_taps = !__any(!modest) && (a_sum == 0 || (uint64_t)s_mag < room / a_sum) && !force_wrap_taps;
        wave_sync();
    }
    uint64_t t0_lane = 0; // sum of this lane's zig-zagged residues
    bool wide = false;
    if (fp64_taps) {
        int32_t* const sT = lds.st;
        for (int m = lane; m < kGenPad; m += 64)
            sT[m + (m >> kGenPadShift)] = 0;
        for (uint32_t i0 = 0; i0 < n; i0 += kGenStretch) {
            if (i0) { // the stretch before this one left its last 128 samples behind: they become this one's history
                int32_t keep[2];
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const int e = kGenStretch + lane + 64 * h; // = kGenPad + (kGenStretch - kGenPad) + ...
                    keep[h] = sT[e + (e >> kGenPadShift)];
                }
                wave_sync();
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const int e = lane + 64 * h;
                    sT[e + (e >> kGenPadShift)] = keep[h];
                }
            }
#pragma unroll 8
            for (int t = 0; t < kGenPerLane; t++) {
                const uint32_t i = i0 + lane + 64 * t;
                const int e = kGenPad + lane + 64 * t;
                sT[e + (e >> kGenPadShift)] = i < n ? s[i] : 0;
            }
            wave_sync();
            const int32_t* mine_s = sT + (kGenPad + kGenPerLane * lane) + ((kGenPad + kGenPerLane * lane) >> kGenPadShift); // &s[i0 + kGenPerLane lane]: no pad word inside
            double win_f[kGenPerLane], acc_f[kGenPerLane];
#pragma unroll
            for (int t = 0; t < kGenPerLane; t++) {
                acc_f[t] = (double)((int64_t)1 << (SELA_Q_SHIFT - 1));
                win_f[t] = (double)mine_s[t];
            }
#pragma unroll 1
            for (int j0 = 0; j0 < order; j0 += kGenPerLane)
                gen_taps_f64<0>(j0, order, lane, sT, lds.af, win_f, acc_f);
            int32_t rr[kGenPerLane];
#pragma unroll
            for (int t = 0; t < kGenPerLane; t++) { // floor(sum / 2^35): |.| < 2^18
                int32_t pred;
                if constexpr (kLossless) // -floor(1 - sum / 2^35) = ceil(sum / 2^35) - 1: one less than the floor exactly at a tie
                    pred = (int32_t)__builtin_ceil(acc_f[t] * (1.0 / (double)((int64_t)1 << SELA_Q_SHIFT))) - 1;
                else
                    pred = (int32_t)__builtin_floor(acc_f[t] * (1.0 / (double)((int64_t)1 << SELA_Q_SHIFT)));
                rr[t] = (int32_t)((uint32_t)mine_s[t] - (uint32_t)pred);
            }
            const uint32_t first = i0 + (uint32_t)kGenPerLane * (uint32_t)lane;
#pragma unroll
            for (int t = 0; t < kGenPerLane; t++)
                if (first + t < n) {
                    r[first + t] = rr[t];
                    t0_lane += zigzag32(rr[t]);
                    wide |= (rr[t] >= (1 << 30)) || (rr[t] < -(1 << 30));
                }
            wave_sync(); // (the samples are re-staged by the next stretch)
        }
    } else {
        // 64-bit wrap-around taps: a round's 64 samples, the 64 before them and the 64 before those in registers; tap j wants
        // sample i - j = the value j lanes down, so a window starts as the round's own samples and moves up one lane per tap,
        // lane 0 fed from the rounds before (zero before the block: a tap that reaches there adds 0).
        const uint32_t o = (uint32_t)order;
        int32_t before1 = 0, before2 = 0; // samples i0 - 64 + lane, i0 - 128 + lane
        for (uint32_t i0 = 0; i0 < n; i0 += 64) {
            const bool valid = i0 + lane < n;
            const int32_t mine = valid ? s[i0 + lane] : 0;
            uint64_t temp = (uint64_t)1 << (SELA_Q_SHIFT - 1);
            int32_t win = mine;
#pragma unroll 4
            for (uint32_t j = 1; j <= o; j++) {
                const int32_t feed = j <= 64u ? __builtin_amdgcn_readlane(before1, (int)(64u - j)) : __builtin_amdgcn_readlane(before2, (int)(128u - j));
                win = __builtin_amdgcn_update_dpp(feed, win, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
                temp += (uint64_t)lds.a[j] * (uint64_t)(int64_t)win;
            }
            if (valid) {
                uint32_t pred;
                if constexpr (kLossless)
                    pred = 0u - (uint32_t)(int32_t)((int64_t)(((uint64_t)1 << SELA_Q_SHIFT) - temp) >> SELA_Q_SHIFT);
                else
                    pred = (uint32_t)(int32_t)((int64_t)temp >> SELA_Q_SHIFT);
                const int32_t rt = (int32_t)((uint32_t)mine - pred);
                r[i0 + lane] = rt;
                t0_lane += zigzag32(rt);
                wide |= (rt >= (1 << 30)) || (rt < -(1 << 30));
            }
            before2 = before1;
            before1 = mine;
        }
    }
    // the lanes read each other's residues back for the Rice plan
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");

    // ---- the two Rice plans -------------------------------------------------------------------------------------------------
    uint32_t ck, rk;
    uint64_t cbits, rbits;
    {
        const int32_t* const q = lds.q;
        uint64_t c0 = 0;
        for (int i = lane; i < order; i += 64)
            c0 += zigzag32(q[i]);
        rice_plan_convex([&](uint32_t i) { return q[i]; }, (uint32_t)order, lane, wave_sum_wrap(c0), ck, cbits);
        rice_plan_convex([&](uint32_t i) { return r[i]; }, n, lane, wave_sum_wrap(t0_lane), rk, rbits);
    }
    if (__any(wide))
        flags |= SELA_HIP_FLAG_RICE_RANGE;
    // requiredInts = ceil((float)bits / 32) (rice_encoder.cpp:37,63): exact below 2^24 bits, and a count the u16 field of the
    // subframe can carry (65535 words = 2,097,120 bits) is far below that
    const uint32_t cwords = cbits <= 32ull * kCoefWordsCap ? words_for_bits(cbits) : 0xFFFFFFFFu;
    const uint32_t rwords = rbits <= 32ull * 65535ull ? words_for_bits(rbits) : 0xFFFFFFFFu;
    if (cwords == 0xFFFFFFFFu || rwords == 0xFFFFFFFFu)
        flags |= SELA_HIP_FLAG_WORDS_CAP;
    flags = wave_or(flags);
    if (lane == 0) {
        GenericMeta m;
        m.order = (uint32_t)order, m.coef_k = ck, m.coef_words = cwords, m.res_k = rk, m.res_words = rwords, m.flags = flags, m.form = fp64_taps ? 0u : 1u;
        meta[b] = m;
    }
}

// ---- plan: the pairs' decisions, frame sizes, offsets -- one workgroup ----------------------------------------------------
// src/frame/frame_encoder.cpp:64-72: the difference candidate wins iff its words (coefficients + residues) are FEWER -- for the
// second channel of a stereo frame, and with kPaired for the odd channel of every pair (n_sig - channels pairs).
// sela_generic_plan.inc is the body of both kernels, k_generic_plan and k_paired_plan, below.
// 1024 threads over tiles of 4096 frames.  Within a tile frame f is sized by thread f mod 1024 -- the records' loads of one pass
// are independent and coalesced (a thread that walks consecutive frames waits for memory once per frame: the second version,
// 46 us at 3875 frames; the first version's single thread walking 256 partial sums: 60) -- its subframes' word counts go to LDS;
// then every thread sums a contiguous run of the tile's frames, the runs are scanned across the workgroup (shuffles within a
// wave, the sixteen waves' totals through LDS), and the offsets and the subframes' word bases are written frame by frame again.
// kDevice (sela_hip_encode_i32_device): base_bytes is 0; the frames that end beyond frames_cap are counted, and the status words are
// written whole (plain stores: the caller's words need no initialisation) -- [0] the flags, [1] that count, [2] and [3] zero.
constexpr int kPlanThreads = 1024, kPlanTile = 4096;
// The two kernels: the plain calls' (the stereo frame's one pair, or none) and the paired calls'  -- kernels of their
// own with one body (sela_generic_plan.inc), so that the plain calls run the code object they ran before there were pairs.
template <bool kDevice>
__global__ __launch_bounds__(kPlanThreads) void k_generic_plan(const GenericMeta* __restrict__ meta, uint32_t n_frames, uint32_t channels, uint32_t n_sig,
    uint64_t base_bytes, uint64_t* __restrict__ frame_offsets /* [n_frames + 1], absolute */, uint64_t* __restrict__ word_base /* [n_frames * channels + 1] */,
    uint32_t* __restrict__ chosen /* [n_frames * channels]: signal index */, uint32_t* __restrict__ status, uint64_t* __restrict__ total_words_out, uint64_t frames_cap)
{
    constexpr bool kPaired = false;
#include "sela_generic_plan.inc"
}
template <bool kDevice>
__global__ __launch_bounds__(kPlanThreads) void k_paired_plan(const GenericMeta* __restrict__ meta, uint32_t n_frames, uint32_t channels, uint32_t n_sig,
    uint64_t base_bytes, uint64_t* __restrict__ frame_offsets, uint64_t* __restrict__ word_base, uint32_t* __restrict__ chosen, uint32_t* __restrict__ status,
    uint64_t* __restrict__ total_words_out, uint64_t frames_cap)
{
    constexpr bool kPaired = true;
#include "sela_generic_plan.inc"
}

// ---- pack: the chosen candidates' two Rice streams, one wave per subframe ---------------------------------------------------
__global__ __launch_bounds__(64) void k_generic_pack(const GenericMeta* __restrict__ meta, uint32_t n_frames, uint32_t channels, uint32_t n_sig, uint32_t n,
    const int32_t* __restrict__ res_ws, const int32_t* __restrict__ q_ws, const uint32_t* __restrict__ chosen, const uint64_t* __restrict__ word_base,
    uint32_t* __restrict__ words /* zeroed */, uint64_t words_cap)
{
    const uint32_t sub = blockIdx.x;
    if (sub >= n_frames * channels)
        return;
    const int lane = threadIdx.x;
    const uint32_t f = sub / channels;
    const size_t b = (size_t)f * n_sig + chosen[sub];
    // everything that only needs to know WHICH block is asked for in one go: the block's record, its coefficients (all 100 places of
    // its row: how many count is in the record), the first stretch of its residues
    int32_t first[kPackPerLane], coefs[kPackPerLane];
    pack_fetch(res_ws + b * n, n, 0, lane, first);
    pack_fetch(q_ws + b * kMaxOrder, kMaxOrder, 0, lane, coefs);
    const GenericMeta m = meta[b];
    if (m.flags & (SELA_HIP_FLAG_WORDS_CAP | SELA_HIP_FLAG_RICE_RANGE))
        return;
    if (word_base[sub] + m.coef_words + m.res_words > words_cap) // (the host sized the words by an estimate: it packs again at the plan's size)
        return;
    __shared__ uint32_t win[kPackWindow];
    uint32_t* const out = words + word_base[sub];
    rice_pack_stream<true>(q_ws + b * kMaxOrder, m.order, m.coef_k, out, lane, win, coefs);
    rice_pack_stream<true>(res_ws + b * n, n, m.res_k, out + m.coef_words, lane, win, first);
}

// ---- assemble: the on-disk bytes (src/file/sela_file.cpp:115-135), one workgroup per subframe -------------------------------
constexpr int kAsmThreads = 256;
__global__ __launch_bounds__(kAsmThreads) void k_generic_assemble(const GenericMeta* __restrict__ meta, uint32_t n_frames, uint32_t channels, uint32_t n_sig,
    uint32_t n, const uint32_t* __restrict__ chosen, const uint64_t* __restrict__ word_base, const uint32_t* __restrict__ words,
    const uint64_t* __restrict__ frame_offsets, uint64_t base_bytes, uint8_t* __restrict__ frames /* the launch's first byte */, uint64_t frames_cap)
{
    const uint32_t sub = blockIdx.x;
    if (sub >= n_frames * channels)
        return;
    const uint32_t f = sub / channels, c = sub % channels;
    if (frame_offsets[f + 1] - base_bytes > frames_cap) // (the call reports ECAPACITY from frame_offsets[n_frames])
        return;
    uint64_t at = frame_offsets[f] - base_bytes + 4;
    for (uint32_t i = 0; i < c; i++) // (<= 254 steps; every thread the same)
        at += SELA_SUBFRAME_HEADER_BYTES + 4 * (word_base[(size_t)f * channels + i + 1] - word_base[(size_t)f * channels + i]);
    const uint32_t sgn = chosen[sub];
    const GenericMeta m = meta[(size_t)f * n_sig + sgn];
    const bool broken = (m.flags & (SELA_HIP_FLAG_WORDS_CAP | SELA_HIP_FLAG_RICE_RANGE)) != 0;
    const uint32_t cw = broken ? 0 : m.coef_words, rw = broken ? 0 : m.res_words;
    uint8_t* const dst = frames + at;
    const uint32_t* const src = words + word_base[sub];
    const uint32_t t = threadIdx.x;
    if (c == 0 && t < 4)
        frames[frame_offsets[f] - base_bytes + t] = (uint8_t)(SELA_SYNC_WORD >> (8 * t));
    if (t == 0) {
        dst[0] = (uint8_t)c;
        dst[1] = sgn >= channels ? 1 : 0;                      // subFrameType
        dst[2] = (uint8_t)(sgn >= channels ? c - 1 : c);       // parentChannelNumber
        dst[3] = (uint8_t)m.coef_k;
        dst[4] = (uint8_t)cw, dst[5] = (uint8_t)(cw >> 8);
        dst[6] = (uint8_t)m.order;
        uint8_t* const h = dst + 7 + 4 * (size_t)cw;
        h[0] = (uint8_t)m.res_k;
        h[1] = (uint8_t)rw, h[2] = (uint8_t)(rw >> 8);
        h[3] = (uint8_t)n, h[4] = (uint8_t)(n >> 8);
    }
    for (size_t i = t; i < 4 * (size_t)cw; i += kAsmThreads)
        dst[7 + i] = (uint8_t)(src[i >> 2] >> (8 * (i & 3)));
    uint8_t* const rdst = dst + 12 + 4 * (size_t)cw;
    for (size_t i = t; i < 4 * (size_t)rw; i += kAsmThreads)
        rdst[i] = (uint8_t)(src[cw + (i >> 2)] >> (8 * (i & 3)));
}

// ---- write: the on-disk bytes at their final place, one wave per subframe (sela_hip_encode_i32_device) -----------------------
// pack + assemble in one pass, with no Rice words in between.  A frame is 4-aligned and so is every subframe (12 header bytes and
// whole words), at byte 4 (f + 1) + 12 sub + 4 word_base[sub] of the stream.  Its first 3 + cw words -- the 7 header bytes, the
// coefficient words 3 bytes off alignment, the residue header's 5 bytes -- are put together from the coefficient stream packed
// in LDS, one aligned word per lane by a funnel shift, and stored once; the residue words follow aligned, packed by
// rice_pack_stream straight into the frame.  That packer ORs into zeroed words and leaves words that come out zero alone: the
// wave zeroes its residue words first and waits for those stores.  A frame that ends beyond frames_cap is not written at all;
// nothing is written outside a subframe's own words (the sync word: by the frame's first subframe).
__global__ __launch_bounds__(64) void k_generic_write(const GenericMeta* __restrict__ meta, uint32_t n_frames, uint32_t channels, uint32_t n_sig, uint32_t n,
    const int32_t* __restrict__ res_ws, const int32_t* __restrict__ q_ws, const uint32_t* __restrict__ chosen, const uint64_t* __restrict__ word_base,
    const uint64_t* __restrict__ frame_offsets, uint8_t* __restrict__ frames /* 4-byte aligned */, uint64_t frames_cap)
{
    const uint32_t sub = blockIdx.x;
    if (sub >= n_frames * channels)
        return;
    const int lane = threadIdx.x;
    const uint32_t f = sub / channels, c = sub % channels;
    const uint32_t sgn = chosen[sub];
    const size_t b = (size_t)f * n_sig + sgn;
    // (as k_generic_pack: the record, the coefficients and the first stretch of residues asked for together)
    int32_t first[kPackPerLane], coefs[kPackPerLane];
    pack_fetch(res_ws + b * n, n, 0, lane, first);
    pack_fetch(q_ws + b * kMaxOrder, kMaxOrder, 0, lane, coefs);
    const GenericMeta m = meta[b];
    const uint64_t wb = word_base[sub];
    if (frame_offsets[f + 1] > frames_cap)
        return;
    const bool broken = (m.flags & (SELA_HIP_FLAG_WORDS_CAP | SELA_HIP_FLAG_RICE_RANGE)) != 0; // (as k_generic_assemble: an empty header)
    const uint32_t cw = broken ? 0 : m.coef_words, rw = broken ? 0 : m.res_words;
    uint32_t* const dst = reinterpret_cast<uint32_t*>(frames) + (f + 1) + 3 * (uint64_t)sub + wb;
    __shared__ uint32_t win[kPackWindow];
    __shared__ uint32_t coef[kCoefWordsCap];
    static_assert(kCoefWordsCap <= 64 - 3, "a subframe's header words: one lane each");
    if (lane < kCoefWordsCap)
        coef[lane] = 0;
    wave_sync();
    if (cw)
        rice_pack_stream<true>(q_ws + b * kMaxOrder, m.order, m.coef_k, coef, lane, win, coefs);
    if (rw) { // zero the residue words; the stores are done before the packer's first OR
        for (uint32_t w = lane; w < rw; w += 64)
            dst[3 + cw + w] = 0;
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    wave_sync();
    // the header words: the byte stream [pad] c type parent coef_k cw(2) order | coefficient words | res_k rw(2) n(2) [pad x 3] as
    // words x(0 .. cw + 3); aligned word j is x(j) >> 8 | x(j + 1) << 24
    auto x = [&](uint32_t i) -> uint32_t {
        if (i == 0)
            return (c << 8) | ((sgn >= channels ? 1u : 0u) << 16) | ((sgn >= channels ? c - 1 : c) << 24);
        if (i == 1)
            return m.coef_k | (cw << 8) | (m.order << 24);
        if (i < cw + 2)
            return coef[i - 2];
        if (i == cw + 2)
            return m.res_k | (rw << 8) | ((n & 0xFFu) << 24);
        return n >> 8;
    };
    if ((uint32_t)lane < 3 + cw)
        dst[lane] = __builtin_amdgcn_alignbit(x((uint32_t)lane + 1), x((uint32_t)lane), 8);
    if (c == 0 && lane == 63)
        dst[-1] = SELA_SYNC_WORD;
    if (rw)
        rice_pack_stream<true>(res_ws + b * n, n, m.res_k, dst + 3 + cw, lane, win, first);
}

// ---- decode: one wave per subframe -------------------------------------------------------------------------------------------
// src/frame/frame_decoder.cpp:19-36 / :42-61 for one subframe: rice::RiceDecoder on the coefficients (n = order) and on the
// residues (n = samplesPerChannel) -- src/rice/rice_decoder.cpp:21-52: the codewords' lengths walked serially, wave-uniform, the
// remainder fields fetched by all lanes at once (RiceScan below) -- and
// lpc::SampleGenerator (src/lpc/sample_generator.cpp:11-39) in transposed form: lane l carries the part of sample i + 1 + l's
// prediction that is already known, P[l] = sum a[i + 1 + l - i'] s[i'] over the samples i' <= i; a new sample adds a[l + 1] s[i]
// to every lane after the lanes have moved down by one.  (Integer arithmetic mod 2^64: the order of the additions is free.)
// The parse is serial only in the codewords' LENGTHS.  RiceScan walks those, wave-uniform, on a 64-bit register window that is
// refilled word by word from a lane-held buffer of the frame's next 64 aligned words (one coalesced load per 2048 bits, no
// load on the chain); each lane keeps the start and the unary count of ONE codeword of a chunk of 64, and then all lanes
// fetch their remainder fields at once.  Bits at or beyond the stream's end read as zero (a stream that ends early raises
// RICE_OVERRUN), exactly as the byte-wise reader of the first version did.
struct RiceScan {
    const uint32_t* words; // the frame's aligned words
    uint32_t n_words;
    uint64_t end;          // the stream's end, in bits from the frame's first byte
    uint64_t pos;          // bit position of the window's first bit
    uint64_t cur;          // the next `avail` bits of the stream, LSB first
    uint32_t avail, wpos;  // wpos: the next word to append
    uint32_t buf, wbase;   // lane l holds word wbase + l (masked to the stream)
    int lane;

    __device__ __forceinline__ uint32_t masked_word(uint32_t w) const
    {
        const uint64_t first = 32ull * w;
        if (w >= n_words || first >= end)
            return 0u;
        const uint32_t v = words[w];
        return first + 32 > end ? v & ((1u << (uint32_t)(end - first)) - 1u) : v;
    }
    __device__ __forceinline__ void load_buf(uint32_t base)
    {
        wbase = base;
        buf = masked_word(base + (uint32_t)lane);
    }
    __device__ __forceinline__ void refill()
    {
        while (avail <= 32) {
            if (wpos - wbase >= 64u)
                load_buf(wpos);
            const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)buf, (int)(wpos - wbase));
            cur |= (uint64_t)w << avail;
            avail += 32;
            wpos++;
        }
    }
    __device__ __forceinline__ void start(const uint32_t* frame_words, uint32_t frame_word_count, uint64_t first_bit, uint64_t end_bit, int lane_)
    {
        words = frame_words, n_words = frame_word_count, end = end_bit, lane = lane_;
        pos = first_bit;
        wpos = (uint32_t)(first_bit >> 5);
        load_buf(wpos);
        cur = 0, avail = 0;
        refill();
        const uint32_t skip = (uint32_t)first_bit & 31; // the stream starts inside its first aligned word
        cur >>= skip, avail -= skip;
        refill();
    }
    __device__ __forceinline__ void consume(uint32_t n) // n <= 32
    {
        cur >>= n;
        avail -= n;
        pos += n;
        refill();
    }
    // one codeword: where it starts and how many ones it has; the window moves past its k remainder bits
    __device__ __forceinline__ void next(uint32_t k, uint64_t& at, uint32_t& ones)
    {
        at = pos;
        ones = 0;
        for (;;) {
            const uint32_t low = (uint32_t)cur;
            const uint32_t t = low == 0xFFFFFFFFu ? 32u : (uint32_t)__builtin_ctz(~low);
            ones += t;
            consume(t);
            if (t < 32)
                break; // (beyond the stream's end everything is zero: the run ends there at the latest)
        }
        consume(1 + k);
    }
};

// the k bits at bit position p of the frame, the first one the most significant (src/rice/rice_decoder.cpp:37-40); bits at or
// beyond `end` are zero.  Per lane (every lane its own position).
__device__ __forceinline__ uint32_t remainder_bits(const uint8_t* base, uint64_t p, uint64_t end, uint32_t k)
{
    if (k == 0)
        return 0u;
    const uint64_t at = p >> 3;
    uint64_t w = 0;
#pragma unroll
    for (int i = 0; i < 5; i++)
        w |= (uint64_t)(8 * (at + i) < end ? base[at + i] : 0u) << (8 * i);
    uint32_t v = (uint32_t)(w >> (p & 7));
    if (p + 32 > end) // (the stream ends inside these 32 bits; its end is a whole number of bytes, so only bytes were masked above)
        v &= p >= end ? 0u : (uint32_t)(((uint64_t)1 << (end - p)) - 1);
    return __brev(v) >> (32 - k);
}

// up to 64 values of a stream, value i0 + lane in each lane (lanes beyond `count` get 0)
__device__ inline int32_t rice_chunk(RiceScan& sc, const uint8_t* base, uint32_t k, uint32_t count, bool& overrun)
{
    uint64_t my_at = 0;
    uint32_t my_ones = 0;
    for (uint32_t i = 0; i < count; i++) {
        uint64_t at;
        uint32_t ones;
        sc.next(k, at, ones);
        if ((uint32_t)sc.lane == i)
            my_at = at, my_ones = ones;
    }
    const bool live = (uint32_t)sc.lane < count;
    const uint64_t field = my_at + my_ones + 1;
    overrun |= live && field + k > sc.end;
    const uint32_t rem = live ? remainder_bits(base, field, sc.end, k) : 0u;
    const uint32_t u = (my_ones << k) | rem; // (uint32 arithmetic: src/rice/rice_decoder.cpp:35)
    return live ? (int32_t)((u >> 1) ^ (0u - (u & 1u))) : 0;
}

__global__ __launch_bounds__(64) void k_generic_decode(const uint8_t* __restrict__ frames, const uint64_t* __restrict__ frame_offsets, uint64_t base_bytes,
    uint32_t n_frames, uint32_t channels, uint32_t stride, int32_t* __restrict__ dec_ws /* [n_frames][channels][stride] by subframe position */,
    GenericSubInfo* __restrict__ info /* [n_frames][channels] */, uint32_t* __restrict__ status,
    const uint32_t* __restrict__ n_frames_found /* or null: frames from *n_frames_found on are not decoded */,
    const uint32_t* __restrict__ left_alone /* or null: the workgroup returns at once while *left_alone is 0 (the judge's decision on the device) */)
{
    __shared__ int64_t a_lds[kMaxOrder + 1];
    __shared__ int32_t q_lds[256];
    const uint32_t sub = blockIdx.x;
    if (sub >= n_frames * channels)
        return;
    if (left_alone && *left_alone == 0)
        return;
    const int lane = threadIdx.x;
    const uint32_t f = sub / channels, c = sub % channels;
    if (n_frames_found && f >= *n_frames_found)
        return;
    const uint8_t* const fb = frames + (frame_offsets[f] - base_bytes);
    const uint64_t fbytes = frame_offsets[f + 1] - frame_offsets[f];
    GenericSubInfo si;
    si.channel = si.type = si.parent = 0, si.n = 0, si.ok = 0;
    uint32_t flags = 0;
    // ---- the headers up to this subframe (sela_format.h), byte by byte: a frame here may lie anywhere ----
    bool ok = fbytes >= 4 && fbytes < (1ull << 31) && fb[0] == 0x00 && fb[1] == 0xFF && fb[2] == 0x55 && fb[3] == 0xAA;
    uint64_t p = 4;
    SelaSubframeHeader h = {};
    for (uint32_t i = 0; ok && i <= c; i++) {
        const uint64_t next = sela_subframe_read_bytes(fb, fbytes, p, &h);
        ok = next != 0;
        if (i < c)
            p = next;
    }
    si.channel = (uint8_t)h.channel, si.type = (uint8_t)h.type, si.parent = (uint8_t)h.parent;
    const uint32_t cw = h.cw, order = h.order, rw = h.rw, n = h.n, ck = h.ck, rk = h.rk;
    ok = ok && sela_subframe_decodable(&h) && n <= stride;
    if (!ok) {
        if (lane == 0) {
            info[sub] = si;
            atomicOr(&status[0], (uint32_t)SELA_HIP_FLAG_BAD_FRAME);
            atomicAdd(&status[1], 1u);
        }
        return;
    }
    si.n = n, si.ok = 1;
    if (n == 0 || n <= order) // lpc::SampleGenerator writes samples[0] and samples[1 .. order] whatever the length (src/lpc/sample_generator.cpp:14-22): past its vector
        flags |= SELA_HIP_FLAG_SHORT_BLOCK;
    const uint32_t* const fw = reinterpret_cast<const uint32_t*>(fb); // (frames are whole words at word-aligned offsets)
    const uint32_t n_fw = (uint32_t)(fbytes >> 2);
    bool overrun = false;
    RiceScan sc;
    // ---- the coefficients ----
    {
        const uint64_t first = 8 * (p + 7);
        sc.start(fw, n_fw, first, first + 32ull * cw, lane);
        for (uint32_t i0 = 0; i0 < order; i0 += 64) {
            const int32_t v = rice_chunk(sc, fb, ck, order - i0 < 64u ? order - i0 : 64u, overrun);
            if (i0 + lane < order)
                q_lds[i0 + lane] = v;
        }
    }
    wave_sync();
    {
        const uint32_t o = order;
        const int32_t q_lo = (uint32_t)lane < o ? q_lds[lane] : 0;
        const int32_t q_hi = (uint32_t)lane + 64 < o ? q_lds[lane + 64] : 0;
        step_up_from_q<false>(o, q_lo, q_hi, a_lds, lane, flags); // (a_lds ends at the largest order: no room to park them)
    }
    // lane l: a[l + 1], a[l + 65] (0 beyond the order)
    const uint64_t a_lo = (uint32_t)lane + 1 <= order ? (uint64_t)a_lds[lane + 1] : 0;
    const uint64_t a_hi = (uint32_t)lane + 65 <= order ? (uint64_t)a_lds[lane + 65] : 0;
    // ---- residues -> samples, 64 at a time ----
    {
        const uint64_t first = 8 * (p + 12 + 4 * (uint64_t)cw);
        sc.start(fw, n_fw, first, first + 32ull * rw, lane);
    }
    int32_t* const out = dec_ws + (size_t)sub * stride;
    uint64_t p_lo = 0, p_hi = 0;
    for (uint32_t i0 = 0; i0 < n; i0 += 64) {
        const uint32_t cnt = n - i0 < 64u ? n - i0 : 64u;
        const int32_t mine = rice_chunk(sc, fb, rk, cnt, overrun);
        int32_t made = 0;
        for (uint32_t l = 0; l < cnt; l++) {
            const int32_t res = __builtin_amdgcn_readlane(mine, (int)l);
            const uint64_t sum = read_first_lane(p_lo);
            const uint64_t temp = ((uint64_t)1 << (SELA_Q_SHIFT - 1)) - sum;
            const int32_t smp = (int32_t)((uint32_t)res - (uint32_t)(int32_t)((int64_t)temp >> SELA_Q_SHIFT));
            if ((uint32_t)lane == l)
                made = smp;
            if (order > 64) { // two registers: lags 1..64 and 65..100
                const uint64_t carry = read_first_lane(p_hi);
                // lane l <- lane l + 1
                const uint32_t nlo = (uint32_t)wave_shl1((int)(uint32_t)carry, (int)(uint32_t)p_lo);
                const uint32_t nhi = (uint32_t)wave_shl1((int)(uint32_t)(carry >> 32), (int)(uint32_t)(p_lo >> 32));
                p_lo = (((uint64_t)nhi << 32) | nlo) + a_lo * (uint64_t)(int64_t)smp;
                p_hi = wave_shl1_zero(p_hi) + a_hi * (uint64_t)(int64_t)smp;
            } else {
                p_lo = wave_shl1_zero(p_lo) + a_lo * (uint64_t)(int64_t)smp;
            }
        }
        if (i0 + lane < n)
            out[i0 + lane] = made;
    }
    if (__any(overrun))
        flags |= SELA_HIP_FLAG_RICE_OVERRUN;
    flags = wave_or(flags);
    if (lane == 0) {
        info[sub] = si;
        if (flags)
            atomicOr(&status[0], flags);
    }
}

// ---- combine: src/frame/frame_decoder.cpp:17-69 over the decoded subframes of a frame ----------------------------------------
// One workgroup per (frame, slice of kCombineSlice samples): every slice walks the frame's subframes in the reference's order --
// independent ones first, then dependent ones IN SUBFRAME ORDER, a later subframe of a channel overwriting an earlier one, an
// unknown type skipped -- and moves its own samples only (a thread meets the same samples in every pass: the passes need no
// barrier for the data, only for the channels' counts).  A frame of 65535 samples is 16 workgroups instead of one.
// kOut16: interleaved int16 at sample_offsets[f] (src/file/wav_file.cpp:244-266 narrows so); every channel of the frame must
// have come out with the first one's length, or the frame counts as malformed.
constexpr int kCombineThreads = 256;
constexpr uint32_t kCombineSlice = 4096;
template <bool kOut16>
__global__ __launch_bounds__(kCombineThreads) void k_generic_combine(const int32_t* __restrict__ dec_ws, const GenericSubInfo* __restrict__ info, uint32_t n_frames,
    uint32_t channels, uint32_t stride, int32_t* __restrict__ all /* [n_frames][channels][stride] by channel */, uint32_t* __restrict__ counts,
    const uint64_t* __restrict__ sample_offsets, int16_t* __restrict__ pcm_out, uint32_t* __restrict__ status,
    const uint32_t* __restrict__ n_frames_found /* or null, as in k_generic_decode */)
{
    __shared__ uint32_t cnt[256];
    const uint32_t f = blockIdx.x;
    if (f >= n_frames || (n_frames_found && f >= *n_frames_found))
        return;
    const uint32_t t = threadIdx.x;
    const uint32_t lo = blockIdx.y * kCombineSlice, hi = lo + kCombineSlice; // this workgroup's samples
    const bool first_slice = blockIdx.y == 0;
    const GenericSubInfo* const inf = info + (size_t)f * channels;
    int32_t* const fa = all + (size_t)f * channels * stride;
    const int32_t* const fd = dec_ws + (size_t)f * channels * stride;
    for (uint32_t c = t; c < channels; c += kCombineThreads)
        cnt[c] = 0;
    __syncthreads();
    bool bad = false;
    for (uint32_t c = 0; c < channels; c++) { // :17-37
        const GenericSubInfo si = inf[c];
        if (!si.ok || si.type != 0)
            continue;
        if (si.channel >= channels) {
            bad = true;
            continue;
        }
        const uint32_t end = min(si.n, hi);
        for (uint32_t i = lo + t; i < end; i += kCombineThreads)
            fa[(size_t)si.channel * stride + i] = fd[(size_t)c * stride + i];
        __syncthreads();
        if (t == 0)
            cnt[si.channel] = si.n;
        __syncthreads();
    }
    for (uint32_t c = 0; c < channels; c++) { // :40-69
        const GenericSubInfo si = inf[c];
        if (!si.ok || si.type != 1)
            continue;
        if (si.channel >= channels || si.parent >= channels || cnt[si.parent] < si.n) {
            bad = true;
            continue;
        }
        const uint32_t end = min(si.n, hi);
        for (uint32_t i = lo + t; i < end; i += kCombineThreads)
            fa[(size_t)si.channel * stride + i] = (int32_t)((uint32_t)fa[(size_t)si.parent * stride + i] - (uint32_t)fd[(size_t)c * stride + i]);
        __syncthreads();
        if (t == 0)
            cnt[si.channel] = si.n;
        __syncthreads();
    }
    if (kOut16) {
        const uint32_t n = (uint32_t)(sample_offsets[f + 1] - sample_offsets[f]);
        for (uint32_t c = 0; c < channels; c++)
            bad |= cnt[c] != n;
        if (!bad && lo < n) {
            const uint32_t end = min(n, hi);
            int16_t* const o = pcm_out + sample_offsets[f] * channels;
            if (channels == 1) {
                for (uint32_t i = lo + t; i < end; i += kCombineThreads)
                    o[i] = (int16_t)(uint16_t)fa[i];
            } else if (channels == 2) { // (a sample pair per thread: one 32-bit store)
                uint32_t* const o2 = reinterpret_cast<uint32_t*>(o);
                for (uint32_t i = lo + t; i < end; i += kCombineThreads)
                    o2[i] = ((uint32_t)fa[i] & 0xFFFFu) | ((uint32_t)fa[(size_t)stride + i] << 16);
            } else {
                for (size_t i = (size_t)lo * channels + t; i < (size_t)end * channels; i += kCombineThreads) {
                    const uint32_t smp = (uint32_t)(i / channels), c = (uint32_t)(i % channels);
                    o[i] = (int16_t)(uint16_t)fa[(size_t)c * stride + smp];
                }
            }
        }
    } else if (first_slice) {
        for (uint32_t c = t; c < channels; c += kCombineThreads)
            counts[(size_t)f * channels + c] = cnt[c];
    }
    if (bad && t == 0 && first_slice) {
        atomicOr(&status[0], (uint32_t)SELA_HIP_FLAG_BAD_FRAME);
        atomicAdd(&status[1], 1u);
    }
}

// ---- the sample index on the device (sela_hip_decode_i32_device) --------------------------------------------
// generic_index_samples (sela_capi_generic.hip) taken apart: every frame's header walk is independent of the others, only the
// running total is not.  A thread walks kSampleFramesPerThread frames as that function does (sela_subframe_read_bytes, its stop
// rule and counts), and a workgroup scans its kSampleTileFrames frames' first samplesPerChannel.  Up to one tile (a track:
// 4096 frames) that is the whole index, in one launch; above, every tile scans its own frames (k_index_samples<false>), one workgroup scans the tiles'
// totals (k_sample_tiles) and every tile adds its base (k_sample_spread).  The launch that finishes also writes the caller's
// status words ([2] = what sela_hip_index_samples would return, SELA_HIP_FLAG_STRIDE where sela_hip_decode_i32 would refuse
// the stride) and zeroes the fast kernel's counters in the workspace: nothing else on the stream initialises them.
constexpr uint32_t kSampleThreads = 1024, kSampleFramesPerThread = 4, kSampleTileFrames = kSampleThreads * kSampleFramesPerThread;
constexpr uint32_t kSampleBroken = 1, kSampleDecreasing = 2;
constexpr uint32_t kSampleOdd = 4, kSampleMisaligned = 8; // (k_route_n: a subframe that does not say 2048, a frame offset not a multiple of 4)
struct SampleTile {
    uint64_t total; // this tile's samples per channel; k_sample_tiles replaces it by the samples before the tile
    uint32_t largest, bad;
};

// one frame of generic_index_samples: its first subframe's samplesPerChannel; largest / bad accumulate
__device__ inline uint32_t sample_head(const uint8_t* __restrict__ frames, const uint64_t* __restrict__ frame_offsets, uint32_t f, uint32_t channels,
    uint32_t& largest, uint32_t& bad)
{
    const uint64_t o0 = frame_offsets[f], o1 = frame_offsets[f + 1];
    if (o1 < o0)
        bad |= kSampleDecreasing;
    if (o0 & 3)
        bad |= kSampleMisaligned;
    const uint8_t* const fb = frames + o0;
    const uint64_t fbytes = o1 >= o0 ? o1 - o0 : 0;
    uint64_t p = 4;
    uint32_t first = 0;
    for (uint32_t c = 0; c < channels; c++) {
        SelaSubframeHeader h = {}; // (n is read, and counts, even when only the residue words run past the frame)
        p = sela_subframe_read_bytes(fb, fbytes, p, &h);
        if (c == 0)
            first = h.n;
        largest = max(largest, h.n);
        if (h.n != (uint32_t)kBlock)
            bad |= kSampleOdd;
        if (p == 0) {
            bad |= kSampleBroken;
            break;
        }
    }
    return first;
}

// exclusive scan of one value per thread over the workgroup (blockDim.x a multiple of 64, at most 1024); *total: the sum
__device__ inline uint64_t block_exclusive_scan(uint64_t v, uint64_t* part /* LDS [17] */, uint64_t& total)
{
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    uint64_t inc = v;
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint64_t o = __shfl_up(inc, d, 64);
        if (lane >= d)
            inc += o;
    }
    if (lane == 63)
        part[wave] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t run = 0;
        for (uint32_t w = 0; w < waves; w++) {
            const uint64_t t = part[w];
            part[w] = run;
            run += t;
        }
        part[16] = run;
    }
    __syncthreads();
    const uint64_t excl = part[wave] + inc - v;
    total = part[16];
    __syncthreads();
    return excl;
}

// the status words as the host call would leave them after its walk, the fast kernel's counters zeroed, and the walk's verdict
// bits in counters[4] (k_route_n reads them: sela_hip_decode's "2048 everywhere")
__device__ inline void finish_sample_index(uint32_t largest, uint32_t bad, uint32_t stride, uint32_t* __restrict__ status, uint32_t* __restrict__ counters)
{
    const uint32_t walked = (bad & kSampleBroken) ? 0u : largest; // sela_hip_index_samples: 0 for a stream the walk cannot follow
    status[0] = !(bad & kSampleDecreasing) && walked > stride ? (uint32_t)SELA_HIP_FLAG_STRIDE : 0u;
    status[1] = 0;
    status[2] = walked;
    status[3] = 0;
    for (int i = 0; i < 4; i++)
        counters[i] = 0;
    counters[4] = bad;
}

template <bool kOneTile>
__global__ __launch_bounds__(kSampleThreads) void k_index_samples(const uint8_t* __restrict__ frames, const uint64_t* __restrict__ frame_offsets, uint32_t max_frames,
    const uint32_t* __restrict__ n_frames_found /* or null */, uint32_t channels, uint32_t stride, uint64_t* __restrict__ sample_offsets /* or null */,
    uint32_t* __restrict__ status, uint32_t* __restrict__ counters, SampleTile* __restrict__ tiles)
{
    __shared__ uint64_t part[17];
    __shared__ uint32_t s_largest, s_bad;
    const uint32_t n = n_frames_found ? min(*n_frames_found, max_frames) : max_frames;
    const uint32_t t = threadIdx.x;
    if (t == 0)
        s_largest = 0, s_bad = 0;
    const uint64_t f0 = (uint64_t)blockIdx.x * kSampleTileFrames + (uint64_t)t * kSampleFramesPerThread;
    uint32_t first[kSampleFramesPerThread];
    uint32_t largest = 0, bad = 0;
    uint64_t sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < kSampleFramesPerThread; j++) {
        first[j] = f0 + j < n ? sample_head(frames, frame_offsets, (uint32_t)(f0 + j), channels, largest, bad) : 0u;
        sum += first[j];
    }
    __syncthreads();
    if (largest)
        atomicMax(&s_largest, largest);
    if (bad)
        atomicOr(&s_bad, bad);
    uint64_t total;
    uint64_t run = block_exclusive_scan(sum, part, total); // (its barriers also close the atomics above)
    if (sample_offsets) {
#pragma unroll
        for (uint32_t j = 0; j < kSampleFramesPerThread; j++) {
            if (f0 + j < n)
                sample_offsets[f0 + j] = run;
            run += first[j];
        }
    }
    if (t != 0)
        return;
    if (kOneTile) {
        if (sample_offsets)
            sample_offsets[n] = total;
        finish_sample_index(s_largest, s_bad, stride, status, counters);
    } else {
        SampleTile st;
        st.total = total, st.largest = s_largest, st.bad = s_bad;
        tiles[blockIdx.x] = st;
    }
}

__global__ __launch_bounds__(kSampleThreads) void k_sample_tiles(SampleTile* __restrict__ tiles, uint32_t n_tiles, uint32_t max_frames,
    const uint32_t* __restrict__ n_frames_found, uint32_t stride, uint64_t* __restrict__ sample_offsets, uint32_t* __restrict__ status,
    uint32_t* __restrict__ counters)
{
    __shared__ uint64_t part[17];
    __shared__ uint32_t s_largest, s_bad;
    const uint32_t t = threadIdx.x;
    if (t == 0)
        s_largest = 0, s_bad = 0;
    __syncthreads();
    uint64_t carry = 0;
    for (uint32_t i0 = 0; i0 < n_tiles; i0 += kSampleThreads) {
        const uint32_t i = i0 + t;
        SampleTile st;
        st.total = 0, st.largest = 0, st.bad = 0;
        if (i < n_tiles)
            st = tiles[i];
        if (st.largest)
            atomicMax(&s_largest, st.largest);
        if (st.bad)
            atomicOr(&s_bad, st.bad);
        uint64_t sum;
        const uint64_t excl = block_exclusive_scan(st.total, part, sum);
        if (i < n_tiles)
            tiles[i].total = carry + excl;
        carry += sum;
    }
    if (t != 0)
        return;
    const uint32_t n = n_frames_found ? min(*n_frames_found, max_frames) : max_frames;
    if (sample_offsets)
        sample_offsets[n] = carry;
    finish_sample_index(s_largest, s_bad, stride, status, counters);
}

__global__ __launch_bounds__(kSampleThreads) void k_sample_spread(const SampleTile* __restrict__ tiles, uint32_t max_frames,
    const uint32_t* __restrict__ n_frames_found, uint64_t* __restrict__ sample_offsets)
{
    const uint32_t n = n_frames_found ? min(*n_frames_found, max_frames) : max_frames;
    const uint64_t base = tiles[blockIdx.x].total;
    const uint64_t f0 = (uint64_t)blockIdx.x * kSampleTileFrames;
    for (uint32_t j = threadIdx.x; j < kSampleTileFrames; j += kSampleThreads)
        if (f0 + j < n)
            sample_offsets[f0 + j] += base;
}

// ---- the int16 decode of any length on the device (sela_hip_decode_n_device) --------------------------------
// sela_hip_decode picks its route on the host: the fast kernels for a stream of 2048 everywhere, the any-length route for the
// rest.  Here the sample index has walked every header already; k_route_n takes the same decision from what it left and hands
// each route a frame count of its own in the workspace -- n for the route taken, 0 for the other -- which the kernels of both
// routes, launched on their largest grids, read as their device-side frame count (a route not taken returns at once).
//   counters[4] the walk's verdict bits (finish_sample_index), [5] the fast decoder's count, [6] the any-length route's;
//   status[3] the route: 0 nothing decoded, 1 the 2048-sample decoder, 2 the any-length route.
// A stream that takes no route and is not refused for its stride is a malformed one (the walk breaks, offsets decrease, no
// subframe says a length, or a 2048 stream has a frame offset that is not a multiple of 4): SELA_HIP_FLAG_BAD_FRAME, as the host
// call's EFORMAT.
__global__ __launch_bounds__(64) void k_route_n(uint32_t max_frames, const uint32_t* __restrict__ n_frames_found /* or null */, uint32_t stride,
    uint32_t* __restrict__ status, uint32_t* __restrict__ counters)
{
    if (threadIdx.x != 0)
        return;
    const uint32_t n = n_frames_found ? min(*n_frames_found, max_frames) : max_frames;
    const uint32_t bad = counters[4], largest = status[2];
    uint32_t route = 0;
    if (n != 0 && !(bad & kSampleOdd)) // 2048 everywhere: the fast kernels, or nothing (their job refuses offsets that are not
        route = bad == 0 && stride >= (uint32_t)kBlock ? 1u : 0u; // multiples of 4, and the host's walk then refuses the stream)
    else if (n != 0 && largest != 0 && largest <= stride && !(bad & kSampleDecreasing))
        route = 2;
    if (n != 0 && route == 0 && !(status[0] & SELA_HIP_FLAG_STRIDE))
        status[0] |= SELA_HIP_FLAG_BAD_FRAME;
    status[3] = route;
    counters[5] = route == 1 ? n : 0u;
    counters[6] = route == 2 ? n : 0u;
}

// k_generic_combine<true> without its channel-major copy: one workgroup per (frame, slice of kInterleaveSlice samples), a thread
// per sample.  Thread 0 turns the frame's subframe records into the reference's order of writes (src/frame/frame_decoder.cpp:
// 17-69: independent subframes first, then dependent ones in subframe order, a later subframe of a channel overwriting an earlier
// one, an unknown type skipped) under the combine's rules (the channel and the parent exist, the parent is long enough, every
// channel ends at the first one's length); then every thread runs those writes for its own sample in a channel table of its own
// in LDS -- each decoded sample read once -- and the table goes out as interleaved int16 (src/file/wav_file.cpp:244-266), one
// store per sample.  Frames of more than kInterleaveChannels channels take k_generic_combine<true>.
constexpr uint32_t kInterleaveThreads = 256, kInterleaveChannels = 8, kInterleaveSlice = 4096, kNoParent = 0xFFu;
__global__ __launch_bounds__(kInterleaveThreads) void k_interleave16(const int32_t* __restrict__ dec_ws /* [frames][channels][stride] by position */,
    const GenericSubInfo* __restrict__ info, uint32_t max_frames, uint32_t channels /* <= kInterleaveChannels */, uint32_t stride,
    const uint64_t* __restrict__ sample_offsets, int16_t* __restrict__ pcm_out, uint32_t* __restrict__ status,
    const uint32_t* __restrict__ n_frames_found /* or null, as in k_generic_decode */)
{
    __shared__ int32_t tab[kInterleaveChannels][kInterleaveThreads];
    __shared__ uint32_t op_sub[kInterleaveChannels], op_n[kInterleaveChannels], op_dst[kInterleaveChannels], op_parent[kInterleaveChannels];
    __shared__ uint32_t cnt[kInterleaveChannels];
    __shared__ uint32_t s_ops, s_n, s_ok;
    const uint32_t f = blockIdx.x;
    if (f >= max_frames || (n_frames_found && f >= *n_frames_found))
        return;
    const uint32_t t = threadIdx.x;
    if (t == 0) {
        const GenericSubInfo* const inf = info + (size_t)f * channels;
        for (uint32_t c = 0; c < channels; c++)
            cnt[c] = 0;
        bool bad = false;
        uint32_t k = 0;
        for (uint32_t type = 0; type < 2; type++) { // :17-37, then :40-69
            for (uint32_t c = 0; c < channels; c++) {
                const GenericSubInfo si = inf[c];
                if (!si.ok || si.type != type)
                    continue;
                if (si.channel >= channels || (type == 1 && (si.parent >= channels || cnt[si.parent] < si.n))) {
                    bad = true;
                    continue;
                }
                op_sub[k] = c, op_n[k] = si.n, op_dst[k] = si.channel, op_parent[k] = type == 1 ? si.parent : kNoParent;
                k++;
                cnt[si.channel] = si.n;
            }
        }
        const uint32_t n = (uint32_t)(sample_offsets[f + 1] - sample_offsets[f]);
        for (uint32_t c = 0; c < channels; c++)
            bad |= cnt[c] != n;
        s_ops = k, s_n = n, s_ok = bad ? 0u : 1u;
        if (bad && blockIdx.y == 0) {
            atomicOr(&status[0], (uint32_t)SELA_HIP_FLAG_BAD_FRAME);
            atomicAdd(&status[1], 1u);
        }
    }
    __syncthreads();
    const uint32_t n = s_n, ops = s_ops, lo = blockIdx.y * kInterleaveSlice;
    if (!s_ok || lo >= n)
        return;
    const uint32_t hi = min(n, lo + kInterleaveSlice);
    const int32_t* const fd = dec_ws + (size_t)f * channels * stride;
    int16_t* const o = pcm_out + sample_offsets[f] * channels;
    const bool pairs = channels == 2 && ((uintptr_t)o & 3) == 0;
    for (uint32_t base = lo; base < hi; base += kInterleaveThreads) {
        const uint32_t i = base + t;
        if (i < hi) {
            for (uint32_t k = 0; k < ops; k++) {
                if (i >= op_n[k])
                    continue;
                int32_t v = fd[(size_t)op_sub[k] * stride + i];
                const uint32_t p = op_parent[k];
                if (p != kNoParent)
                    v = (int32_t)((uint32_t)tab[p][t] - (uint32_t)v);
                tab[op_dst[k]][t] = v;
            }
            if (channels == 1)
                o[i] = (int16_t)(uint16_t)tab[0][t];
            else if (pairs) // (a sample pair per thread: one 32-bit store)
                reinterpret_cast<uint32_t*>(o)[i] = ((uint32_t)tab[0][t] & 0xFFFFu) | ((uint32_t)tab[1][t] << 16);
        }
        if (channels != 1 && !pairs) { // through the table: consecutive threads store consecutive int16
            __syncthreads();
            const uint32_t m = min(kInterleaveThreads, hi - base) * channels;
            int16_t* const ob = o + (size_t)base * channels;
            for (uint32_t j = t; j < m; j += kInterleaveThreads) {
                const uint32_t s = j / channels, c = j - s * channels;
                ob[j] = (int16_t)(uint16_t)tab[c][s];
            }
            __syncthreads();
        }
    }
}

// ---- launchers --------------------------------------------------------------------------------------------------------------
size_t generic_encode_workspace_bytes(uint32_t n_frames, uint32_t channels, uint32_t n)
{
    const size_t n_sig = generic_signals(channels, false), blocks = (size_t)n_frames * n_sig;
    return blocks * n * (4 + 4) + blocks * kMaxOrder * 4 + blocks * sizeof(GenericMeta) + ((size_t)n_frames * channels + 1) * (8 + 4) + 1024;
}

static std::atomic<int> g_force_wrap_taps{0};
void set_generic_wrap_taps(int on) { g_force_wrap_taps.store(on, std::memory_order_relaxed); }

hipError_t launch_generic_analyse(const void* d_input, bool in16, uint32_t n_frames, uint32_t channels, uint32_t n_sig, uint32_t n, int32_t* d_sig,
    int32_t* d_res, int32_t* d_q, GenericMeta* d_meta, hipStream_t stream, bool lossless, bool paired)
{
    const uint32_t blocks = n_frames * n_sig;
    if (blocks == 0)
        return hipSuccess;
    const uint32_t wrap = g_force_wrap_taps.load(std::memory_order_relaxed) ? 1u : 0u;
    auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(blocks), dim3(64), 0, stream, d_input, n_frames, channels, n_sig, n, d_sig, d_res, d_q, d_meta, wrap); };
    if (paired) {
        if (in16 && lossless)
            launch(k_generic_analyse<true, true, true>);
        else if (lossless)
            launch(k_generic_analyse<false, true, true>);
        else if (in16)
            launch(k_generic_analyse<true, false, true>);
        else
            launch(k_generic_analyse<false, false, true>);
    } else if (in16 && lossless)
        launch(k_generic_analyse<true, true, false>);
    else if (lossless)
        launch(k_generic_analyse<false, true, false>);
    else if (in16)
        launch(k_generic_analyse<true, false, false>);
    else
        launch(k_generic_analyse<false, false, false>);
    return hipGetLastError();
}

hipError_t launch_generic_plan(const GenericMeta* d_meta, uint32_t n_frames, uint32_t channels, uint32_t n_sig, uint64_t base_bytes, uint64_t* d_frame_offsets,
    uint64_t* d_word_base, uint32_t* d_chosen, uint32_t* d_status, uint64_t* d_total_words, hipStream_t stream, bool paired)
{
    if (paired)
        hipLaunchKernelGGL(k_paired_plan<false>, dim3(1), dim3(kPlanThreads), 0, stream, d_meta, n_frames, channels, n_sig, base_bytes, d_frame_offsets,
            d_word_base, d_chosen, d_status, d_total_words, (uint64_t)0);
    else
        hipLaunchKernelGGL(k_generic_plan<false>, dim3(1), dim3(kPlanThreads), 0, stream, d_meta, n_frames, channels, n_sig, base_bytes, d_frame_offsets,
            d_word_base, d_chosen, d_status, d_total_words, (uint64_t)0);
    return hipGetLastError();
}

hipError_t launch_generic_emit(const GenericMeta* d_meta, uint32_t n_frames, uint32_t channels, uint32_t n_sig, uint32_t n, const int32_t* d_res, const int32_t* d_q,
    const uint32_t* d_chosen, const uint64_t* d_word_base, uint32_t* d_words /* zeroed */, uint64_t words_cap, const uint64_t* d_frame_offsets, uint64_t base_bytes,
    uint8_t* d_frames, uint64_t frames_cap, hipStream_t stream)
{
    const uint32_t subs = n_frames * channels;
    if (subs == 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_generic_pack, dim3(subs), dim3(64), 0, stream, d_meta, n_frames, channels, n_sig, n, d_res, d_q, d_chosen, d_word_base, d_words, words_cap);
    hipLaunchKernelGGL(k_generic_assemble, dim3(subs), dim3(kAsmThreads), 0, stream, d_meta, n_frames, channels, n_sig, n, d_chosen, d_word_base, d_words,
        d_frame_offsets, base_bytes, d_frames, frames_cap);
    return hipGetLastError();
}

// The any-length route's grid of k_generic_combine: a workgroup per (frame, slice of kCombineSlice samples).
static dim3 combine_grid(uint32_t n_frames, uint32_t stride) { return dim3(n_frames, (stride + kCombineSlice - 1) / kCombineSlice); }

hipError_t launch_generic_decode(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint64_t base_bytes, uint32_t n_frames, uint32_t channels, uint32_t stride,
    int32_t* d_dec, GenericSubInfo* d_info, int32_t* d_all, uint32_t* d_counts, const uint64_t* d_sample_offsets, int16_t* d_pcm_out, uint32_t* d_status,
    bool fast_first, bool standard_path, hipStream_t stream)
{
    const uint32_t subs = n_frames * channels;
    if (subs == 0)
        return hipSuccess;
    // (the host's two attempts are two calls: one kernel or the other, the count read on the host in between -- not
    // launch_any_length_subframes, which runs both and lets the device gate the second)
    if (fast_first) {
        const hipError_t e = launch_decode_subframes32(d_frames, d_frame_offsets, base_bytes, n_frames, channels, stride, d_dec, d_info, d_status, standard_path, stream);
        if (e != hipSuccess)
            return e;
    } else
        hipLaunchKernelGGL(k_generic_decode, dim3(subs), dim3(64), 0, stream, d_frames, d_frame_offsets, base_bytes, n_frames, channels, stride, d_dec, d_info, d_status,
            nullptr, nullptr);
    if (d_pcm_out)
        hipLaunchKernelGGL(k_generic_combine<true>, combine_grid(n_frames, stride), dim3(kCombineThreads), 0, stream, d_dec, d_info, n_frames, channels, stride, d_all,
            d_counts, d_sample_offsets, d_pcm_out, d_status, nullptr);
    else
        hipLaunchKernelGGL(k_generic_combine<false>, combine_grid(n_frames, stride), dim3(kCombineThreads), 0, stream, d_dec, d_info, n_frames, channels, stride, d_all,
            d_counts, d_sample_offsets, d_pcm_out, d_status, nullptr);
    return hipGetLastError();
}

// ---- the device-pointer calls' workspaces (sela_workspace.h): one description each, run by the size, the launch and the hooks ---
// What every decode and verify call opens its workspace with: the subframes as decoded, by position (the fast decoder parks its
// residues there too: the routes never run together) | one GenericSubInfo per subframe | the counters | one SampleTile per 4096 frames.
struct DecodeHeadWs {
    int32_t* dec;
    GenericSubInfo* info;
    uint32_t* counters;
    SampleTile* tiles;
};
static DecodeHeadWs carve_decode_head(Carve& c, uint32_t max_frames, uint32_t channels, uint32_t stride, uint32_t n_counters)
{
    const uint64_t subs = (uint64_t)max_frames * channels, n_tiles = ((uint64_t)max_frames + kSampleTileFrames - 1) / kSampleTileFrames;
    DecodeHeadWs w;
    w.dec = c.take<int32_t>(subs * stride);
    w.info = c.take<GenericSubInfo>(subs);
    w.counters = c.take<uint32_t>(n_counters);
    w.tiles = c.take<SampleTile>(std::max<uint64_t>(n_tiles, 1));
    return w;
}

// The device-pointer 32-bit decode: the head, with the fast kernel's four counters.
static DecodeHeadWs carve_decode_i32(Carve& c, uint32_t max_frames, uint32_t channels, uint32_t stride) { return carve_decode_head(c, max_frames, channels, stride, 4); }

size_t decode_i32_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride, Carve* at)
{
    if ((uint64_t)max_frames * channels * stride >= (1ull << 60))
        return SIZE_MAX;
    return measured(at, [&](Carve& c) { carve_decode_i32(c, max_frames, channels, stride); });
}

// The sample index (the host's header walk) on `stream`: one launch up to a tile of frames, three above.
static void launch_sample_index(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t max_frames, const uint32_t* d_n_found, uint32_t channels,
    uint32_t stride, uint64_t* d_sample_offsets, uint32_t* d_status, uint32_t* d_counters, SampleTile* d_tiles, hipStream_t stream)
{
    if (max_frames <= kSampleTileFrames) {
        hipLaunchKernelGGL(k_index_samples<true>, dim3(1), dim3(kSampleThreads), 0, stream, d_frames, d_frame_offsets, max_frames, d_n_found, channels, stride,
            d_sample_offsets, d_status, d_counters, d_tiles);
    } else {
        const uint32_t n_tiles = (uint32_t)(((uint64_t)max_frames + kSampleTileFrames - 1) / kSampleTileFrames);
        hipLaunchKernelGGL(k_index_samples<false>, dim3(n_tiles), dim3(kSampleThreads), 0, stream, d_frames, d_frame_offsets, max_frames, d_n_found, channels, stride,
            d_sample_offsets, d_status, d_counters, d_tiles);
        hipLaunchKernelGGL(k_sample_tiles, dim3(1), dim3(kSampleThreads), 0, stream, d_tiles, n_tiles, max_frames, d_n_found, stride, d_sample_offsets, d_status,
            d_counters);
        if (d_sample_offsets)
            hipLaunchKernelGGL(k_sample_spread, dim3(n_tiles), dim3(kSampleThreads), 0, stream, d_tiles, max_frames, d_n_found, d_sample_offsets);
    }
}

// The any-length route's decode of every subframe, its decisions taken on the device: k_decode_subframes32 counting what it leaves
// alone in the counters (attempt 0), then k_generic_decode over every subframe, each workgroup returning at once unless that count
// is non-zero (attempt 1: then it decodes every subframe again, as the host's second attempt does).  mode 0: the serial kernel
// alone; 2: the fast kernel by segments.  gate: the device's count of frames the route is to touch.  (max_frames * channels is not 0.)
static hipError_t launch_any_length_subframes(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t max_frames, uint32_t channels, uint32_t stride,
    const DecodeHeadWs& w, uint32_t* d_status, int mode, const uint32_t* gate, hipStream_t stream)
{
    if (mode != 0) {
        const hipError_t e = launch_decode_subframes32(d_frames, d_frame_offsets, 0, max_frames, channels, stride, w.dec, w.info, w.counters, mode != 2, stream, gate);
        if (e != hipSuccess)
            return e;
    }
    hipLaunchKernelGGL(k_generic_decode, dim3(max_frames * channels), dim3(64), 0, stream, d_frames, d_frame_offsets, (uint64_t)0, max_frames, channels, stride, w.dec,
        w.info, d_status, gate, mode != 0 ? w.counters + 2 : nullptr);
    return hipGetLastError();
}

// The host route (generic_decode) on one chunk, with its decisions taken on the device: the sample index and the stride check
// (the host's header walk), the subframes (launch_any_length_subframes), and one combine.
hipError_t launch_decode_i32_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t max_frames, const uint32_t* d_n_found, uint32_t channels,
    uint32_t stride, int32_t* d_samples_out, uint32_t* d_counts_out, uint64_t* d_sample_offsets, uint32_t* d_status, void* d_workspace, int mode, hipStream_t stream)
{
    Carve c(d_workspace);
    const DecodeHeadWs w = carve_decode_i32(c, max_frames, channels, stride);
    launch_sample_index(d_frames, d_frame_offsets, max_frames, d_n_found, channels, stride, d_sample_offsets, d_status, w.counters, w.tiles, stream);
    if (max_frames * channels == 0)
        return hipGetLastError();
    const hipError_t e = launch_any_length_subframes(d_frames, d_frame_offsets, max_frames, channels, stride, w, d_status, mode, d_n_found, stream);
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_generic_combine<false>, combine_grid(max_frames, stride), dim3(kCombineThreads), 0, stream, w.dec, w.info, max_frames, channels, stride,
        d_samples_out, d_counts_out, nullptr, nullptr, d_status, d_n_found);
    return hipGetLastError();
}

// The device-pointer int16 decode: the head, with eight counters | the sample offsets | above kInterleaveChannels channels,
// k_generic_combine's channel-major copy.
struct DecodeNWs {
    DecodeHeadWs head;
    uint64_t* offsets;
    int32_t* all;
};
static DecodeNWs carve_decode_n(Carve& c, uint32_t max_frames, uint32_t channels, uint32_t stride)
{
    DecodeNWs w;
    w.head = carve_decode_head(c, max_frames, channels, stride, 8);
    w.offsets = c.take<uint64_t>((uint64_t)max_frames + 1);
    w.all = c.take<int32_t>(channels > kInterleaveChannels ? (uint64_t)max_frames * channels * stride : 0);
    return w;
}

size_t decode_n_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride, Carve* at)
{
    if ((uint64_t)max_frames * channels * stride >= (1ull << 60))
        return SIZE_MAX;
    return measured(at, [&](Carve& c) { carve_decode_n(c, max_frames, channels, stride); });
}

// Route 2 of the int16 calls on device pointers (launch_decode_n_device, launch_verify_n_device): the subframes as in
// launch_decode_i32_device, gated by the any-length route's count (counters[6]), then the int16 writer into d_pcm_out at the
// sample offsets.  (max_frames * channels is not 0.)
static hipError_t launch_any_length_n(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t max_frames, uint32_t channels, uint32_t stride,
    const DecodeNWs& w, const uint64_t* d_so, int16_t* d_pcm_out, uint32_t* d_status, int mode, hipStream_t stream)
{
    const uint32_t* const n_any = w.head.counters + 6;
    const hipError_t e = launch_any_length_subframes(d_frames, d_frame_offsets, max_frames, channels, stride, w.head, d_status, mode, n_any, stream);
    if (e != hipSuccess)
        return e;
    if (channels <= kInterleaveChannels)
        hipLaunchKernelGGL(k_interleave16, dim3(max_frames, (stride + kInterleaveSlice - 1) / kInterleaveSlice), dim3(kInterleaveThreads), 0, stream, w.head.dec,
            w.head.info, max_frames, channels, stride, d_so, d_pcm_out, d_status, n_any);
    else
        hipLaunchKernelGGL(k_generic_combine<true>, combine_grid(max_frames, stride), dim3(kCombineThreads), 0, stream, w.head.dec, w.head.info, max_frames, channels,
            stride, w.all, nullptr, d_so, d_pcm_out, d_status, n_any);
    return hipGetLastError();
}

// sela_hip_decode on one chunk with its decisions taken on the device: the sample index, k_route_n, the 2048-sample decoder
// (k_decode_frames / _wide, sela_decode.hip) on its count, the any-length route on its own (k_decode_subframes32 and
// k_generic_decode as in launch_decode_i32_device) and the int16 writer.  mode as sela_hip_debug_standard_first (the any-length
// route only); recurrence_form and synth_priorities go to the fast decoder (launch_decode).
hipError_t launch_decode_n_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t max_frames, const uint32_t* d_n_found, uint32_t channels,
    uint32_t stride, int16_t* d_pcm_out, uint64_t* d_sample_offsets, uint32_t* d_status, void* d_workspace, int mode, int recurrence_form, uint32_t synth_priorities,
    hipStream_t stream)
{
    Carve c(d_workspace);
    const DecodeNWs w = carve_decode_n(c, max_frames, channels, stride);
    uint64_t* const d_so = d_sample_offsets ? d_sample_offsets : w.offsets;
    const uint32_t* const n_fast = w.head.counters + 5;
    launch_sample_index(d_frames, d_frame_offsets, max_frames, d_n_found, channels, stride, d_so, d_status, w.head.counters, w.head.tiles, stream);
    hipLaunchKernelGGL(k_route_n, dim3(1), dim3(64), 0, stream, max_frames, d_n_found, stride, d_status, w.head.counters);
    if (max_frames * channels == 0)
        return hipGetLastError();
    // route 1: frame f at f * 2048 * channels (= sample_offsets[f] * channels there); flags and malformed frames into d_status
    // as the route's kernels leave them, the words the index wrote kept (no zeroing); its workspace: the decoded subframes' piece,
    // big enough whenever stride >= 2048, the only case in which the route runs
    hipError_t e = launch_decode(d_frames, d_frame_offsets, max_frames, channels, d_pcm_out, d_status, w.head.dec, stream, nullptr, nullptr, nullptr, recurrence_form,
        synth_priorities, n_fast, false);
    if (e != hipSuccess)
        return e;
    // route 2
    return launch_any_length_n(d_frames, d_frame_offsets, max_frames, channels, stride, w, d_so, d_pcm_out, d_status, mode, stream);
}

// ---- verification on the device (sela_hip_verify_device) ----------------------------------------------------
// Workspace: launch_decode_n_device's | the PCM of the routes that are not fused (as sela_hip_decode_n_device writes it) |
// k_verify_compare's words per (frame, slice).
struct VerifyWs {
    DecodeNWs n;
    int16_t* pcm;
    uint64_t* parts;
};
static VerifyWs carve_verify(Carve& c, uint32_t max_frames, uint32_t channels, uint32_t stride)
{
    VerifyWs w;
    w.n = carve_decode_n(c, max_frames, channels, stride);
    w.pcm = c.take<int16_t>((uint64_t)max_frames * channels * stride);
    w.parts = c.take<uint64_t>(std::max<uint64_t>((uint64_t)max_frames * verify_slices(channels, stride), 1));
    return w;
}

size_t verify_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride, Carve* at)
{
    // (frames x channels first: the product of all three can wrap 64 bits; the launch calls keep it below 2^31)
    if ((uint64_t)max_frames * channels >= (1ull << 31) || (uint64_t)max_frames * channels * stride >= (1ull << 60))
        return SIZE_MAX;
    return measured(at, [&](Carve& c) { carve_verify(c, max_frames, channels, stride); });
}

// The int16 family's sequence (verify, levels): launch_decode_n_device with a consumer in place of the PCM.  The sample index,
// k_route_n, k_verify_begin, then
//   route 1, up to kVerifyFusedChannels channels: the consumer's fused kernel on the fast decoder's count -- nothing decoded
//   reaches memory;
//   route 1 above (k_decode_frames_wide) and route 2 (the any-length kernels and the int16 writer): decoded into `pcm` as
//   sela_hip_decode_n_device decodes into d_pcm_out, then the consumer's kernels on the count of the route that ran.
// status[2], the largest samplesPerChannel while k_route_n reads it, is zeroed behind it by k_verify_begin (one thread): the
// consumer's kernels count their frames there.
__global__ __launch_bounds__(64) void k_verify_begin(uint32_t* __restrict__ status)
{
    if (threadIdx.x == 0)
        status[2] = 0;
}

// What every call of either family is given: the stream, where its status goes, and how to launch.
struct StreamCall {
    const uint8_t* d_frames;
    const uint64_t* d_frame_offsets;
    uint32_t max_frames;
    const uint32_t* d_n_found;
    uint32_t channels, stride;
    uint32_t* d_status;
    int mode;
    hipStream_t stream;
};

// fused(dec, n_fast): the consumer's kernel over route 1's frames; consume(d_so, n_any, n_fast or null): the consumer over `pcm`.
template <typename Fused, typename Consume>
static hipError_t launch_n_sequence(const StreamCall& s, const DecodeNWs& n, int16_t* pcm, uint64_t* d_sample_offsets, int recurrence_form, uint32_t synth_priorities,
    Fused fused_step, Consume consume)
{
    const DecodeHeadWs& head = n.head;
    uint64_t* const d_so = d_sample_offsets ? d_sample_offsets : n.offsets;
    const uint32_t* const n_fast = head.counters + 5;
    const uint32_t* const n_any = head.counters + 6;
    launch_sample_index(s.d_frames, s.d_frame_offsets, s.max_frames, s.d_n_found, s.channels, s.stride, d_so, s.d_status, head.counters, head.tiles, s.stream);
    hipLaunchKernelGGL(k_route_n, dim3(1), dim3(64), 0, s.stream, s.max_frames, s.d_n_found, s.stride, s.d_status, head.counters);
    hipLaunchKernelGGL(k_verify_begin, dim3(1), dim3(64), 0, s.stream, s.d_status);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || s.max_frames * s.channels == 0)
        return e;
    // route 1 (its workspace: the decoded subframes' piece, as in launch_decode_n_device)
    const bool fused = s.channels <= kVerifyFusedChannels;
    if (fused)
        e = fused_step(head.dec, n_fast);
    else
        e = launch_decode(s.d_frames, s.d_frame_offsets, s.max_frames, s.channels, pcm, s.d_status, head.dec, s.stream, nullptr, nullptr, nullptr, recurrence_form,
            synth_priorities, n_fast, false);
    if (e != hipSuccess)
        return e;
    // route 2
    e = launch_any_length_n(s.d_frames, s.d_frame_offsets, s.max_frames, s.channels, s.stride, n, d_so, pcm, s.d_status, s.mode, s.stream);
    if (e != hipSuccess)
        return e;
    return consume(d_so, n_any, fused ? nullptr : n_fast);
}

// Verify plugs in k_verify_frames, and k_verify_compare / k_verify_combine.
hipError_t launch_verify_n_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t max_frames, const uint32_t* d_n_found, uint32_t channels,
    uint32_t stride, const int16_t* d_pcm, uint32_t* d_diff_counts, uint32_t* d_first_diff, uint64_t* d_sample_offsets, uint32_t* d_status, void* d_workspace,
    int mode, int recurrence_form, uint32_t synth_priorities, hipStream_t stream)
{
    Carve c(d_workspace);
    const VerifyWs w = carve_verify(c, max_frames, channels, stride);
    return launch_n_sequence({d_frames, d_frame_offsets, max_frames, d_n_found, channels, stride, d_status, mode, stream}, w.n, w.pcm, d_sample_offsets, recurrence_form,
        synth_priorities,
        [&](int32_t* dec, const uint32_t* n_fast) {
            return launch_verify_frames(d_frames, d_frame_offsets, max_frames, channels, d_pcm, d_diff_counts, d_first_diff, d_status, dec, stream, recurrence_form,
                synth_priorities, n_fast);
        },
        [&](const uint64_t* d_so, const uint32_t* n_any, const uint32_t* n_fast) {
            return launch_verify_compare(w.pcm, d_pcm, d_so, max_frames, channels, stride, n_any, n_fast, w.parts, d_diff_counts, d_first_diff, d_status, stream);
        });
}

// ---- levels on the device (sela_hip_levels_device) -------------------------------------------------------------
// Workspace: launch_decode_n_device's | the PCM of the routes that are not fused (as sela_hip_decode_n_device writes it).
struct LevelsWs {
    DecodeNWs n;
    int16_t* pcm;
};
static LevelsWs carve_levels(Carve& c, uint32_t max_frames, uint32_t channels, uint32_t stride)
{
    LevelsWs w;
    w.n = carve_decode_n(c, max_frames, channels, stride);
    w.pcm = c.take<int16_t>((uint64_t)max_frames * channels * stride);
    return w;
}

size_t levels_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride, Carve* at)
{
    if (channels == 0 || verify_workspace_bytes(max_frames, channels, stride) == SIZE_MAX)
        return SIZE_MAX;
    return measured(at, [&](Carve& c) { carve_levels(c, max_frames, channels, stride); });
}

// Levels plug k_level_frames, and k_level_channels / k_level_count, into launch_n_sequence: status[2] becomes the count of frames
// that are not silent.
hipError_t launch_levels_n_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t max_frames, const uint32_t* d_n_found, uint32_t channels,
    uint32_t stride, sela_hip_level* d_levels, uint64_t* d_sample_offsets, uint32_t* d_status, void* d_workspace, int mode, int recurrence_form,
    uint32_t synth_priorities, hipStream_t stream)
{
    Carve c(d_workspace);
    const LevelsWs w = carve_levels(c, max_frames, channels, stride);
    return launch_n_sequence({d_frames, d_frame_offsets, max_frames, d_n_found, channels, stride, d_status, mode, stream}, w.n, w.pcm, d_sample_offsets, recurrence_form,
        synth_priorities,
        [&](int32_t* dec, const uint32_t* n_fast) {
            return launch_level_frames(d_frames, d_frame_offsets, max_frames, channels, d_levels, d_status, dec, stream, recurrence_form, synth_priorities, n_fast);
        },
        [&](const uint64_t* d_so, const uint32_t* n_any, const uint32_t* n_fast) {
            return launch_level_channels(w.pcm, d_so, max_frames, channels, stride, n_any, n_fast, d_levels, d_status, stream);
        });
}

// ---- the envelope on the device (sela_hip_envelope_device) -------------------------------------------------------
// The envelope plugs k_envelope_frames and k_envelope_channels into launch_n_sequence on the levels call's workspace
// (carve_levels): status[2] stays 0.
hipError_t launch_envelope_n_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t max_frames, const uint32_t* d_n_found, uint32_t channels,
    uint32_t stride, uint32_t bucket, struct sela_hip_envelope* d_env, uint64_t* d_sample_offsets, uint32_t* d_status, void* d_workspace, int mode, int recurrence_form,
    uint32_t synth_priorities, hipStream_t stream)
{
    Carve c(d_workspace);
    const LevelsWs w = carve_levels(c, max_frames, channels, stride);
    return launch_n_sequence({d_frames, d_frame_offsets, max_frames, d_n_found, channels, stride, d_status, mode, stream}, w.n, w.pcm, d_sample_offsets, recurrence_form,
        synth_priorities,
        [&](int32_t* dec, const uint32_t* n_fast) {
            return launch_envelope_frames(d_frames, d_frame_offsets, max_frames, channels, stride, bucket, d_env, d_status, dec, stream, recurrence_form, synth_priorities,
                n_fast);
        },
        [&](const uint64_t* d_so, const uint32_t* n_any, const uint32_t* n_fast) {
            return launch_envelope_channels(w.pcm, d_so, max_frames, channels, stride, bucket, n_any, n_fast, d_env, stream);
        });
}

// ---- the digest on the device (sela_hip_digest_device) ----------------------------------------------------------
// Workspace: the levels call's two pieces | a word per (frame, slice) of the routes that are not fused | the fold's word per
// workgroup.
struct DigestWs {
    LevelsWs levels;
    uint32_t *parts, *fold;
};
static DigestWs carve_digest(Carve& c, uint32_t max_frames, uint32_t channels, uint32_t stride)
{
    DigestWs w;
    w.levels = carve_levels(c, max_frames, channels, stride);
    w.parts = c.take<uint32_t>(std::max<uint64_t>((uint64_t)max_frames * digest_slices(channels, stride), 1));
    w.fold = c.take<uint32_t>(digest_fold_blocks(max_frames));
    return w;
}

size_t digest_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride, Carve* at)
{
    if (levels_workspace_bytes(max_frames, channels, stride) == SIZE_MAX)
        return SIZE_MAX;
    return measured(at, [&](Carve& c) { carve_digest(c, max_frames, channels, stride); });
}

// The digest plugs k_digest_frames, and k_digest_pcm / k_digest_slices, into launch_n_sequence (status[2] stays 0), and folds the
// records into d_track behind it: with no frames only the fold runs, and writes {0, 0}.
hipError_t launch_digest_n_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t max_frames, const uint32_t* d_n_found, uint32_t channels,
    uint32_t stride, struct sela_hip_digest* d_digests, uint64_t* d_track, uint64_t* d_sample_offsets, uint32_t* d_status, void* d_workspace, int mode,
    int recurrence_form, uint32_t synth_priorities, hipStream_t stream)
{
    Carve c(d_workspace);
    const DigestWs w = carve_digest(c, max_frames, channels, stride);
    const hipError_t e = launch_n_sequence({d_frames, d_frame_offsets, max_frames, d_n_found, channels, stride, d_status, mode, stream}, w.levels.n, w.levels.pcm,
        d_sample_offsets, recurrence_form, synth_priorities,
        [&](int32_t* dec, const uint32_t* n_fast) {
            return launch_digest_frames(d_frames, d_frame_offsets, max_frames, channels, d_digests, d_status, dec, stream, recurrence_form, synth_priorities, n_fast);
        },
        [&](const uint64_t* d_so, const uint32_t* n_any, const uint32_t* n_fast) {
            return launch_digest_pcm(w.levels.pcm, d_so, max_frames, channels, stride, n_any, n_fast, w.parts, d_digests, stream);
        });
    if (e != hipSuccess)
        return e;
    return launch_digest_fold(d_digests, d_sample_offsets ? d_sample_offsets : w.levels.n.offsets, max_frames, d_n_found, channels, 2, w.fold, d_track, stream);
}

// ---- verification of 32-bit and ragged streams on the device (sela_hip_verify_i32_device) --------------------
// Workspace: launch_decode_i32_device's | the fallback's samples by channel, [frames][channels][stride] | its counts | a mark per
// frame | k_verify32_direct's / _rest's words per (frame, slice) | the two control words.
struct VerifyI32Ws {
    DecodeHeadWs d;
    int32_t* all;
    uint32_t *counts, *marks;
    uint64_t* parts;
    uint32_t* ctl;
};
static VerifyI32Ws carve_verify_i32(Carve& c, uint32_t max_frames, uint32_t channels, uint32_t stride, uint32_t slices /* of a frame: two words each */)
{
    const uint64_t subs = (uint64_t)max_frames * channels;
    VerifyI32Ws w;
    w.d = carve_decode_i32(c, max_frames, channels, stride);
    w.all = c.take<int32_t>(subs * stride);
    w.counts = c.take<uint32_t>(subs);
    w.marks = c.take<uint32_t>(std::max<uint64_t>(max_frames, 1));
    w.parts = c.take<uint64_t>(std::max<uint64_t>((uint64_t)max_frames * slices, 1));
    w.ctl = c.take<uint32_t>(2);
    return w;
}

size_t verify_i32_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride, Carve* at)
{
    // (frames x channels first: the product of all three can wrap 64 bits; the launch calls keep it below 2^31)
    if ((uint64_t)max_frames * channels >= (1ull << 31) || (uint64_t)max_frames * channels * stride >= (1ull << 60))
        return SIZE_MAX;
    return measured(at, [&](Carve& c) { carve_verify_i32(c, max_frames, channels, stride, verify32_slices(stride)); });
}

const uint32_t* verify_i32_control_words(const void* d_workspace, uint32_t max_frames, uint32_t channels, uint32_t stride)
{
    Carve c(d_workspace);
    return carve_verify_i32(c, max_frames, channels, stride, verify32_slices(stride)).ctl;
}

// The int32 family's sequence (verify against int32 and against packed PCM, levels): launch_decode_i32_device with a consumer in
// place of the combine.  The sample index (into d_so), the consumer's begin (status[2], the largest samplesPerChannel, becomes the
// consumer's count of frames; nothing on this route reads it behind the index; the two control words), k_decode_subframes32 and the
// judge into the workspace by position, then the consumer's direct kernel on the subframes as decoded.  The frames it leaves alone
// (any layout that is not direct) send the whole call through k_generic_combine<false> -- gated on the device by k_verify32_gate's
// count, 0 when no frame was left: every workgroup returns at once -- and the consumer's rest kernels take those frames from the
// combine's output and add the slices up.  SELA_HIP_FLAG_BAD_FRAME and status[1] come from the combine as in the decode call: a
// direct frame is never malformed there.
template <typename Begin, typename Direct, typename Rest>
static hipError_t launch_i32_sequence(const StreamCall& s, const VerifyI32Ws& w, uint64_t* d_so, Begin begin, Direct direct, Rest rest)
{
    launch_sample_index(s.d_frames, s.d_frame_offsets, s.max_frames, s.d_n_found, s.channels, s.stride, d_so, s.d_status, w.d.counters, w.d.tiles, s.stream);
    hipError_t e = begin();
    if (e != hipSuccess || s.max_frames * s.channels == 0)
        return e;
    e = launch_any_length_subframes(s.d_frames, s.d_frame_offsets, s.max_frames, s.channels, s.stride, w.d, s.d_status, s.mode, s.d_n_found, s.stream);
    if (e != hipSuccess)
        return e;
    e = direct();
    if (e == hipSuccess)
        e = launch_verify32_gate(s.max_frames, s.d_n_found, w.ctl, s.stream);
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_generic_combine<false>, combine_grid(s.max_frames, s.stride), dim3(kCombineThreads), 0, s.stream, w.d.dec, w.d.info, s.max_frames, s.channels,
        s.stride, w.all, w.counts, nullptr, nullptr, s.d_status, w.ctl + 1);
    return rest();
}

// Verify against int32 plugs in k_verify32_begin, k_verify32_direct, and k_verify32_rest with k_verify32_sum.
hipError_t launch_verify_i32_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t max_frames, const uint32_t* d_n_found, uint32_t channels,
    uint32_t stride, const int32_t* d_samples, const uint32_t* d_lengths, uint32_t* d_diff_counts, uint32_t* d_first_diff, uint64_t* d_sample_offsets,
    uint32_t* d_status, void* d_workspace, int mode, hipStream_t stream)
{
    Carve c(d_workspace);
    const VerifyI32Ws w = carve_verify_i32(c, max_frames, channels, stride, verify32_slices(stride));
    return launch_i32_sequence({d_frames, d_frame_offsets, max_frames, d_n_found, channels, stride, d_status, mode, stream}, w, d_sample_offsets,
        [&] { return launch_verify32_begin(d_status, w.ctl, stream); },
        [&] {
            return launch_verify32_direct(w.d.dec, w.d.info, max_frames, d_n_found, channels, stride, d_samples, d_lengths, d_status, w.ctl, w.marks, w.parts, stream);
        },
        [&] {
            return launch_verify32_rest(w.all, w.counts, max_frames, d_n_found, channels, stride, d_samples, d_lengths, d_status, w.ctl, w.marks, w.parts, d_diff_counts,
                d_first_diff, stream);
        });
}

// ---- levels of 32-bit and ragged streams on the device (sela_hip_levels_i32_device) --------------------------
// Workspace: launch_verify_i32_device's pieces, with a partial record (four 8-byte words) per (frame, slice, channel) where that
// call has two words per (frame, slice).
constexpr uint32_t kLevel32PartWords = 4;
static VerifyI32Ws carve_levels_i32(Carve& c, uint32_t max_frames, uint32_t channels, uint32_t stride)
{
    return carve_verify_i32(c, max_frames, channels, stride, verify32_slices(stride) * channels * kLevel32PartWords);
}

size_t levels_i32_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride, Carve* at)
{
    if (channels == 0 || verify_i32_workspace_bytes(max_frames, channels, stride) == SIZE_MAX)
        return SIZE_MAX;
    return measured(at, [&](Carve& c) { carve_levels_i32(c, max_frames, channels, stride); });
}

const uint32_t* levels_i32_control_words(const void* d_workspace, uint32_t max_frames, uint32_t channels, uint32_t stride)
{
    Carve c(d_workspace);
    return carve_levels_i32(c, max_frames, channels, stride).ctl;
}

// Levels plug k_level32_begin, k_level32_direct, and k_level32_rest with k_level32_sum into launch_i32_sequence: status[2] becomes
// the count of frames that are not silent.
hipError_t launch_levels_i32_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t max_frames, const uint32_t* d_n_found, uint32_t channels,
    uint32_t stride, sela_hip_level32* d_levels, uint64_t* d_sample_offsets, uint32_t* d_status, void* d_workspace, int mode, hipStream_t stream)
{
    Carve c(d_workspace);
    const VerifyI32Ws w = carve_levels_i32(c, max_frames, channels, stride);
    return launch_i32_sequence({d_frames, d_frame_offsets, max_frames, d_n_found, channels, stride, d_status, mode, stream}, w, d_sample_offsets,
        [&] { return launch_level32_begin(d_status, w.ctl, false, stream); },
        [&] { return launch_level32_direct(w.d.dec, w.d.info, max_frames, d_n_found, channels, stride, d_status, w.ctl, w.marks, w.parts, stream); },
        [&] { return launch_level32_rest(w.all, w.counts, max_frames, d_n_found, channels, stride, d_status, w.ctl, w.marks, w.parts, d_levels, stream); });
}

// The partial records alone.
static uint64_t* carve_levels_samples_i32(Carve& c, uint32_t max_frames, uint32_t channels, uint32_t stride)
{
    return c.take<uint64_t>(std::max<uint64_t>((uint64_t)max_frames * verify32_slices(stride) * channels * kLevel32PartWords, 1));
}

size_t levels_samples_i32_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride, Carve* at)
{
    if (channels == 0 || verify_i32_workspace_bytes(max_frames, channels, stride) == SIZE_MAX)
        return SIZE_MAX;
    return measured(at, [&](Carve& c) { carve_levels_samples_i32(c, max_frames, channels, stride); });
}

hipError_t launch_levels_samples_i32_device(const int32_t* d_samples, const uint32_t* d_counts, uint32_t max_frames, uint32_t channels, uint32_t stride,
    sela_hip_level32* d_levels, uint32_t* d_status, void* d_workspace, hipStream_t stream)
{
    Carve c(d_workspace);
    uint64_t* const parts = carve_levels_samples_i32(c, max_frames, channels, stride);
    const hipError_t e = launch_level32_begin(d_status, nullptr, true, stream);
    if (e != hipSuccess || max_frames * channels == 0)
        return e;
    return launch_level32_rest(d_samples, d_counts, max_frames, nullptr, channels, stride, d_status, nullptr, nullptr, parts, d_levels, stream);
}

// ---- the envelope of 32-bit and ragged streams on the device (sela_hip_envelope_i32_device) --------------------
// Workspace: launch_verify_i32_device's pieces as that call carves them.  Its words per (frame, slice) lie unused: a slice holds
// whole buckets, so the kernels write the records themselves.
static VerifyI32Ws carve_envelope_i32(Carve& c, uint32_t max_frames, uint32_t channels, uint32_t stride)
{
    return carve_verify_i32(c, max_frames, channels, stride, verify32_slices(stride));
}

size_t envelope_i32_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride, Carve* at)
{
    if (verify_i32_workspace_bytes(max_frames, channels, stride) == SIZE_MAX)
        return SIZE_MAX;
    return measured(at, [&](Carve& c) { carve_envelope_i32(c, max_frames, channels, stride); });
}

const uint32_t* envelope_i32_control_words(const void* d_workspace, uint32_t max_frames, uint32_t channels, uint32_t stride)
{
    Carve c(d_workspace);
    return carve_envelope_i32(c, max_frames, channels, stride).ctl;
}

// The envelope plugs k_level32_begin, k_envelope32_direct and k_envelope32_rest into launch_i32_sequence: status[2] stays 0.
hipError_t launch_envelope_i32_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t max_frames, const uint32_t* d_n_found, uint32_t channels,
    uint32_t stride, uint32_t bucket, struct sela_hip_envelope32* d_env, uint64_t* d_sample_offsets, uint32_t* d_status, void* d_workspace, int mode, hipStream_t stream)
{
    Carve c(d_workspace);
    const VerifyI32Ws w = carve_envelope_i32(c, max_frames, channels, stride);
    return launch_i32_sequence({d_frames, d_frame_offsets, max_frames, d_n_found, channels, stride, d_status, mode, stream}, w, d_sample_offsets,
        [&] { return launch_level32_begin(d_status, w.ctl, false, stream); },
        [&] { return launch_envelope32_direct(w.d.dec, w.d.info, max_frames, d_n_found, channels, stride, bucket, d_status, w.ctl, w.marks, d_env, stream); },
        [&] { return launch_envelope32_rest(w.all, w.counts, max_frames, channels, stride, bucket, d_status, w.ctl, w.marks, d_env, stream); });
}

// A token: the one kernel leaves nothing between launches.
size_t envelope_samples_i32_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride, Carve* at)
{
    if (channels == 0 || verify_i32_workspace_bytes(max_frames, channels, stride) == SIZE_MAX)
        return SIZE_MAX;
    return measured(at, [&](Carve& c) { c.take<uint64_t>(1); });
}

hipError_t launch_envelope_samples_i32_device(const int32_t* d_samples, const uint32_t* d_counts, uint32_t max_frames, uint32_t channels, uint32_t stride, uint32_t bucket,
    struct sela_hip_envelope32* d_env, uint32_t* d_status, hipStream_t stream)
{
    const hipError_t e = launch_level32_begin(d_status, nullptr, true, stream);
    if (e != hipSuccess || max_frames * channels == 0)
        return e;
    return launch_envelope32_rest(d_samples, d_counts, max_frames, channels, stride, bucket, d_status, nullptr, nullptr, d_env, stream);
}

// ---- verification against packed PCM on the device (sela_hip_verify_pcm_device) -------------------------------
// Workspace: launch_verify_i32_device's pieces, the words per (frame, slice) sized by the tiles of sela_pcm_layout.h | the sample
// offsets of a caller that asks for none.
struct VerifyPcmWs {
    VerifyI32Ws v;
    uint64_t* offsets;
};
static VerifyPcmWs carve_verify_pcm(Carve& c, uint32_t max_frames, uint32_t channels, uint32_t stride)
{
    VerifyPcmWs w;
    w.v = carve_verify_i32(c, max_frames, channels, stride, verify_pcm_tiles(stride, channels));
    w.offsets = c.take<uint64_t>((uint64_t)max_frames + 1);
    return w;
}

size_t verify_pcm_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride, Carve* at)
{
    if (channels == 0 || verify_i32_workspace_bytes(max_frames, channels, stride) == SIZE_MAX)
        return SIZE_MAX;
    return measured(at, [&](Carve& c) { carve_verify_pcm(c, max_frames, channels, stride); });
}

const uint32_t* verify_pcm_control_words(const void* d_workspace, uint32_t max_frames, uint32_t channels, uint32_t stride)
{
    Carve c(d_workspace);
    return carve_verify_pcm(c, max_frames, channels, stride).v.ctl;
}

// Verify against packed PCM plugs sela_verify_pcm.hip's kernels into launch_i32_sequence: k_verify32_begin, k_verify_pcm<., false>,
// and k_verify_pcm<., true> with k_verify32_sum over the tiles.  The sample index goes into the caller's offsets or the workspace's:
// the compare reads them.
hipError_t launch_verify_pcm_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t max_frames, const uint32_t* d_n_found, uint32_t channels,
    uint32_t stride, const void* d_pcm, uint32_t bytes_per_sample, uint64_t pcm_samples, uint32_t* d_diff_counts, uint32_t* d_first_diff, uint64_t* d_sample_offsets,
    uint32_t* d_status, void* d_workspace, int mode, hipStream_t stream)
{
    Carve c(d_workspace);
    const VerifyPcmWs pw = carve_verify_pcm(c, max_frames, channels, stride);
    const VerifyI32Ws& w = pw.v;
    uint64_t* const d_so = d_sample_offsets ? d_sample_offsets : pw.offsets;
    return launch_i32_sequence({d_frames, d_frame_offsets, max_frames, d_n_found, channels, stride, d_status, mode, stream}, w, d_so,
        [&] { return launch_verify32_begin(d_status, w.ctl, stream); },
        [&] {
            return launch_verify_pcm_direct(w.d.dec, w.d.info, max_frames, d_n_found, channels, stride, d_pcm, bytes_per_sample, pcm_samples, d_so, d_status, w.ctl,
                w.marks, w.parts, stream);
        },
        [&] {
            const hipError_t e = launch_verify_pcm_rest(w.all, w.counts, max_frames, channels, stride, d_pcm, bytes_per_sample, pcm_samples, d_so, d_status, w.ctl,
                w.marks, w.parts, stream);
            if (e != hipSuccess)
                return e;
            return launch_verify32_sum(w.parts, verify_pcm_tiles(stride, channels), max_frames, d_n_found, d_diff_counts, d_first_diff, d_status, stream);
        });
}

// ---- the digest of 24- and 32-bit streams on the device (sela_hip_digest_pcm_device) ---------------------------
// Workspace: launch_verify_pcm_device's pieces (of its two words per (frame, tile) the tile's raw CRC takes the first max_frames *
// tiles; its sample offsets for a caller that passes none) | the track fold's word per workgroup.
struct DigestPcmWs {
    VerifyPcmWs p;
    uint32_t* fold;
};
static DigestPcmWs carve_digest_pcm(Carve& c, uint32_t max_frames, uint32_t channels, uint32_t stride)
{
    DigestPcmWs w;
    w.p = carve_verify_pcm(c, max_frames, channels, stride);
    w.fold = c.take<uint32_t>(digest_fold_blocks(max_frames));
    return w;
}

size_t digest_pcm_workspace_bytes(uint32_t max_frames, uint32_t channels, uint32_t stride, Carve* at)
{
    if (verify_pcm_workspace_bytes(max_frames, channels, stride) == SIZE_MAX)
        return SIZE_MAX;
    return measured(at, [&](Carve& c) { carve_digest_pcm(c, max_frames, channels, stride); });
}

const uint32_t* digest_pcm_control_words(const void* d_workspace, uint32_t max_frames, uint32_t channels, uint32_t stride)
{
    Carve c(d_workspace);
    return carve_digest_pcm(c, max_frames, channels, stride).p.v.ctl;
}

// The digest plugs sela_digest_pcm.hip's kernels into launch_i32_sequence -- k_digest32_begin, k_digest32_tiles<., false>, and
// k_digest32_tiles<., true> -- and runs sela_digest.hip's folds behind it with bytes_per_sample for the bytes of a value: the
// tiles' words into the records, the records into d_track.  With no frames only the track fold runs, and writes {0, 0}.
hipError_t launch_digest_pcm_device(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t max_frames, const uint32_t* d_n_found, uint32_t channels,
    uint32_t stride, uint32_t bytes_per_sample, struct sela_hip_digest* d_digests, uint64_t* d_track, uint64_t* d_sample_offsets, uint32_t* d_status,
    void* d_workspace, int mode, hipStream_t stream)
{
    Carve c(d_workspace);
    const DigestPcmWs dw = carve_digest_pcm(c, max_frames, channels, stride);
    const VerifyI32Ws& w = dw.p.v;
    uint64_t* const d_so = d_sample_offsets ? d_sample_offsets : dw.p.offsets;
    uint32_t* const parts = reinterpret_cast<uint32_t*>(w.parts);
    const uint32_t n_tiles = verify_pcm_tiles(stride, channels);
    hipError_t e = launch_i32_sequence({d_frames, d_frame_offsets, max_frames, d_n_found, channels, stride, d_status, mode, stream}, w, d_so,
        [&] { return launch_digest32_begin(w.ctl, stream); },
        [&] {
            return launch_digest32_direct(w.d.dec, w.d.info, max_frames, d_n_found, channels, stride, bytes_per_sample, d_so, d_status, w.ctl, w.marks, parts, stream);
        },
        [&] { return launch_digest32_rest(w.all, w.counts, max_frames, channels, stride, bytes_per_sample, d_so, d_status, w.ctl, w.marks, parts, stream); });
    if (e == hipSuccess)
        e = launch_digest_slices(parts, d_so, max_frames, channels, stride, d_n_found, nullptr, digest_pcm_tile_bytes(channels, bytes_per_sample), n_tiles,
            bytes_per_sample, d_digests, stream);
    if (e != hipSuccess)
        return e;
    return launch_digest_fold(d_digests, d_so, max_frames, d_n_found, channels, bytes_per_sample, dw.fold, d_track, stream);
}

// Workspace of the device-pointer encode: signals | residues | q | meta records | word bases | choices | the plan's total.  No
// Rice words: k_generic_write packs into the frames.
struct EncodeI32Ws {
    int32_t *sig, *res, *q;
    GenericMeta* meta;
    uint64_t* word_base;
    uint32_t* chosen;
    uint64_t* total;
};
static EncodeI32Ws carve_encode_i32(Carve& c, uint32_t n_frames, uint32_t channels, uint32_t n, bool paired)
{
    const uint64_t blocks = (uint64_t)n_frames * generic_signals(channels, paired), subs = (uint64_t)n_frames * channels;
    EncodeI32Ws w;
    w.sig = c.take<int32_t>(blocks * n);
    w.res = c.take<int32_t>(blocks * n);
    w.q = c.take<int32_t>(blocks * kMaxOrder);
    w.meta = c.take<GenericMeta>(blocks);
    w.word_base = c.take<uint64_t>(subs + 1);
    w.chosen = c.take<uint32_t>(subs);
    w.total = c.take<uint64_t>(1);
    return w;
}

size_t encode_i32_device_workspace_bytes(uint32_t n_frames, uint32_t channels, uint32_t n, bool paired, Carve* at)
{
    if (channels == 0 || channels > 255 || n == 0 || n > 65535 || (uint64_t)n_frames * generic_signals(channels, paired) >= (1ull << 31))
        return SIZE_MAX;
    return measured(at, [&](Carve& c) { carve_encode_i32(c, n_frames, channels, n, paired); });
}

// sela_hip_encode_i32_device / sela_hip_encode_n_device: analyse, plan (base 0, the offsets straight into the
// caller's, the status words written whole) and write, all on `stream`, nothing waited for.  Arguments checked by the caller.
// paired (sela_hip_encode_paired_*_device): the same three launches over generic_signals(channels, true) signals.
hipError_t launch_encode_i32_device(const void* d_input, bool in16, uint32_t n_frames, uint32_t channels, uint32_t n, uint8_t* d_frames, uint64_t frames_cap,
    uint64_t* d_frame_offsets, uint32_t* d_status, void* d_workspace, hipStream_t stream, bool lossless, bool paired)
{
    Carve c(d_workspace);
    const EncodeI32Ws w = carve_encode_i32(c, n_frames, channels, n, paired);
    const uint32_t n_sig = generic_signals(channels, paired);
    hipError_t e = launch_generic_analyse(d_input, in16, n_frames, channels, n_sig, n, w.sig, w.res, w.q, w.meta, stream, lossless, paired);
    if (e != hipSuccess)
        return e;
    if (paired)
        hipLaunchKernelGGL(k_paired_plan<true>, dim3(1), dim3(kPlanThreads), 0, stream, w.meta, n_frames, channels, n_sig, (uint64_t)0, d_frame_offsets,
            w.word_base, w.chosen, d_status, w.total, frames_cap);
    else
        hipLaunchKernelGGL(k_generic_plan<true>, dim3(1), dim3(kPlanThreads), 0, stream, w.meta, n_frames, channels, n_sig, (uint64_t)0, d_frame_offsets,
            w.word_base, w.chosen, d_status, w.total, frames_cap);
    const uint32_t subs = n_frames * channels;
    if (subs)
        hipLaunchKernelGGL(k_generic_write, dim3(subs), dim3(64), 0, stream, w.meta, n_frames, channels, n_sig, n, w.res, w.q, w.chosen, w.word_base,
            d_frame_offsets, d_frames, frames_cap);
    return hipGetLastError();
}

} // namespace sela
