// sela_synth.h -- the decoder's synthesis filter (lpc::SampleGenerator as a transposed-form recurrence over the lanes of a wave), its
// coefficient table, and the few things it shares with the parsers of sela_decode_core.inc: the Rice value, the stream's buffer
// resource and the 64-bit window.  Every translation unit that decodes a subframe includes it in front of sela_decode_core.inc and
// compiles its own copy of the templates (the kernels live on their register budgets -- tests/test_isa_*.py -- and the synthesis is
// a real call, see synthesize); DESIGN.md 5.5.
#ifndef SELA_SYNTH_H_
#define SELA_SYNTH_H_

#include "sela_device.h"

namespace sela {

typedef const volatile __attribute__((address_space(3))) uint64_t* LdsTable;

__device__ __forceinline__ int32_t rice_value(uint32_t ones, uint32_t field, uint32_t k)
{
    const uint32_t rem = k ? (__brev(field) >> (32 - k)) : 0u; // remainder is MSB first in the stream
    const uint32_t u = (ones << k) | rem;                      // uint32 arithmetic as src/rice/rice_decoder.cpp:35
    return (int32_t)((u >> 1) ^ (0u - (u & 1u)));               // un-zig-zag, src/rice/rice_decoder.cpp:49-50
}

// ---- the subframe's aligned words, where they lie ------------------------------------------------------------
// A raw-dword buffer resource over [words, words + n_words): reads beyond return 0 (hardware bounds check),
// which is exactly the zero padding the parser wants behind a stream.  Rebuilt from scalars at every use site
// that a function call separates from its creation (a resource that travelled through arguments is no longer
// known to be wave-uniform).
struct StreamWords {
    const uint32_t* words;
    uint32_t n_words;
};
__device__ __forceinline__ __amdgpu_buffer_rsrc_t stream_rsrc(const StreamWords& s)
{
    return __builtin_amdgcn_make_buffer_rsrc(
        reinterpret_cast<void*>(read_first_lane(reinterpret_cast<uint64_t>(s.words))), 0,
        4u * (uint32_t)__builtin_amdgcn_readfirstlane((int)s.n_words), 0x00020000);
}
// 64 stream bits at bit position p
__device__ __forceinline__ void window64(__amdgpu_buffer_rsrc_t rs, uint32_t p, uint32_t& x0, uint32_t& x1)
{
    const uint32_t b = 4 * (p >> 5), sh = p & 31;
    const uint32_t w0 = __builtin_amdgcn_raw_buffer_load_b32(rs, b, 0, 0), w1 = __builtin_amdgcn_raw_buffer_load_b32(rs, b + 4, 0, 0),
                   w2 = __builtin_amdgcn_raw_buffer_load_b32(rs, b + 8, 0, 0);
    x0 = __builtin_amdgcn_alignbit(w1, w0, sh);
    x1 = __builtin_amdgcn_alignbit(w2, w1, sh);
}

// ---- synthesis filter ----------------------------------------------------------------------------------
// lpc::SampleGenerator::generateSamples (src/lpc/sample_generator.cpp:11-30).  Transposed direct form
// without data movement: every sample that is still to come owns a partial sum, and the sum of sample j
// lives in lane j mod 64 for its whole life (a ring over the lanes; orders above 60 use two registers per
// lane = a ring of 128).  Once sample s_i is known, the lane that owns sample i + d adds a[d] * s_i; its
// coefficient a[(lane - i) mod ring] comes out of a doubled table in LDS at a compile-time offset (the 64
// steps of a block are unrolled), so nothing is shifted between lanes.  The recurrence itself (sum -> s_i)
// runs on the scalar unit: v_readlane of the finished sum, one SALU op (two in the exact form), and the result
// feeds the multiply-adds as a scalar operand.
//
// What is accumulated is N = 2^34 - sum(a_j s_(i-j)) = 2^34 + sum(a_j (-s_(i-j))): every sum starts at the
// rounding constant 2^34 and the multiplier of a step is MINUS its sample, so the prediction
// (int32)((2^34 - P) >> 35) is the arithmetic shift (int32)N_hi >> 3 of the HIGH word alone (the reference's cast
// keeps exactly those 29 bits).
//
// A finished sum is not touched again until its lane is recycled: the coefficients of lags
// ring - G + 1 .. ring - 1 are zero (order <= ring - G), so lanes are recycled in aligned groups of G
// (three DPP moves under a row/bank mask: keep the finished high words, restart the sums), and the
// 64 samples of a block are derived from the kept words in one vector step.  Per sample that is
// 3 + 3/G VALU instructions (5 + 3/G on the ring of 128) and one (two) ds_read_b64.
//
// 64x32-bit products: a' = ah*2^32 + al with al = (int32)a', so
//     z + a*m mod 2^64 = (z + al*m)  [v_mad_i64_i32, exact]  +  ((ah*m mod 2^32) << 32)
//
// kFold: the residue is folded into its sum at the start of its block of 64,
//     N' = N - r * 2^35  (one subtract on the high word per 64 samples)   ==>   s = -(N' >> 35),
// which drops the per-sample v_readlane of r, and the high product is one v_mad_i32_i24.  Both need
// small operands: the high word keeps r only mod 2^29, so the folded s is (r - pred) reduced to 29 signed
// bits, and the multiplier takes 24.  With |a| < 2^55 (checked when the table is built), |r| < 2^23 (checked
// on the block's residues before it starts) and |pred| < 2^28 (a 29-bit value), the true |s| is below
// 2^28 + 2^23: where it is below 2^28 the reduction is s itself, elsewhere the reduced value exceeds 2^23 in
// size.  So with the check of every 64 samples against 2^23 the folded form equals the reference's 32-bit
// r - (int32)((2^34 - P) >> 35) exactly, or gives up.  A block whose residues fail their check runs, with the
// rest of the subframe, in the exact form (v_readlane of r, v_mul_lo_u32 + v_add_u32); one whose samples fail
// theirs has stored nothing: the caller puts the sums back as they were at the block's start and does the
// same.  16-bit audio never gets there; wide audio and crafted streams do (tests).
// kShift: also hand back (new high word) >> 3, the next step's multiplier if the next step's sum is in this register
// (kVecShift, see synth_steps).
template <bool kFold, bool kShift>
__device__ __forceinline__ void synth_mac(uint32_t& zl, uint32_t& zh, uint64_t coef, int32_t s_i, int32_t& shifted)
{
    const int32_t al = (int32_t)(uint32_t)coef, ah = (int32_t)(uint32_t)(coef >> 32);
    const uint64_t z = ((uint64_t)zh << 32) | zl;
    const uint64_t lo = (uint64_t)((int64_t)z + (int64_t)al * (int64_t)s_i);
    if (kFold) { // both factors fit 24 bits in the folded form (checked)
        if (kShift)
            asm("v_mad_i32_i24 %0, %2, %3, %4\n\tv_ashrrev_i32 %1, 3, %0" : "=v"(zh), "=v"(shifted) : "v"(ah), "s"(s_i), "v"((uint32_t)(lo >> 32)));
        else
            asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(zh) : "v"(ah), "s"(s_i), "v"((uint32_t)(lo >> 32)));
    } else {
        zh = (uint32_t)(lo >> 32) + (uint32_t)ah * (uint32_t)s_i;
        if (kShift) {
            shifted = (int32_t)zh >> 3;
            asm volatile("" : "+v"(shifted)); // (stays a vector shift: the compiler would move it behind the readlane)
        }
    }
    zl = (uint32_t)lo;
}

// Coefficient prefetch depth (steps).  The table reads have compile-time addresses, so left alone the
// scheduler hoists all 64 (128) of a block to its top and spills; instead each step consumes the
// value fetched kAhead steps earlier, issues the fetch for step M + kAhead and ends in a scheduling
// barrier.  (LdsTable is volatile: that keeps the two reads of a ring-of-128 step as ds_read_b64, 2 LDS
// cycles each; merged into one ds_read2_b64 they would take 8 and the loop turns LDS-bound.)
constexpr int kAhead = 4;

// Steps M .. 63 of one block of 64 samples.  (cl, ch): the register whose sums finish in this block;
// (ol, oh): the other register of the ring of 128 (R == 2).  tab_lane = table + lane.
//
// kVecShift: where the >> 3 of the prediction happens.  false: on the scalar unit, behind the v_readlane (three vector
// instructions per step: what a SIMD shared by seven waves, bound by vector issue, wants).  true: on the vector unit, in
// front of it (four, but the step's dependency chain loses its detour through the scalar ALU: 36 instead of 50 cycles per
// sample for a wave that has its SIMD to itself -- tools/chain_ubench.py -- which is how small batches and the last
// workgroups of a launch run).  Same bits either way.
template <int R, bool kFold, int G, bool kVecShift, int M>
__device__ __forceinline__ void synth_steps(uint32_t& cl, uint32_t& ch, uint32_t& ol, uint32_t& oh, uint32_t& kept,
    LdsTable tab_lane, int32_t r_block, uint32_t four, uint32_t zero, uint64_t (&pf_c)[kAhead], uint64_t (&pf_o)[kAhead], int32_t& shifted)
{
    // scalar side: the sum of this sample sits in lane M.  What goes back into the sums is -a_d * s_i; the table holds
    // +a_d, so the multiplier is -s_i: in the folded form that IS the shifted sum (s_i = -pred: one scalar operation
    // between the readlane and the multiply-adds instead of two), in the exact form pred - r_i.
    // (kVecShift: `shifted` = ch >> 3 as of the end of the step before -- the lanes a step recycles are behind it)
    const int32_t pred = kVecShift ? __builtin_amdgcn_readlane(shifted, M) : __builtin_amdgcn_readlane((int)ch, M) >> 3;
    int32_t m_i;
    if (kFold)
        m_i = pred;
    else
        m_i = (int32_t)((uint32_t)pred - (uint32_t)__builtin_amdgcn_readlane(r_block, M));
    // vector side: lane L adds a[(L - M) mod ring] * (-s_i)  (a[0] = 0: the finished sum stays)
    synth_mac<kFold, kVecShift>(cl, ch, pf_c[M % kAhead], m_i, shifted);
    if (R == 2) {
        int32_t unused;
        synth_mac<kFold, false>(ol, oh, pf_o[M % kAhead], m_i, unused);
    }
    if constexpr (M + kAhead < 64) {
        pf_c[M % kAhead] = tab_lane[64 * R - (M + kAhead)];
        if (R == 2)
            pf_o[M % kAhead] = tab_lane[64 - (M + kAhead)];
    }
    if constexpr ((M + 1) % G == 0) { // recycle lanes M + 1 - G .. M
        constexpr int first_lane = M + 1 - G;
        constexpr int row_mask = 1 << (first_lane / 16);
        constexpr int bank_mask = G == 16 ? 0xf : 1 << ((first_lane % 16) / 4);
        kept = (uint32_t)__builtin_amdgcn_update_dpp((int)kept, (int)ch, 0xE4 /* quad_perm:[0,1,2,3] */, row_mask, bank_mask, false);
        ch = (uint32_t)__builtin_amdgcn_update_dpp((int)ch, (int)four, 0xE4, row_mask, bank_mask, false);
        cl = (uint32_t)__builtin_amdgcn_update_dpp((int)cl, (int)zero, 0xE4, row_mask, bank_mask, false);
    }
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (M < 63)
        synth_steps<R, kFold, G, kVecShift, M + 1>(cl, ch, ol, oh, kept, tab_lane, r_block, four, zero, pf_c, pf_o, shifted);
}

// One block of 64 samples with residues r_block (one per lane).  The folded form returns false if a sample
// of the block left its range (s is then meaningless).
template <int R, bool kFold, int G, bool kVecShift>
__device__ __forceinline__ bool synth_block(int32_t r_block, int32_t& s, uint32_t& cl, uint32_t& ch, uint32_t& ol, uint32_t& oh,
    LdsTable tab_lane, uint32_t four, uint32_t zero)
{
    uint64_t pf_c[kAhead], pf_o[kAhead];
#pragma unroll
    for (int m = 0; m < kAhead; m++) {
        pf_c[m] = tab_lane[64 * R - m];
        pf_o[m] = R == 2 ? tab_lane[64 - m] : 0;
    }
    if (kFold)
        ch -= (uint32_t)r_block << 3; // sample lane of this block: N -= r * 2^35
    uint32_t kept = 0;
    int32_t shifted = 0;
    if (kVecShift) {
        shifted = (int32_t)ch >> 3;
        asm volatile("" : "+v"(shifted)); // (stays a vector shift: the compiler would move it behind the readlane)
    }
    __builtin_amdgcn_sched_barrier(0);
    synth_steps<R, kFold, G, kVecShift, 0>(cl, ch, ol, oh, kept, tab_lane, r_block, four, zero, pf_c, pf_o, shifted);
    s = (int32_t)((kFold ? 0u : (uint32_t)r_block) - (uint32_t)((int32_t)kept >> 3));
    // (the multiplier of a folded step is -s: both s and -s must fit the 24-bit operand)
    return !kFold || !__any((uint32_t)(s + (1 << 23) - 1) >= (1u << 24) - 1u);
}

// All 2048 samples of a subframe.  R = ring / 64 (1: order <= 64 - G, 2: order <= 128 - G); G = recycling
// group (4 or 16).  fold = start in the folded form (the coefficients fit it).  Residues: decoded just in time
// from the codeword positions in pos_smp[] (ws == nullptr), the words fetched one block ahead -- or read from
// the workspace array ws[] (generic mode).  Samples go to pos_smp[] as int16, over the positions of the
// block just consumed.
// Where the 32-bit instantiations leave their samples.  (An empty record for the 16-bit ones: the AMDGPU calling convention
// passes nothing for it, so the frame kernels' instantiations stay, instruction for instruction, what they were.)
template <bool kOut32>
struct SynthOut {
};
template <>
struct SynthOut<true> {
    int32_t* samples; // global memory, the subframe's first sample
    uint32_t n;       // how many samples the subframe has (any number: the last block of 64 is masked, a ring of 128 may end on an odd block)
};

template <int R, int G, bool kVecShift, bool kOut32 = false>
__device__ __attribute__((noinline)) void synthesize( // (a real call: six of these inlined into three kernels cost the kernels their registers)
    const uint32_t* words, uint32_t n_words, uint32_t k, uint16_t* pos_smp, const int32_t* ws,
    const uint64_t* tab, bool fold, int lane, SynthOut<kOut32> out32 = SynthOut<kOut32>())
{
    // kOut32 (the stage on its own, k_stage_lpc_decode, and the 32-bit frame kernel, k_decode_subframes32): the samples go to
    // out32.samples as the 32-bit values lpc::SampleGenerator returns; pos_smp[] is only read (the positions, when ws == nullptr).
    // There the subframe's length is a run-time value (out32.n): residues beyond it read as zero and their samples are not stored
    // (ws may BE out32.samples: a block's residues are in registers before its samples are stored).
    static_assert(G == 4 || G == 16, "groups are DPP banks or rows");
    const StreamWords sw = { words, n_words };
    const __amdgpu_buffer_rsrc_t rs = stream_rsrc(sw);
    k = (uint32_t)__builtin_amdgcn_readfirstlane((int)k);
    const uint32_t kmask = k ? (0xFFFFFFFFu >> (32 - k)) : 0u;
    const bool jit = read_first_lane(reinterpret_cast<uint64_t>(ws)) == 0;
    uint32_t zl[2], zh[2];
#pragma unroll
    for (int h = 0; h < 2; h++) { // every sum starts at 2^34
        zl[h] = 0;
        zh[h] = 4;
    }
    uint32_t four = 4, zero = 0;
    asm volatile("" : "+v"(four), "+v"(zero)); // DPP sources must be VGPRs
    const LdsTable tab_lane = (LdsTable)(tab + lane); // the table is in LDS: ds_read with immediate offsets
    // the block ahead: its codeword's position and three stream words (or its residue, generic mode)
    // (The 16-bit instantiations keep the workspace mode's residue in w2.  With a variable of its own, assigned in the other arm
    // of the branch that assigns w2, the compiler sinks the two stores into one through a selected address, both variables
    // live in scratch memory, and the words just asked for are waited for at once and go round through it, once per block.
    // The 32-bit instantiations still do exactly that, and still run the ring of 128 as two copies of the block, one per role
    // of its registers: tests/test_isa_verify32.py holds k_decode_subframes32 to 69 / 56 VGPRs by equality, and neither
    // change leaves it there.)
    uint32_t p = 0, w0 = 0, w1 = 0, w2 = 0;
    int32_t r_ws = 0; // kOut32 only
    uint32_t n_samples = (uint32_t)kBlock;
    if constexpr (kOut32)
        n_samples = (uint32_t)__builtin_amdgcn_readfirstlane((int)out32.n);
    const int n_blocks = kOut32 ? (int)((n_samples + 63) / 64) : kBlock / 64;
    auto issue = [&](int blk) {
        if (jit) {
            p = pos_smp[64 * blk + lane];
            const uint32_t b = 4 * (p >> 5);
            w0 = __builtin_amdgcn_raw_buffer_load_b32(rs, b, 0, 0);
            w1 = __builtin_amdgcn_raw_buffer_load_b32(rs, b + 4, 0, 0);
            w2 = __builtin_amdgcn_raw_buffer_load_b32(rs, b + 8, 0, 0);
        } else if constexpr (kOut32) {
            r_ws = (uint32_t)(64 * blk + lane) < n_samples ? ws[64 * blk + lane] : 0;
        } else {
            w2 = (uint32_t)ws[64 * blk + lane];
        }
    };
    auto land = [&]() -> int32_t {
        if (!jit)
            return kOut32 ? r_ws : (int32_t)w2;
        uint32_t x0 = __builtin_amdgcn_alignbit(w1, w0, p & 31), x1 = __builtin_amdgcn_alignbit(w2, w1, p & 31), ones = 0;
        while (__any(x0 == 0xFFFFFFFFu)) { // runs of 32 ones and more (rare): follow them word by word
            const bool more = x0 == 0xFFFFFFFFu;
            ones += more ? 32u : 0u;
            p += more ? 32u : 0u;
            window64(rs, p, x0, x1);
        }
        const uint32_t t = (uint32_t)__builtin_ctz(~x0);
        const uint32_t field = (uint32_t)(((((uint64_t)x1) << 32) | x0) >> (t + 1)) & kmask;
        return rice_value(ones + t, field, k);
    };
    // one block: (cl, ch) = the register whose sums finish in it, (ol, oh) = the other register of a ring of 128
    auto run_block = [&](int blk, uint32_t& cl, uint32_t& ch, uint32_t& ol, uint32_t& oh) {
        const int32_t r_block = land();
        if (blk + 1 < n_blocks)
            issue(blk + 1); // in flight during this block's 64 steps
        int32_t s;
        bool done = false;
        // (a residue the folded subtraction cannot carry whole: see synth_mac)
        fold = fold && !__any((uint32_t)(r_block + (1 << 23) - 1) >= (1u << 24) - 1u);
        if (fold) {
            const uint32_t s0 = cl, s1 = ch, s2 = ol, s3 = oh;
            done = synth_block<R, true, G, kVecShift>(r_block, s, cl, ch, ol, oh, tab_lane, four, zero);
            if (!done) { // back to the block's start, exact form from here on
                cl = s0, ch = s1;
                if (R == 2)
                    ol = s2, oh = s3;
                fold = false;
            }
        }
        if (!done)
            synth_block<R, false, G, kVecShift>(r_block, s, cl, ch, ol, oh, tab_lane, four, zero);
        if constexpr (kOut32) {
            if ((uint32_t)(64 * blk + lane) < n_samples)
                out32.samples[64 * blk + lane] = s;
        } else
            reinterpret_cast<int16_t*>(pos_smp)[64 * blk + lane] = (int16_t)(uint16_t)(uint32_t)s;
    };
    if (n_blocks > 0)
        issue(0);
    if constexpr (kOut32) {
#pragma unroll 1
        for (int pair = 0; pair < n_blocks; pair += R) {
            run_block(pair, zl[0], zh[0], zl[R - 1], zh[R - 1]);
            if (R == 2 && pair + 1 < n_blocks)
                run_block(pair + 1, zl[1], zh[1], zl[0], zh[0]);
        }
    } else {
        // One copy of the block's text for both rings: zl[0] / zh[0] is always the register whose sums finish in the block.
        // On the ring of 128 the two registers change roles behind every block (four moves per 64 samples) instead of the
        // block being written out once per role, which doubled the function's code.
#pragma unroll 1
        for (int blk = 0; blk < n_blocks; blk++) {
            run_block(blk, zl[0], zh[0], zl[R - 1], zh[R - 1]);
            if (R == 2) {
                const uint32_t tl = zl[0], th = zh[0];
                zl[0] = zl[1], zh[0] = zh[1];
                zl[1] = tl, zh[1] = th;
            }
        }
    }
    wave_sync();
}

// ring / recycling group by order: <= 48: 64 / 16, <= 60: 64 / 4, else 128 / 16
template <bool kVecShift, bool kOut32 = false>
__device__ __forceinline__ void synthesize_by_order(uint32_t order, const uint32_t* words, uint32_t n_words, uint32_t k, uint16_t* pos_smp,
    const int32_t* ws, const uint64_t* tab, bool fold, int lane, SynthOut<kOut32> out32 = SynthOut<kOut32>())
{
    if (order <= 48)
        synthesize<1, 16, kVecShift, kOut32>(words, n_words, k, pos_smp, ws, tab, fold, lane, out32);
    else if (order <= 60)
        synthesize<1, 4, kVecShift, kOut32>(words, n_words, k, pos_smp, ws, tab, fold, lane, out32);
    else
        synthesize<2, 16, kVecShift, kOut32>(words, n_words, k, pos_smp, ws, tab, fold, lane, out32);
}

// The coefficients a[d] (0 for d = 0 and beyond `order`), packed {al, ah}, ring-periodic and doubled, written
// over the wave's k[] / a[] arrays.  Returns whether every ah fits 24 bits.  (The sums accumulate
// 2^34 - sum a_d s = 2^34 + sum a_d (-s): the multiplier carries the sign, see synth_steps.)
__device__ inline bool build_synth_table(const int64_t* a, uint64_t* tab, int order, int lane)
{
    uint64_t c[2];
    bool fits = true;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int d = lane + 64 * h;
        const uint64_t nv = (uint64_t)(d >= 1 && d <= order ? a[d] : 0);
        const int32_t al = (int32_t)(uint32_t)nv;
        const int32_t ah = (int32_t)(uint32_t)((nv - (uint64_t)(int64_t)al) >> 32); // nv = ah 2^32 + al, al signed
        fits &= ah >= -(1 << 23) && ah < (1 << 23);
        c[h] = ((uint64_t)(uint32_t)ah << 32) | (uint32_t)al;
    }
    wave_sync(); // a[] has been read by every lane
    if (order <= 60) { // ring of 64
        tab[lane] = c[0];
        tab[lane + 64] = c[0];
    } else {           // ring of 128
        tab[lane] = c[0];
        tab[lane + 64] = c[1];
        tab[lane + 128] = c[0]; // (a step reads entries lane + 128 - M and lane + 64 - M, M = 0 .. 63: 1 .. 191)
    }
    wave_sync();
    return !__any(!fits);
}

} // namespace sela

#endif // SELA_SYNTH_H_
