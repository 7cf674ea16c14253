// sela_encode_tail.inc -- a block from its reflection coefficients to its slot; #included (textually, inside a function
// body) by the kernels of sela_encode.hip.
//
// Everything behind the Schur recursion, for ONE block by one wave: order, quantisation, dequantisation, step-up, residues,
// the two Rice streams, slot + BlockMeta.  Shared by k_encode_blocks (one block per wave from start to end) and
// k_encode_teams (the analysis of several blocks side by side in one wave, then this, block after block).  Textual rather
// than a function: as a forceinline function the same statements cost k_encode_blocks 11 spilled registers (168 VGPRs
// instead of 163) -- the register allocation of that kernel sits at the edge of its three-waves-per-SIMD budget.
//
// Expects in scope:  kMode, kFused (template parameters), kTrace, kAcInLds (constexpr bool: the trace finds ac[] in sm->ac),
//   unsigned char* big (the LDS plan of k_encode_blocks), uint32_t* cw_buf, SmallArrays* sm, int lane,
//   int32_t s[kPerLane] (s[t] = sample lane + 64 t), double k_lo, k_hi (reflection coefficient lane / lane + 64), double mean,
//   uint32_t flags, uint32_t block_id, BlockMeta* meta, uint32_t* slots, sela_hip_trace* trace, int force_plain_fir,
//   long long stamp[14]; uint64_t* sizes_pub, uint64_t sizes_tag, uint32_t channels, sig (the stereo candidates' sizes, see
//   "slot + meta" below; sizes_pub may be null).
// With SELA_TAIL_HAVE_Q defined by the includer, the order and the quantised coefficients are not computed here but found in
// scope (int order; int32_t q_lo, q_hi: coefficient lane / lane + 64), and k_lo / k_hi are not needed: k_encode_teams
// quantises all of a wave's blocks right behind their Schur recursion and keeps 100 bytes per block instead of 800.
// (Preprocessor rather than `if constexpr`: the token stream k_encode_blocks sees is exactly the one it had.)

    SELA_STAMP(5);
#ifndef SELA_TAIL_HAVE_Q
    // ---- order (src/lpc/residue_generator.cpp:70-78): 1 + last i with |k[i]| > 0.05 ----------------
    int order;
    {
        const unsigned long long b_lo = __ballot(fabs(k_lo) > SELA_ORDER_THRESHOLD);
        const unsigned long long b_hi = __ballot(lane < 36 && fabs(k_hi) > SELA_ORDER_THRESHOLD);
        order = b_hi ? 128 - __clzll(b_hi) : (b_lo ? 64 - __clzll(b_lo) : 1);
    }
#endif

    // ---- quantise (src/lpc/residue_generator.cpp:80-96), dequantise (linear_predictor.cpp:16-28) ----
    {
#ifndef SELA_TAIL_HAVE_Q
        const double sqrt2 = SELA_SQRT2;
        double v_lo;
        if (lane == 0)
            v_lo = floor(64 * (-1 + (sqrt2 * sqrt(k_lo + 1))));
        else if (lane == 1)
            v_lo = floor(64 * (-1 + (sqrt2 * sqrt(-k_lo + 1))));
        else
            v_lo = floor(64 * k_lo);
        const double v_hi = floor(64 * k_hi);
        const int32_t q_lo = isnan(v_lo) ? 0 : (int32_t)v_lo;
        const int32_t q_hi = isnan(v_hi) ? 0 : (int32_t)v_hi;
#endif
        if (lane < order) {
            sm->q[lane] = q_lo;
            sm->k[lane] = order <= 1 ? 0.0 : dequant(lane, q_lo, flags);
        }
        if (lane + 64 < order) {
            sm->q[lane + 64] = q_hi;
            sm->k[lane + 64] = dequant(lane + 64, q_hi, flags);
        }
        if (kTrace) {
            sela_hip_trace* tr = trace + block_id;
            if (lane == 0) {
                if (kAcInLds) // (k_encode_teams has written mean and ac[] from its own registers)
                    tr->mean = mean;
                tr->order = order;
            }
            for (int i = lane; kAcInLds && i <= kMaxOrder; i += 64)
                tr->ac[i] = sm->ac[i];
#ifndef SELA_TAIL_HAVE_Q
            tr->k[lane] = k_lo;
            if (lane < 36)
                tr->k[lane + 64] = k_hi;
#endif
        }
    }
    wave_sync();

    SELA_STAMP(6);
    // ---- step-up to the Q35 predictor (src/lpc/linear_predictor.cpp:30-61) ---------------------------
    step_up(sm->k, sm->a, order, lane, flags);
#ifndef SELA_TAIL_HAVE_Q
    __builtin_amdgcn_s_setprio(0);
#endif
    if (kTrace) {
        sela_hip_trace* tr = trace + block_id;
        for (int i = lane; i <= order; i += 64)
            tr->a[i] = sm->a[i];
        for (int i = lane; i < order; i += 64)
            tr->q[i] = sm->q[i];
    }

    SELA_STAMP(7);
    // ---- residues (src/lpc/residue_generator.cpp:98-119) -----------------------------------------------
    // r[i] = s[i] - (int32)((2^34 + sum_{j=1..order} a[j] s[i-j]) >> 35), samples before the block
    // count as absent (0).  kMode 4 (lossless, DESIGN.md 5.16) subtracts the DECODER's prediction instead,
    // -(int32)((2^34 - sum) >> 35) (src/lpc/sample_generator.cpp:25-28): the same number unless 2^34 + sum is a
    // multiple of 2^35, and one less there.  Integer arithmetic is associative, so the taps are accumulated per sample in
    // any order -- and, where no partial sum can leave 53 bits, in FP64 (the three forms below).
    //
    // Lane l owns the 32 CONSECUTIVE samples 32l .. 32l+31 (the layout the Rice packer wants) and
    // slides a 32-register window over its history: tap j needs s[32l + t - j] for t = 0..31, i.e.
    // the window of tap j-1 moved down by one, so every tap costs ONE new LDS word per lane (index
    // i stored at i + i/32: the lanes' 32-word strides fall on different banks) and 32 multiply-adds
    // (fir_taps_f64).  The tap loop is unrolled by 32 so that the window registers are addressed statically.
    int32_t* const sT = reinterpret_cast<int32_t*>(big);
    for (int m = lane; m < kPadS; m += 64)
        sT[m + (m >> 5)] = 0;
    int32_t s_max = 0, s_min = 0; // (of this lane's samples: the FP64 form of the taps below needs the block's largest magnitude)
    int32_t* const put_s = sT + (kPadS + lane) + ((kPadS + lane) >> 5); // index i = kPadS + lane + 64 t sits at i + i / 32: 66 words on per t
#pragma unroll
    for (int t = 0; t < kPerLane; t++) {
        put_s[66 * t] = s[t];
        s_max = max(s_max, s[t]);
        s_min = min(s_min, s[t]);
    }
    wave_sync();

    uint32_t ru[kPerLane]; // zig-zagged residues of samples 32 lane + t
    bool wide = false;
    uint32_t form_bits = 0;
    {
        const int32_t* mine_s = sT + (kPadS + 32 * lane) + ((kPadS + 32 * lane) >> 5); // &s[32 l], 32 words without a pad inside
        // Three forms, by the block (round 4; rounds 1-3 ran 64-bit integer taps, v_mad_i64_i32 at half rate + v_mad_i32_i24):
        //   one pass of FP64 taps   a fused multiply-add of integers is exact while no partial sum reaches 2^53, and
        //                           2^34 + sum |a[j]| x max |s| bounds them all in any order: v_fma_f64 at full rate, the
        //                           samples and coefficients as doubles.  Every block of the bench track.
        //   two passes              loud blocks with long, large predictors get past 2^53.  a = a_hi 2^20 + a_lo with
        //                           0 <= a_lo < 2^20: L = 2^34 + sum a_lo s stays below 2^44, and of L only floor(L / 2^20)
        //                           matters -- (a_hi-sum 2^20 + L) >> 35 = (a_hi-sum + floor(L / 2^20)) >> 15, the dropped
        //                           fraction cannot carry -- so the second pass starts from that and adds the a_hi taps.
        //                           Taken while order x (max |a| / 2^20 + 1) x max |s| stays below 2^42: then the whole sum
        //                           stays below 2^63 -- the reference's own int64 does not wrap, which these passes would
        //                           not follow -- and the second pass far below 2^53.  That is every predictor up to 2^39
        //                           at full-scale samples; 16-bit audio stays below 2^37.
        //   the plain loop          64-bit wrap-around arithmetic, slow, out of line: anything else (tests).
        bool modest = true; // (every |a[j]| below 2^39, so that the sum of the magnitudes fits wave_sum_40)
        uint64_t a_abs = 0, a_any = 0; // the sum / the OR of the |a[j]| of this lane's one or two taps
        for (int j = 1 + lane; j <= order; j += 64) {
            const int64_t aj = sm->a[j];
            const uint64_t mag = aj < 0 ? 0 - (uint64_t)aj : (uint64_t)aj;
            modest &= mag < ((uint64_t)1 << 39);
            a_abs += modest ? mag : 0u;
            a_any |= mag;
        }
        const uint32_t s_mag = wave_max_u32((uint32_t)max(s_max, -s_min)); // (17-bit samples: <= 65536)
        bool single = false, split = false;
        if (!kTrace && !(force_plain_fir & 1) && s_mag <= 65536u) {
            if (!__any(!modest) && !(force_plain_fir & 2))
                single = wave_sum_40(a_abs) * (uint64_t)s_mag + ((uint64_t)1 << (SELA_Q_SHIFT - 1)) < ((uint64_t)1 << 53);
            if (!single) {
                const uint64_t a_top = ((uint64_t)wave_or((uint32_t)(a_any >> 32)) << 32) | wave_or((uint32_t)a_any); // >= max |a[j]|
                split = a_top < ((uint64_t)1 << 55) && (uint64_t)order * ((a_top >> 20) + 1) * (uint64_t)s_mag < ((uint64_t)1 << 42);
            }
        }
        // (the trace build, which only tests run, always takes the plain loop; so does every block while the debug hook
        // sela_hip_debug_force_plain_fir says 1; 2: two passes wherever one would do)
        if (!kTrace) // which form, for BlockMeta::flags (kBlockFormBits; wave-uniform, two scalar selects)
            form_bits = single ? 0u : (split ? kBlockFormTwoPass : kBlockFormPlain);
        uint32_t pred_u[kPerLane];
        if (!single && !split) {
            uint32_t* const plain_pred = slots + (size_t)block_id * kSlotWords; // 2048 words of the block's own slot
            if constexpr (kMode == 4)
                fir_plain<true>(order, lane, sT, sm->a, plain_pred);
            else
                fir_plain<false>(order, lane, sT, sm->a, plain_pred);
#pragma unroll
            for (int t = 0; t < kPerLane; t++) {
                pred_u[t] = plain_pred[t * 64 + lane];
                // zig-zag would not fit 32 bits: only this form can get there -- the FP64 forms are taken with samples within
                // 2^16 and leave predictions (floor(sum / 2^35), |sum| < 2^53) within 2^18
                const int32_t rt = (int32_t)((uint32_t)mine_s[t] - pred_u[t]);
                wide |= (rt >= (1 << 30)) || (rt < -(1 << 30));
            }
        } else {
            // the coefficients as doubles: one pass -- (double)a[j] in place of a[j] (|a[j]| < 2^39: 2^20 x its high part + its
            // low 20 bits, both exact); two passes -- the low 20 bits in place, the high part (< 2^35: 2^16 x its high part +
            // its low 16 bits) over the dequantised reflection coefficients, which the step-up has consumed
            double* const c_first = reinterpret_cast<double*>(sm->a);
            double* const c_second = single ? c_first : sm->k;
            for (int j = 1 + lane; j <= order; j += 64) {
                const int64_t aj = sm->a[j];
                const int64_t top = aj >> 20;
                const double lo = (double)(uint32_t)((uint64_t)aj & 0xFFFFFu);
                const double hi = (double)(int32_t)(top >> 16) * 65536.0 + (double)(uint32_t)((uint64_t)top & 0xFFFFu);
                if (single) {
                    c_first[j] = hi * 1048576.0 + lo;
                } else {
                    c_first[j] = lo;
                    c_second[j] = hi;
                }
            }
            wave_sync();
            double win_f[kPerLane], acc_f[kPerLane];
            double half = (double)((int64_t)1 << (SELA_Q_SHIFT - 1));
            asm volatile("" : "+s"(half)); // (in a scalar register pair: one 64-bit move per sum; as a literal it took two 32-bit ones)
#pragma unroll
            for (int t = 0; t < kPerLane; t++)
                acc_f[t] = half;
            if (single) { // (its own copy of the unrolled taps: with one loop over one or two passes k_encode_blocks spilled 40 registers)
#pragma unroll
                for (int t = 0; t < kPerLane; t++)
                    win_f[t] = (double)mine_s[t];
#pragma unroll 1
                for (int j0 = 0; j0 < order; j0 += 32)
                    fir_taps_f64<0>(j0, order, fir_group_window(sT, lane, j0), fir_group_coefs(c_first, j0), win_f, acc_f);
#pragma unroll
                for (int t = 0; t < kPerLane; t++) { // floor(sum / 2^35): |.| < 2^18
                    if constexpr (kMode == 4) // the decoder's rounding, -floor(1 - sum / 2^35) = ceil(sum / 2^35) - 1: one less than the floor exactly at a tie
                        pred_u[t] = (uint32_t)((int32_t)__builtin_ceil(acc_f[t] * (1.0 / (double)((int64_t)1 << SELA_Q_SHIFT))) - 1);
                    else
                        pred_u[t] = (uint32_t)(int32_t)__builtin_floor(acc_f[t] * (1.0 / (double)((int64_t)1 << SELA_Q_SHIFT)));
                }
            } else {
                // (lossless: ceil(sum / 2^35) - 1, and ceil((H + L / 2^20) / 2^15) = ceil(ceil(H + L / 2^20) / 2^15) = ceil((H + ceil(L / 2^20)) / 2^15)
                // for the whole number H of the second pass: the same two passes with both floors turned into ceilings)
#pragma unroll 1
                for (int pass = 0; pass < 2; pass++) {
                    const double* const coef = pass ? c_second : c_first;
#pragma unroll
                    for (int t = 0; t < kPerLane; t++)
                        win_f[t] = (double)mine_s[t];
#pragma unroll 1
                    for (int j0 = 0; j0 < order; j0 += 32)
                        fir_taps_f64<0>(j0, order, fir_group_window(sT, lane, j0), fir_group_coefs(coef, j0), win_f, acc_f);
                    const double down = pass ? 1.0 / (double)((int64_t)1 << (SELA_Q_SHIFT - 20)) : 1.0 / 1048576.0;
#pragma unroll
                    for (int t = 0; t < kPerLane; t++) { // floor(L / 2^20), then floor(sum / 2^15)
                        if constexpr (kMode == 4)
                            acc_f[t] = __builtin_ceil(acc_f[t] * down);
                        else
                            acc_f[t] = __builtin_floor(acc_f[t] * down);
                    }
                }
#pragma unroll
                for (int t = 0; t < kPerLane; t++) {
                    if constexpr (kMode == 4)
                        pred_u[t] = (uint32_t)((int32_t)acc_f[t] - 1);
                    else
                        pred_u[t] = (uint32_t)(int32_t)acc_f[t];
                }
            }
        }
#pragma unroll
        for (int t = 0; t < kPerLane; t++) {
            const int32_t rt = (int32_t)((uint32_t)mine_s[t] - pred_u[t]);
            ru[t] = zigzag32(rt);
#ifdef SELA_TAIL_TRACE_RESIDUES
            if (kTrace && (SELA_TAIL_TRACE_RESIDUES)) // (the LPC stage on its own, sela_hip_lpc_encode: the trace build also leaves the residues)
                (SELA_TAIL_TRACE_RESIDUES)[(size_t)block_id * kBlock + 32 * lane + t] = rt;
#endif
        }
    }
    wave_sync(); // sT is dead

    SELA_STAMP(8);
    // ---- Rice parameters -----------------------------------------------------------------------------
    // coefficients: value i of q[] sits in lane i / 2 slot i % 2 (lane-contiguous for packing)
    uint32_t cu[2];
    cu[0] = 2 * lane < order ? zigzag32(sm->q[2 * lane]) : 0u;
    cu[1] = 2 * lane + 1 < order ? zigzag32(sm->q[2 * lane + 1]) : 0u;
    uint32_t coef_k, coef_top, coef_quotients;
    uint64_t coef_bits;
    rice_plan<2>(cu, (uint32_t)order, coef_k, coef_bits, coef_top, coef_quotients);
    const uint32_t coef_words = words_for_bits(coef_bits);

    if (__any(wide))
        flags |= SELA_HIP_FLAG_RICE_RANGE;
    uint32_t res_k, res_top, res_quotients;
    uint64_t res_bits;
    rice_plan<kPerLane>(ru, (uint32_t)kBlock, res_k, res_bits, res_top, res_quotients);
    // Is any residue codeword longer than a word?  Once for the block and the same for every lane: the longest is that of the
    // largest value, (max >> k) + 1 + k bits.
    const bool res_all_short = (wave_max_u32(res_top) >> res_k) + 1 + res_k <= 32;
    uint32_t res_words = words_for_bits(res_bits);
    if (res_words > (uint32_t)kResWordsCap || coef_words > (uint32_t)kCoefWordsCap) {
        flags |= SELA_HIP_FLAG_WORDS_CAP;
        res_words = 0;
    }

    // ---- the stereo candidates tell each other their sizes (round 4) ----------------------------------
    // Of an exactly-stereo frame's second channel and its difference signal only the smaller is stored
    // (src/frame/frame_encoder.cpp:64-72); they are two blocks in two waves, and round 3 wrote both slots (11 MB of 46 per
    // 3875-frame launch, never read).  Each publishes its size as soon as it is known -- one 64-bit word: this launch's tag |
    // words, through the L2 -- packs its streams, and then looks at the other's word: if that is this launch's and says the
    // other one wins BY THE RULE THE FRAMES ARE ASSEMBLED BY (frame_words: the difference only if strictly smaller), the slot
    // is not written.  A word that is not there yet, or is another launch's, or is read stale from another XCD's L2, means
    // "unknown": the slot is written as before.  The rule has exactly one loser, and a winner never skips.
    const bool paired = sizes_pub != nullptr && channels == 2 && sig >= 1;
    const uint32_t my_words = coef_words + res_words;
    if (paired && lane == 0)
        store_through(sizes_pub + block_id, sizes_tag | (uint64_t)my_words);

    SELA_STAMP(9);
    // ---- pack the coefficient stream (<= 100 values) ----------------------------------------------
    if (lane < kCoefWordsCap)
        cw_buf[lane] = 0;
    wave_sync();
    if (!(flags & SELA_HIP_FLAG_WORDS_CAP)) {
        const uint32_t n0 = 2 * lane < order ? (cu[0] >> coef_k) + 1 + coef_k : 0u;
        const uint32_t n1 = 2 * lane + 1 < order ? (cu[1] >> coef_k) + 1 + coef_k : 0u;
        uint32_t pos = wave_exclusive_scan(n0 + n1, lane);
        if (n0)
            pos = put_codeword(cw_buf, pos, cu[0], coef_k);
        if (n1)
            pos = put_codeword(cw_buf, pos, cu[1], coef_k);
    }

    // (the other candidate's word is asked for here and looked at behind the packing of the residues: the trip to the L2
    // hides behind 6 k cycles of work -- asked for at the slot store itself, the kernel was 1.2 % slower)
    uint64_t other = 0;
    if (paired)
        other = load_through(sizes_pub + (sig == 1 ? block_id + 1 : block_id - 1));

    SELA_STAMP(10);
    // ---- pack the residue stream ----------------------------------------------------------------------
    // Lane l already owns the 32 consecutive residues 32l .. 32l+31: scan the per-lane bit counts, then
    // every lane appends its codewords.  The sample buffer is dead: out_words overlays it.
    uint32_t* const out_words = reinterpret_cast<uint32_t*>(big); // over the dead sample buffer
    for (uint32_t w = lane; w < res_words; w += 64)
        out_words[w] = 0;
    // (the lane's bits = its quotients, which the parameter search has summed already, + 32 terminators and remainders)
    const uint32_t lane_bits = res_quotients + (uint32_t)kPerLane * (1 + res_k);
    wave_sync();
    if (res_words) {
        // fully unrolled: the residues are addressed statically and stay in registers
        uint32_t pos = wave_exclusive_scan(lane_bits, lane);
        // A codeword that fits a word (all but spikes in quiet blocks) is put together in a register -- the unary part and the
        // bit-reversed remainder -- and OR-ed into the two words it may touch, without a branch; longer ones go through an
        // out-of-line helper.
        if (res_all_short) {
            // No codeword of the block is longer than a word (decided once, above): the same words without the test, the
            // masking and the call -- 11 vector instructions a codeword.  ones <= 31 - k here.
            uint32_t k_v = res_k, rem_at = 32 - res_k; // (k in ONE vector register for all 32 v_bfe_u32, which take one scalar operand)
            asm volatile("" : "+v"(k_v));
            asm volatile("" : "+s"(rem_at));
#pragma unroll
            for (int t = 0; t < kPerLane; t++) {
                const uint32_t u = ru[t], ones = u >> res_k;
                const uint32_t rem = __builtin_amdgcn_ubfe(__brev(u), rem_at, k_v);
                const uint32_t next = ones + 1;
                or_bits_both(out_words, pos, low_ones(ones) | (rem << (next & 31))); // (ones + 1 = 32 only with k = 0, rem = 0)
                pos = pos + next + k_v;
            }
        } else {
#pragma unroll
            for (int t = 0; t < kPerLane; t++) {
                const uint32_t u = ru[t], ones = u >> res_k, len = ones + 1 + res_k;
                if (len <= 32) {
                    const uint32_t rem = __builtin_amdgcn_ubfe(__brev(u), 32 - res_k, res_k); // low k bits of u, reversed: the top k bits of brev(u) (k = 0: a field of no bits)
                    or_bits_both(out_words, pos, ((1u << ones) - 1u) | (rem << ((ones + 1) & 31))); // (ones + 1 = 32 only with k = 0, rem = 0)
                    pos += len;
                } else {
                    pos = put_long_codeword(out_words, pos, u, res_k);
                }
            }
        }
    }
    wave_sync();

    SELA_STAMP(11);
    // ---- slot + meta -------------------------------------------------------------------------------------
    uint32_t* slot = slots + (size_t)block_id * kSlotWords;
    bool loser = false;
    if (paired) {
        const uint32_t other_words = (uint32_t)other & 0xFFFu;
        // sig 1 (the channel itself) loses to a strictly smaller difference; sig 2 (the difference) loses unless strictly smaller
        loser = (other & ~(uint64_t)0xFFF) == sizes_tag && (sig == 1 ? other_words < my_words : !(my_words < other_words));
        loser = __builtin_amdgcn_readfirstlane((int)loser) != 0;
    }
    if (loser) {
        // (nothing: frame_words will pick the other candidate, whose slot is written)
    } else if (kFused) { // host pipeline: the group's last block reads them in this launch -- through the L2 (store_through)
        uint64_t* const slot2 = reinterpret_cast<uint64_t*>(slot);
        if (lane < kCoefWordsCap / 2) // (all 32 coefficient words: what lies behind coef_words is never read)
            store_through(slot2 + lane, (uint64_t)cw_buf[2 * lane] | ((uint64_t)cw_buf[2 * lane + 1] << 32));
        const uint64_t* const out2 = reinterpret_cast<const uint64_t*>(out_words);
        for (uint32_t w2 = lane; w2 < (res_words + 1) / 2; w2 += 64)
            store_through(slot2 + kCoefWordsCap / 2 + w2, out2[w2]);
    } else {
        if (lane < (int)coef_words && lane < kCoefWordsCap)
            slot[lane] = cw_buf[lane];
        for (uint32_t w = lane; w < res_words; w += 64)
            slot[kCoefWordsCap + w] = out_words[w];
    }
    const uint32_t all_flags = wave_or(flags);
    if (lane == 0) {
        BlockMeta bm;
        bm.order = (uint8_t)order;
        bm.coef_k = (uint8_t)coef_k;
        bm.res_k = (uint8_t)res_k;
        bm.flags = (uint8_t)(all_flags | form_bits);
        bm.coef_words = (uint16_t)coef_words;
        bm.res_words = (uint16_t)res_words;
        if (kFused)
            store_through(reinterpret_cast<uint64_t*>(meta + block_id), __builtin_bit_cast(uint64_t, bm));
        else
            meta[block_id] = bm;
        if (kTrace) {
            sela_hip_trace* tr = trace + block_id;
            tr->coef_k = coef_k;
            tr->coef_words = coef_words;
            tr->res_k = res_k;
            tr->res_words = res_words;
            tr->flags = all_flags;
        }
    }
