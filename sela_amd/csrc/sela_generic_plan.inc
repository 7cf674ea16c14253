// sela_generic_plan.inc -- the body of k_generic_plan<kDevice> and k_paired_plan<kDevice> (sela_generic.hip), textually shared as
// sela_encode_tail.inc is: each kernel sets `constexpr bool kPaired` and includes it, so the plain calls' kernel is compiled from
// the source it always had and the pairs (DESIGN.md 5.18) are a kernel of their own.  Uses the kernel's parameters by name.
    constexpr int kWaves = kPlanThreads / 64;
    __shared__ uint64_t wave_bytes[kWaves], wave_words[kWaves];
    __shared__ uint32_t frame_words[kPlanTile]; // words of the frames of one tile (their bytes follow: 4 + 12 channels + 4 words)
    __shared__ uint32_t frame_first_hi[kPlanTile];
    __shared__ uint32_t all_flags, all_over;
    const uint32_t t = threadIdx.x;
    const int lane = t % 64, wave = t / 64;
    [[maybe_unused]] const uint32_t n_pairs = n_sig - channels; // kPaired: channels / 2 (generic_signals())
    if (t == 0)
        all_flags = 0, all_over = 0;
    uint64_t base_b = 0, base_w = 0; // bytes / words of the tiles before this one (the same in every thread)
    uint32_t my_flags = 0, my_over = 0;
    for (uint32_t tile0 = 0; tile0 < n_frames; tile0 += kPlanTile) {
        const uint32_t tile_n = min((uint32_t)kPlanTile, n_frames - tile0);
        __syncthreads(); // (the tile before has been read)
        for (uint32_t i = t; i < tile_n; i += kPlanThreads) {
            const uint32_t f = tile0 + i;
            uint32_t words = 0;
            // (values, not pointers, are selected: a record chosen by pointer is loaded again through it -- a chain of dependent
            // loads, 32 us for 3875 frames)
            const GenericMeta* const fm = meta + (size_t)f * n_sig;
            if constexpr (kPaired) {
                uint32_t* const fc = chosen + (size_t)f * channels;
                // the pairs (2p, 2p + 1) with their difference at signal channels + p (DESIGN.md 5.18).  The three records' places
                // depend on p alone, never on a record: a step's nine loads are independent of each other and of the step before.
                for (uint32_t p = 0; p < n_pairs; p++) {
                    const GenericMeta *const m0 = fm + 2 * p, *const m1 = m0 + 1, *const m2 = fm + channels + p;
                    const uint32_t c0 = m0->coef_words, r0 = m0->res_words, f0 = m0->flags;
                    const uint32_t c1 = m1->coef_words, r1 = m1->res_words, f1 = m1->flags;
                    const uint32_t c2 = m2->coef_words, r2 = m2->res_words, f2 = m2->flags;
                    const bool diff = (uint64_t)c2 + r2 < (uint64_t)c1 + r1;
                    my_flags |= f0 | f1 | f2; // (both candidates were computed: either's trouble is the frame's, as in the stereo frame)
                    fc[2 * p] = 2 * p;
                    fc[2 * p + 1] = diff ? channels + p : 2 * p + 1;
                    const uint32_t fs = diff ? f2 : f1, ws = diff ? c2 + r2 : c1 + r1;
                    words += ((f0 & SELA_HIP_FLAG_WORDS_CAP) ? 0u : c0 + r0) + ((fs & SELA_HIP_FLAG_WORDS_CAP) ? 0u : ws);
                }
                if (channels & 1) { // an odd last channel, coded alone
                    const uint32_t c = channels - 1, fl = fm[c].flags, w = fm[c].coef_words + fm[c].res_words;
                    my_flags |= fl;
                    fc[c] = c;
                    words += (fl & SELA_HIP_FLAG_WORDS_CAP) ? 0u : w;
                }
            } else if (channels == 2) {
                const uint32_t w0 = fm[0].coef_words + fm[0].res_words, w1 = fm[1].coef_words + fm[1].res_words, w2 = fm[2].coef_words + fm[2].res_words;
                const uint32_t f0 = fm[0].flags, f1 = fm[1].flags, f2 = fm[2].flags;
                const bool diff = (uint64_t)fm[2].coef_words + fm[2].res_words < (uint64_t)fm[1].coef_words + fm[1].res_words;
                my_flags |= f0 | f1 | f2; // (both candidates were computed by the reference too: either's trouble is the frame's)
                chosen[(size_t)f * 2] = 0;
                chosen[(size_t)f * 2 + 1] = diff ? 2u : 1u;
                const uint32_t fs = diff ? f2 : f1, ws = diff ? w2 : w1;
                words = ((f0 & SELA_HIP_FLAG_WORDS_CAP) ? 0u : w0) + ((fs & SELA_HIP_FLAG_WORDS_CAP) ? 0u : ws);
            } else {
                for (uint32_t c = 0; c < channels; c++) {
                    const uint32_t fl = fm[c].flags, w = fm[c].coef_words + fm[c].res_words;
                    my_flags |= fl;
                    chosen[(size_t)f * channels + c] = c;
                    words += (fl & SELA_HIP_FLAG_WORDS_CAP) ? 0u : w; // (<= 255 x 131,070 words: fits)
                }
            }
            frame_words[i] = words;
        }
        __syncthreads();
        const uint32_t per = (tile_n + kPlanThreads - 1) / kPlanThreads;
        const uint32_t begin = min(t * per, tile_n), end = min(begin + per, tile_n);
        uint64_t my_words = 0;
        for (uint32_t i = begin; i < end; i++)
            my_words += frame_words[i];
        const uint64_t my_bytes = (uint64_t)(end - begin) * (4 + (uint64_t)channels * SELA_SUBFRAME_HEADER_BYTES) + 4 * my_words;
        auto scan64 = [&](uint64_t v) -> uint64_t { // inclusive, within the wave
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d, 64);
                const uint32_t hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d, 64);
                if (lane >= d)
                    v += ((uint64_t)hi << 32) | lo;
            }
            return v;
        };
        const uint64_t incl_b = scan64(my_bytes), incl_w = scan64(my_words);
        if (lane == 63)
            wave_bytes[wave] = incl_b, wave_words[wave] = incl_w;
        __syncthreads();
        uint64_t at_w = base_w + incl_w - my_words, tile_b = 0, tile_w = 0;
        for (int w = 0; w < kWaves; w++) {
            const uint64_t wb = wave_bytes[w], ww = wave_words[w];
            if (w < wave)
                at_w += ww;
            tile_b += wb, tile_w += ww;
        }
        // every frame's first word: an exclusive scan of the run in place (frame_words[i] <- words before frame i in the stream) ...
        for (uint32_t i = begin; i < end; i++) {
            const uint32_t w = frame_words[i];
            frame_words[i] = (uint32_t)(at_w - base_w); // (relative to the tile: 4096 frames x 255 x 131,070 words fit 2^32 only just -- kept in 64 bits below)
            frame_first_hi[i] = (uint32_t)((at_w - base_w) >> 32);
            at_w += w;
        }
        __syncthreads();
        // ... and then frame by frame again as in the first pass -- thread f mod 1024, independent loads (the third version: the
        // run's owner walked its frames' subframes through `chosen`, a chain of dependent loads: 38 us at 3875 frames)
        for (uint32_t i = t; i < tile_n; i += kPlanThreads) {
            const uint32_t f = tile0 + i;
            const uint64_t first = base_w + (((uint64_t)frame_first_hi[i] << 32) | frame_words[i]);
            uint64_t w_at = first;
            const GenericMeta* const fm = meta + (size_t)f * n_sig;
            if constexpr (kPaired) {
                uint64_t* const fb = word_base + (size_t)f * channels;
                // (the decision is taken again from the three records, not read back through `chosen`: values, independent loads)
                for (uint32_t p = 0; p < n_pairs; p++) {
                    const GenericMeta *const m0 = fm + 2 * p, *const m1 = m0 + 1, *const m2 = fm + channels + p;
                    const uint32_t c0 = m0->coef_words, r0 = m0->res_words, f0 = m0->flags;
                    const uint32_t c1 = m1->coef_words, r1 = m1->res_words, f1 = m1->flags;
                    const uint32_t c2 = m2->coef_words, r2 = m2->res_words, f2 = m2->flags;
                    const bool diff = (uint64_t)c2 + r2 < (uint64_t)c1 + r1;
                    const uint32_t fs = diff ? f2 : f1, ws = diff ? c2 + r2 : c1 + r1;
                    fb[2 * p] = w_at;
                    w_at += (f0 & SELA_HIP_FLAG_WORDS_CAP) ? 0u : c0 + r0;
                    fb[2 * p + 1] = w_at;
                    w_at += (fs & SELA_HIP_FLAG_WORDS_CAP) ? 0u : ws;
                }
                if (channels & 1)
                    fb[channels - 1] = w_at;
            } else if (channels == 2) {
                const uint32_t w0 = fm[0].coef_words + fm[0].res_words, f0 = fm[0].flags;
                word_base[(size_t)f * 2] = w_at;
                word_base[(size_t)f * 2 + 1] = w_at + ((f0 & SELA_HIP_FLAG_WORDS_CAP) ? 0u : w0);
            } else {
                for (uint32_t c = 0; c < channels; c++) {
                    const uint32_t fl = fm[c].flags, w = fm[c].coef_words + fm[c].res_words;
                    word_base[(size_t)f * channels + c] = w_at;
                    w_at += (fl & SELA_HIP_FLAG_WORDS_CAP) ? 0u : w;
                }
            }
            // bytes before frame f = (frames before it) x (4 + 12 channels) + 4 x (words before it)
            frame_offsets[f] = base_bytes + (uint64_t)f * (4 + (uint64_t)channels * SELA_SUBFRAME_HEADER_BYTES) + 4 * first;
            if constexpr (kDevice) { // (the frame's end: the next frame's first word, from the scan)
                const uint64_t next = i + 1 < tile_n ? base_w + (((uint64_t)frame_first_hi[i + 1] << 32) | frame_words[i + 1]) : base_w + tile_w;
                my_over += (uint64_t)(f + 1) * (4 + (uint64_t)channels * SELA_SUBFRAME_HEADER_BYTES) + 4 * next > frames_cap;
            }
        }
        base_b += tile_b, base_w += tile_w;
    }
    if (my_flags)
        atomicOr(&all_flags, my_flags);
    if (kDevice && my_over)
        atomicAdd(&all_over, my_over);
    __syncthreads();
    if (t == 0) {
        frame_offsets[n_frames] = base_bytes + base_b;
        word_base[(size_t)n_frames * channels] = base_w;
        *total_words_out = base_w;
        if constexpr (kDevice) {
            status[0] = all_flags, status[1] = all_over, status[2] = 0, status[3] = 0;
        } else {
            atomicOr(&status[0], all_flags);
        }
    }
