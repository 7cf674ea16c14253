// sela_decode_core.inc -- the decoder's device code, once, for every kernel that decodes a subframe.  Included inside namespace
// sela by sela_decode.hip (k_decode_frames, k_decode_frames_wide, the stage kernels), sela_verify.hip (k_verify_frames) and
// sela_decode32.hip (k_decode_subframes32, k_lpc_decode_any); the algorithms are described at the top of sela_decode.hip.
//
//   the per-wave LDS records, the segment-parallel Rice parser, the serial parser, the header walk
//                                                                    -- every kernel above
//   (the synthesis, its table, the Rice value and the stream's buffer resource: sela_synth.h, included in front of this file)
//   predictor_table: dequantise, step-up, synthesis table            -- the three frame kernels and k_decode_subframes32
//   decode_subframe: one 2048-sample subframe, bytes -> int16 in LDS -- k_decode_frames, k_decode_frames_wide, k_verify_frames
//   the sub_info word, decode_lds_bytes_for, frame_prologue          -- k_decode_frames, k_verify_frames (the word: the wide kernel too)
//   the second pass: stereo_pass / stereo_words, channel_value16, layout_flags, parent_refused
//                                                                    -- k_decode_frames stores what they give, k_verify_frames compares it
//
// Each translation unit compiles its own copy (the kernels live on their register budgets -- tests/test_isa_*.py -- and the
// synthesis is a real call, see synthesize); profiles/decode_subframe/README.md has what the kernels cost.

constexpr int kDecMaxWaves = 8;     // waves per workgroup; frames with more channels take k_decode_frames_wide
constexpr int kDecMaxChannels = 255; // what the 8-bit channel field of the .sela header can say (src/file/sela_file.cpp:40)
constexpr int kCoefLanes = 4;       // lanes of a wave that parse the coefficient stream
constexpr int kResLanes = kWave - kCoefLanes;
// Aligned words of one subframe the segment-parallel parser takes: coefficient words + 2 + residue words
// (start bitmap: one bit per stream bit; positions must fit 16 bits).
constexpr int kStreamCap = 1072;
constexpr int kStreamMargin = 4;    // a window may run this many words past the end (they read as zero)
constexpr uint32_t kEndOfStream = 0xFFFFFFFFu;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// ---- per-wave LDS scratch --------------------------------------------------------------------------------
struct SynthTables {
    union {
        int64_t a[104];     // Q35 predictor; in front of it the dequantised reflection coefficients, which the step-up's stages read back one by one (step_up_from_q)
        uint64_t tab[192];  // synthesis coefficient table (build_synth_table), replaces a[]: entries 1 .. 191 are read
    };
};
struct DecWaveScratch {
    SynthTables t;
    // (the parsed coefficient values q[0 .. order) live inside t, see coef_values(): between the parse, whose scratch lies
    // in front of them, and the dequantisation, which reads them into registers before a[] is written)
};
constexpr int kCoefValuesAt = 896; // byte offset in SynthTables: behind the parse's positions (0..256), chain flags (512..577) and entries (640..896)
static_assert(kCoefValuesAt + 104 * 4 <= (int)sizeof(SynthTables) && kCoefValuesAt >= 104 * 8, "the coefficient values lie behind a[] inside the table's space");
__device__ __forceinline__ int32_t* coef_values(DecWaveScratch* s)
{
    return reinterpret_cast<int32_t*>(reinterpret_cast<unsigned char*>(&s->t) + kCoefValuesAt);
}
// per subframe POSITION (not per wave: the combine pass reads every channel)
union DecSubframeLds {
    uint32_t marks[kStreamCap + kStreamMargin]; // start bitmap (parse)
    uint16_t pos[kBlock];                       // bit position of every residue codeword (after the parse)
    int16_t smp[kBlock];                        // finished samples, written over the positions block by block
};
static_assert(sizeof(DecSubframeLds) == (kStreamCap + kStreamMargin) * 4 && sizeof(DecSubframeLds) % 16 == 0, "LDS plan");
static_assert(32 * (kStreamCap + kStreamMargin) <= 65536, "positions are 16-bit");

// Four codewords at bit position p, provided they are all short: off[j] = offset of codeword j's start,
// off[4] = offset behind the fourth.  simple = every run length < 31 and every codeword <= 31 bits (the
// funnel shifts below take their amounts mod 32, and the 160-bit window then always covers the next start).
__device__ __forceinline__ void analyse4(__amdgpu_buffer_rsrc_t rs, uint32_t p, uint32_t k, uint32_t (&off)[5], bool& simple)
{
    const uint32_t b = 4 * (p >> 5), sh = p & 31;
    const u32x4 w = __builtin_amdgcn_raw_buffer_load_b128(rs, b, 0, 0);
    const uint32_t w4 = __builtin_amdgcn_raw_buffer_load_b32(rs, b + 16, 0, 0);
    uint32_t n0 = __builtin_amdgcn_alignbit(w.y, w.x, sh), n1 = __builtin_amdgcn_alignbit(w.z, w.y, sh);
    uint32_t n2 = __builtin_amdgcn_alignbit(w.w, w.z, sh), n3 = __builtin_amdgcn_alignbit(w4, w.w, sh);
    uint32_t used = 0;
    simple = true;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t t = (uint32_t)__builtin_ctz(~n0 | 0x80000000u); // <= 31
        const uint32_t len = t + 1 + k;
        simple = simple && len <= 31;
        off[j] = used;
        used += len;
        if (j < 3) { // (a codeword that is not simple garbles the rest of a group that is then not used)
            n0 = __builtin_amdgcn_alignbit(n1, n0, len);
            n1 = __builtin_amdgcn_alignbit(n2, n1, len);
            if (j < 2)
                n2 = __builtin_amdgcn_alignbit(n3, n2, len);
            if (j < 1)
                n3 >>= len & 31;
        }
    }
    off[4] = used;
}

// One step of the careful walk: over (part of) one codeword at p.  A run of 32 ones and more is taken 32
// bits at a time (in_run).
__device__ __forceinline__ void single_step(__amdgpu_buffer_rsrc_t rs, uint32_t p, uint32_t k, uint32_t& adv, bool& full)
{
    const uint32_t b = 4 * (p >> 5), sh = p & 31;
    const uint32_t x = __builtin_amdgcn_alignbit(__builtin_amdgcn_raw_buffer_load_b32(rs, b + 4, 0, 0), __builtin_amdgcn_raw_buffer_load_b32(rs, b, 0, 0), sh);
    full = x == 0xFFFFFFFFu;
    adv = full ? 32u : (uint32_t)__builtin_ctz(~x | 0x80000000u) + 1 + k;
}

// ---- segment-parallel parse of one subframe (fast mode) ------------------------------------------------
// Bit space: stream bit t of the subframe's aligned words = bit t % 32 of word t / 32.  Coefficient stream =
// bits [24, 24 + 32 cw), residue stream = bits [32 (cw + 2), 32 (cw + 2 + rw)).  marks[] and pos_out[] are the
// same LDS bytes (the bitmap is dead before the first position is stored).  Outputs: pos_out[0 .. 2048) =
// start of every residue codeword, q[0 .. order) = the coefficients (decoded here: there are few);
// returns SELA_HIP_FLAG_RICE_OVERRUN or 0.  cpos: 128 uint16 of scratch.
struct ParseProfile {
    long long t[4];
};

// The value of the codeword at bit position p (runs of 32 ones and more are followed word by word).
__device__ __forceinline__ int32_t decode_at(__amdgpu_buffer_rsrc_t rs, uint32_t p, uint32_t k, uint32_t kmask, bool valid)
{
    uint32_t x0, x1, ones = 0;
    window64(rs, p, x0, x1);
    while (__any(valid && x0 == 0xFFFFFFFFu)) {
        const bool more = valid && x0 == 0xFFFFFFFFu;
        ones += more ? 32u : 0u;
        p += more ? 32u : 0u;
        window64(rs, p, x0, x1);
    }
    const uint32_t t = (uint32_t)__builtin_ctz(~x0 | 0x80000000u);
    const uint32_t field = (uint32_t)(((((uint64_t)x1) << 32) | x0) >> (t + 1)) & kmask;
    return rice_value(ones + t, field, k);
}

template <bool kProf>
__device__ __forceinline__ uint32_t parse_subframe(const StreamWords& sw, uint32_t* marks, uint16_t* pos_out, uint16_t* cpos, int32_t* q,
    uint32_t cw, uint32_t rw, uint32_t ck, uint32_t rk, uint32_t order, int lane, ParseProfile& prof,
    const uint32_t n_values = (uint32_t)kBlock /* residue codewords wanted, <= kBlock (the frame kernels: kBlock, a constant after inlining) */)
{
    const __amdgpu_buffer_rsrc_t rs = stream_rsrc(sw);
    // ---- zones ---------------------------------------------------------------------------------------------
    const bool coef_lane = lane < kCoefLanes;
    const uint32_t zc = max(1u, (cw + 1 + kCoefLanes - 1) / kCoefLanes); // words per coefficient zone
    const uint32_t zr = max(1u, (rw + kResLanes - 1) / kResLanes);       // words per residue zone
    const uint32_t rs_word = cw + 2;
    const uint32_t last_mark_word = cw + 2 + rw + kStreamMargin - 1;
    uint32_t first_word, end_word, stream_end, k, need;
    if (coef_lane) {
        first_word = min((uint32_t)lane * zc, cw + 1);
        end_word = min((uint32_t)(lane + 1) * zc, cw + 1);
        stream_end = 24 + 32 * cw;
        k = ck;
        need = order;
    } else {
        const uint32_t r = (uint32_t)(lane - kCoefLanes);
        first_word = rs_word + min(r * zr, rw);
        end_word = rs_word + min((r + 1) * zr, rw);
        stream_end = 32 * (rs_word + rw);
        k = rk;
        need = n_values;
    }
    const uint32_t entry = lane == 0 ? 24u : 32 * first_word;
    const uint32_t zone_end = min(32 * end_word, stream_end);

    // ---- phase A: own zone, marking every codeword start ---------------------------------------------------
    // (predicated rather than branched: lanes that are through OR a zero into the first word of the bitmap)
    uint32_t pos = entry;
    bool in_run = false; // inside a unary run longer than the window
    while (__any(pos < zone_end)) {
        const bool act = pos < zone_end;
        uint32_t off[5];
        bool simple;
        analyse4(rs, pos, k, off, simple);
        if (!__any(act && (in_run || !simple))) { // four codewords per round trip
            uint32_t adv = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t p = pos + off[j];
                const bool a = act && p < zone_end;
                atomicOr(&marks[a ? p >> 5 : 0u], a ? 1u << (p & 31) : 0u); // (LDS ds_or_b32; a zone's words are marked by its lane alone)
                adv = a ? off[j + 1] : adv;
            }
            pos += adv;
        } else { // one (part of a) codeword at a time
            uint32_t adv;
            bool full;
            single_step(rs, pos, k, adv, full);
            const bool start = act && !in_run;
            atomicOr(&marks[start ? pos >> 5 : 0u], start ? 1u << (pos & 31) : 0u);
            pos += act ? adv : 0u;
            in_run = act ? full : in_run;
        }
    }
    wave_sync();
    if (kProf)
        prof.t[0] = clock64();

    // ---- phase B: on through the following zones until standing on a later lane's start -----------------------
    uint32_t n_cont = 0, merged = 0;
    bool walking = true;
    while (__any(walking)) {
        uint32_t off[5];
        bool simple;
        analyse4(rs, pos, k, off, simple);
        if (!__any(walking && (in_run || !simple))) {
            uint32_t mk[4];
#pragma unroll
            for (int j = 0; j < 4; j++)
                mk[j] = marks[min((pos + off[j]) >> 5, last_mark_word)];
            uint32_t adv = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t p = pos + off[j];
                const bool ended = walking && p >= stream_end;
                const bool met = walking && !ended && ((mk[j] >> (p & 31)) & 1u);
                merged = ended ? kEndOfStream : (met ? p : merged);
                walking = walking && !ended && !met;
                n_cont += walking ? 1u : 0u;
                adv = walking ? off[j + 1] : adv;
            }
            pos += adv;
        } else {
            uint32_t adv;
            bool full;
            single_step(rs, pos, k, adv, full);
            const uint32_t mk = marks[min(pos >> 5, last_mark_word)];
            const bool at_start = walking && !in_run;
            const bool ended = at_start && pos >= stream_end;
            const bool met = at_start && !ended && ((mk >> (pos & 31)) & 1u);
            merged = ended ? kEndOfStream : (met ? pos : merged);
            walking = walking && !ended && !met;
            n_cont += (at_start && walking) ? 1u : 0u;
            pos += walking ? adv : 0u;
            in_run = walking ? full : in_run;
        }
    }
    if (kProf)
        prof.t[1] = clock64();

    // ---- resolve: the chains of lanes the true trajectories run through -----------------------------------------
    uint32_t succ = 64; // lane whose zone holds `merged`
    if (merged != kEndOfStream) {
        const uint32_t wm = merged >> 5;
        succ = wm < rs_word ? min(wm / zc, (uint32_t)kCoefLanes - 1) : (uint32_t)kCoefLanes + (wm - rs_word) / zr;
    }
    // The lanes a chain runs through = the orbit of its first lane under succ.  Pointer doubling: after round r
    // the set holds every lane within 2^(r+1) hops (six rounds cover the wave); a lane joins when a member's
    // pointer lands on it (a byte flag in LDS), and the pointers are squared with ds_bpermute.  (The walk
    // hop by hop on the scalar unit, 64 x readlane -> compare -> branch, cost 19 k cycles of latency.)
    if (coef_lane ? succ >= (uint32_t)kCoefLanes : false)
        succ = 64;
    succ = succ > (uint32_t)lane ? succ : 64u; // (always true of a zone further on; keeps the orbit finite whatever the stream holds)
    uint8_t* const flag = reinterpret_cast<uint8_t*>(cpos) + 512;   // 65 bytes of the scratch (the tables' space, dead until the parse is over)
    uint32_t* const entry_of = reinterpret_cast<uint32_t*>(cpos) + 160; // 64 words behind them
    flag[lane] = 0;
    if (lane == 0)
        flag[64] = 0;
    bool on_chain = lane == 0 || lane == kCoefLanes;
    uint32_t jump = succ;
    wave_sync();
#pragma unroll
    for (int r = 0; r < 6; r++) {
        if (on_chain && jump < 64)
            flag[jump] = 1;
        wave_sync();
        on_chain = on_chain || flag[lane] != 0;
        const uint32_t next = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(4 * min(jump, 63u)), (int)jump);
        jump = jump < 64 ? next : 64u;
        wave_sync();
    }
    // a chain lane's true entry = where its predecessor merged
    if (on_chain && succ < 64)
        entry_of[succ] = merged;
    wave_sync();
    uint32_t e_true = kEndOfStream; // this lane's true entry; kEndOfStream = not on a chain
    if (on_chain)
        e_true = lane == 0 ? 24u : (lane == kCoefLanes ? 32 * rs_word : entry_of[lane]);
    wave_sync();
    // codewords of this lane's path from its true entry: the marked starts at or behind the entry + phase B's
    uint32_t count = 0;
    {
        const uint32_t we = e_true >> 5;
        const uint32_t zmax = max(zc, zr);
        for (uint32_t j = 0; j < zmax; j++) {
            const bool valid = on_chain && we + j < end_word;
            if (!__any(valid))
                break;
            uint32_t word = valid ? marks[we + j] : 0u;
            if (j == 0)
                word &= 0xFFFFFFFFu << (e_true & 31);
            count += (uint32_t)__builtin_popcount(word);
        }
        count = on_chain ? count + n_cont : 0u;
    }
    uint32_t idx = wave_exclusive_scan(count, lane);
    const uint32_t coef_total = (uint32_t)__builtin_amdgcn_readlane((int)idx, kCoefLanes);
    const uint32_t all_total = (uint32_t)__builtin_amdgcn_readlane((int)(idx + count), kWave - 1);
    const uint32_t res_total = all_total - coef_total;
    if (!coef_lane)
        idx -= coef_total;
    uint32_t remaining = idx < need ? min(count, need - idx) : 0u;
    wave_sync(); // every lane has read the bitmap: the positions may overwrite it
    if (kProf)
        prof.t[2] = clock64();

    // ---- pass 2: list the starts, every chain lane from its true entry -----------------------------------------------
    uint16_t* out = (coef_lane ? cpos : pos_out) + idx;
    pos = on_chain ? e_true : 0u;
    in_run = false;
    bool overrun = false;
    while (__any(remaining != 0)) {
        const bool act = remaining != 0;
        uint32_t off[5];
        bool simple;
        analyse4(rs, pos, k, off, simple);
        if (!__any(act && (in_run || !simple))) {
            uint32_t adv = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const bool a = (uint32_t)j < remaining;
                if (a)
                    out[j] = (uint16_t)(pos + off[j]);
                adv = a ? off[j + 1] : adv;
            }
            const uint32_t take = min(remaining, 4u);
            out += take;
            remaining -= take;
            pos += adv;
            overrun |= act && pos > stream_end;
        } else {
            uint32_t adv;
            bool full;
            single_step(rs, pos, k, adv, full);
            const bool start = act && !in_run;
            if (start)
                *out = (uint16_t)pos;
            out += start ? 1 : 0;
            pos += act ? adv : 0u;
            in_run = act ? full : in_run;
            remaining -= (act && !full) ? 1u : 0u;
            overrun |= act && !full && pos > stream_end;
        }
    }
    // a stream that ends before all its values were read: the missing codewords read as zero bits, i.e. they
    // "start" behind the stream's end, where the resource returns zeros
    // (... and so do the lanes of the last block of 64 beyond a subframe that is shorter than kBlock)
    {
        const uint32_t listed = min(res_total, n_values), upto = min((n_values + (uint32_t)kWave - 1) & ~((uint32_t)kWave - 1), (uint32_t)kBlock);
        if (listed < upto)
            for (uint32_t i = listed + lane; i < upto; i += kWave)
                pos_out[i] = (uint16_t)(32 * (rs_word + rw + 1));
    }
    wave_sync();
    // the coefficients themselves (<= 100 values: two rounds)
    {
        const uint32_t ckmask = ck ? (0xFFFFFFFFu >> (32 - ck)) : 0u;
        for (uint32_t i0 = 0; i0 < order; i0 += kWave) {
            const uint32_t i = i0 + (uint32_t)lane;
            const bool valid = i < min(order, coef_total);
            const int32_t v = decode_at(rs, valid ? cpos[i] : 0u, ck, ckmask, valid);
            if (i < order)
                q[i] = valid ? v : 0;
        }
    }
    const bool bad = __any(overrun) || coef_total < order || res_total < n_values;
    wave_sync();
    if (kProf)
        prof.t[3] = clock64();
    return bad ? (uint32_t)SELA_HIP_FLAG_RICE_OVERRUN : 0u;
}

// ---- generic mode: one stream, serially, straight from global memory ---------------------------------------
// src/rice/rice_decoder.cpp:21-52 as written: count the ones up to the first zero, read k bits MSB first.
// Every lane runs the same (wave-uniform) parse; lane 0 stores.  `words` = the frame's aligned words,
// n_frame_words of them; reads beyond the stream's own words (or the frame) are zero.
__device__ inline uint32_t parse_stream_serial(const uint32_t* __restrict__ words, uint32_t first_bit, uint32_t stream_end,
    uint32_t n_frame_words, uint32_t k, uint32_t count, int32_t* out, int lane)
{
    auto word_at = [&](uint32_t w) -> uint32_t { return (w < n_frame_words && 32 * w < stream_end) ? words[w] : 0u; };
    auto bit_at = [&](uint32_t p) -> uint32_t { return p < stream_end ? (word_at(p >> 5) >> (p & 31)) & 1u : 0u; };
    uint32_t pos = first_bit;
#pragma unroll 1
    for (uint32_t i = 0; i < count; i++) {
        uint32_t ones = 0;
        for (;;) { // up to a whole word of ones at a time
            const uint32_t sh = pos & 31, have = 32 - sh;
            const uint32_t lo = word_at(pos >> 5) >> sh;
            const uint32_t t = (uint32_t)__builtin_ctzll(~(uint64_t)lo | ((uint64_t)1 << have)); // <= have
            ones += t;
            pos += t;
            if (t < have || pos >= stream_end)
                break;
        }
        pos++; // the terminator
        uint32_t rem = 0;
        for (uint32_t b = 0; b < k; b++)
            rem = (rem << 1) | bit_at(pos + b);
        pos += k;
        const uint32_t u = (ones << k) | rem;
        if (lane == 0)
            out[i] = (int32_t)((u >> 1) ^ (0u - (u & 1u)));
    }
    wave_sync();
    return pos > stream_end ? (uint32_t)SELA_HIP_FLAG_RICE_OVERRUN : 0u;
}

// ---- subframe header walk (the layout and its bounds: sela_format.h) ---------------------------------------------------------
// The decoders take frames of whole words at word-aligned places and read each header with two pairs of 32-bit loads
// (sela_subframe_read_words).  The walk stops on the header asked for; what a decoder accepts there is its own test
// (block_header_ok for the 2048-sample kernels, k_decode_subframes32 its own).
struct SubHeader : SelaSubframeHeader {
    bool ok;    // the walk got here: this header and the subframe's words lie inside the frame
    uint32_t p; // byte offset of the subframe in the frame
};
struct HeaderCursor {
    uint32_t index; // subframe the cursor stands in front of
    uint64_t p;     // its byte offset in the frame
    bool ok;        // (a frame is walked front to back: behind a broken header there is nothing to find)
};

__device__ inline HeaderCursor frame_cursor(const uint8_t* fb, uint64_t fbytes)
{
    HeaderCursor cur;
    cur.index = 0;
    cur.p = 4;
    cur.ok = fbytes >= 4 && fbytes < 0x7FFFFFFFull && (fbytes & 3) == 0 && reinterpret_cast<const uint32_t*>(fb)[0] == SELA_SYNC_WORD;
    return cur;
}

// On from the cursor over the headers up to and including subframe c; the cursor is left behind it.
__device__ inline SubHeader walk_to(const uint8_t* fb, uint64_t fbytes, HeaderCursor& cur, uint32_t c)
{
    SubHeader h;
    h.channel = h.type = h.parent = h.ck = h.cw = h.order = h.rk = h.rw = h.n = 0;
    h.ok = cur.ok;
    h.p = (uint32_t)cur.p;
    while (h.ok && cur.index <= c) {
        h.p = (uint32_t)cur.p;
        cur.p = sela_subframe_read_words(fb, fbytes, cur.p, &h);
        h.ok = cur.p != 0;
        cur.index++;
    }
    cur.ok = h.ok;
    return h;
}

__device__ inline SubHeader walk_headers(const uint8_t* fb, uint64_t fbytes, uint32_t c)
{
    HeaderCursor cur = frame_cursor(fb, fbytes);
    return walk_to(fb, fbytes, cur, c);
}

// What k_decode_frames and k_decode_frames_wide decode: a 2048-sample subframe of a channel the frame has, independent or
// difference-coded against one.
__device__ inline bool block_header_ok(const SubHeader& h, uint32_t channels)
{
    return h.ok && sela_subframe_decodable(&h) && h.n == (uint32_t)kBlock && h.channel < channels && h.type <= 1 && (h.type == 0 || h.parent < channels);
}

// ---- quantised reflection coefficients -> synthesis table ------------------------------------------------------------------
// dequantise (src/lpc/linear_predictor.cpp:16-28), step-up into t->a, the table over it.  Returns build_synth_table's answer
// (every high word fits 24 bits: the synthesis may start in the folded form).
__device__ __forceinline__ bool predictor_table(uint32_t order, int32_t q_lo, int32_t q_hi, SynthTables* t, int lane, uint32_t& flags)
{
    step_up_from_q(order, q_lo, q_hi, t->a, lane, flags);
    return build_synth_table(t->a, t->tab, (int)order, lane);
}

// ---- one 2048-sample subframe, from the frame's bytes to int16 samples in its record ----------------------------------------
// The body of a wave of k_decode_frames, k_decode_frames_wide and k_verify_frames.  fast: the segment-parallel parse into the
// record (the caller has checked hd.cw + 2 + hd.rw <= kStreamCap); otherwise the serial parse, the residues parked in block
// ws_block of the workspace (int32[kBlock] each, 256-byte aligned).  flags is a reference on purpose: a local that is returned
// stays alive across the synthesis in a register of its own, which k_verify_frames does not have (two spilled VGPRs).
// kProf: stamps 2 .. 8 of k_decode_frames' phase counts.
template <bool kProf>
__device__ __forceinline__ void decode_subframe(const uint8_t* fb, uint64_t fbytes, const SubHeader& hd, bool fast, DecSubframeLds* sl, DecWaveScratch* scratch,
    int32_t* ws_residues, size_t ws_block, bool vec_shift, uint32_t synth_priorities /* as k_decode_frames takes them; 0: none */, int lane, uint32_t& flags,
    long long* stamp /* kProf only */)
{
    const uint32_t nw = hd.cw + 2 + hd.rw;
    const uint32_t* const gw = reinterpret_cast<const uint32_t*>(fb + hd.p + 4); // the subframe's aligned words
    const int32_t* ws_c = nullptr;
    ParseProfile pp;
    if (fast) {
        for (uint32_t w = lane; w < nw + kStreamMargin; w += kWave) // the start bitmap
            sl->marks[w] = 0;
        wave_sync();
        if (kProf)
            stamp[2] = clock64();
        const StreamWords sw = { gw, nw };
        flags |= parse_subframe<kProf>(sw, sl->marks, sl->pos, reinterpret_cast<uint16_t*>(&scratch->t), coef_values(scratch), hd.cw, hd.rw, hd.ck, hd.rk,
            hd.order, lane, pp);
    } else {
        if (kProf)
            stamp[2] = clock64();
        int32_t* const wres = ws_residues + ws_block * kBlock;
        const uint32_t n_frame_words = (uint32_t)((fbytes - hd.p - 4) / 4);
        flags |= parse_stream_serial(gw, 24, 24 + 32 * hd.cw, n_frame_words, hd.ck, hd.order, coef_values(scratch), lane);
        flags |= parse_stream_serial(gw, 32 * (hd.cw + 2), 32 * (hd.cw + 2 + hd.rw), n_frame_words, hd.rk, (uint32_t)kBlock, wres, lane);
        // lane 0's stores to the workspace are read back by every lane of this wave: they have left the CU, and nothing older is
        // served from its vector cache -- every block of the workspace is 8 KB at a 256-byte boundary, written before it is first
        // read (not __threadfence(): its release half writes back the whole L2)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        ws_c = wres;
        pp.t[0] = pp.t[1] = pp.t[2] = pp.t[3] = kProf ? clock64() : 0;
    }
    if (kProf)
        stamp[3] = pp.t[0], stamp[4] = pp.t[1], stamp[5] = pp.t[2], stamp[6] = pp.t[3];

    const uint32_t order = hd.order;
    const int32_t q_lo = (uint32_t)lane < order ? coef_values(scratch)[lane] : 0, q_hi = (uint32_t)lane + 64 < order ? coef_values(scratch)[lane + 64] : 0;
    wave_sync();
    const bool fits24 = predictor_table(order, q_lo, q_hi, &scratch->t, lane, flags);
    if (kProf)
        stamp[7] = clock64();
    if (synth_priorities)
        set_wave_priority((int)((synth_priorities >> (order <= 48 ? 0 : (order <= 60 ? 8 : 16))) & 0xFF));
    if (vec_shift)
        synthesize_by_order<true>(order, gw, nw, hd.rk, sl->pos, ws_c, scratch->t.tab, fits24, lane);
    else
        synthesize_by_order<false>(order, gw, nw, hd.rk, sl->pos, ws_c, scratch->t.tab, fits24, lane);
    if (synth_priorities)
        __builtin_amdgcn_s_setprio(0);
    if (kProf)
        stamp[8] = clock64();
}

// ---- what a frame's subframes delivered: one word per CHANNEL ---------------------------------------------------------------
constexpr uint32_t kNoSubframe = 0xFFFFFFFFu; // "no subframe delivered this channel"
__device__ __forceinline__ uint32_t sub_info_word(uint32_t type, uint32_t parent, uint32_t position) { return type | (parent << 8) | (position << 16); }
__device__ __forceinline__ uint32_t sub_info_type(uint32_t info) { return info & 0xFF; }
__device__ __forceinline__ uint32_t sub_info_parent(uint32_t info) { return (info >> 8) & 0xFF; }
__device__ __forceinline__ uint32_t sub_info_position(uint32_t info) { return info >> 16; }

// LDS plan of k_decode_frames and k_verify_frames (dynamic): one DecSubframeLds per subframe POSITION | one DecWaveScratch per
// wave | sub_info[channels] | too_big[n_waves].
__host__ __device__ inline size_t decode_lds_bytes_for(uint32_t channels, int n_waves)
{
    return (size_t)channels * sizeof(DecSubframeLds) + (size_t)n_waves * sizeof(DecWaveScratch) + (size_t)channels * 4 + (size_t)n_waves * 4;
}
struct DecFrameLds {
    DecSubframeLds* sub;       // [channels]
    DecWaveScratch* scratch0;  // [n_waves]
    uint32_t* sub_info;        // [channels]
    uint32_t* too_big;         // [n_waves]: this wave's subframe does not fit the fast plan
};
__device__ __forceinline__ DecFrameLds carve_frame_lds(unsigned char* dyn, uint32_t channels, int n_waves)
{
    DecFrameLds l;
    l.sub = reinterpret_cast<DecSubframeLds*>(dyn);
    l.scratch0 = reinterpret_cast<DecWaveScratch*>(dyn + (size_t)channels * sizeof(DecSubframeLds));
    l.sub_info = reinterpret_cast<uint32_t*>(dyn + (size_t)channels * sizeof(DecSubframeLds) + (size_t)n_waves * sizeof(DecWaveScratch));
    l.too_big = l.sub_info + channels;
    return l;
}

// The start of a frame's workgroup: nothing delivered yet, this wave's first header (hd, ok), and the vote on the mode -- every
// subframe of the frame must fit the fast plan.  Returns the vote's result; ends in a workgroup barrier.
__device__ __forceinline__ bool frame_prologue(const DecFrameLds& l, const uint8_t* fb, uint64_t fbytes, uint32_t channels, int n_waves, int wave, int lane,
    SubHeader& hd, bool& ok)
{
    for (uint32_t c = threadIdx.x; c < channels; c += blockDim.x)
        l.sub_info[c] = kNoSubframe;
    const bool fast_plan = channels <= (uint32_t)kDecMaxWaves;
    hd = walk_headers(fb, fbytes, (uint32_t)wave < channels ? (uint32_t)wave : 0u);
    ok = block_header_ok(hd, channels);
    if (lane == 0)
        l.too_big[wave] = (fast_plan && (!ok || (hd.cw + 2 + hd.rw <= (uint32_t)kStreamCap && hd.order <= 2 * (uint32_t)kWave))) ? 0u : 1u;
    __syncthreads();
    bool fast = fast_plan;
    for (int w = 0; w < n_waves; w++)
        fast = fast && l.too_big[w] == 0;
    return fast;
}

// ---- second pass of frame::FrameDecoder + interleave to int16 (src/frame/frame_decoder.cpp:40-69) ---------------------------
// Dependent channels become parent - difference (parents are independent subframes); a channel that no valid subframe
// delivered decodes to silence.  All of it mod 2^16: the reference truncates to int16 when it writes the WAV
// (src/file/wav_file.cpp:248-251).  k_decode_frames stores what these give, k_verify_frames compares it.

// A difference-coded subframe whose parent is missing or itself dependent is refused by policy.  (The reference resolves its
// type-1 subframes in stream order: a chain in that order is defined there, and the 32-bit decoders decode it; against that
// order it subtracts from a vector that is still empty.)
__device__ __forceinline__ bool parent_refused(uint32_t pinfo) { return pinfo == kNoSubframe || sub_info_type(pinfo) != 0; }

// SELA_HIP_FLAG_BAD_FRAME if a channel is missing or a parent refused, else 0.
__device__ __forceinline__ uint32_t layout_flags(const uint32_t* sub_info, uint32_t channels)
{
    uint32_t flags = 0;
    for (uint32_t c = 0; c < channels; c++) {
        const uint32_t info = sub_info[c];
        if (info == kNoSubframe || (sub_info_type(info) == 1 && parent_refused(sub_info[sub_info_parent(info)])))
            flags |= SELA_HIP_FLAG_BAD_FRAME;
    }
    return flags;
}

// The 16-bit value of channel c at sample i.
__device__ __forceinline__ uint32_t channel_value16(const DecSubframeLds* sub, const uint32_t* sub_info, uint32_t c, uint32_t i)
{
    const uint32_t info = sub_info[c];
    uint32_t v = info == kNoSubframe ? 0u : (uint32_t)(uint16_t)sub[sub_info_position(info)].smp[i];
    if (info != kNoSubframe && sub_info_type(info) == 1) {
        const uint32_t pinfo = sub_info[sub_info_parent(info)];
        const uint32_t pv = pinfo == kNoSubframe ? 0u : (uint32_t)(uint16_t)sub[sub_info_position(pinfo)].smp[i];
        v = pv - v;
    }
    return v & 0xFFFFu;
}

// Stereo: four samples of both channels per thread.  The case analysis is wave-uniform and done once ...
struct StereoPass {
    bool have0, have1, dep0, dep1;
    uint32_t par0, par1;  // parent channel of a dependent subframe (0 or 1: block_header_ok)
    const uint2 *s0, *s1; // the channels' raw samples, two per word
};
__device__ __forceinline__ StereoPass stereo_pass(const DecSubframeLds* sub, const uint32_t* sub_info)
{
    const uint32_t i0 = sub_info[0], i1 = sub_info[1];
    StereoPass sp;
    sp.have0 = i0 != kNoSubframe, sp.have1 = i1 != kNoSubframe;
    sp.dep0 = sp.have0 && sub_info_type(i0) == 1, sp.dep1 = sp.have1 && sub_info_type(i1) == 1;
    sp.par0 = sub_info_parent(i0), sp.par1 = sub_info_parent(i1);
    sp.s0 = reinterpret_cast<const uint2*>(sub[sp.have0 ? sub_info_position(i0) : 0].smp);
    sp.s1 = reinterpret_cast<const uint2*>(sub[sp.have1 ? sub_info_position(i1) : 0].smp);
    return sp;
}
// ... and these are the four output words of samples 4 i4 .. 4 i4 + 3 (sample i: channel 0 | channel 1 << 16).
__device__ __forceinline__ uint4 stereo_words(const StereoPass& sp, uint32_t i4)
{
    const uint2 zero = make_uint2(0, 0);
    const uint2 r0 = sp.have0 ? sp.s0[i4] : zero, r1 = sp.have1 ? sp.s1[i4] : zero; // raw subframe outputs
    // per 16-bit half: parent - difference (the parent's own, independent samples)
    auto sub16 = [](uint32_t a, uint32_t b) -> uint32_t { return ((a - (b & 0xFFFFu)) & 0xFFFFu) | ((a & 0xFFFF0000u) - (b & 0xFFFF0000u)); };
    uint2 a = r0, b = r1;
    if (sp.dep0) {
        const uint2 pv = sp.par0 == 0 ? r0 : r1;
        a = make_uint2(sub16(pv.x, r0.x), sub16(pv.y, r0.y));
    }
    if (sp.dep1) {
        const uint2 pv = sp.par1 == 0 ? r0 : r1;
        b = make_uint2(sub16(pv.x, r1.x), sub16(pv.y, r1.y));
    }
    uint4 w;
    w.x = (a.x & 0xFFFFu) | (b.x << 16);
    w.y = (a.x >> 16) | (b.x & 0xFFFF0000u);
    w.z = (a.y & 0xFFFFu) | (b.y << 16);
    w.w = (a.y >> 16) | (b.y & 0xFFFF0000u);
    return w;
}

// Launches of at most this many waves run their recurrence in the form for a wave that has its SIMD (nearly) to itself
// (synth_steps, kVecShift; vec_shift_from_for in sela_decode.hip).
constexpr uint32_t kLonelyWaves = 2560; // 2.5 per SIMD (tools/chain_ubench.py: the forms break even between 2 and 4)
