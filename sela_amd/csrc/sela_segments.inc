// sela_segments.inc -- a Rice stream of any length parsed segment by segment across the lanes of one wave (gfx950).
// Included inside namespace sela, behind sela_decode_core.inc, by sela_decode32.hip (k_decode_subframes32) and
// sela_window_whole.hip (k_tailwin_decode): one text, each translation unit its own copy.

// ---- one SEGMENT of a Rice stream, parsed across the lanes (any stream length, any number of values) --------------------------
// parse_subframe (sela_decode_core.inc) knows one shape: 2048 residues whose words fit one bitmap.  A stream of any length is
// cut into segments instead: up to kSegWords aligned words and up to kSegValues codewords, each parsed by the same three walks
// (phase A: every lane marks the codeword starts of its zone; phase B: on through the following zones until standing on a
// later lane's start; the true chain by pointer doubling; pass 2: the chain's lanes list the starts from their true entries)
// -- but with ONE stream per call, an entry anywhere in the segment's first word, a run-time number of codewords wanted, and
// a LIMIT: a codeword that starts at or behind it belongs to the next segment (the walks end there as they end at a stream's
// end).  A codeword that starts in front of the limit is this segment's however far it reaches.  Returns how many starts were
// listed (pos_out[0 .. found), relative to the segment's first word; found >= 1 whenever the entry lies in front of the limit),
// the bit behind the last of them -- the next segment's entry -- and whether one of them reaches beyond the stream's end.
constexpr int kSegWords = kStreamCap;                // words of one segment's start bitmap
constexpr uint32_t kSegValues = (uint32_t)kBlock;    // codewords listed per segment: their positions overwrite the bitmap (DecSubframeLds)
struct Segment {
    uint32_t found, next;
    bool overrun;
};

__device__ __attribute__((noinline)) Segment parse_segment(const uint32_t* seg_words /* the segment's first word */, uint32_t words_left /* of the subframe from there: reads beyond are zero */,
    uint32_t entry /* 0..31: the first codeword's bit */, uint32_t n_seg_words /* >= 1 */, uint32_t stream_end /* bit, relative to the segment's first word */, uint32_t k,
    uint32_t need /* 1 .. kSegValues */, uint32_t* marks /* zeroed: n_seg_words + kStreamMargin words */, uint16_t* pos_out, uint16_t* scratch16, int lane)
{
    const StreamWords sw = { seg_words, words_left };
    const __amdgpu_buffer_rsrc_t rs = stream_rsrc(sw);
    k = (uint32_t)__builtin_amdgcn_readfirstlane((int)k);
    const uint32_t W = n_seg_words;
    const uint32_t zr = (W + (uint32_t)kWave - 1) / (uint32_t)kWave; // words per zone
    const uint32_t first_word = min((uint32_t)lane * zr, W), end_word = min((uint32_t)(lane + 1) * zr, W);
    const uint32_t limit = min(32 * W, stream_end);
    const uint32_t last_mark_word = W + kStreamMargin - 1;
    const uint32_t zone_end = min(32 * end_word, limit);

    // ---- phase A: own zone, marking every codeword start ----
    uint32_t pos = lane == 0 ? entry : 32 * first_word;
    bool in_run = false;
    while (__any(pos < zone_end)) {
        const bool act = pos < zone_end;
        uint32_t off[5];
        bool simple;
        analyse4(rs, pos, k, off, simple);
        if (!__any(act && (in_run || !simple))) {
            uint32_t adv = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t p = pos + off[j];
                const bool a = act && p < zone_end;
                atomicOr(&marks[a ? p >> 5 : 0u], a ? 1u << (p & 31) : 0u);
                adv = a ? off[j + 1] : adv;
            }
            pos += adv;
        } else {
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

    // ---- phase B: on through the following zones until standing on a later lane's start, or at the limit ----
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
                const bool ended = walking && p >= limit;
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
            const bool ended = at_start && pos >= limit;
            const bool met = at_start && !ended && ((mk >> (pos & 31)) & 1u);
            merged = ended ? kEndOfStream : (met ? pos : merged);
            walking = walking && !ended && !met;
            n_cont += (at_start && walking) ? 1u : 0u;
            pos += walking ? adv : 0u;
            in_run = walking ? full : in_run;
        }
    }

    // ---- the chain of lanes the true trajectory runs through (pointer doubling, as in parse_subframe) ----
    uint32_t succ = merged != kEndOfStream ? (merged >> 5) / zr : 64u;
    succ = (succ > (uint32_t)lane && succ < 64u) ? succ : 64u; // (always a zone further on; keeps the orbit finite whatever the stream holds)
    uint8_t* const flag = reinterpret_cast<uint8_t*>(scratch16) + 512;
    uint32_t* const entry_of = reinterpret_cast<uint32_t*>(scratch16) + 160;
    flag[lane] = 0;
    bool on_chain = lane == 0;
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
    if (on_chain && succ < 64)
        entry_of[succ] = merged;
    wave_sync();
    uint32_t e_true = kEndOfStream;
    if (on_chain)
        e_true = lane == 0 ? entry : entry_of[lane];
    wave_sync();
    uint32_t count = 0;
    {
        const uint32_t we = e_true >> 5;
        for (uint32_t j = 0; j < zr; j++) {
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
    const uint32_t idx = wave_exclusive_scan(count, lane);
    const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)(idx + count), kWave - 1);
    Segment seg;
    seg.found = min(total, need);
    const uint32_t taken = idx < need ? min(count, need - idx) : 0u;
    uint32_t remaining = taken;
    wave_sync(); // every lane has read the bitmap: the positions may overwrite it

    // ---- pass 2: list the starts, every chain lane from its true entry ----
    uint16_t* out = pos_out + idx;
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
    // the lane that listed the segment's last codeword stands behind it
    const unsigned long long last = __ballot(taken != 0 && idx + taken == seg.found);
    seg.next = last ? (uint32_t)__builtin_amdgcn_readlane((int)pos, (int)__builtin_ctzll(last)) : entry;
    seg.overrun = __any(overrun);
    wave_sync();
    return seg;
}

// rice::RiceDecoder::process (src/rice/rice_decoder.cpp:21-61) for `count` values of the stream that occupies bits
// [first_bit, stream_end) of the subframe's aligned words, segment by segment; value i goes to out[i] (LDS or global memory).
// Returns SELA_HIP_FLAG_RICE_OVERRUN when a codeword reaches beyond the stream's end (the rest is then not defined).
__device__ __forceinline__ uint32_t parse_stream_segments(const uint32_t* gw, uint32_t nw, uint32_t first_bit, uint32_t stream_end, uint32_t k, uint32_t count,
    uint32_t words_per_value_x256 /* the stream's own average, for the segments' sizes */, DecSubframeLds* sl, uint16_t* scratch16, int32_t* out, int lane)
{
    const uint32_t kmask = k ? (0xFFFFFFFFu >> (32 - k)) : 0u;
    const uint32_t end_word = (stream_end + 31) >> 5;
    uint32_t done = 0, entry = first_bit, boost = 0;
    bool overrun = false;
#pragma unroll 1
    while (done < count) {
        if (entry >= stream_end) { // the stream has run dry: what is missing reads as zero bits
            for (uint32_t i = done + lane; i < count; i += kWave)
                out[i] = 0;
            overrun = true;
            break;
        }
        const uint32_t need = min(count - done, kSegValues);
        const uint32_t w0 = entry >> 5;
        // as many words as `need` codewords of the stream's average length take (+ 1/16 + 2): a segment that finds fewer simply
        // hands the rest to the next one (and makes that one twice as long: a stream whose codewords grow must not be walked
        // a few codewords at a time), one that covers many more than it may list parses them for nothing
        const uint64_t guess = ((uint64_t)need * words_per_value_x256) >> 8;
        const uint64_t wanted = (guess + (guess >> 4) + 2) << boost; // (< 2^28 x 2^12: no wrap in 64 bits)
        const uint32_t W = max(1u, min(min((uint32_t)kSegWords, end_word - w0), (uint32_t)min(wanted, (uint64_t)kSegWords)));
        for (uint32_t w = lane; w < W + kStreamMargin; w += kWave)
            sl->marks[w] = 0;
        wave_sync();
        const Segment seg = parse_segment(gw + w0, nw - w0, entry & 31, W, stream_end - 32 * w0, k, need, sl->marks, sl->pos, scratch16, lane);
        const StreamWords sw = { gw + w0, nw - w0 };
        const __amdgpu_buffer_rsrc_t rs = stream_rsrc(sw);
        for (uint32_t i0 = 0; i0 < seg.found; i0 += kWave) {
            const bool valid = i0 + lane < seg.found;
            const int32_t v = decode_at(rs, valid ? sl->pos[i0 + lane] : 0u, k, kmask, valid);
            if (valid)
                out[done + i0 + lane] = v;
        }
        wave_sync();
        done += seg.found;
        entry = 32 * w0 + seg.next;
        overrun |= seg.overrun;
        boost = (seg.found < need && boost < 12) ? boost + 1 : boost;
    }
    return overrun ? (uint32_t)SELA_HIP_FLAG_RICE_OVERRUN : 0u;
}
