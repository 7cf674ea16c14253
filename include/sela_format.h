/*
 * sela_format.h -- format-defining constants of the SELA frame codec, and the reader of a subframe header.
 *
 * These numbers and that layout ARE the bitstream contract; every implementation in this repo
 * (HIP kernels, CPU oracle, C++ host) includes this one header so they cannot drift.
 * Each constant cites the reference line that fixes it (paths relative to the
 * reference checkout, sahaRatul/sela v2.0.2).
 */
#ifndef SELA_FORMAT_H_
#define SELA_FORMAT_H_

#include <stdbool.h>
#include <stdint.h>

#define SELA_MAX_LPC_ORDER 100          /* src/include/lpc.hpp:7  */
#define SELA_Q_SHIFT 35                 /* CORRECTION_FACTOR, src/include/lpc.hpp:8 */
#define SELA_SQRT2 1.4142135623730950488016887242096 /* src/include/lpc.hpp:9 (literal, rounds to 0x1.6a09e667f3bcdp+0) */
#define SELA_MAX_RICE_PARAM 20          /* k in [0,20), src/include/rice.hpp:7 */
#define SELA_BLOCK 2048                 /* samplesPerChannelPerFrame, src/include/file/wav_file.hpp:12 */
#define SELA_SAMPLE_SCALE 32767.0       /* quantizationFactor = INT16_MAX, src/include/lpc.hpp:93 */
#define SELA_ORDER_THRESHOLD 0.05       /* src/lpc/residue_generator.cpp:73 */
#define SELA_SYNC_WORD 0xAA55FF00u      /* src/include/data/sela_frame.hpp:9 */
#define SELA_FILE_HEADER_BYTES 15       /* 'SeLa' u32 rate u16 bps u8 ch u32 frames, src/file/sela_file.cpp:108-112 */
#define SELA_SUBFRAME_HEADER_BYTES 12   /* 3 + 4 + 5 bytes of fields, src/file/sela_file.cpp:121-133 */

/* Dequantisation tables, src/include/lpc.hpp:10-71 (verbatim data, see tools/gen_tables.py). */
#ifndef SELA_TABLE_QUAL
#define SELA_TABLE_QUAL static const
#endif
#include "sela_tables.inc"

/* On-disk size of one frame given the per-subframe word counts. */
#if defined(__HIPCC__)
#define SELA_HOST_DEVICE __host__ __device__
#else
#define SELA_HOST_DEVICE
#endif
SELA_HOST_DEVICE static inline uint32_t sela_frame_bytes(uint32_t channels, uint32_t total_words)
{
    return 4u + channels * SELA_SUBFRAME_HEADER_BYTES + 4u * total_words;
}

/* One subframe header (src/file/sela_file.cpp:58-91): channel, type, parent, coefficient k (u8 each), coefficient word
 * count (u16), order (u8), the coefficient words, then residue k (u8), residue word count (u16), samplesPerChannel (u16).
 * Every walk over a frame's subframes reads them through one of the two readers below. */
typedef struct {
    uint32_t channel, type, parent, ck, cw, order, rk, rw, n;
} SelaSubframeHeader;

/* The subframe header at byte p of a frame (or payload) of fbytes bytes: returns the byte offset of the next subframe, or 0 when
 * the header or its words run past fbytes.  The fields are filled as far as the header lies inside the frame: channel .. order
 * once p + 12 <= fbytes, rk, rw and n once the coefficient words and the rest of the header fit as well (so a 0 with those set
 * means only the residue words run past).  What the reader cannot reach it leaves as it was.
 *
 * Two forms, with the same bounds and the same results.  sela_subframe_read_bytes works at any alignment;
 * sela_subframe_read_words is for a word-aligned frame and p (every subframe of a well-formed frame is: 4 + 12 per subframe
 * + 4 per word): two 32-bit loads at p and two at p + 4 + 4 cw, the last three coefficient bytes and the residue header. */
SELA_HOST_DEVICE static inline uint64_t sela_subframe_read_bytes(const uint8_t* frame, uint64_t fbytes, uint64_t p, SelaSubframeHeader* h)
{
    if (p + SELA_SUBFRAME_HEADER_BYTES > fbytes)
        return 0;
    const uint8_t* b = frame + p;
    h->channel = b[0], h->type = b[1], h->parent = b[2], h->ck = b[3];
    h->cw = b[4] | ((uint32_t)b[5] << 8), h->order = b[6];
    const uint64_t q = p + 7 + 4 * (uint64_t)h->cw; /* residue k */
    if (q + 5 > fbytes)
        return 0;
    b = frame + q;
    h->rk = b[0], h->rw = b[1] | ((uint32_t)b[2] << 8), h->n = b[3] | ((uint32_t)b[4] << 8);
    const uint64_t next = q + 5 + 4 * (uint64_t)h->rw;
    return next <= fbytes ? next : 0;
}

SELA_HOST_DEVICE static inline uint64_t sela_subframe_read_words(const uint8_t* frame, uint64_t fbytes, uint64_t p, SelaSubframeHeader* h)
{
    if (p + SELA_SUBFRAME_HEADER_BYTES > fbytes)
        return 0;
    const uint32_t h0 = *(const uint32_t*)(frame + p), h1 = *(const uint32_t*)(frame + p + 4);
    h->channel = h0 & 0xFF, h->type = (h0 >> 8) & 0xFF, h->parent = (h0 >> 16) & 0xFF, h->ck = h0 >> 24;
    h->cw = h1 & 0xFFFF, h->order = (h1 >> 16) & 0xFF;
    const uint64_t q = p + 4 + 4 * (uint64_t)h->cw; /* the word that ends in residue k */
    if (q + 8 > fbytes)
        return 0;
    const uint32_t h2 = *(const uint32_t*)(frame + q), h3 = *(const uint32_t*)(frame + q + 4);
    h->rk = h2 >> 24, h->rw = h3 & 0xFFFF, h->n = h3 >> 16;
    const uint64_t next = q + 8 + 4 * (uint64_t)h->rw;
    return next <= fbytes ? next : 0;
}

/* What every decoder asks of a header before it parses: an order the tables cover and Rice parameters a 32-bit word holds. */
SELA_HOST_DEVICE static inline bool sela_subframe_decodable(const SelaSubframeHeader* h)
{
    return h->order <= SELA_MAX_LPC_ORDER && h->ck < 32 && h->rk < 32;
}

#endif /* SELA_FORMAT_H_ */
