/* header_forms.c -- the two forms of the subframe header reader in include/sela_format.h (bytes at any alignment, 32-bit
 * words on an aligned frame) agree: the same `next` and the same fields on every input, and neither reads past the frame.
 *
 *   header_forms FRAME CHANNELS [FRAME CHANNELS ...]
 *
 * Each FRAME (a file holding one frame of CHANNELS subframes) is first walked whole: both forms must follow it to its last
 * byte.  Then it is cut at every length, and both forms read at every word-aligned place of every cut.  A seeded fuzz of
 * word-aligned frames with random headers follows: read whole they must give back the fields they were written with, and cut
 * and read anywhere the two forms must agree.  Every comparison runs twice, with the bytes past the cut zero and with them all
 * ones: a reader that looked past the cut would not agree with itself.  Prints "<checks> <mismatches>".
 *   Build: gcc -O2 -std=c11 -Wall -Wextra -Iinclude header_forms.c */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sela_format.h"

#define CAP_WORDS (1 << 15)

static uint32_t zero_tail[CAP_WORDS], ones_tail[CAP_WORDS]; /* (declared uint32_t: the word form's loads are well-typed) */
static unsigned long long checks, mismatches;

static void report(const char* what, uint64_t fbytes, uint64_t p)
{
    if (mismatches++ < 20)
        fprintf(stderr, "mismatch: %s, frame of %llu bytes, header at %llu\n", what, (unsigned long long)fbytes, (unsigned long long)p);
}

/* Both forms, on both tails; returns the byte form's `next` (zero tail) and its fields in *out. */
static uint64_t read_both(uint64_t fbytes, uint64_t p, SelaSubframeHeader* out)
{
    SelaSubframeHeader h[4];
    uint64_t next[4];
    for (int i = 0; i < 4; i++) {
        memset(&h[i], 0xA5, sizeof h[i]); /* what the readers leave as it was must agree too */
        const uint8_t* frame = (const uint8_t*)(i & 1 ? ones_tail : zero_tail);
        next[i] = i < 2 ? sela_subframe_read_bytes(frame, fbytes, p, &h[i]) : sela_subframe_read_words(frame, fbytes, p, &h[i]);
    }
    checks++;
    for (int i = 1; i < 4; i++)
        if (next[i] != next[0] || memcmp(&h[i], &h[0], sizeof h[0]) != 0) {
            report(i == 1 ? "byte form reads past the frame" : (i == 2 ? "word form differs from byte form" : "word form reads past the frame"), fbytes, p);
            break;
        }
    *out = h[0];
    return next[0];
}

/* The frame's first `cut` bytes, the rest of the buffers zero / ones.  (Only the bytes the last load wrote are put back.) */
static void load(const uint8_t* bytes, uint64_t len, uint64_t cut)
{
    static uint64_t written;
    static int ready;
    if (!ready)
        memset(ones_tail, 0xFF, sizeof ones_tail), ready = 1;
    if (cut > len)
        cut = len;
    memset(zero_tail, 0x00, written);
    memset(ones_tail, 0xFF, written);
    memcpy(zero_tail, bytes, cut);
    memcpy(ones_tail, bytes, cut);
    written = cut;
}

/* Every cut of the frame, both forms at every word-aligned place of it. */
static void every_cut(const uint8_t* bytes, uint64_t len)
{
    for (uint64_t cut = 0; cut <= len; cut++) {
        load(bytes, len, cut);
        for (uint64_t p = 0; p <= cut + 4; p += 4) {
            SelaSubframeHeader h;
            read_both(cut, p, &h);
        }
    }
}

static int golden(const char* path, uint32_t channels)
{
    static uint8_t bytes[4 * CAP_WORDS];
    FILE* f = fopen(path, "rb");
    if (!f)
        return 1;
    const size_t len = fread(bytes, 1, sizeof bytes, f);
    fclose(f);
    if (len == 0 || len >= sizeof bytes)
        return 1;
    load(bytes, len, len);
    uint64_t p = 4;
    for (uint32_t c = 0; c < channels && p; c++) {
        SelaSubframeHeader h;
        p = read_both(len, p, &h);
    }
    if (p != len)
        report("a golden frame is not walked to its end", len, p);
    every_cut(bytes, len);
    return 0;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(void)
{
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 32);
}

static void put16(uint8_t* b, uint32_t v) { b[0] = (uint8_t)v, b[1] = (uint8_t)(v >> 8); }

/* A frame of 1..6 subframes with random header bytes and word counts (now and then one far beyond the frame). */
static void fuzz(int frames)
{
    static uint8_t bytes[4 * CAP_WORDS];
    for (int t = 0; t < frames; t++) {
        const uint32_t channels = 1 + rnd() % 6;
        SelaSubframeHeader want[6];
        uint64_t len = 4;
        const uint32_t sync = SELA_SYNC_WORD;
        memcpy(bytes, &sync, 4);
        int broken = 0;
        for (uint32_t c = 0; c < channels; c++) {
            SelaSubframeHeader* w = &want[c];
            w->channel = rnd() & 0xFF, w->type = rnd() & 0xFF, w->parent = rnd() & 0xFF, w->ck = rnd() & 0xFF, w->order = rnd() & 0xFF;
            w->rk = rnd() & 0xFF, w->n = rnd() & 0xFFFF;
            w->cw = rnd() % 24 == 0 ? rnd() & 0xFFFF : rnd() % 40;
            w->rw = rnd() % 24 == 0 ? rnd() & 0xFFFF : rnd() % 60;
            if (len + SELA_SUBFRAME_HEADER_BYTES + 4 * ((uint64_t)w->cw + w->rw) > 4096) { /* written as far as it goes: a frame that lies */
                broken = 1;
                uint8_t* b = bytes + len;
                b[0] = (uint8_t)w->channel, b[1] = (uint8_t)w->type, b[2] = (uint8_t)w->parent, b[3] = (uint8_t)w->ck;
                put16(b + 4, w->cw), b[6] = (uint8_t)w->order;
                len += 7;
                break;
            }
            uint8_t* b = bytes + len;
            b[0] = (uint8_t)w->channel, b[1] = (uint8_t)w->type, b[2] = (uint8_t)w->parent, b[3] = (uint8_t)w->ck;
            put16(b + 4, w->cw), b[6] = (uint8_t)w->order;
            for (uint32_t i = 0; i < 4 * w->cw; i++)
                b[7 + i] = (uint8_t)rnd();
            b += 7 + 4 * w->cw;
            b[0] = (uint8_t)w->rk, put16(b + 1, w->rw), put16(b + 3, w->n);
            for (uint32_t i = 0; i < 4 * w->rw; i++)
                b[5 + i] = (uint8_t)rnd();
            len += SELA_SUBFRAME_HEADER_BYTES + 4 * ((uint64_t)w->cw + w->rw);
        }
        len = (len + 3) & ~(uint64_t)3;
        if (!broken) { /* read whole: the fields it was written with, subframe after subframe, to its last byte */
            load(bytes, len, len);
            uint64_t p = 4;
            for (uint32_t c = 0; c < channels; c++) {
                SelaSubframeHeader h;
                const uint64_t at = p;
                p = read_both(len, p, &h);
                if (memcmp(&h, &want[c], sizeof h) != 0 || p == 0)
                    report("a fuzzed header is not read back as written", len, at);
                if (p == 0)
                    break;
            }
            if (p != len)
                report("a fuzzed frame is not walked to its end", len, p);
        }
        if (t % 16 == 0)
            every_cut(bytes, len);
        else { /* a few random cuts and places */
            for (int k = 0; k < 8; k++) {
                const uint64_t cut = rnd() % (len + 1);
                load(bytes, len, cut);
                for (uint64_t p = 0; p <= cut + 4; p += 4) {
                    SelaSubframeHeader h;
                    read_both(cut, p, &h);
                }
            }
        }
    }
}

int main(int argc, char** argv)
{
    if (argc < 3 || argc % 2 == 0) {
        fprintf(stderr, "usage: %s FRAME CHANNELS [FRAME CHANNELS ...]\n", argv[0]);
        return 2;
    }
    for (int i = 1; i + 1 < argc; i += 2)
        if (golden(argv[i], (uint32_t)atoi(argv[i + 1]))) {
            fprintf(stderr, "cannot read %s\n", argv[i]);
            return 2;
        }
    fuzz(4000);
    printf("%llu %llu\n", checks, mismatches);
    return 0;
}
