// salvage_walk_unaligned.cpp -- sela_amd/csrc/sela_salvage_walk_unaligned.h alone (plain C++17, no HIP), under
// -fsanitize=address,undefined: the walk on crafted streams with bytes inserted between frames, cut at EVERY byte, each in a heap
// buffer of exactly that many bytes and at each of the four alignments (the buffer ends where the payload ends, so a read past
// the end traps; every B % 4 occurs), with what must hold of any result checked, and the cases whose answer is known by
// construction.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sela_salvage_walk_unaligned.h"

static int failures = 0;
#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);      \
            failures++;                                                \
        }                                                              \
    } while (0)

// a frame of `channels` subframes: the first with `cw` coefficient words and `rw` Rice words, the others with none
static void append_frame(std::vector<uint8_t>& out, uint32_t channels, uint32_t cw, uint32_t rw)
{
    const uint32_t sync = SELA_SYNC_WORD;
    const uint8_t* s = reinterpret_cast<const uint8_t*>(&sync);
    out.insert(out.end(), s, s + 4);
    for (uint32_t c = 0; c < channels; c++) {
        const uint32_t w0 = c ? 0 : cw, w1 = c ? 0 : rw;
        const uint8_t head[7] = { (uint8_t)c, 0, 0, 4, (uint8_t)(w0 & 0xFF), (uint8_t)(w0 >> 8), 2 };
        out.insert(out.end(), head, head + 7);
        out.insert(out.end(), 4 * (size_t)w0, (uint8_t)0x11);
        const uint8_t tail[5] = { 6, (uint8_t)(w1 & 0xFF), (uint8_t)(w1 >> 8), 0x00, 0x08 };
        out.insert(out.end(), tail, tail + 5);
        out.insert(out.end(), 4 * (size_t)w1, (uint8_t)0x22);
    }
}

// the walk on a copy of bytes [0, n) that ends where its allocation ends, `shift` bytes into it; what holds of any result
static uint32_t walk_exact(const std::vector<uint8_t>& stream, size_t n, size_t shift, uint32_t max_frames, uint32_t channels,
    std::vector<sela_hip_salvaged>& records, uint64_t totals[4])
{
    uint8_t* room = static_cast<uint8_t*>(std::malloc(n + shift ? n + shift : 1));
    if (n)
        std::memcpy(room + shift, stream.data(), n);
    records.assign(max_frames, sela_hip_salvaged{ 1, 1, 1, 1 });
    const uint32_t found = sela::salvage_walk_unaligned(room + shift, n, max_frames, channels, records.data(), totals);
    std::free(room);
    CHECK(found <= max_frames && totals[0] == found);
    uint64_t end = 0, gaps = 0, kept = 0;
    for (uint32_t f = 0; f < found; f++) {
        const sela_hip_salvaged& r = records[f];
        CHECK(r.bytes % 4 == 0 && r.bytes >= 4 + 12 * channels && r.reserved == 0);
        CHECK(r.offset >= end && r.skipped_before == r.offset - end && r.offset + r.bytes <= n);
        gaps += r.skipped_before != 0;
        kept += r.bytes;
        end = r.offset + r.bytes;
    }
    CHECK(totals[1] == gaps && totals[2] == kept && totals[3] == end);
    for (uint32_t f = found; f < max_frames; f++)
        CHECK(records[f].offset == 1 && records[f].bytes == 1); // entries beyond the count are not written
    return found;
}

int main()
{
    std::vector<sela_hip_salvaged> records;
    uint64_t totals[4];
    for (uint32_t channels : { 1u, 2u, 3u })
        for (size_t extra = 0; extra < 6; extra++) { // bytes of garbage in front of frame 2: frames 2 .. 5 sit at phase extra % 4
            std::vector<uint8_t> stream;
            std::vector<size_t> starts, ends;
            const uint32_t shapes[6][2] = { { 0, 0 }, { 1, 3 }, { 0, 5 }, { 2, 0 }, { 0, 0 }, { 1, 1 } };
            for (int f = 0; f < 6; f++) {
                if (f == 2)
                    stream.insert(stream.end(), extra, (uint8_t)0x33);
                starts.push_back(stream.size());
                append_frame(stream, channels, shapes[f][0], shapes[f][1]);
                ends.push_back(stream.size());
            }
            // every truncation, at every alignment.  Frames 0 and 1 are trusted as they fit; behind the garbage a frame needs a
            // whole successor, or fewer than 4 bytes behind its end, to be confirmed -- unless it is trusted in its turn
            for (size_t n = 0; n <= stream.size(); n++)
                for (size_t shift = 0; shift < 4; shift++) {
                    const uint32_t found = walk_exact(stream, n, shift, 8, channels, records, totals);
                    uint32_t whole = 0;
                    while (whole < 6 && ends[whole] <= n)
                        whole++;
                    uint32_t want = whole;
                    if (extra && whole >= 3) {
                        // frame 2 is searched for: it is taken once frame 3 is whole, or while it is the last whole one with < 4 bytes behind
                        const bool two = whole >= 4 || n - ends[2] < 4;
                        want = two ? whole : 2;
                        // (once frame 2 is taken, 3 .. are trusted: each is taken as soon as it fits)
                    }
                    CHECK(found == want);
                    if (found > 2)
                        CHECK(records[2].offset == starts[2] && records[2].skipped_before == extra && totals[1] == (extra ? 1u : 0u));
                }
            // a flipped sync word behind the garbage as well: frame 4 is lost, frame 5 is found again at its odd phase
            std::vector<uint8_t> bad = stream;
            bad[starts[4]] ^= 0xFF;
            CHECK(walk_exact(bad, bad.size(), extra % 4, 8, channels, records, totals) == 5 && totals[1] == (extra ? 2u : 1u));
            CHECK(records[4].offset == starts[5] && records[4].skipped_before == starts[5] - starts[4]);
            // the caps, and channel counts the format cannot say
            CHECK(walk_exact(bad, bad.size(), 1, 0, channels, records, totals) == 0);
            CHECK(walk_exact(bad, bad.size(), 2, 2, channels, records, totals) == 2 && totals[1] == 0);
            CHECK(walk_exact(bad, bad.size(), 3, 3, channels, records, totals) == 3 && totals[1] == (extra ? 1u : 0u));
            CHECK(sela::salvage_walk_unaligned(bad.data(), bad.size(), 8, 0, nullptr, totals) == 0 && totals[0] == 0);
            CHECK(sela::salvage_walk_unaligned(bad.data(), bad.size(), 8, 256, nullptr, nullptr) == 0);
            CHECK(sela::salvage_walk_unaligned(bad.data(), bad.size(), 8, channels, nullptr, nullptr) == 5);
        }
    // payloads of 0 .. 19 bytes, and a sync word (or what fits of it) at each of the last 7 byte positions: nothing is found,
    // and nothing is read behind the end
    const uint32_t sync = SELA_SYNC_WORD;
    for (size_t n = 0; n < 20; n++)
        for (size_t back = 0; back <= 7 && back <= n; back++) {
            std::vector<uint8_t> lone(n, 0);
            if (back)
                std::memcpy(lone.data() + n - back, &sync, back < 4 ? back : 4);
            for (size_t shift = 0; shift < 4; shift++)
                CHECK(walk_exact(lone, n, shift, 4, 1, records, totals) == 0);
        }
    // length fields that point far past the end: the bounds refuse them before anything is read there
    std::vector<uint8_t> wild(3, 0x44);
    append_frame(wild, 1, 0xFFFF, 0xFFFF);
    wild.resize(43);
    CHECK(walk_exact(wild, wild.size(), 0, 4, 1, records, totals) == 0);
    std::printf("salvage_walk_unaligned: %d failures\n", failures);
    return failures ? 1 : 0;
}
