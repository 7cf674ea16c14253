// salvage_walk.cpp -- sela_amd/csrc/sela_salvage_walk.h alone (plain C++17, no HIP), under -fsanitize=address,undefined: the
// walk on crafted streams cut at EVERY byte, each in a heap buffer of exactly that many bytes and at each of the four
// alignments (the buffer ends where the payload ends, so a read past the end traps), with what must hold of any result
// checked, and the cases whose answer is known by construction.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sela_salvage_walk.h"

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
    const uint32_t found = sela::salvage_walk(room + shift, n, max_frames, channels, records.data(), totals);
    std::free(room);
    CHECK(found <= max_frames && totals[0] == found);
    uint64_t end = 0, gaps = 0, kept = 0;
    for (uint32_t f = 0; f < found; f++) {
        const sela_hip_salvaged& r = records[f];
        CHECK(r.offset % 4 == 0 && r.bytes % 4 == 0 && r.bytes >= 4 + 12 * channels && r.reserved == 0);
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
    for (uint32_t channels : { 1u, 2u, 3u }) {
        std::vector<uint8_t> stream;
        std::vector<size_t> starts;
        const uint32_t shapes[6][2] = { { 0, 0 }, { 1, 3 }, { 0, 5 }, { 2, 0 }, { 0, 0 }, { 1, 1 } };
        for (const auto& s : shapes) {
            starts.push_back(stream.size());
            append_frame(stream, channels, s[0], s[1]);
        }
        starts.push_back(stream.size());
        // every truncation, at every alignment: the frames that fit whole, in order, without a gap
        for (size_t n = 0; n <= stream.size(); n++)
            for (size_t shift = 0; shift < 4; shift++) {
                const uint32_t found = walk_exact(stream, n, shift, 8, channels, records, totals);
                uint32_t whole = 0;
                while (whole < 6 && starts[whole + 1] <= n)
                    whole++;
                CHECK(found == whole && totals[1] == 0 && totals[3] == starts[whole]);
            }
        // a flipped sync word in the middle, then every truncation of that: frame 2 is lost, frame 3 is found again while
        // frame 4 (or the payload's end) confirms it
        std::vector<uint8_t> bad = stream;
        bad[starts[2]] ^= 0xFF;
        for (size_t n = 0; n <= bad.size(); n++) {
            const uint32_t found = walk_exact(bad, n, n % 4, 8, channels, records, totals);
            uint32_t whole = 0;
            while (whole < 6 && starts[whole + 1] <= n)
                whole++;
            const bool confirmed = n / 4 * 4 == starts[4] || whole >= 5; // frame 3 ends the payload's whole words, or frame 4 follows whole
            const uint32_t want = whole < 2 ? whole : !confirmed ? 2 : whole - 1;
            CHECK(found == want);
            if (found > 2)
                CHECK(records[2].offset == starts[3] && records[2].skipped_before == starts[3] - starts[2] && totals[1] == 1);
        }
        // the caps, and channel counts the format cannot say
        CHECK(walk_exact(bad, bad.size(), 1, 0, channels, records, totals) == 0);
        CHECK(walk_exact(bad, bad.size(), 2, 2, channels, records, totals) == 2 && totals[1] == 0);
        CHECK(walk_exact(bad, bad.size(), 3, 3, channels, records, totals) == 3 && totals[1] == 1);
        CHECK(sela::salvage_walk(bad.data(), bad.size(), 8, 0, nullptr, totals) == 0 && totals[0] == 0);
        CHECK(sela::salvage_walk(bad.data(), bad.size(), 8, 256, nullptr, nullptr) == 0);
        CHECK(sela::salvage_walk(bad.data(), bad.size(), 8, channels, nullptr, nullptr) == 5);
    }
    // length fields that point far past the end: the bounds refuse them before anything is read there
    std::vector<uint8_t> wild;
    append_frame(wild, 1, 0xFFFF, 0xFFFF);
    wild.resize(40);
    CHECK(walk_exact(wild, wild.size(), 0, 4, 1, records, totals) == 0);
    std::printf("salvage_walk: %d failures\n", failures);
    return failures ? 1 : 0;
}
