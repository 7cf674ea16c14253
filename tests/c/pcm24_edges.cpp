// pcm24_edges.cpp -- the packed 3-byte store of k_window32_store (sela_amd/csrc/sela_window32.hip) replayed on the CPU from the
// arithmetic it is compiled from (sela_pcm24_edges.h): a share of the output at every byte phase, stored in rounds as the kernel
// stores it -- the round's values in a table behind the lead, head bytes, aligned dwords, tail bytes, the last value carried to
// the next round.  Checked against a byte-by-byte brute force, for every shape: every byte of the share is written exactly once
// and holds its value's byte; nothing outside it is written (the buffer is exact-size: AddressSanitizer sees a byte beyond, and
// the neighbours' bytes are counted); every dword stored is aligned; bytes are stored singly only at the share's two ends, at
// most three each.  Built with -fsanitize=address,undefined by tests/test_decode_windows_i32_cpu.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sela_pcm24_edges.h"

using namespace sela;

static int g_failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (g_failures++ < 20) {                      \
                std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
                std::printf(__VA_ARGS__);                 \
                std::printf("\n");                        \
            }                                             \
        }                                                 \
    } while (0)

static uint32_t rng_state = 2463534242u;
static uint32_t rng()
{
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 4;
}

// One share: `front` bytes of a neighbour in front of it (so that it starts at phase front % 4 of an aligned buffer), n samples of
// `channels` channels, `behind` bytes of a neighbour behind; stored in rounds of `round` samples.
static void share_case(uint32_t front, uint32_t n, uint32_t channels, uint32_t behind, uint32_t round)
{
    const uint64_t B0 = front, B1 = B0 + 3ull * n * channels, total = B1 + behind;
    std::vector<int32_t> value((size_t)n * channels);
    for (auto& v : value)
        v = (int32_t)(rng() << 4 ^ rng()); // (all 32 bits: the top byte must not leak into a neighbour's)
    std::vector<uint8_t> out(total, 0x5A), written(total, 0);
    std::vector<int32_t> vals(1 + (size_t)round * channels + 1, 0x77777777);
    int32_t carry = 0x66666666;
    uint32_t singles_head = 0, singles_tail = 0;
    for (uint32_t base = 0; base < n; base += round) {
        const uint32_t here = n - base < round ? n - base : round, m = here * channels;
        if (base != 0)
            vals[0] = carry;
        for (uint32_t v = 0; v < m; v++)
            vals[1 + v] = value[(size_t)base * channels + v];
        const uint64_t b0 = B0 + 3ull * base * channels, lead_at = b0 - 3; // (modulo 2^64 where b0 < 3, as on the device)
        const Pcm24Span sp = pcm24_span(b0, b0 + 3ull * m, base == 0, base + round >= n);
        CHECK(sp.head <= 3 && sp.tail <= 3 && sp.mid_at % 4 == 0, "head %u tail %u mid_at %llu", sp.head, sp.tail, (unsigned long long)sp.mid_at);
        CHECK((sp.head == 0 || base == 0) && (sp.tail == 0 || base + round >= n), "bytes stored singly inside a share");
        singles_head += sp.head, singles_tail += sp.tail;
        auto store_byte = [&](uint64_t at) {
            CHECK(at >= B0 && at < B1, "byte store outside the share: %llu", (unsigned long long)at);
            const uint32_t from_lead = (uint32_t)(at - lead_at);
            CHECK(pcm24_slot_of(from_lead) <= m && (base != 0 || pcm24_slot_of(from_lead) >= 1), "slot %u of %u", pcm24_slot_of(from_lead), m);
            if (at < total)
                out[at] = pcm24_byte(vals, from_lead), written[at]++;
        };
        for (uint32_t t = 0; t < sp.head; t++)
            store_byte(sp.head_at + t);
        for (uint64_t e = 0; e < sp.dwords; e++) {
            const uint64_t at = sp.mid_at + 4 * e;
            CHECK(at % 4 == 0 && at >= B0 && at + 4 <= B1, "dword store misaligned or outside the share: %llu", (unsigned long long)at);
            const uint32_t from_lead = (uint32_t)(at - lead_at);
            CHECK(pcm24_slot_of(from_lead) + 1 <= m && (base != 0 || pcm24_slot_of(from_lead) >= 1), "dword slots %u, %u of %u", pcm24_slot_of(from_lead),
                pcm24_slot_of(from_lead) + 1, m);
            const uint32_t d = pcm24_dword(vals, from_lead);
            for (uint32_t b = 0; b < 4; b++)
                if (at + b < total)
                    out[at + b] = (uint8_t)(d >> (8 * b)), written[at + b]++;
        }
        for (uint32_t t = 0; t < sp.tail; t++)
            store_byte(sp.tail_at + t);
        carry = vals[m];
    }
    CHECK(singles_head <= 3 && singles_tail <= 3, "%u + %u bytes stored singly", singles_head, singles_tail);
    // the brute force: byte k of the share is byte k % 3 of value k / 3, and everything else is untouched
    uint64_t wrong = 0, not_once = 0, outside = 0;
    for (uint64_t at = 0; at < total; at++) {
        if (at >= B0 && at < B1) {
            const uint64_t k = at - B0;
            wrong += out[at] != (uint8_t)((uint32_t)value[k / 3] >> (8 * (k % 3)));
            not_once += written[at] != 1;
        } else {
            outside += written[at] != 0 || out[at] != 0x5A;
        }
    }
    CHECK(wrong == 0 && not_once == 0 && outside == 0, "front %u n %u ch %u behind %u round %u: %llu wrong, %llu not written once, %llu outside", front, n, channels, behind,
        round, (unsigned long long)wrong, (unsigned long long)not_once, (unsigned long long)outside);
}

int main()
{
    const uint32_t channel_set[] = { 1, 2, 3, 5, 8 }, round_set[] = { 1, 2, 3, 4, 7, 256 }, behind_set[] = { 0, 1, 5 };
    int cases = 0;
    for (uint32_t channels : channel_set)
        for (uint32_t phase = 0; phase < 4; phase++)
            for (uint32_t front : { phase, phase + 4 }) // (a share at the very start of the buffer too: its lead would lie in front of byte 0)
                for (uint32_t n = 0; 3 * n * channels <= 40 + 3 * channels; n++) // every share length of 0 .. 40 bytes that this many channels can have, and one beyond
                    for (uint32_t round : round_set)
                        for (uint32_t behind : behind_set) {
                            share_case(front, n, channels, behind, round);
                            cases++;
                        }
    // the kernel's own round (256 samples) on shares of more than one round, whole frames among them
    for (uint32_t channels : channel_set)
        for (uint32_t phase = 0; phase < 4; phase++)
            for (uint32_t n : { 255u, 256u, 257u, 511u, 513u, 2047u, 2048u }) {
                share_case(phase, n, channels, 3, 256);
                cases++;
            }
    if (g_failures) {
        std::printf("pcm24_edges: %d failures\n", g_failures);
        return 1;
    }
    std::printf("pcm24_edges ok: %d shapes\n", cases);
    return 0;
}
