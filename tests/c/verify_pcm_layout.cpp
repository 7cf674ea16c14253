// verify_pcm_layout.cpp -- the packed side of k_verify_pcm (sela_amd/csrc/sela_verify_pcm.hip) replayed on the CPU
// from the index arithmetic it is compiled from (sela_pcm_layout.h: pcm_held_frame, pcm_tile, pcm_load_plan, PcmTile::item,
// pcm_extract): every workgroup of the grid -- the kernel's own loop over a frame's tiles -- and every lane of it, a phase at a
// time (what a barrier separates on the device).  The original is an exact-size heap buffer, rounded up to its last dword as the
// contract says, so AddressSanitizer sees a byte beyond.  Checked for every shape, every pcm_samples and every table of sample
// offsets, garbage included: no dword outside the buffer is read, and every dword read is aligned and holds a byte of it; every
// sample below L_f is extracted exactly once, with the scalar restatement's value; no sample at or beyond L_f is extracted.
// Built with -fsanitize=address,undefined by tests/test_verify_pcm_cpu.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sela_pcm_layout.h"

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

static uint32_t rng_state = 24680;
static uint32_t rng()
{
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

// the three-line restatement
static int32_t sample_at(const uint8_t* pcm, uint64_t value, uint32_t bytes)
{
    uint32_t v = 0;
    for (uint32_t b = 0; b < bytes; b++)
        v |= (uint32_t)pcm[value * bytes + b] << (8 * b);
    return bytes == 3 ? (int32_t)(v << 8) >> 8 : (int32_t)v;
}

static uint64_t g_cases = 0;

// One launch: the frames of `so` (n_frames + 1 entries, whatever they say) against a buffer of pcm_samples samples per channel.
static void verify_case(uint32_t channels, uint32_t stride, const std::vector<uint64_t>& so, uint64_t pcm_samples, uint32_t bytes, const char* what)
{
    g_cases++;
    const uint32_t n_frames = (uint32_t)so.size() - 1;
    const uint64_t in_bytes = pcm_samples * channels * bytes;
    const size_t dwords_held = (size_t)((in_bytes + 3) / 4);
    uint8_t* const pcm = static_cast<uint8_t*>(std::malloc(dwords_held * 4 ? dwords_held * 4 : 1)); // (exact size: nothing behind the last dword)
    for (size_t i = 0; i < dwords_held * 4; i++)
        pcm[i] = (uint8_t)rng();
    const uint32_t n_tiles = pcm_tiles(stride, channels), tile_samples = pcm_tile_samples(channels);
    std::vector<uint32_t> image(kPcmImageDwords);
    std::vector<uint8_t> taken;
    const uint32_t lane = pcm_lane_dwords(bytes);
    for (uint32_t f = 0; f < n_frames; f++) {
        const PcmHeld h = pcm_held_frame(so[f], so[f + 1], stride, pcm_samples);
        CHECK(h.so <= pcm_samples && h.n <= stride && h.so + h.n <= pcm_samples, "%s: frame %u held outside the buffer", what, f);
        // the definition: L_f = min(n_f, max(pcm_samples - so[f], 0)), n_f clamped to stride
        const uint64_t n_f = std::min<uint64_t>(so[f + 1] - so[f], stride);
        const uint64_t want_L = std::min<uint64_t>(n_f, so[f] < pcm_samples ? pcm_samples - so[f] : 0);
        CHECK(h.n == want_L, "%s: frame %u: L %u, by the definition %llu", what, f, h.n, (unsigned long long)want_L);
        const uint32_t L = h.n;
        taken.assign((size_t)L * channels, 0);
        for (uint32_t tile = 0; tile < n_tiles; tile++) { // (the grid's y, and the kernel's stride over it)
            if ((uint64_t)tile * tile_samples >= L)
                continue;
            std::fill(image.begin(), image.end(), 0xDEADBEEFu);
            const PcmTile k = pcm_tile(h.so * channels * bytes, tile, L, channels, bytes);
            const PcmLoadPlan l = pcm_load_plan(k, bytes);
            CHECK(k.a0 % 4 == 0 && l.dwords <= kPcmImageDwords - 1 && k.s1 <= L && k.s0 < k.s1, "%s: tile %u of frame %u", what, tile, f);
            auto load = [&](uint32_t d) {
                const uint64_t at = k.a0 + 4ull * d;
                CHECK(at < k.a0 + k.p + k.bytes && at + 4 > k.a0 + k.p && at < in_bytes, "%s: a dword read holds no byte of the buffer: %llu", what, (unsigned long long)at);
                CHECK(at + 4 <= dwords_held * 4, "%s: read beyond the buffer's last dword", what);
                std::memcpy(&image[d], pcm + at, 4); // (AddressSanitizer: the heap buffer is exact)
            };
            for (uint32_t t = 0; t < kPcmThreads; t++) {
                for (uint32_t r = t; r < l.runs; r += kPcmThreads)
                    for (uint32_t i = 0; i < lane; i++)
                        load(r * lane + i);
                for (uint32_t d = l.runs * lane + t; d < l.dwords; d += kPcmThreads)
                    load(d);
            }
            const uint32_t items = k.items();
            for (uint32_t t = 0; t < kPcmThreads; t++) {
                for (uint32_t j = t; j < items; j += kPcmThreads) {
                    const PcmItem it = k.item(j);
                    CHECK(it.c < channels && it.count >= 1 && it.count <= 4 && it.s % 4 == 0, "%s: item %u", what, j);
                    for (uint32_t i = 0; i < it.count; i++) {
                        const uint32_t s = it.s + i;
                        CHECK(s < L, "%s: a sample at or beyond L is extracted: frame %u channel %u sample %u, L %u", what, f, it.c, s, L);
                        if (s >= L || it.c >= channels)
                            continue;
                        const uint32_t at = k.at(it.c, s, bytes);
                        const int32_t v = pcm_extract(image[at >> 2], image[(at >> 2) + 1], at & 3, bytes);
                        CHECK(v == sample_at(pcm, (h.so + s) * channels + it.c, bytes), "%s: frame %u channel %u sample %u: value", what, f, it.c, s);
                        taken[(size_t)s * channels + it.c]++;
                    }
                }
            }
        }
        uint64_t not_once = 0;
        for (uint8_t n : taken)
            not_once += n != 1;
        CHECK(not_once == 0, "%s: frame %u (ch %u, L %u, bytes %u): %llu samples not extracted exactly once", what, f, channels, L, bytes, (unsigned long long)not_once);
    }
    std::free(pcm);
}

int main()
{
    const uint32_t channel_counts[] = { 1, 2, 3, 5, 8, 255 };
    const uint32_t lengths[] = { 1, 2, 3, 5, 7, 15, 16, 17, 33, 2047, 2048, 2049 };
    for (uint32_t bytes = 3; bytes <= 4; bytes++) {
        for (uint32_t ch : channel_counts) {
            for (uint32_t n : lengths) {
                // three frames back to back: all byte phases occur (n * ch * 3 mod 4 runs through them where it is odd)
                const std::vector<uint64_t> so = { 0, n, 2ull * n, 3ull * n };
                const uint64_t end = 3ull * n;
                verify_case(ch, n, so, end, bytes, "exact");
                verify_case(ch, n, so, end - 1, bytes, "one short");
                verify_case(ch, n, so, n + n / 2, bytes, "inside the middle frame");
                verify_case(ch, n, so, 0, bytes, "empty");
                verify_case(ch, n + 3, so, end, bytes, "a larger stride");
                verify_case(ch, n, { 0, n }, n, bytes, "one frame");
                // tables with garbage: decreasing, huge, and both
                verify_case(ch, n, { 2ull * n, n, 0, n }, end, bytes, "decreasing");
                verify_case(ch, n, { 0, 0xFFFFFFFFFFFFFFF0ull, n, 2ull * n }, end, bytes, "huge");
                verify_case(ch, n, { 0xFFFFFFFFFFFFFFFFull, 5, 0x8000000000000000ull, 1 }, end, bytes, "huge and decreasing");
                verify_case(ch, n, { end - 1, end + 7, end + 7 + n, 0 }, end, bytes, "across the end");
            }
            // frames of different lengths, one launch (the stride is the largest)
            verify_case(ch, 2825, { 0, 2048, 4096, 4096 + 2825, 4096 + 2825 + 128 }, 4096 + 2825 + 128, bytes, "mixed lengths");
            verify_case(ch, 2825, { 0, 2048, 4096, 4096 + 2825, 4096 + 2825 + 128 }, 4096 + 1000, bytes, "mixed lengths, short");
        }
    }
    if (g_failures) {
        std::printf("verify_pcm_layout: %d failures\n", g_failures);
        return 1;
    }
    std::printf("verify_pcm_layout ok: %llu launches\n", (unsigned long long)g_cases);
    return 0;
}
