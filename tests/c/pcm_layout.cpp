// pcm_layout.cpp -- k_pcm_unpack / k_pcm_pack (sela_amd/csrc/sela_pcm.hip) replayed on the CPU from the index arithmetic they are
// compiled from (sela_pcm_layout.h): every workgroup of the grid, every thread of it in the kernel's own loops, a phase at a time
// (what a barrier separates on the device).  Checked, for every shape: every output byte is written exactly once and none
// outside (the buffers are exact-size: AddressSanitizer sees a byte beyond); every dword read on the packed side is aligned and
// holds a byte of the input; packed bytes are stored singly only at a frame's two ends, at most 3 each, and no dword is stored by
// two workgroups; the result is the scalar restatement's.  Built with -fsanitize=address,undefined by tests/test_pcm_cpu.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
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

static uint32_t rng_state = 12345;
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

static void unpack_case(uint32_t channels, uint32_t n, uint32_t n_frames, uint32_t bytes)
{
    const uint64_t values = (uint64_t)n_frames * n * channels, in_bytes = values * bytes;
    std::vector<uint8_t> pcm((in_bytes + 3) & ~(uint64_t)3); // (the last aligned dword that holds an input byte is readable)
    for (auto& b : pcm)
        b = (uint8_t)rng();
    std::vector<int32_t> out(values);
    std::vector<uint8_t> written(values, 0);
    std::vector<uint32_t> image(kPcmImageDwords);
    const uint32_t lane = pcm_lane_dwords(bytes), tiles = pcm_tiles(n, channels);
    for (uint32_t f = 0; f < n_frames; f++) {
        for (uint32_t tile = 0; tile < tiles; tile++) {
            std::fill(image.begin(), image.end(), 0xDEADBEEFu);
            const PcmTile k = pcm_tile((uint64_t)f * n * channels * bytes, tile, n, channels, bytes);
            const PcmLoadPlan l = pcm_load_plan(k, bytes);
            CHECK(k.a0 % 4 == 0 && l.dwords <= kPcmImageDwords - 1, "image: a0 %llu dwords %u", (unsigned long long)k.a0, l.dwords);
            auto load = [&](uint32_t d) {
                const uint64_t at = k.a0 + 4ull * d;
                CHECK(at % 4 == 0 && at < k.a0 + k.p + k.bytes && at + 4 > k.a0 + k.p && at < in_bytes, "a dword read holds no byte of the tile: %llu", (unsigned long long)at);
                CHECK(at + 4 <= pcm.size(), "read beyond the input's last dword");
                if (at + 4 <= pcm.size())
                    std::memcpy(&image[d], &pcm[at], 4);
            };
            for (uint32_t t = 0; t < kPcmThreads; t++) {
                for (uint32_t r = t; r < l.runs; r += kPcmThreads)
                    for (uint32_t i = 0; i < lane; i++)
                        load(r * lane + i);
                for (uint32_t d = l.runs * lane + t; d < l.dwords; d += kPcmThreads)
                    load(d);
            }
            auto store = [&](uint32_t c, uint32_t s) {
                const uint32_t at = k.at(c, s, bytes);
                const uint64_t o = ((uint64_t)f * channels + c) * n + s;
                CHECK(c < channels && s < n, "store outside the frame");
                if (c < channels && s < n) {
                    out[o] = pcm_extract(image[at >> 2], image[(at >> 2) + 1], at & 3, bytes);
                    written[o]++;
                }
            };
            for (uint32_t t = 0; t < kPcmThreads; t++) {
                for (uint32_t j = t; j < k.items(); j += kPcmThreads) {
                    const PcmItem it = k.item(j);
                    if (it.count != 4)
                        continue;
                    for (uint32_t i = 0; i < 4; i++)
                        store(it.c, it.s + i);
                }
                const uint32_t rest = k.rest();
                for (uint32_t j = t; j < channels * rest; j += kPcmThreads) {
                    const uint32_t c = j / rest;
                    store(c, k.s1 - rest + (j - c * rest));
                }
            }
        }
    }
    uint64_t wrong = 0, not_once = 0;
    for (uint32_t f = 0; f < n_frames; f++)
        for (uint32_t c = 0; c < channels; c++)
            for (uint32_t s = 0; s < n; s++) {
                const uint64_t o = ((uint64_t)f * channels + c) * n + s;
                not_once += written[o] != 1;
                wrong += out[o] != sample_at(pcm.data(), ((uint64_t)f * n + s) * channels + c, bytes);
            }
    CHECK(wrong == 0 && not_once == 0, "unpack ch %u n %u frames %u bytes %u: %llu wrong, %llu not written once", channels, n, n_frames, bytes,
        (unsigned long long)wrong, (unsigned long long)not_once);
}

static void pack_case(uint32_t channels, uint32_t stride, const std::vector<uint32_t>& lengths, uint32_t bytes)
{
    const uint32_t n_frames = (uint32_t)lengths.size();
    std::vector<uint64_t> so(n_frames + 1, 0);
    for (uint32_t f = 0; f < n_frames; f++)
        so[f + 1] = so[f] + lengths[f];
    std::vector<int32_t> samples((size_t)n_frames * channels * stride);
    for (auto& v : samples)
        v = (int32_t)(rng() << 8 | (rng() & 0xFF));
    const uint64_t out_bytes = so[n_frames] * channels * bytes;
    std::vector<uint8_t> out(out_bytes, 0);
    std::vector<uint8_t> written(out_bytes, 0);
    std::map<uint64_t, uint32_t> dword_owner; // aligned byte -> the workgroup that stored it whole
    std::vector<uint8_t> image(kPcmImageDwords * 4);
    const uint32_t lane = pcm_lane_dwords(bytes), tiles = pcm_tiles(stride, channels);
    uint64_t wide = 0, wide_want = 0;
    for (uint32_t f = 0; f < n_frames; f++) {
        const uint32_t n = lengths[f];
        uint32_t single_head = 0, single_tail = 0;
        for (uint32_t tile = 0; tile < tiles; tile++) {
            if (tile * pcm_tile_samples(channels) >= n)
                continue;
            std::fill(image.begin(), image.end(), 0xEE);
            const PcmTile k = pcm_tile(so[f] * channels * bytes, tile, n, channels, bytes);
            const PcmStorePlan p = pcm_store_plan(k, n, bytes);
            const int32_t* const fi = samples.data() + (size_t)f * channels * stride;
            auto put = [&](uint32_t at, int32_t v, uint32_t first) {
                for (uint32_t b = first; b < bytes; b++) {
                    const uint32_t i = at + b; // (as on the device: 32-bit, may wrap through 0)
                    CHECK(i < image.size(), "image byte %u", i);
                    if (i < image.size())
                        image[i] = (uint8_t)((uint32_t)v >> (8 * b));
                }
            };
            if (bytes == 3 && p.lead)
                put(k.p - bytes, fi[(size_t)(channels - 1) * stride + k.s0 - 1], bytes - k.p);
            CHECK(bytes == 3 || !p.lead, "a 4-byte tile has no phase");
            for (uint32_t t = 0; t < kPcmThreads; t++)
                for (uint32_t j = t; j < k.items(); j += kPcmThreads) {
                    const PcmItem it = k.item(j);
                    for (uint32_t i = 0; i < it.count; i++) {
                        CHECK(it.c < channels && it.s + i < n, "a sample read beyond the channel's count");
                        const int32_t v = fi[(size_t)it.c * stride + it.s + i];
                        put(k.at(it.c, it.s + i, bytes), v, 0);
                        if (bytes == 3)
                            wide += v < -(1 << 23) || v >= (1 << 23);
                    }
                }
            auto store_byte = [&](uint32_t at) {
                const uint64_t o = k.a0 + at;
                CHECK(o < out_bytes, "byte store outside the output");
                if (o < out_bytes)
                    out[o] = image[at], written[o]++;
            };
            auto store_dword = [&](uint32_t d) {
                const uint64_t o = k.a0 + 4ull * d;
                CHECK(o % 4 == 0 && o + 4 <= out_bytes, "dword store outside the output or misaligned");
                CHECK(dword_owner.emplace(o, f * tiles + tile).second, "a dword stored by two workgroups (or twice)");
                if (o + 4 <= out_bytes)
                    for (uint32_t b = 0; b < 4; b++)
                        out[o + b] = image[4 * d + b], written[o + b]++;
            };
            CHECK(p.head <= 3 && p.tail <= 3 && p.mid_at % 4 == 0, "head %u tail %u mid_at %u", p.head, p.tail, p.mid_at);
            CHECK((p.head == 0 || tile == 0) && (p.tail == 0 || k.s1 == n), "bytes stored singly inside a frame");
            single_head += p.head, single_tail += p.tail;
            for (uint32_t t = 0; t < kPcmThreads; t++) {
                if (t < p.head)
                    store_byte(p.head_at + t);
                if (t < p.tail)
                    store_byte(p.tail_at + t);
                const uint32_t mid = p.mid_at >> 2;
                for (uint32_t r = t; r < p.runs; r += kPcmThreads)
                    for (uint32_t i = 0; i < lane; i++)
                        store_dword(mid + r * lane + i);
                for (uint32_t d = p.runs * lane + t; d < p.dwords; d += kPcmThreads)
                    store_dword(mid + d);
            }
        }
        CHECK(single_head <= 3 && single_tail <= 3, "frame %u: %u + %u bytes stored singly", f, single_head, single_tail);
    }
    uint64_t wrong = 0, not_once = 0;
    for (uint32_t f = 0; f < n_frames; f++)
        for (uint32_t s = 0; s < lengths[f]; s++)
            for (uint32_t c = 0; c < channels; c++) {
                const int32_t v = samples[((size_t)f * channels + c) * stride + s];
                if (bytes == 3)
                    wide_want += v < -(1 << 23) || v >= (1 << 23);
                for (uint32_t b = 0; b < bytes; b++) {
                    const uint64_t o = ((so[f] + s) * channels + c) * bytes + b;
                    wrong += out[o] != (uint8_t)((uint32_t)v >> (8 * b));
                    not_once += written[o] != 1;
                }
            }
    CHECK(wrong == 0 && not_once == 0 && wide == wide_want, "pack ch %u stride %u frames %u bytes %u: %llu wrong, %llu not written once, wide %llu / %llu", channels,
        stride, n_frames, bytes, (unsigned long long)wrong, (unsigned long long)not_once, (unsigned long long)wide, (unsigned long long)wide_want);
}

int main()
{
    const uint32_t channel_set[] = { 1, 2, 3, 5, 8, 255 }, length_set[] = { 1, 2, 3, 5, 7, 64, 2047, 2048, 2049 }, frame_set[] = { 1, 3 }, byte_set[] = { 3, 4 };
    int cases = 0;
    for (uint32_t c : channel_set)
        for (uint32_t n : length_set)
            for (uint32_t frames : frame_set)
                for (uint32_t bytes : byte_set) {
                    unpack_case(c, n, frames, bytes);
                    pack_case(c, n, std::vector<uint32_t>(frames, n), bytes);
                    if (frames == 3) // mixed lengths under one stride: the frames start wherever the ones before end
                        pack_case(c, n, { n, (n + 1) / 2, 1 }, bytes);
                    cases++;
                }
    for (uint32_t c : channel_set) { // the tile sizes: a multiple of 4, within the image
        const uint32_t t = pcm_tile_samples(c);
        CHECK(t % 4 == 0 && t >= 4 && (uint64_t)t * c <= kPcmTileValues, "tile of %u channels: %u samples", c, t);
    }
    if (g_failures) {
        std::printf("pcm_layout: %d failures\n", g_failures);
        return 1;
    }
    std::printf("pcm_layout ok: %d shapes\n", cases);
    return 0;
}
