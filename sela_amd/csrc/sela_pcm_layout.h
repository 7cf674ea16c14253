// sela_pcm_layout.h -- the index arithmetic of k_pcm_unpack / k_pcm_pack (sela_pcm.hip): which bytes, dwords and
// samples a workgroup touches.  Plain C++ compiled for the device and for the host, so that tests/c/pcm_layout.cpp walks exactly
// the tiling the kernels use.
//
// Packed side: little-endian interleaved PCM, kBytes (3 or 4) per sample, [frame][sample][channel].  Planar side: int32
// [frame][channel][samples].  A frame's n * channels samples in interleaved order are its VALUES: value v = s * channels + c.
// One workgroup covers one (frame, tile): pcm_tile_samples(channels) samples of every channel, at most kPcmTileValues values --
// the tile's packed bytes stand in LDS as an IMAGE whose byte 0 is the aligned dword that holds the tile's first byte, so every
// global access on the packed side is an aligned dword (or a run of 3 or 4 of them per lane).
#ifndef SELA_PCM_LAYOUT_H_
#define SELA_PCM_LAYOUT_H_

#include <cstdint>

#if defined(__HIPCC__)
#define SELA_PCM_HD __host__ __device__ inline
#else
#define SELA_PCM_HD inline
#endif

namespace sela {

constexpr uint32_t kPcmThreads = 256;
constexpr uint32_t kPcmTileValues = 4096;                                   // values per tile at most: 16 KiB of LDS as 4-byte samples
constexpr uint32_t kPcmImageDwords = kPcmTileValues + 4;                    // the image: the values, the phase in front, one lane's run behind

// Samples of each channel per tile: a multiple of 4, so that a tile's packed bytes are a multiple of 12 (every tile of a frame
// starts at the frame's own phase mod 4) -- 2048 for stereo, 16 for 255 channels.
SELA_PCM_HD uint32_t pcm_tile_samples(uint32_t channels)
{
    const uint32_t t = (kPcmTileValues / channels) & ~3u;
    return t < 4 ? 4 : t;
}
SELA_PCM_HD uint32_t pcm_tiles(uint32_t samples, uint32_t channels)
{
    const uint32_t t = pcm_tile_samples(channels);
    return (samples + t - 1) / t;
}
// dwords a lane moves per access on the packed side: 12 bytes are four 3-byte samples, 16 bytes four 4-byte ones
SELA_PCM_HD uint32_t pcm_lane_dwords(uint32_t bytes_per_sample) { return bytes_per_sample; }

// The planar side of a tile, both kernels: item j of items() is up to four consecutive samples of one channel -- consecutive
// items are consecutive runs of a channel, so a wave's accesses are contiguous.
struct PcmItem {
    uint32_t c, s, count; // channel; first sample (in the frame); 1..4 samples
};

struct PcmTile {
    uint32_t s0, s1;   // the tile's samples of every channel, [s0, s1)
    uint32_t channels;
    uint32_t groups;   // runs of four per channel
    uint64_t a0;       // packed side: the byte the image's byte 0 stands for (a multiple of 4)
    uint32_t p;        // the image byte of value s0 * channels (0..3: the tile's phase)
    uint32_t bytes;    // of the tile's values
    SELA_PCM_HD uint32_t items() const { return channels * groups; }
    SELA_PCM_HD uint32_t rest() const { return (s1 - s0) & 3; } // samples of each channel behind its last whole run of four
    SELA_PCM_HD PcmItem item(uint32_t j) const
    {
        PcmItem it;
        it.c = j / groups;
        it.s = s0 + 4 * (j - it.c * groups);
        it.count = s1 - it.s < 4 ? s1 - it.s : 4;
        return it;
    }
    // the image byte at which sample s of channel c starts
    SELA_PCM_HD uint32_t at(uint32_t c, uint32_t s, uint32_t bytes_per_sample) const { return p + ((s - s0) * channels + c) * bytes_per_sample; }
};

// frame_byte0: where the frame's first value lies on the packed side; n: the frame's samples per channel
SELA_PCM_HD PcmTile pcm_tile(uint64_t frame_byte0, uint32_t tile, uint32_t n, uint32_t channels, uint32_t bytes_per_sample)
{
    const uint32_t t = pcm_tile_samples(channels);
    PcmTile k;
    k.s0 = tile * t;
    k.s1 = n - k.s0 < t ? n : k.s0 + t;
    k.channels = channels;
    k.groups = (k.s1 - k.s0 + 3) / 4;
    const uint64_t b0 = frame_byte0 + (uint64_t)k.s0 * channels * bytes_per_sample;
    k.a0 = b0 & ~(uint64_t)3;
    k.p = (uint32_t)(b0 - k.a0);
    k.bytes = (k.s1 - k.s0) * channels * bytes_per_sample;
    return k;
}

// k_pcm_unpack's loads: the aligned dwords that hold at least one byte of the tile, image dwords [0, dwords): the first
// `runs` * lane_dwords of them as one run per lane, the rest one dword per lane.
struct PcmLoadPlan {
    uint32_t dwords, runs;
};
SELA_PCM_HD PcmLoadPlan pcm_load_plan(const PcmTile& k, uint32_t bytes_per_sample)
{
    PcmLoadPlan l;
    l.dwords = (k.p + k.bytes + 3) / 4;
    l.runs = l.dwords / pcm_lane_dwords(bytes_per_sample);
    return l;
}

// k_pcm_pack's stores.  A workgroup OWNS the bytes [own0, own1) of the packed side: its tile's, with every boundary between two
// tiles of a frame moved down to a multiple of 4 (the dword that straddles it belongs to the later tile, which therefore also
// forms the bytes of the value in front of its own: `lead`).  So only a frame's two ends are ever stored by bytes -- `head` bytes
// up to the first multiple of 4, `tail` bytes behind the last -- and what lies between goes out as whole dwords, the first
// `runs` * lane_dwords of them one run per lane.  All positions are image bytes.
struct PcmStorePlan {
    uint32_t lead;                // 1: the image also holds the trailing bytes of value s0 * channels - 1, in front of p
    uint32_t head_at, head;       // bytes stored singly
    uint32_t mid_at, dwords, runs; // whole dwords (mid_at is a multiple of 4)
    uint32_t tail_at, tail;       // bytes stored singly
};
SELA_PCM_HD PcmStorePlan pcm_store_plan(const PcmTile& k, uint32_t n, uint32_t bytes_per_sample)
{
    PcmStorePlan s;
    s.lead = k.s0 != 0 && k.p != 0 ? 1u : 0u;
    const uint32_t own0 = k.s0 == 0 ? k.p : 0u;
    const uint32_t end = k.p + k.bytes, own1 = k.s1 == n ? end : end & ~3u;
    const uint32_t up = (own0 + 3) & ~3u;
    s.head_at = own0;
    s.head = (up < own1 ? up : own1) - own0;
    s.mid_at = own0 + s.head;
    s.dwords = (own1 - s.mid_at) / 4;
    s.runs = s.dwords / pcm_lane_dwords(bytes_per_sample);
    s.tail_at = s.mid_at + 4 * s.dwords;
    s.tail = own1 - s.tail_at;
    return s;
}

// a sample from the two aligned image dwords around it (lo holds its first byte at byte `shift` = at & 3): align-byte, then the
// sign extension of a 3-byte sample
SELA_PCM_HD int32_t pcm_extract(uint32_t lo, uint32_t hi, uint32_t shift, uint32_t bytes_per_sample)
{
    const uint32_t v = shift ? (lo >> (8 * shift)) | (hi << (32 - 8 * shift)) : lo;
    return bytes_per_sample == 3 ? (int32_t)(v << 8) >> 8 : (int32_t)v;
}

// k_verify_pcm's view of an original frame (sela_verify_pcm.hip): a buffer of pcm_samples samples per channel, a
// frame said to run from sample so0 to so1 -- by a header walk that may have broken: anything, so1 < so0 too.  The frame's
// length is clamped to stride and its start to pcm_samples before anything is addressed: [so, so + n) lies inside the buffer.
struct PcmHeld {
    uint64_t so; // the frame's first sample, at most pcm_samples
    uint32_t n;  // the samples of each channel the buffer holds of it: min(so1 - so0, stride, pcm_samples - so)
};
SELA_PCM_HD PcmHeld pcm_held_frame(uint64_t so0, uint64_t so1, uint32_t stride, uint64_t pcm_samples)
{
    PcmHeld h;
    h.so = so0 < pcm_samples ? so0 : pcm_samples;
    uint64_t n = so1 - so0; // (mod 2^64)
    n = n < stride ? n : stride;
    const uint64_t left = pcm_samples - h.so;
    h.n = (uint32_t)(n < left ? n : left);
    return h;
}

} // namespace sela
#endif
