// wav_probe.cpp -- file::probeWav (host/src/wide.cpp) on WAV headers written here: what it accepts, what it says of each, and the
// message of every refusal.  A stand-alone program; tests/test_pcm_cpu.py builds it with -fsanitize=address,undefined and runs it
// in a scratch directory (argv[1]).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "sela_host/wide.hpp"

namespace {

int g_failures = 0;
std::string g_dir;

void le(std::vector<uint8_t>& v, uint32_t x, int bytes)
{
    for (int b = 0; b < bytes; b++)
        v.push_back((uint8_t)(x >> (8 * b)));
}
void tag(std::vector<uint8_t>& v, const char* t) { v.insert(v.end(), t, t + 4); }

struct Fmt {
    uint16_t format = 1, channels = 2, bits = 16, valid = 0;
    uint32_t rate = 44100;
    int body = 16;      // bytes of the chunk's body actually written (16, 18, 40, or something between for a truncated one)
    bool pcmGuid = true;
};

std::vector<uint8_t> fmtChunk(const Fmt& f)
{
    std::vector<uint8_t> b;
    le(b, f.format, 2), le(b, f.channels, 2), le(b, f.rate, 4), le(b, f.rate * f.channels * f.bits / 8, 4), le(b, f.channels * f.bits / 8u, 2), le(b, f.bits, 2);
    le(b, 22, 2), le(b, f.valid, 2), le(b, 3, 4);
    const uint8_t pcm[16] = { 0x01, 0x00, 0x00, 0x00, 0x00, 0x00, 0x10, 0x00, 0x80, 0x00, 0x00, 0xAA, 0x00, 0x38, 0x9B, 0x71 };
    const uint8_t flt[16] = { 0x03, 0x00, 0x00, 0x00, 0x00, 0x00, 0x10, 0x00, 0x80, 0x00, 0x00, 0xAA, 0x00, 0x38, 0x9B, 0x71 };
    b.insert(b.end(), f.pcmGuid ? pcm : flt, (f.pcmGuid ? pcm : flt) + 16);
    b.resize((size_t)f.body);
    std::vector<uint8_t> c;
    tag(c, "fmt "), le(c, (uint32_t)f.body, 4);
    c.insert(c.end(), b.begin(), b.end());
    return c;
}

std::vector<uint8_t> dataChunk(size_t bytes, uint8_t fill)
{
    std::vector<uint8_t> c;
    tag(c, "data"), le(c, (uint32_t)bytes, 4);
    c.insert(c.end(), bytes, fill);
    return c;
}

std::string writeWav(const char* name, const std::vector<std::vector<uint8_t>>& chunks)
{
    std::vector<uint8_t> body;
    for (const auto& c : chunks)
        body.insert(body.end(), c.begin(), c.end());
    std::vector<uint8_t> file;
    tag(file, "RIFF"), le(file, (uint32_t)(4 + body.size()), 4), tag(file, "WAVE");
    file.insert(file.end(), body.begin(), body.end());
    const std::string path = g_dir + "/" + name;
    std::ofstream(path, std::ios::binary).write(reinterpret_cast<const char*>(file.data()), (std::streamsize)file.size());
    return path;
}

void accept(const char* name, const std::vector<std::vector<uint8_t>>& chunks, uint16_t bits, uint16_t valid, uint16_t channels, bool extensible, uint64_t offset,
    uint64_t bytes)
{
    try {
        const file::WavProbe p = file::probeWav(writeWav(name, chunks));
        const bool ok = p.bitsPerSample == bits && p.validBits == valid && p.channels == channels && p.sampleRate == 44100 && p.extensible == extensible
            && p.dataOffset == offset && p.dataBytes == bytes;
        if (!ok) {
            g_failures++;
            std::printf("FAIL %s: bits %u valid %u channels %u rate %u extensible %d data %llu + %llu\n", name, p.bitsPerSample, p.validBits, p.channels, p.sampleRate,
                (int)p.extensible, (unsigned long long)p.dataOffset, (unsigned long long)p.dataBytes);
        }
    } catch (const data::Exception& e) {
        g_failures++;
        std::printf("FAIL %s: refused: %s\n", name, e.exceptionMessage.c_str());
    }
}

void refuse(const char* name, const std::vector<std::vector<uint8_t>>& chunks, const char* message)
{
    try {
        (void)file::probeWav(writeWav(name, chunks));
        g_failures++;
        std::printf("FAIL %s: accepted\n", name);
    } catch (const data::Exception& e) {
        if (e.exceptionMessage != message) {
            g_failures++;
            std::printf("FAIL %s: \"%s\", not \"%s\"\n", name, e.exceptionMessage.c_str(), message);
        }
    }
}

} // namespace

int main(int argc, char** argv)
{
    g_dir = argc > 1 ? argv[1] : ".";
    Fmt f;
    // plain 16 / 24 / 32: the data behind the 12-byte RIFF head and the 24-byte fmt chunk, 8 bytes of chunk head in
    for (uint16_t bits : { 16, 24, 32 }) {
        f = Fmt(), f.bits = bits;
        accept(("plain" + std::to_string(bits) + ".wav").c_str(), { fmtChunk(f), dataChunk(96, 1) }, bits, bits, 2, false, 44, 96);
    }
    f = Fmt(), f.bits = 24, f.channels = 5;
    accept("five.wav", { fmtChunk(f), dataChunk(150, 1) }, 24, 24, 5, false, 44, 150);
    // extensible, 24 in 24 and 20 in 24
    f = Fmt(), f.format = 0xFFFE, f.bits = 24, f.valid = 24, f.body = 40;
    accept("ext24.wav", { fmtChunk(f), dataChunk(96, 2) }, 24, 24, 2, true, 68, 96);
    f.valid = 20;
    accept("ext20.wav", { fmtChunk(f), dataChunk(96, 2) }, 24, 20, 2, true, 68, 96);
    // two data chunks: the last wins; an odd chunk between
    f = Fmt(), f.bits = 24;
    std::vector<uint8_t> list;
    tag(list, "LIST"), le(list, 6, 4), list.insert(list.end(), 6, 0x55);
    accept("two_data.wav", { fmtChunk(f), dataChunk(12, 3), list, dataChunk(60, 4) }, 24, 24, 2, false, 12 + 24 + 20 + 14 + 8, 60);
    // fmt behind data
    accept("fmt_behind_data.wav", { dataChunk(60, 5), fmtChunk(f) }, 24, 24, 2, false, 20, 60);
    // fmt twice, the second behind the data: the later one describes the file, the data stays the one found
    Fmt g = Fmt();
    g.bits = 32;
    accept("fmt_again_behind_data.wav", { fmtChunk(f), dataChunk(48, 6), fmtChunk(g) }, 32, 32, 2, false, 44, 48);
    // a data chunk that says more than the file holds is clipped
    std::vector<uint8_t> longData = dataChunk(40, 7);
    longData[4] = 0xFF, longData[5] = 0xFF;
    accept("clipped.wav", { fmtChunk(f), longData }, 24, 24, 2, false, 44, 40);

    // the refusals
    f = Fmt(), f.format = 3, f.bits = 32;
    refuse("float.wav", { fmtChunk(f), dataChunk(64, 0) }, "Only PCM wav is supported (audioFormat 3 is float).");
    f = Fmt(), f.bits = 8;
    refuse("eight.wav", { fmtChunk(f), dataChunk(64, 0) }, "Only 16, 24 and 32bits per sample wav is supported.");
    f = Fmt(), f.bits = 20;
    refuse("twenty_packed.wav", { fmtChunk(f), dataChunk(64, 0) }, "Only 16, 24 and 32bits per sample wav is supported.");
    f = Fmt(), f.format = 0xFFFE, f.bits = 24, f.valid = 24, f.body = 24;
    refuse("ext_truncated.wav", { fmtChunk(f), dataChunk(64, 0) }, "Only PCM wav is supported (an extensible fmt subChunk needs 40 bytes).");
    f.body = 40, f.pcmGuid = false;
    refuse("ext_float.wav", { fmtChunk(f), dataChunk(64, 0) }, "Only PCM wav is supported (the extensible subformat is not PCM).");
    f = Fmt(), f.format = 6;
    refuse("alaw.wav", { fmtChunk(f), dataChunk(64, 0) }, "Only PCM wav is supported.");
    refuse("no_fmt.wav", { list, list, list, list }, "fmt subChunk is missing from file");
    f = Fmt(), f.bits = 24;
    refuse("no_data.wav", { fmtChunk(f), list }, "data subChunk is missing from file");
    refuse("small.wav", { list }, "File is too small, probably not a wav file.");

    if (g_failures) {
        std::printf("wav_probe: %d failures\n", g_failures);
        return 1;
    }
    std::printf("wav_probe ok\n");
    return 0;
}
