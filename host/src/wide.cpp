// wide.cpp -- 24- and 32-bit WAV files to and from .sela (see wide.hpp).  The containers are written here as files.cpp writes
// them (the canonical 44-byte PCM header of src/file/wav_file.cpp:224-243, the 15-byte .sela header of src/file/sela_file.cpp:
// 40-50 with the file's own bitsPerSample); the samples never leave their packed form on the host.
#include "sela_host/wide.hpp"

#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <vector>

#include "sela_hip.h"
#include "sela_host/buffer.hpp"

namespace {

uint16_t le16(const uint8_t* p) { return (uint16_t)(p[0] | (p[1] << 8)); }
uint32_t le32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
void put16(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v, p[1] = (uint8_t)(v >> 8); }
void put32(uint8_t* p, uint32_t v) { put16(p, v), put16(p + 2, v >> 16); }

bool readExact(std::ifstream& in, void* dst, size_t n)
{
    in.read(static_cast<char*>(dst), (std::streamsize)n);
    return (size_t)in.gcount() == n;
}

// KSDATAFORMAT_SUBTYPE_PCM: 00000001-0000-0010-8000-00AA00389B71
const uint8_t kPcmSubformat[16] = { 0x01, 0x00, 0x00, 0x00, 0x00, 0x00, 0x10, 0x00, 0x80, 0x00, 0x00, 0xAA, 0x00, 0x38, 0x9B, 0x71 };
constexpr uint32_t kFrameSamples = 2048;

[[noreturn]] void failHip(const char* what) { throw data::Exception(std::string(what) + ": " + sela_hip_last_error()); }

} // namespace

namespace file {

WavProbe probeWav(const std::string& path)
{
    std::ifstream in(path, std::ios::binary);
    if (!in)
        throw data::Exception("cannot open " + path);
    in.seekg(0, std::ios::end);
    const std::streamoff end = in.tellg();
    const uint64_t size = end > 0 ? (uint64_t)end : 0;
    in.seekg(0, std::ios::beg);
    if (size < 44)
        throw data::Exception("File is too small, probably not a wav file.");
    uint8_t riff[12];
    if (!readExact(in, riff, 12) || std::memcmp(riff, "RIFF", 4) != 0)
        throw data::Exception("chunkId is not RIFF, probably not a wav file.");
    if ((uint64_t)le32(riff + 4) > size)
        throw data::Exception("chunkSize exceeds file size, probably a corrupted file");
    if (std::memcmp(riff + 8, "WAVE", 4) != 0)
        throw data::Exception("format is not WAVE, probably not a wav file.");
    WavProbe p;
    bool haveFmt = false, haveData = false;
    uint64_t pos = 12;
    while (pos + 8 <= size) {
        uint8_t head[8];
        in.seekg((std::streamoff)pos, std::ios::beg);
        if (!readExact(in, head, 8))
            break;
        uint64_t chunk = le32(head + 4);
        if (pos + 8 + chunk > size)
            chunk = size - pos - 8; // tolerate a short last chunk
        if (std::memcmp(head, "fmt ", 4) == 0 && chunk >= 16) {
            uint8_t body[40] = {};
            const size_t have = (size_t)std::min<uint64_t>(chunk, 40);
            if (!readExact(in, body, have))
                break;
            const uint16_t tag = le16(body);
            p.channels = le16(body + 2);
            p.sampleRate = le32(body + 4);
            p.bitsPerSample = p.validBits = le16(body + 14);
            p.extensible = tag == 0xFFFE;
            if (tag == 3)
                throw data::Exception("Only PCM wav is supported (audioFormat 3 is float).");
            if (p.extensible) {
                if (have < 40)
                    throw data::Exception("Only PCM wav is supported (an extensible fmt subChunk needs 40 bytes).");
                if (std::memcmp(body + 24, kPcmSubformat, 16) != 0)
                    throw data::Exception("Only PCM wav is supported (the extensible subformat is not PCM).");
                p.validBits = le16(body + 18);
            } else if (tag != 1) {
                throw data::Exception("Only PCM wav is supported.");
            }
            if (p.bitsPerSample != 16 && p.bitsPerSample != 24 && p.bitsPerSample != 32)
                throw data::Exception("Only 16, 24 and 32bits per sample wav is supported.");
            haveFmt = true;
        } else if (std::memcmp(head, "data", 4) == 0) {
            haveData = true; // ('fmt ' may stand behind it: the format is asked for only once the walk is over)
            p.dataOffset = pos + 8;
            p.dataBytes = chunk;
        }
        pos += 8 + chunk;
    }
    if (!haveFmt)
        throw data::Exception("fmt subChunk is missing from file");
    if (!haveData)
        throw data::Exception("data subChunk is missing from file");
    return p;
}

} // namespace file

namespace sela {

WideReport encodeWideFile(const std::string& in, const std::string& out, bool lossless, bool keepTail)
{
    const file::WavProbe p = file::probeWav(in);
    if (p.bitsPerSample != 24 && p.bitsPerSample != 32)
        throw data::Exception("encodeWideFile takes 24- and 32-bit wav (16-bit: encodeFile)");
    if (p.channels == 0 || p.channels > 255)
        throw data::Exception("a .sela file holds 1 to 255 channels");
    const uint32_t bytes = p.bitsPerSample / 8u;
    // keepTail: the whole data chunk, the layout sela_hip_whole_frames gives it
    const uint64_t samples = p.dataBytes / ((uint64_t)p.channels * bytes), frames64 = keepTail ? sela_hip_whole_frames(samples) : samples / kFrameSamples;
    if (frames64 >= (1ull << 31))
        throw data::Exception("the file holds too many frames");
    WideReport report;
    report.frames = (uint32_t)frames64;
    const uint64_t coded = keepTail ? samples : frames64 * kFrameSamples; // samples per channel that go into the stream
    report.droppedSamples = samples - coded;
    sela_host::PinnedBuffer<uint8_t> pcm((size_t)(coded * p.channels * bytes));
    std::ifstream file(in, std::ios::binary);
    file.seekg((std::streamoff)p.dataOffset, std::ios::beg);
    if (!pcm.empty() && !readExact(file, pcm.data(), pcm.size()))
        throw data::Exception("data subChunk is shorter than its header says");
    std::vector<uint64_t> offsets((size_t)report.frames + 1, 0);
    sela_host::PinnedBuffer<uint8_t> stream;
    // room by the estimate the library's own chunks use (4.5 bytes a sample); the certain bound only for a file that needs it
    const size_t estimate = ((size_t)coded * p.channels * 9) / 2 + (size_t)report.frames * ((size_t)p.channels * 192 + 64);
    const size_t rooms[2] = { estimate, keepTail ? sela_hip_encode_whole_pcm_bound_bytes(samples, p.channels, bytes)
                                                 : sela_hip_encode_pcm_bound_bytes(report.frames, p.channels, kFrameSamples, bytes) };
    const uint32_t options = lossless ? SELA_HIP_ENCODE_LOSSLESS : 0u;
    for (size_t room : rooms) {
        stream.resize(std::max<size_t>(room, 4));
        const int rc = keepTail ? sela_hip_encode_whole_pcm(pcm.data(), bytes, samples, p.channels, options, stream.data(), stream.size(), offsets.data())
                                : sela_hip_encode_pcm(pcm.data(), bytes, report.frames, p.channels, kFrameSamples, options, stream.data(), stream.size(), offsets.data());
        if (rc == SELA_HIP_OK)
            break;
        if (rc != SELA_HIP_ECAPACITY || room == rooms[1])
            failHip("Encoder");
    }
    uint8_t header[15];
    std::memcpy(header, "SeLa", 4);
    put32(header + 4, p.sampleRate);
    put16(header + 8, p.bitsPerSample);
    header[10] = (uint8_t)p.channels;
    put32(header + 11, report.frames);
    std::ofstream o(out, std::ios::binary | std::ios::trunc);
    if (!o)
        throw data::Exception("cannot open " + out + " for writing");
    o.write(reinterpret_cast<const char*>(header), 15);
    o.write(reinterpret_cast<const char*>(stream.data()), (std::streamsize)offsets[report.frames]);
    if (!o)
        throw data::Exception("cannot write " + out);
    return report;
}

uint16_t selaFileBits(const std::string& path)
{
    std::ifstream in(path, std::ios::binary);
    uint8_t head[15];
    if (!in || !readExact(in, head, 15) || std::memcmp(head, "SeLa", 4) != 0)
        return 0;
    return le16(head + 8);
}

namespace {

// A .sela file of 24- or 32-bit samples as decodeWideFile and decodeWideFileRange read it: the header's fields, the payload in
// page-locked memory and the frames as SelaFile::readFromFile finds them -- the header's count is not trusted for sizing, the walk
// stops at the first frame without a sync word.
struct WideSela {
    uint32_t rate = 0, bits = 0, channels = 0, found = 0;
    sela_host::PinnedBuffer<uint8_t> stream;
    std::vector<uint64_t> offsets;
};

void readWideSela(const std::string& in, const char* who, WideSela& s)
{
    std::ifstream file(in, std::ios::binary);
    if (!file)
        throw data::Exception("cannot open " + in);
    file.seekg(0, std::ios::end);
    const std::streamoff end = file.tellg();
    file.seekg(0, std::ios::beg);
    uint8_t head[15];
    if (end < 15 || !readExact(file, head, 15))
        throw data::Exception("File is too small, probably not a sela file.");
    if (std::memcmp(head, "SeLa", 4) != 0)
        throw data::Exception("Magic number is incorrect, probably not a sela file.");
    s.rate = le32(head + 4), s.bits = le16(head + 8), s.channels = head[10];
    const uint32_t numFrames = le32(head + 11);
    if (s.bits != 24 && s.bits != 32)
        throw data::Exception(std::string(who) + " takes .sela files of 24- and 32-bit samples (16-bit: decodeFile)");
    if (s.channels == 0)
        throw data::Exception("the .sela header says no channels");
    s.stream.resize((size_t)(end - 15));
    if (!s.stream.empty() && !readExact(file, s.stream.data(), s.stream.size()))
        throw data::Exception("File is too small, probably not a sela file.");
    const size_t least = 4 + 12 * (size_t)s.channels;
    const uint32_t plausible = (uint32_t)std::min<size_t>(numFrames, s.stream.size() / least);
    s.offsets.assign((size_t)plausible + 1, 0);
    s.found = sela_hip_index_frames(s.stream.data(), s.stream.size(), plausible, s.channels, s.offsets.data());
    s.offsets.resize((size_t)s.found + 1);
}

// the canonical 44-byte PCM header and the data chunk
void writeWideWav(const std::string& out, const WideSela& s, const uint8_t* pcm, uint64_t dataBytes)
{
    const uint32_t bytes = s.bits / 8u;
    uint8_t wav[44];
    std::memcpy(wav, "RIFF", 4);
    put32(wav + 4, 36 + (uint32_t)dataBytes);
    std::memcpy(wav + 8, "WAVEfmt ", 8);
    put32(wav + 16, 16);
    put16(wav + 20, 1); // PCM
    put16(wav + 22, s.channels);
    put32(wav + 24, s.rate);
    put32(wav + 28, s.rate * s.channels * bytes);
    put16(wav + 32, s.channels * bytes);
    put16(wav + 34, s.bits);
    std::memcpy(wav + 36, "data", 4);
    put32(wav + 40, (uint32_t)dataBytes);
    std::ofstream o(out, std::ios::binary | std::ios::trunc);
    if (!o)
        throw data::Exception("cannot open " + out + " for writing");
    o.write(reinterpret_cast<const char*>(wav), 44);
    o.write(reinterpret_cast<const char*>(pcm), (std::streamsize)dataBytes);
    if (!o)
        throw data::Exception("cannot write " + out);
}

} // namespace

WideReport decodeWideFile(const std::string& in, const std::string& out)
{
    WideSela s;
    readWideSela(in, "decodeWideFile", s);
    const uint32_t channels = s.channels, bytes = s.bits / 8u, found = s.found;
    std::vector<uint64_t> sampleOffsets((size_t)found + 1, 0);
    if (found && sela_hip_index_samples(s.stream.data(), s.offsets.data(), found, channels, sampleOffsets.data()) == 0)
        throw data::Exception("Decoder: malformed frame stream");
    const uint64_t dataBytes = sampleOffsets[found] * channels * bytes;
    if (dataBytes > 0xFFFFFFFFull - 36)
        throw data::Exception("the samples do not fit a wav file");
    WideReport report;
    report.frames = found;
    sela_host::PinnedBuffer<uint8_t> pcm((size_t)std::max<uint64_t>(dataBytes, 4));
    if (found && sela_hip_decode_pcm(s.stream.data(), s.offsets.data(), found, channels, bytes, pcm.data(), (size_t)dataBytes, &report.wideSamples) != SELA_HIP_OK)
        failHip("Decoder");
    writeWideWav(out, s, pcm.data(), dataBytes);
    return report;
}

// A range of a wide file's samples: the range is one window of the whole stream (sela_hip_decode_windows_i32_whole copies and decodes the
// frames it touches and no others; a range longer than the call's 2^24 samples goes in pieces of that length), in the file's
// own packed layout.  Nothing is created before the samples are there.
size_t decodeWideFileRange(const std::string& in, const std::string& out, uint64_t startSample, uint64_t sampleCount)
{
    WideSela s;
    readWideSela(in, "decodeWideFileRange", s);
    const uint32_t channels = s.channels, bytes = s.bits / 8u;
    // the stream's length by what its frames say (a whole-track stream ends in a frame of 1 .. 4095 samples)
    std::vector<uint64_t> sampleOffsets((size_t)s.found + 1, 0);
    if (s.found && sela_hip_index_samples(s.stream.data(), s.offsets.data(), s.found, channels, sampleOffsets.data()) == 0)
        throw data::Exception("Decode: malformed frame stream");
    const uint64_t streamSamples = sampleOffsets[s.found];
    if (startSample >= streamSamples)
        throw data::Exception("Decode: --start " + std::to_string(startSample) + " is at or past the end of the stream (" + std::to_string(streamSamples)
            + " samples per channel)");
    const uint64_t count = std::min(sampleCount, streamSamples - startSample);
    const uint64_t dataBytes = count * channels * bytes;
    if (dataBytes > 0xFFFFFFFFull - 36)
        throw data::Exception("the samples do not fit a wav file");
    std::vector<uint8_t> pcm((size_t)std::max<uint64_t>(dataBytes, 4));
    const uint64_t piece = (uint64_t)1 << 24;
    for (uint64_t done = 0; done < count; done += piece) {
        const sela_hip_window window = { startSample + done, 0, s.found };
        if (sela_hip_decode_windows_i32_whole(s.stream.data(), s.offsets.data(), s.found, channels, &window, 1, (uint32_t)std::min(piece, count - done),
                bytes == 3 ? SELA_HIP_WINDOW_PCM24_INTERLEAVED : SELA_HIP_WINDOW_PCM32_INTERLEAVED, s.bits, pcm.data() + (size_t)(done * channels * bytes), nullptr)
            != SELA_HIP_OK)
            failHip("Decode");
    }
    writeWideWav(out, s, pcm.data(), dataBytes);
    return (size_t)count;
}

// ---- levels --------------------------------------------------------------------------------------------------
static_assert(sizeof(LevelRecord32) == sizeof(sela_hip_level32) && offsetof(LevelRecord32, samples) == offsetof(sela_hip_level32, samples)
        && offsetof(LevelRecord32, sum) == offsetof(sela_hip_level32, sum) && offsetof(LevelRecord32, sumSquaresLo) == offsetof(sela_hip_level32, sum_squares_lo)
        && offsetof(LevelRecord32, sumSquaresHi) == offsetof(sela_hip_level32, sum_squares_hi),
    "levels.hpp restates the device's record");

WideLevelReport measureWideFile(const std::string& selaPath)
{
    WideSela s;
    readWideSela(selaPath, "measureWideFile", s);
    WideLevelReport r;
    r.channels = s.channels, r.sampleRate = s.rate, r.bitsPerSample = s.bits;
    std::vector<sela_hip_level32> levels((size_t)s.found * s.channels + 1);
    if (sela_hip_levels_i32(s.stream.data(), s.offsets.data(), s.found, s.channels, levels.data()) != SELA_HIP_OK)
        failHip("Measure");
    r.frames = s.found;
    r.perChannel = foldChannels(reinterpret_cast<const LevelRecord32*>(levels.data()), s.found, s.channels);
    for (uint32_t f = 0; f < s.found; f++) {
        bool silent = true;
        for (uint32_t c = 0; c < s.channels; c++)
            silent = silent && levels[(size_t)f * s.channels + c].peak == 0;
        r.silentFrames += silent ? 1 : 0;
    }
    for (const ChannelLevelWide& c : r.perChannel)
        fold(r.track, c);
    return r;
}

// ---- envelope ------------------------------------------------------------------------------------------------
static_assert(sizeof(EnvelopeRecord32) == sizeof(struct sela_hip_envelope32) && offsetof(EnvelopeRecord32, max) == offsetof(struct sela_hip_envelope32, max)
        && offsetof(EnvelopeRecord32, sum) == offsetof(struct sela_hip_envelope32, sum)
        && offsetof(EnvelopeRecord32, sumSquaresLo) == offsetof(struct sela_hip_envelope32, sum_squares_lo)
        && offsetof(EnvelopeRecord32, sumSquaresHi) == offsetof(struct sela_hip_envelope32, sum_squares_hi),
    "envelope.hpp restates the device's record");

EnvelopeReport32 envelopeWideFile(const std::string& selaPath, uint32_t bucket)
{
    if (!envelopeBucketOk(bucket))
        throw data::Exception(envelopeBucketRefusal(bucket));
    WideSela s;
    readWideSela(selaPath, "envelopeWideFile", s);
    EnvelopeReport32 r;
    r.channels = s.channels, r.bucket = bucket, r.sampleRate = s.rate, r.bitsPerSample = s.bits;
    std::vector<uint64_t> sampleOffsets((size_t)s.found + 1, 0);
    uint32_t largest = 0;
    if (s.found && (largest = sela_hip_index_samples(s.stream.data(), s.offsets.data(), s.found, s.channels, sampleOffsets.data())) == 0)
        throw data::Exception("Envelope: malformed frame stream");
    const uint32_t stride = std::max(largest, 1u);
    const uint32_t slots = envelopeSlots(stride, bucket);
    std::vector<EnvelopeRecord32> records((size_t)s.found * slots * s.channels + 1);
    if (sela_hip_envelope_i32(s.stream.data(), s.offsets.data(), s.found, s.channels, stride, bucket, reinterpret_cast<struct sela_hip_envelope32*>(records.data()))
        != SELA_HIP_OK)
        failHip("Envelope");
    r.samplesPerChannel = sampleOffsets[s.found];
    try {
        r.records = compactEnvelope32(records.data(), sampleOffsets.data(), s.found, slots, s.channels, bucket);
    } catch (const std::invalid_argument& e) {
        throw data::Exception(e.what());
    }
    return r;
}

EnvelopeReport32 writeEnvelopeWideFile(const std::string& selaPath, const std::string& envPath, uint32_t bucket)
{
    const EnvelopeReport32 r = envelopeWideFile(selaPath, bucket);
    const std::vector<uint8_t> bytes = envelopeFileBytes32(r);
    std::ofstream o(envPath, std::ios::binary | std::ios::trunc);
    if (!o)
        throw data::Exception("cannot open " + envPath + " for writing");
    o.write(reinterpret_cast<const char*>(bytes.data()), (std::streamsize)bytes.size());
    if (!o)
        throw data::Exception("cannot write " + envPath);
    return r;
}

// ---- digest --------------------------------------------------------------------------------------------------
DigestReport digestWideFile(const std::string& selaPath, const std::string& wavPath)
{
    WideSela s;
    readWideSela(selaPath, "digestWideFile", s);
    const uint32_t channels = s.channels, bytes = s.bits / 8u;
    DigestReport r;
    r.channels = channels;
    if (sela_hip_digest_pcm(s.stream.data(), s.offsets.data(), s.found, channels, bytes, nullptr, &r.crc32, &r.bytes, &r.wideSamples) != SELA_HIP_OK)
        failHip("Digest");
    r.frames = s.found;
    if (wavPath.empty())
        return r;
    const file::WavProbe wav = file::probeWav(wavPath);
    if (wav.bitsPerSample != s.bits)
        throw data::Exception("Digest: the .wav holds " + std::to_string(wav.bitsPerSample) + "-bit samples, the .sela " + std::to_string(s.bits)
            + "-bit samples: files of different widths are not held against each other");
    if (wav.channels != channels)
        throw data::Exception("Digest: " + std::to_string(wav.channels) + " channels in the .wav, " + std::to_string(channels) + " in the .sela");
    // the part of the data chunk the .sela can hold: whole samples, and no more of them than its frames have
    const uint64_t sampleBytes = (uint64_t)channels * bytes;
    r.haveWav = true;
    r.wavBytes = std::min<uint64_t>(wav.dataBytes / sampleBytes * sampleBytes, r.bytes);
    r.wavTailBytes = wav.dataBytes - r.wavBytes;
    Crc32 crc;
    std::vector<uint8_t> piece((size_t)std::min<uint64_t>(r.wavBytes, (uint64_t)4 << 20) + 8);
    std::ifstream file(wavPath, std::ios::binary);
    file.seekg((std::streamoff)wav.dataOffset, std::ios::beg);
    for (uint64_t at = 0; at < r.wavBytes;) {
        const size_t n = (size_t)std::min<uint64_t>(r.wavBytes - at, (uint64_t)4 << 20);
        if (!readExact(file, piece.data(), n))
            throw data::Exception("data subChunk is shorter than its header says");
        crc.update(piece.data(), n);
        at += n;
    }
    r.wavCrc32 = crc.value();
    return r;
}

namespace {
std::string wideLevelFigures(const ChannelLevelWide& l, double scale)
{
    char figures[128];
    std::snprintf(figures, sizeof(figures), " peak_dbfs=%.2f rms_dbfs=%.2f dc=%.4f", peakDbfs(l, scale), rmsDbfs(l, scale), dcOffset(l));
    return "peak=" + std::to_string(l.peak) + " samples=" + std::to_string(l.samples) + " sum=" + std::to_string(l.sum) + " sum_squares=" + energyDecimal(l) + figures;
}
} // namespace

std::string formatLevelReport(const WideLevelReport& r)
{
    const double scale = fullScale(r.bitsPerSample);
    std::string out;
    for (size_t c = 0; c < r.perChannel.size(); c++)
        out += "channel " + std::to_string(c) + ": " + wideLevelFigures(r.perChannel[c], scale) + "\n";
    out += "track: " + wideLevelFigures(r.track, scale) + " (" + std::to_string(r.frames) + " frames, " + std::to_string(r.silentFrames) + " silent)\n";
    return out;
}

// verifyFile for a 24- or 32-bit pair: the headers held against each other as verifyFile holds them, the frames the .sela really
// holds against the WAV's packed data chunk in ONE sela_hip_verify_pcm call -- pcm_samples is what the WAV holds, so samples the
// .sela has beyond it count as differences of their frames, and the WAV's tail is reported as now.
VerifyReport verifyWideFile(const std::string& wavPath, const std::string& selaPath)
{
    const file::WavProbe wav = file::probeWav(wavPath);
    const uint16_t selaBits = selaFileBits(selaPath);
    if (selaBits != 0 && selaBits != wav.bitsPerSample)
        throw data::Exception("Verify: the .wav holds " + std::to_string(wav.bitsPerSample) + "-bit samples, the .sela " + std::to_string(selaBits)
            + "-bit samples: files of different widths are not held against each other");
    if (wav.bitsPerSample != 24 && wav.bitsPerSample != 32)
        throw data::Exception("verifyWideFile takes 24- and 32-bit wav (16-bit: verifyFile)");
    WideSela s;
    readWideSela(selaPath, "verifyWideFile", s);
    std::ifstream head(selaPath, std::ios::binary);
    uint8_t header[15] = {};
    (void)readExact(head, header, 15);
    const uint32_t channels = s.channels, bytes = s.bits / 8u, found = s.found;
    VerifyReport r;
    r.channels = channels;
    r.wavRate = wav.sampleRate, r.selaRate = s.rate;
    r.wavChannels = wav.channels, r.selaChannels = channels;
    r.rateDiffers = r.wavRate != r.selaRate;
    r.channelsDiffer = r.wavChannels != r.selaChannels;
    r.selaHeaderFrames = le32(header + 11);
    std::vector<uint64_t> sampleOffsets((size_t)found + 1, 0);
    if (found && sela_hip_index_samples(s.stream.data(), s.offsets.data(), found, channels, sampleOffsets.data()) == 0)
        throw data::Exception("Verify: malformed frame stream");
    const uint64_t selaSamples = sampleOffsets[found];
    bool ordinary = true;
    for (uint32_t f = 0; ordinary && f <= found; f++)
        ordinary = sampleOffsets[f] == (uint64_t)f * kFrameSamples;
    const uint64_t wavSamples = wav.channels ? wav.dataBytes / ((uint64_t)wav.channels * bytes) : 0;
    r.selaFrames = found;
    r.wavFrames = wavSamples / kFrameSamples;
    r.frameCountDiffers = r.selaHeaderFrames != found || (ordinary && !r.channelsDiffer && found != r.wavFrames);
    if (r.channelsDiffer)
        return r; // (nothing to hold against each other)
    r.tailSamplesPerChannel = wavSamples > selaSamples ? wavSamples - selaSamples : 0;
    r.missingSamplesPerChannel = selaSamples > wavSamples ? selaSamples - wavSamples : 0;
    const uint64_t held = std::min(wavSamples, selaSamples);
    sela_host::PinnedBuffer<uint8_t> pcm((size_t)std::max<uint64_t>(held * channels * bytes, 4));
    std::ifstream file(wavPath, std::ios::binary);
    file.seekg((std::streamoff)wav.dataOffset, std::ios::beg);
    if (held && !readExact(file, pcm.data(), (size_t)(held * channels * bytes)))
        throw data::Exception("data subChunk is shorter than its header says");
    std::vector<uint32_t> counts((size_t)found + 1), first((size_t)found + 1);
    uint32_t lossy = 0;
    if (sela_hip_verify_pcm(s.stream.data(), s.offsets.data(), found, channels, bytes, pcm.data(), wavSamples, counts.data(), first.data(),
            &lossy)
        != SELA_HIP_OK)
        failHip("Verify");
    r.framesCompared = found;
    for (uint32_t f = 0; f < found; f++)
        if (counts[f])
            r.lossy.push_back({ f, counts[f], first[f] });
    return r;
}

} // namespace sela
