// codec.hpp -- sela::Encoder / sela::Decoder with the reference's signatures
// (src/include/sela/encoder.hpp:9-22, src/include/sela/decoder.hpp:9-22).
//
// Where the reference reads the whole file and then fans the frames out to hardware_concurrency() threads
// (src/sela/encoder.cpp:40-100), these stream the file through the MI355X: the file is read piece by
// piece into page-locked memory and every piece is handed to the GPU (sela_hip_encode_feed /
// sela_hip_decode_feed) while the next one is still being read.  There is no CPU fallback: if the GPU path
// is unavailable process() throws data::Exception.
#pragma once

#include <cstdint>
#include <fstream>
#include <string>
#include <vector>

#include "sela_host/files.hpp"
#include "sela_host/digest.hpp"
#include "sela_host/envelope.hpp"
#include "sela_host/levels.hpp"

namespace sela {

class Encoder {
    std::ifstream& ifStream;
    file::WavFile wavFile;

public:
    // Also build the data::SelaFrame objects in SelaFile::selaFrames (API fidelity).  Tools that only
    // write the file can switch this off: the byte stream is complete without them.
    static bool materializeFrames;
    // Residues against the decoder's rounding (SELA_HIP_ENCODE_LOSSLESS): every frame decodes back exactly,
    // with any decoder of the format.  Off: the reference's stream bit for bit.
    bool lossless = false;
    // Channel pairs (sela_hip_encode_paired): every odd channel may be stored as the difference against the even
    // channel before it, in a stream every decoder of the format reads.  One and two channels: the same bytes either way.
    bool pairChannels = false;
    // The whole file: the samples beyond the last whole 2048-sample frame are folded into a long last frame
    // (2049 .. 4095 samples; a file below 2048 samples is one frame) instead of dropped.  The 2048-sample frames go through the
    // streaming job, the last frame through the one-shot call once the job has ended.  Not with pairChannels (data::Exception).
    bool keepTail = false;
    explicit Encoder(std::ifstream& in) : ifStream(in) {}
    file::SelaFile process();
};

class Decoder {
    std::ifstream& ifStream;
    file::SelaFile selaFile;

public:
    static bool demuxFrames; // also fill WavFile::wavFrames (per-frame de-interleaved copies)
    explicit Decoder(std::ifstream& in) : ifStream(in) {}
    file::WavFile process();
};

// File to file (what the reference's main.cpp:29-41 does with process() + writeToFile()): the same
// streaming read, and finished frames / samples are written out while later pieces are still on the device.
// Return the number of frames coded.
size_t encodeFile(std::ifstream& in, std::ofstream& out, bool lossless = false, bool pairChannels = false,
    bool keepTail = false); // (as Encoder::lossless, ::pairChannels, ::keepTail)
size_t decodeFile(std::ifstream& in, std::ofstream& out);
// The same by path -- what the CLI's -e / -d use: the file is read with several pread()s in flight on a small pool of I/O
// threads (sela_host/fileio.hpp) while earlier pieces are on the device, and finished ranges are written by a task of
// that pool -- over pages allocated in one go while the input was still on its way -- while later pieces are being coded.
// One thread reads or writes a page-cache file at a few GB/s; the device codes 10 G samples/s.
size_t encodeFile(const std::string& inPath, const std::string& outPath, bool lossless = false, bool pairChannels = false, bool keepTail = false);
size_t decodeFile(const std::string& inPath, const std::string& outPath);
// Samples [startSample, startSample + sampleCount) per channel of a .sela of 2048-sample frames, as a WAV of exactly the samples
// delivered: only the frames the range touches are copied to the device and decoded (sela_hip_decode_windows_whole: the long last
// frame of a --keep-tail file is part of the stream).  The count is cut
// at the stream's end; a start at or past the end is a data::Exception, and no file is written then.  Returns the samples per
// channel written.
size_t decodeFileRange(const std::string& selaPath, const std::string& wavPath, uint64_t startSample, uint64_t sampleCount);
// Decoding for a consumer that takes the samples in order (the player, sela_host/player.hpp): begin() once the header is
// known, then ready(pcm, n) -- on the calling thread -- whenever the first n interleaved samples of pcm are final (n only
// grows; pcm is the caller's buffer `into`, sized here before the first call, so the samples outlive the decoding: a player is
// still handing them out long after the last frame was decoded).  Returns the frames decoded.
class DecodedStream {
public:
    virtual ~DecodedStream() {}
    virtual void begin(const data::SelaHeader& header, size_t announcedFrames) = 0;
    virtual void ready(const int16_t* pcm, size_t samples) = 0;
};
size_t decodeFileTo(const std::string& inPath, DecodedStream& to, sela_host::PinnedBuffer<int16_t>& into);
// Threads of that pool (before its first use; 0 = default: min(6, hardware threads / 2)).
void setIoThreads(unsigned n);

// ---- verification: does this .sela give this WAV back? ---------------------------------------------------------------
// The codec reproduces the reference bit for bit, and the reference is not lossless on every frame;
// Encoder::lossless / encodeFile(..., true) avoid that loss;
// the encoder also drops the WAV's samples beyond the last whole 2048-sample frame.  verifyFile() says which frames of a
// .sela come back different from the WAV (sela_hip_verify: compared on the GPU, nothing decoded into host memory) and what
// of the WAV the .sela never held.  A .sela whose frames say other lengths is compared at the positions decodeFile writes them.
struct VerifyReport {
    struct Frame {
        uint64_t frame;
        uint32_t differing, first; // values that differ; the first of them, i * channels + c from the frame's start
    };
    size_t framesCompared = 0;
    std::vector<Frame> lossy;
    uint64_t tailSamplesPerChannel = 0; // WAV samples beyond what the .sela's frames hold
    // Samples the .sela's frames hold beyond the WAV's end.  They are compared against silence, so the frames they lie in are
    // listed in `lossy` as well (unless they decode to silence): one cause, reported by its own line and by those frames.
    uint64_t missingSamplesPerChannel = 0;
    uint32_t channels = 0;
    bool rateDiffers = false, channelsDiffer = false, frameCountDiffers = false;
    uint32_t wavRate = 0, selaRate = 0, wavChannels = 0, selaChannels = 0;
    uint64_t wavFrames = 0, selaFrames = 0, selaHeaderFrames = 0;
    bool headersDisagree() const { return rateDiffers || channelsDiffer || frameCountDiffers; }
};
VerifyReport verifyFile(const std::string& wavPath, const std::string& selaPath);
// One line per lossy frame, one per header disagreement, one for the tail, one summary; no GPU needed.
std::string formatVerifyReport(const VerifyReport& report);
// 0: everything in the WAV comes back exactly; 3: a frame differs or the headers disagree; 4: only tail samples are missing.
int verifyExitCode(const VerifyReport& report);

// ---- levels: how loud is this .sela? ------------------------------------------------------------------
// measureFile() reads the file the way verifyFile does (the frames it really holds; a --keep-tail file's long last frame as it
// stands) and asks sela_hip_levels for every frame's records: measured on the GPU, nothing decoded into host memory.  A 24- or
// 32-bit .sela is refused by name: the records are those of 16-bit samples.
struct LevelReport {
    uint32_t channels = 0, sampleRate = 0;
    uint64_t frames = 0, silentFrames = 0; // frames held; those of them in which every channel is digital silence
    std::vector<ChannelLevel> perChannel;  // [channels]
    ChannelLevel track;                    // all channels folded into one
};
LevelReport measureFile(const std::string& selaPath);
// One line per channel -- the exact integers (peak= samples= sum= sum_squares=), then dBFS peak, dBFS RMS and DC -- and a last
// line for the track; no GPU needed.
std::string formatLevelReport(const LevelReport& report);
// The same for a .sela of 24- or 32-bit samples (host/src/wide.cpp): the width and the channel count are the
// header's, the frames are found as measureFile finds them, and sela_hip_levels_i32 gives every frame's records -- a --whole
// file's long last frame as it stands.  The energy is 128 bits wide; dBFS is against the file's own full scale, 2^(bits - 1).
struct WideLevelReport {
    uint32_t channels = 0, sampleRate = 0, bitsPerSample = 0;
    uint64_t frames = 0, silentFrames = 0;
    std::vector<ChannelLevelWide> perChannel; // [channels]
    ChannelLevelWide track;                   // all channels folded into one
};
WideLevelReport measureWideFile(const std::string& selaPath);
// formatLevelReport's lines, with the integers of the wide records; no GPU needed.
std::string formatLevelReport(const WideLevelReport& report);

// ---- digest: does this .sela still decode to that audio? -------------------------------------------------------
// digestFile() reads the file the way verifyFile does (the frames it really holds; a --keep-tail file's long last frame as it
// stands) and asks sela_hip_digest for the CRC-32 of the PCM it decodes to: computed on the GPU, nothing decoded into host
// memory.  With a WAV named, the host's own CRC-32 of its data chunk is set beside it -- cut to the samples the .sela holds, as
// verifyFile cuts it.  A 24- or 32-bit .sela is refused by name: the digest is that of 16-bit samples.
DigestReport digestFile(const std::string& selaPath, const std::string& wavPath = std::string());

// ---- envelope: a waveform overview of this .sela ---------------------------------------------------------------
// envelopeFile() reads the file the way measureFile does (the frames it really holds; a --keep-tail file's long last frame as it
// stands) and asks sela_hip_envelope for every frame's records: min, max, sum and sum of squares per `bucket` samples and channel,
// measured on the GPU, nothing decoded into host memory -- then compacts them onto the track's grid (envelope.hpp).  A bucket
// outside {32, 64, ..., 2048} is refused with the set named, a 24- or 32-bit .sela by name: the records are those of 16-bit samples.
EnvelopeReport envelopeFile(const std::string& selaPath, uint32_t bucket = kEnvelopeDefaultBucket);
// envelopeFile(), then the .env file of envelope.hpp written to envPath.
EnvelopeReport writeEnvelopeFile(const std::string& selaPath, const std::string& envPath, uint32_t bucket = kEnvelopeDefaultBucket);

// ---- many files, all GPUs of the node ------------------------------------------------------------------
// BASELINE.json configs[3]: an album's tracks are one index space of frames, cut into contiguous balanced
// ranges -- the reference's static partition (src/sela/encoder.cpp:58-73) with the remainder spread -- one
// per device, one host thread per device.  A range may begin or end inside a track.  The compressed sizes
// of the pieces meet in host memory (this is one process; sela_amd/sharding.py is the one-process-per-GPU
// form with the RCCL all-gather).  Results are what Encoder / Decoder give file by file.
//
// Devices to use: setDevices({0, 1, ...}); an index may repeat (two workers on one GPU -- used by the
// tests).  Default: every visible device.
void setDevices(const std::vector<int>& devices);
std::vector<int> devices();
std::vector<file::SelaFile> encodeBatch(const std::vector<file::WavFile>& wavs);
std::vector<file::WavFile> decodeBatch(const std::vector<file::SelaFile>& selas);
// The same jobs by path (CLI -E / -D): nothing is read or written up front -- every GPU worker reads ITS pieces of the
// input files (read-ahead on the I/O pool), codes them, and writes the results at their place in the output files
// while its next piece is on the device.  Small tracks that follow each other are read into one buffer and coded as
// one job.  A track cut between two workers: the later piece is placed when the earlier one's size is known; no
// worker waits for another one before its own work is done.
void encodeFiles(const std::vector<std::string>& inputs, const std::vector<std::string>& outputs);
void decodeFiles(const std::vector<std::string>& inputs, const std::vector<std::string>& outputs);

} // namespace sela
