// wide.hpp -- 24- and 32-bit WAV files to and from .sela, beside file::WavFile and sela::encodeFile / decodeFile,
// which stay the 16-bit path they are (file::WavFile::readFromFile refuses every other container, as the reference's reader does).
//
//   * file::probeWav walks a WAV file's chunk headers as WavFile::readHeader does -- a 'fmt ' chunk counts wherever it stands
//     (behind the data too), the LAST 'data' chunk is the audio -- and says what the file holds, refusing nothing a 16-bit reader
//     would take: the CLI asks it which path a file goes.
//   * sela::encodeWideFile / decodeWideFile move the packed data chunk through page-locked memory and ONE call to
//     sela_hip_encode_pcm / sela_hip_decode_pcm: 3 bytes per sample of a 24-bit file travel to the device, and the layout
//     conversion is the device's.
//   * sela::verifyWideFile is verifyFile for such a pair: ONE call to sela_hip_verify_pcm holds the stream against the WAV's packed
//     data chunk.
//   * sela::decodeWideFileRange is decodeFileRange for such files: one window of the stream through sela_hip_decode_windows_i32.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>

#include "sela_host/codec.hpp"
#include "sela_host/data.hpp"
#include "sela_host/digest.hpp"

namespace file {

struct WavProbe {
    uint32_t sampleRate = 0;
    uint16_t channels = 0;
    uint16_t bitsPerSample = 0; // the container: 16, 24 or 32
    uint16_t validBits = 0;     // an extensible header's wValidBitsPerSample (20 in 24, say); else bitsPerSample
    bool extensible = false;
    uint64_t dataOffset = 0, dataBytes = 0; // the last 'data' chunk's payload, clipped to the file
};

// Throws data::Exception: the reader's messages for what is no WAV file at all or lacks a chunk; "Only 16, 24 and 32bits per sample
// wav is supported." for another container; "Only PCM wav is supported ..." for float and every other format tag (0xFFFE,
// extensible, needs 40 bytes of 'fmt ' body and the PCM subformat).
WavProbe probeWav(const std::string& path);

} // namespace file

namespace sela {

struct WideReport {
    uint32_t frames = 0;         // frames coded / decoded
    uint64_t droppedSamples = 0; // encode: samples per channel behind the last whole frame (dropped, as plain -e drops them)
    uint32_t wideSamples = 0;    // decode: samples that did not fit a 3-byte container (their low bytes were written)
};

// in: a 24- or 32-bit PCM WAV (probeWav) -> out: a .sela file whose header carries the file's bitsPerSample; frames of 2048 samples.
// keepTail: the whole data chunk through sela_hip_encode_whole_pcm -- the samples behind the last whole frame are
// folded into a long last frame, numFrames is sela_hip_whole_frames' and droppedSamples 0.
WideReport encodeWideFile(const std::string& in, const std::string& out, bool lossless = false, bool keepTail = false);
// in: a .sela file whose header says 24 or 32 -> out: a WAV with the canonical 44-byte PCM header of that width.
WideReport decodeWideFile(const std::string& in, const std::string& out);
// in: such a .sela file -> out: a WAV of that width holding samples startSample .. startSample + sampleCount - 1 per channel, cut at
// the stream's end (only the frames the range touches are decoded).  Returns the samples per channel written;
// throws decodeFileRange's message where startSample is at or past the end.  (Samples of a 24-bit file that lie outside 24 bits
// go out as their low three bytes, as from decodeWideFile, but are not counted here: the host window call returns no status words.)
size_t decodeWideFileRange(const std::string& in, const std::string& out, uint64_t startSample, uint64_t sampleCount);
// wavPath: a 24- or 32-bit PCM WAV, selaPath: a .sela file of the same width -> verifyFile's report (formatVerifyReport and
// verifyExitCode apply unchanged): the frames that come back different, the WAV's tail, the samples the .sela holds beyond the WAV.
// Throws data::Exception, naming both widths, where the two files' widths disagree.
VerifyReport verifyWideFile(const std::string& wavPath, const std::string& selaPath);
// digestFile for a 24- or 32-bit .sela: ONE call to sela_hip_digest_pcm gives the CRC-32 of the packed PCM the
// file decodes to -- nothing is decoded into memory -- and, with a WAV of the same width and channel count, the host's Crc32 runs
// over its data chunk cut to the samples the .sela holds, as verifyWideFile cuts it: all of it for a --whole file, its whole
// 2048-sample frames for any other; wavTailBytes is the rest.  formatDigestReport applies unchanged.  Throws data::Exception,
// naming both, where the WAV's width or channel count is not the file's.
DigestReport digestWideFile(const std::string& selaPath, const std::string& wavPath = std::string());
// envelopeFile for a 24- or 32-bit .sela: the frames the file really holds, a --whole file's long last frame as it
// stands, through ONE call to sela_hip_envelope_i32 -- min, max, sum and the 128-bit sum of squares per `bucket` samples and
// channel of the samples as they are, nothing decoded into host memory -- compacted onto the track's grid (envelope.hpp).  A bucket
// outside {32, 64, ..., 2048} is refused with the set named.
EnvelopeReport32 envelopeWideFile(const std::string& selaPath, uint32_t bucket = kEnvelopeDefaultBucket);
// envelopeWideFile(), then the wide .env file of envelope.hpp written to envPath.
EnvelopeReport32 writeEnvelopeWideFile(const std::string& selaPath, const std::string& envPath, uint32_t bucket = kEnvelopeDefaultBucket);
// what the .sela header at `path` says its samples' width is; 0 where there is no such header (the caller's path then reports it)
uint16_t selaFileBits(const std::string& path);

} // namespace sela
