// sela_cli.cpp -- command line front end of the MI355X SELA host:
//   sela_mi355x -e in.wav out.sela     encode
//   sela_mi355x -e --lossless in.wav out.sela   encode with the residues taken against the decoder's rounding: every frame comes
//                                      back exactly from any decoder of the format (plain -e is the reference's stream bit for bit,
//                                      a few frames in ten thousand of which do not: -v lists them)
//   sela_mi355x -e --pair-channels [--lossless] in.wav out.sela   encode a file of more than two channels with every odd channel
//                                      stored as the difference against the even channel before it where that takes fewer words
//                                      (any decoder of the format reads it; one and two channels: the same bytes as without)
//   sela_mi355x -e --keep-tail [--lossless] in.wav out.sela   encode the whole file: the samples beyond the last whole 2048-sample
//                                      frame are folded into a long last frame instead of dropped (with --lossless, -v then exits 0);
//                                      not with --pair-channels, not with -E
//   sela_mi355x -e --whole [--lossless] in.wav out.sela   the same by the file's own header: a 16-bit file exactly as --keep-tail, a
//                                      24- or 32-bit file through sela_hip_encode_whole_pcm (--keep-tail itself keeps to 16-bit files);
//                                      -d, -d --start S --count N and -v read such files without a flag
//   sela_mi355x -d in.sela out.wav     decode
//   (-e, -e --lossless, -d, -d --start S --count N and -v take 24- and 32-bit files too, routed by what the WAV's or the .sela's header
//   says: the packed samples go to the device and come back as they lie in the file; every other verb and flag keeps to 16-bit files)
//   sela_mi355x -d --start S --count N in.sela out.wav   decode samples S .. S + N - 1 per channel only (cut at the stream's end):
//                                      the frames the range touches are decoded and no others
//   sela_mi355x -v in.wav in.sela      verify: which frames of in.sela come back different from in.wav (compared on the GPU), and
//                                      what of in.wav it never held; exit 0: all of it comes back exactly, 3: a frame differs or
//                                      the headers disagree, 4: only tail samples are missing, 1: an error (a .wav and a .sela
//                                      of different sample widths among them)
//   sela_mi355x -m in.sela             measure: per channel the exact peak, sample count, sum and sum of squares of the decoded
//                                      int16 samples (reduced on the GPU, nothing decoded into memory), then dBFS peak, dBFS RMS and
//                                      DC offset; a last line for the track.  A --keep-tail file is read as it stands; a 24- or
//                                      32-bit .sela is refused by name (exit 1)
//   sela_mi355x -w [--bucket B] in.sela out.env   waveform: per B samples (a power of two from 32 to 2048; 256 unless given) and channel
//                                      the smallest and the largest sample, the sum and the sum of squares, on the track's own grid
//                                      (reduced on the GPU, nothing decoded into memory) -> out.env: 32 bytes of header ("SELAENV1",
//                                      uint32 channels, uint32 B, uint64 samples per channel, uint32 sample rate, uint32 16), then
//                                      16-byte records [bucket][channel].  A --keep-tail file is read as it stands; a 24- or 32-bit
//                                      .sela is refused by name, a bucket outside the set with the set named (exit 1, as -m)
//   sela_mi355x -W [--bucket B] in.sela out.env   the same by the file's own header: a 16-bit file exactly as -w, -w's bytes; a 24- or
//                                      32-bit file (a --whole one as it stands) through sela_hip_envelope_i32 -- the samples as they are,
//                                      the header's last word the file's bits (24 or 32), then 32-byte records [bucket][channel]: int32
//                                      min, max, int64 sum, the sum of squares in 128 bits
//   sela_mi355x -M in.sela             the same as -m by the file's own header: a 16-bit file exactly as -m, a 24- or 32-bit file through
//                                      sela_hip_levels_i32 -- the integers of its samples as they are (the sum of squares in 128
//                                      bits, printed whole), dBFS against the file's own full scale; a --whole file as it stands
//   sela_mi355x -c in.sela [in.wav]    digest: the CRC-32 (zlib's, `crc32`'s) of the PCM in.sela decodes to -- taken on the GPU, nothing
//                                      decoded into memory -- its byte count and the frame count; with in.wav also the CRC-32 of its
//                                      data chunk (cut to whole frames unless in.sela is a --keep-tail file, as -v cuts it), exit 0
//                                      only if the two agree, else 3.  A 24- or 32-bit .sela is refused by name (exit 1)
//   sela_mi355x -C in.sela [in.wav]    the same by the file's own header: a 16-bit file exactly as -c, a 24- or 32-bit file through
//                                      sela_hip_digest_pcm -- the CRC-32 of the packed 3- or 4-byte samples as a WAV of that width
//                                      holds them; one more line where samples of a 24-bit file lie beyond 24 bits; a --whole file
//                                      as it stands; a .wav of another width is refused by name (exit 1)
//   sela_mi355x -s in.sela out.sela   salvage: the frames of a damaged file found on the GPU past the positions where every other verb
//                                      stops silently, and written back to back under a header that counts them.  Prints the announced
//                                      and the found frame counts, a line per gap (file offset, bytes, index of the frame behind it)
//                                      and the bytes behind the last frame; exit 0: nothing skipped, nothing trailing, found ==
//                                      announced, 2: frames were written but something was lost, 1: no frame found, or not a .sela
//   sela_mi355x -s --any-byte in.sela out.sela   the same with frames looked for at EVERY byte of the payload: what lies
//                                      behind inserted or deleted bytes, or behind a second file's header, is found too.  The same lines
//                                      (gaps in bytes at file offsets) and exit codes
//   sela_mi355x -E out_dir [--gpus N | --devices a,b,..] a.wav b.wav ...    encode many files as one job -> out_dir/<name>.sela
//   sela_mi355x -D out_dir [--gpus N | --devices a,b,..] a.sela b.sela ...  decode many files as one job -> out_dir/<name>.wav
//   (-E / -D also take --io-threads N: threads that read and write files beside the GPU workers)
//   sela_mi355x -p in.sela [out.pcm]   play: the packets the reference's player would hand to libao (src/sela/player.cpp:30-62),
//                                      handed out while the file is still being decoded -- to out.pcm, or to standard output
//                                      (`sela_mi355x -p in.sela | aplay -f S16_LE -c 2 -r 44100`; this build has no audio device)
// Same verbs as the reference CLI (src/main.cpp:16-27).  The batch verbs spread the files' frames over the GPUs of the
// node (default: all of them), one host thread each.
#include <algorithm>
#include <cstdlib>
#include <exception>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include <fcntl.h>
#include <unistd.h>

#include "sela_host/codec.hpp"
#include "sela_host/player.hpp"
#include "sela_host/salvage.hpp"
#include "sela_host/wide.hpp"

namespace {

int usage(const std::string& program)
{
    std::cout << "Usage:\n\n"
              << "Encoding a file (--lossless: every frame decodes back exactly; without it the reference's stream bit for bit):\n"
              << program << " -e [--lossless] path/to/input.wav path/to/output.sela\n\n"
              << "Encoding a multichannel file with adjacent channels paired (odd channels as differences where that is smaller):\n"
              << program << " -e --pair-channels [--lossless] path/to/input.wav path/to/output.sela\n\n"
              << "Encoding a whole file (the samples beyond the last whole frame are kept, in a long last frame):\n"
              << program << " -e --keep-tail [--lossless] path/to/input.wav path/to/output.sela\n\n"
              << "Encoding a whole 16-, 24- or 32-bit file (as --keep-tail, by the file's own header):\n"
              << program << " -e --whole [--lossless] path/to/input.wav path/to/output.sela\n\n"
              << "Decoding a file (--start S --count N: samples S .. S + N - 1 per channel only; 16-, 24- and 32-bit files alike):\n"
              << program << " -d [--start S --count N] path/to/input.sela path/to/output.wav\n\n"
              << "Verifying a file against the .wav it was made from:\n" << program << " -v path/to/input.wav path/to/input.sela\n\n"
              << "Measuring a 16-bit file (per channel and for the track: peak, sum and sum of squares, then dBFS peak, dBFS RMS and DC):\n"
              << program << " -m path/to/input.sela\n\n"
              << "The waveform envelope of a 16-bit file (min, max, sum and sum of squares per B samples and channel; B = 256 unless given):\n"
              << program << " -w [--bucket B] path/to/input.sela path/to/output.env\n\n"
              << "The waveform envelope of a 16-, 24- or 32-bit file (as -w, by the file's own header; 32-byte records for 24 and 32 bits):\n"
              << program << " -W [--bucket B] path/to/input.sela path/to/output.env\n\n"
              << "Measuring a 16-, 24- or 32-bit file (as -m, by the file's own header; dBFS against the file's own full scale):\n"
              << program << " -M path/to/input.sela\n\n"
              << "The CRC-32 of the audio a 16-bit file decodes to (with a .wav: held against the CRC-32 of its data chunk):\n"
              << program << " -c path/to/input.sela [path/to/input.wav]\n\n"
              << "The same for a 16-, 24- or 32-bit file (as -c, by the file's own header; the CRC-32 of the packed samples):\n"
              << program << " -C path/to/input.sela [path/to/input.wav]\n\n"
              << "Salvaging a damaged file (the frames that can still be found, back to back; exit 2 where something was lost):\n"
              << program << " -s path/to/input.sela path/to/output.sela\n\n"
              << "Salvaging a file that bytes were inserted into or deleted from (frames are looked for at every byte, not every 4th):\n"
              << program << " -s --any-byte path/to/input.sela path/to/output.sela\n\n"
              << "Playing a file (raw interleaved int16 to a file, or to standard output):\n" << program << " -p path/to/input.sela [path/to/output.pcm]\n\n"
              << "Many files, all GPUs:\n" << program << " -E|-D path/to/output_dir [--gpus N | --devices 0,1,..] inputs...\n";
    return 2;
}

// out_dir/<file name of `in` with its extension replaced>
std::string sibling(const std::string& out_dir, const std::string& in, const char* extension)
{
    const size_t slash = in.find_last_of('/');
    std::string name = slash == std::string::npos ? in : in.substr(slash + 1);
    const size_t dot = name.find_last_of('.');
    if (dot != std::string::npos)
        name.erase(dot);
    return out_dir + "/" + name + extension;
}

int batch(const std::string& verb, int argc, char** argv)
{
    const std::string out_dir = argv[2];
    std::vector<std::string> inputs;
    for (int i = 3; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "--io-threads" && i + 1 < argc) {
            sela::setIoThreads((unsigned)std::max(0, std::atoi(argv[++i])));
        } else if ((a == "--gpus" || a == "--devices") && i + 1 < argc) {
            std::vector<int> devs;
            const std::string v = argv[++i];
            if (a == "--gpus") {
                for (int d = 0; d < std::atoi(v.c_str()); d++)
                    devs.push_back(d);
            } else {
                for (size_t at = 0; at <= v.size();) {
                    const size_t comma = std::min(v.find(',', at), v.size());
                    devs.push_back(std::atoi(v.substr(at, comma - at).c_str()));
                    at = comma + 1;
                }
            }
            if (devs.empty())
                throw data::Exception("no device selected");
            sela::setDevices(devs);
        } else {
            inputs.push_back(a);
        }
    }
    if (inputs.empty())
        return 2;
    // nothing is read or written here: every GPU worker reads, codes and writes its own pieces of the files
    std::vector<std::string> outputs;
    for (const std::string& in : inputs)
        outputs.push_back(sibling(out_dir, in, verb == "-E" ? ".sela" : ".wav"));
    if (verb == "-E")
        sela::encodeFiles(inputs, outputs);
    else
        sela::decodeFiles(inputs, outputs);
    return 0;
}

// Does `path` hold a 24- or 32-bit PCM WAV?  (Anything else -- no file, no WAV, another format -- is today's path's to take
// or to refuse in its own words.)
bool wideWav(const std::string& path)
{
    try {
        const file::WavProbe p = file::probeWav(path);
        return p.bitsPerSample == 24 || p.bitsPerSample == 32;
    } catch (const data::Exception&) {
        return false;
    }
}

// plain -e and -e --lossless of a 24- or 32-bit file; keepTail: -e --whole (5.25)
int encodeWide(const std::string& in, const std::string& out, bool lossless, bool keepTail = false)
{
    std::cout << "Encoding (" << file::probeWav(in).bitsPerSample << "-bit" << (keepTail ? ", whole file" : "") << (lossless ? ", lossless" : "") << "): " << in << std::endl;
    const sela::WideReport r = sela::encodeWideFile(in, out, lossless, keepTail);
    std::cout << r.frames << " frames, " << r.droppedSamples << " samples per channel behind the last whole frame dropped" << std::endl;
    return 0;
}

// all of `text` as an unsigned decimal number
bool parseCount(const std::string& text, uint64_t* value)
{
    if (text.empty() || text.size() > 19 || text.find_first_not_of("0123456789") != std::string::npos)
        return false;
    *value = std::strtoull(text.c_str(), nullptr, 10);
    return true;
}

int run(int argc, char** argv)
{
    const std::string program = argv[0];
    const std::string verb = argc > 1 ? argv[1] : "";
    // (--keep-tail is -e's alone, right behind it, with --lossless behind it or nothing: with --pair-channels, with -E and anywhere
    // else it is refused, not ignored; so is --whole, which sends a 24- or 32-bit file to encodeWideFile and any other down
    // --keep-tail's path)
    for (int i = 2; i < argc; i++) {
        const bool whole = std::string(argv[i]) == "--whole";
        if (std::string(argv[i]) != "--keep-tail" && !whole)
            continue;
        const bool keepLossless = argc == 6 && std::string(argv[3]) == "--lossless";
        if (!(verb == "-e" && i == 2 && (argc == 5 || keepLossless)))
            return usage(program);
        for (int k = 3; k < argc; k++)
            if (std::string(argv[k]).rfind("--", 0) == 0 && !(keepLossless && k == 3))
                return usage(program);
        if (whole && wideWav(argv[argc - 2]))
            return encodeWide(argv[argc - 2], argv[argc - 1], keepLossless, true);
        std::cout << "Encoding (whole file" << (keepLossless ? ", lossless" : "") << "): " << argv[argc - 2] << std::endl;
        sela::encodeFile(std::string(argv[argc - 2]), std::string(argv[argc - 1]), keepLossless, false, true);
        return 0;
    }
    // (--pair-channels is -e's alone, right behind it; --lossless is -e's alone too, behind the verb or behind --pair-channels:
    // anywhere else they are refused, not ignored)
    const bool paired = verb == "-e" && (argc == 5 || argc == 6) && std::string(argv[2]) == "--pair-channels";
    const bool pairedLossless = paired && argc == 6 && std::string(argv[3]) == "--lossless";
    if (paired && argc == 6 && !pairedLossless)
        return usage(program);
    for (int i = 2; i < argc; i++) {
        if (std::string(argv[i]) == "--pair-channels" && !(paired && i == 2))
            return usage(program);
        if (std::string(argv[i]) == "--lossless" && !(verb == "-e" && i == 2 && argc == 5) && !(pairedLossless && i == 3))
            return usage(program);
    }
    // (--any-byte is -s's alone, right behind it: with any other verb and anywhere else it is refused, not ignored)
    const bool anyByte = verb == "-s" && argc == 5 && std::string(argv[2]) == "--any-byte";
    for (int i = 2; i < argc; i++)
        if (std::string(argv[i]) == "--any-byte" && !(anyByte && i == 2))
            return usage(program);
    // (--start / --count are -d's alone, together, in that place: anywhere else they are refused, not ignored)
    const bool ranged = verb == "-d" && argc == 8 && std::string(argv[2]) == "--start" && std::string(argv[4]) == "--count";
    for (int i = 2; i < argc; i++)
        if ((std::string(argv[i]) == "--start" && !(ranged && i == 2)) || (std::string(argv[i]) == "--count" && !(ranged && i == 4)))
            return usage(program);
    if (ranged) {
        uint64_t start = 0, count = 0;
        if (!parseCount(argv[3], &start) || !parseCount(argv[5], &count))
            return usage(program);
        const uint16_t bits = sela::selaFileBits(argv[6]);
        const bool wide = bits == 24 || bits == 32;
        std::cout << "Decoding" << (wide ? (bits == 24 ? " (24-bit)" : " (32-bit)") : "") << ": " << argv[6] << ", samples " << start << " + " << count << std::endl;
        const size_t written = wide ? sela::decodeWideFileRange(std::string(argv[6]), std::string(argv[7]), start, count)
                                    : sela::decodeFileRange(std::string(argv[6]), std::string(argv[7]), start, count);
        std::cout << written << " samples per channel" << std::endl;
        return 0;
    }
    if (paired) {
        std::cout << "Encoding (channel pairs" << (pairedLossless ? ", lossless" : "") << "): " << argv[argc - 2] << std::endl;
        sela::encodeFile(std::string(argv[argc - 2]), std::string(argv[argc - 1]), pairedLossless, true);
        return 0;
    }
    if (verb == "-e" && argc == 5 && std::string(argv[2]) == "--lossless") {
        if (wideWav(argv[3]))
            return encodeWide(argv[3], argv[4], true);
        std::cout << "Encoding (lossless): " << argv[3] << std::endl;
        sela::encodeFile(std::string(argv[3]), std::string(argv[4]), true);
        return 0;
    }
    if ((verb == "-E" || verb == "-D") && argc >= 4) {
        const int rc = batch(verb, argc, argv);
        return rc == 2 ? usage(program) : rc;
    }
    if (verb == "-p" && (argc == 3 || argc == 4)) {
        int fd = STDOUT_FILENO;
        if (argc == 4) {
            fd = ::open(argv[3], O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
            if (fd < 0)
                throw data::Exception(std::string("cannot open ") + argv[3] + " for writing");
        } else if (::isatty(STDOUT_FILENO)) {
            std::cerr << "-p writes raw samples to standard output: redirect it, or name an output file" << std::endl;
            return 2;
        }
        std::cerr << "Playing: " << argv[2] << std::endl;
        sela::RawPcmSink sink(fd);
        sela::Player player(sink);
        player.showProgress = ::isatty(STDERR_FILENO) != 0;
        size_t frames = 0;
        try {
            frames = player.playFile(argv[2]);
        } catch (...) {
            if (fd != STDOUT_FILENO)
                (void)::close(fd);
            throw;
        }
        if (fd != STDOUT_FILENO)
            (void)::close(fd);
        std::cerr << frames << " frames, first packet after " << player.firstPacketSeconds * 1e3 << " ms" << std::endl;
        return 0;
    }
    if (verb == "-v" && argc == 4) {
        std::cout << "Verifying: " << argv[3] << " against " << argv[2] << std::endl;
        // (by the WAV's header, as -e: a 24- or 32-bit file goes to sela_hip_verify_pcm; a 16-bit WAV held against a
        // wider .sela is refused in the same words)
        const uint16_t selaBits = sela::selaFileBits(argv[3]);
        if (!wideWav(argv[2]) && (selaBits == 24 || selaBits == 32) && file::probeWav(argv[2]).bitsPerSample == 16)
            throw data::Exception("Verify: the .wav holds 16-bit samples, the .sela " + std::to_string(selaBits)
                + "-bit samples: files of different widths are not held against each other");
        const sela::VerifyReport report = wideWav(argv[2]) ? sela::verifyWideFile(std::string(argv[2]), std::string(argv[3]))
                                                           : sela::verifyFile(std::string(argv[2]), std::string(argv[3]));
        std::cout << sela::formatVerifyReport(report) << std::flush;
        return sela::verifyExitCode(report);
    }
    if (verb == "-m") {
        if (argc != 3)
            return usage(program);
        std::cout << "Measuring: " << argv[2] << std::endl;
        std::cout << sela::formatLevelReport(sela::measureFile(std::string(argv[2]))) << std::flush;
        return 0;
    }
    if (verb == "-w" || verb == "-W") {
        long long bucket = sela::kEnvelopeDefaultBucket;
        int at = 2;
        if (argc > at + 1 && std::string(argv[at]) == "--bucket") {
            bucket = std::atoll(argv[at + 1]);
            at += 2;
        }
        if (argc != at + 2)
            return usage(program);
        if (bucket < 0 || bucket > 0xFFFFFFFFll || !sela::envelopeBucketOk((uint32_t)bucket))
            throw data::Exception(sela::envelopeBucketRefusal(bucket));
        // (-W goes by the .sela's header: a 24- or 32-bit file to sela_hip_envelope_i32; any other file, and -w, down -w's path)
        const uint16_t bits = verb == "-W" ? sela::selaFileBits(argv[at]) : 0;
        if (bits == 24 || bits == 32) {
            std::cout << "Envelope (" << bits << "-bit): " << argv[at] << std::endl;
            const sela::EnvelopeReport32 report = sela::writeEnvelopeWideFile(std::string(argv[at]), std::string(argv[at + 1]), (uint32_t)bucket);
            std::cout << report.buckets() << " buckets of " << report.bucket << " samples, " << report.channels << " channels, " << report.samplesPerChannel
                      << " samples per channel -> " << argv[at + 1] << std::endl;
            return 0;
        }
        std::cout << "Envelope: " << argv[at] << std::endl;
        const sela::EnvelopeReport report = sela::writeEnvelopeFile(std::string(argv[at]), std::string(argv[at + 1]), (uint32_t)bucket);
        std::cout << report.buckets() << " buckets of " << report.bucket << " samples, " << report.channels << " channels, " << report.samplesPerChannel
                  << " samples per channel -> " << argv[at + 1] << std::endl;
        return 0;
    }
    if (verb == "-c" || verb == "-C") {
        if (argc != 3 && argc != 4)
            return usage(program);
        // (-C goes by the .sela's header: a 24- or 32-bit file to sela_hip_digest_pcm; any other file, and -c, down -c's path)
        const uint16_t bits = verb == "-C" ? sela::selaFileBits(argv[2]) : 0;
        const std::string wav = argc == 4 ? std::string(argv[3]) : std::string();
        if (bits == 24 || bits == 32) {
            std::cout << "Digest (" << bits << "-bit): " << argv[2] << std::endl;
            const sela::DigestReport report = sela::digestWideFile(std::string(argv[2]), wav);
            std::cout << sela::formatDigestReport(report);
            if (report.wideSamples)
                std::cout << report.wideSamples << " samples beyond 24 bits (their low bytes digested)\n";
            std::cout << std::flush;
            return report.agree() ? 0 : 3;
        }
        std::cout << "Digest: " << argv[2] << std::endl;
        const sela::DigestReport report = sela::digestFile(std::string(argv[2]), wav);
        std::cout << sela::formatDigestReport(report) << std::flush;
        return report.agree() ? 0 : 3;
    }
    if (anyByte) {
        std::cout << "Salvaging (any byte): " << argv[3] << std::endl;
        const sela::SalvageReport report = sela::salvageFile(std::string(argv[3]), std::string(argv[4]), true);
        std::cout << sela::formatSalvageReport(report) << std::flush;
        return sela::salvageExitCode(report);
    }
    if (verb == "-s") {
        if (argc != 4)
            return usage(program);
        std::cout << "Salvaging: " << argv[2] << std::endl;
        const sela::SalvageReport report = sela::salvageFile(std::string(argv[2]), std::string(argv[3]));
        std::cout << sela::formatSalvageReport(report) << std::flush;
        return sela::salvageExitCode(report);
    }
    if (verb == "-M") {
        if (argc != 3)
            return usage(program);
        // (by the .sela's header: a 24- or 32-bit file goes to sela_hip_levels_i32; any other file down -m's path)
        const uint16_t bits = sela::selaFileBits(argv[2]);
        if (bits == 24 || bits == 32) {
            std::cout << "Measuring (" << bits << "-bit): " << argv[2] << std::endl;
            std::cout << sela::formatLevelReport(sela::measureWideFile(std::string(argv[2]))) << std::flush;
        } else {
            std::cout << "Measuring: " << argv[2] << std::endl;
            std::cout << sela::formatLevelReport(sela::measureFile(std::string(argv[2]))) << std::flush;
        }
        return 0;
    }
    if (argc != 4 || (verb != "-e" && verb != "-d"))
        return usage(program);
    if (verb == "-e" && wideWav(argv[2]))
        return encodeWide(argv[2], argv[3], false);
    if (verb == "-d" && (sela::selaFileBits(argv[2]) == 24 || sela::selaFileBits(argv[2]) == 32)) {
        std::cout << "Decoding (" << sela::selaFileBits(argv[2]) << "-bit): " << argv[2] << std::endl;
        const sela::WideReport r = sela::decodeWideFile(std::string(argv[2]), std::string(argv[3]));
        std::cout << r.frames << " frames";
        if (r.wideSamples)
            std::cout << ", " << r.wideSamples << " samples beyond 24 bits (their low bytes written)";
        std::cout << std::endl;
        return 0;
    }
    if (verb == "-e") {
        std::cout << "Encoding: " << argv[2] << std::endl;
        sela::encodeFile(std::string(argv[2]), std::string(argv[3])); // read, GPU and write overlap; only the byte stream is produced
    } else {
        std::cout << "Decoding: " << argv[2] << std::endl;
        sela::decodeFile(std::string(argv[2]), std::string(argv[3]));
    }
    return 0;
}

} // namespace

int main(int argc, char** argv)
{
    // (-p may write the samples to standard output: everything else it says goes to standard error)
    (argc > 1 && std::string(argv[1]) == "-p" ? std::cerr : std::cout) << "SimplE Lossless Audio (.sela v2 bitstream) -- MI355X host" << std::endl;
    try {
        return run(argc, argv);
    } catch (const data::Exception& e) {
        std::cerr << e.exceptionMessage << std::endl;
    } catch (const std::exception& e) { // (std::bad_alloc on an absurd header, ...)
        std::cerr << "error: " << e.what() << std::endl;
    }
    return 1;
}
