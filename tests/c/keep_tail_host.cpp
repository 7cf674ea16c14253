// keep_tail_host.cpp -- the C++ host's keepTail paths that the CLI does not reach, driven by
// tests/test_gpu_encode_whole.py:  keep_tail_host in.wav out_dir
//   out_dir/process.sela   sela::Encoder with keepTail and lossless, process(), SelaFile::writeToFile
//   out_dir/stream.sela    sela::encodeFile(std::ifstream&, std::ofstream&, lossless, false, keepTail)
// and prints, per line: the frames each path reports, and "refused: <message>" for each of the three entries asked for keepTail
// together with pairChannels.  Exit 0 when everything ran; the bytes are judged by the test.
#include <fstream>
#include <iostream>
#include <string>

#include "sela_host/codec.hpp"

int main(int argc, char** argv)
{
    if (argc != 3)
        return 2;
    const std::string wav = argv[1], dir = argv[2];
    try {
        {
            std::ifstream in(wav, std::ios::binary);
            sela::Encoder enc(in);
            enc.keepTail = enc.lossless = true;
            file::SelaFile sela = enc.process();
            std::cout << "process: " << sela.frameCount() << " frames, header " << sela.selaHeader.numFrames << ", " << sela.frameOffsets.back() << " bytes" << std::endl;
            std::ofstream out(dir + "/process.sela", std::ios::binary);
            sela.writeToFile(out);
        }
        {
            std::ifstream in(wav, std::ios::binary);
            std::ofstream out(dir + "/stream.sela", std::ios::binary);
            std::cout << "stream: " << sela::encodeFile(in, out, true, false, true) << " frames" << std::endl;
        }
    } catch (const data::Exception& e) {
        std::cerr << e.exceptionMessage << std::endl;
        return 1;
    }
    int refusals = 0;
    try {
        std::ifstream in(wav, std::ios::binary);
        sela::Encoder enc(in);
        enc.keepTail = enc.pairChannels = true;
        (void)enc.process();
    } catch (const data::Exception& e) {
        std::cout << "refused: " << e.exceptionMessage << std::endl, refusals++;
    }
    try {
        std::ifstream in(wav, std::ios::binary);
        std::ofstream out(dir + "/never_stream.sela", std::ios::binary);
        (void)sela::encodeFile(in, out, false, true, true);
    } catch (const data::Exception& e) {
        std::cout << "refused: " << e.exceptionMessage << std::endl, refusals++;
    }
    try {
        (void)sela::encodeFile(wav, dir + "/never_path.sela", false, true, true);
    } catch (const data::Exception& e) {
        std::cout << "refused: " << e.exceptionMessage << std::endl, refusals++;
    }
    return refusals == 3 ? 0 : 3;
}
