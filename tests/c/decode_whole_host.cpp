// decode_whole_host.cpp -- the C++ host's decode paths that the CLI does not reach, on a file that keeps its tail,
// driven by tests/test_gpu_decode_whole.py:  decode_whole_host in.sela out_dir
//   out_dir/process.wav   sela::Decoder::process(), WavFile::writeToFile
//   out_dir/stream.wav    sela::decodeFile(std::ifstream&, std::ofstream&)
// and prints, per line, what each path reports: the samples (all channels) process() returns, the frames decodeFile returns.
// Exit 0 when everything ran; the bytes are judged by the test.
#include <fstream>
#include <iostream>
#include <string>

#include "sela_host/codec.hpp"

int main(int argc, char** argv)
{
    if (argc != 3)
        return 2;
    const std::string sela = argv[1], dir = argv[2];
    try {
        {
            std::ifstream in(sela, std::ios::binary);
            sela::Decoder dec(in);
            file::WavFile wav = dec.process();
            std::cout << "process: " << wav.pcm.size() << " samples" << std::endl;
            std::ofstream out(dir + "/process.wav", std::ios::binary);
            wav.writeToFile(out);
        }
        {
            std::ifstream in(sela, std::ios::binary);
            std::ofstream out(dir + "/stream.wav", std::ios::binary);
            std::cout << "stream: " << sela::decodeFile(in, out) << " frames" << std::endl;
        }
    } catch (const data::Exception& e) {
        std::cerr << e.exceptionMessage << std::endl;
        return 1;
    }
    return 0;
}
