// salvage.hpp -- the host's side of the salvage (sela_hip_salvage_payload_device, include/sela_hip.h): a .sela
// file whose payload is damaged, read past the positions where every other verb stops, and written out again with the frames
// that survived back to back and a header that counts them.  The report says what was lost and where.  With anyByte the frames
// are looked for at every byte of the payload (sela_hip_salvage_payload_unaligned_device), so what lies behind
// inserted or deleted bytes is found too.
#ifndef SELA_HOST_SALVAGE_HPP_
#define SELA_HOST_SALVAGE_HPP_

#include <cstdint>
#include <string>
#include <vector>

namespace sela {

struct SalvageGap {
    uint64_t fileOffset = 0; // of the first byte skipped, in the input file (its 15-byte header counted)
    uint64_t bytes = 0;
    uint64_t frameBehind = 0; // the index, in the output, of the frame that follows the gap
};

struct SalvageReport {
    uint64_t announced = 0;     // frames the input's header promises
    uint64_t found = 0;         // frames taken, and written
    uint64_t keptBytes = 0;     // their bytes: the output's payload
    uint64_t trailingBytes = 0; // bytes of the input behind the last frame taken
    std::vector<SalvageGap> gaps;
    bool intact() const { return gaps.empty() && trailingBytes == 0 && found == announced; }
};

// Reads inPath's 15-byte header (a file that is not 'SeLa' is refused, as everywhere), walks its payload on the GPU -- up to
// as many frames as its bytes could hold, NOT the announced count -- and, where a frame was found, writes outPath: the header
// with numFrames = found, then the frames taken.  Throws data::Exception; without a frame nothing is written.  anyByte: frames
// at any byte offset of the payload, not only at multiples of 4 (payloads below 4 GiB).
SalvageReport salvageFile(const std::string& inPath, const std::string& outPath, bool anyByte = false);

// "announced A frames, found F" / one "gap: ..." line per gap / "trailing: T bytes"
std::string formatSalvageReport(const SalvageReport& r);

// 0: nothing skipped, nothing trailing, found == announced; 2: frames were written but something was lost (or the header's
// count was wrong); 1: no frame was found
inline int salvageExitCode(const SalvageReport& r) { return r.found == 0 ? 1 : r.intact() ? 0 : 2; }

} // namespace sela
#endif
