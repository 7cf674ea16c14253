// salvage.cpp -- sela::salvageFile (see salvage.hpp): upload the payload, one sela_hip_salvage_payload_device (or its _unaligned
// form), download what it kept.  The one host source that talks to the HIP runtime itself: the call works on device pointers.
#include "sela_host/salvage.hpp"

#include <hip/hip_runtime_api.h>

#include <cstring>
#include <fstream>

#include "sela_hip.h"
#include "sela_host/files.hpp"
#include "sela_host/fileio.hpp"

namespace {

[[noreturn]] void gpuFailure(const std::string& what) { throw data::Exception("Salvage: " + what); }

// device memory that goes when its owner does
struct DeviceBytes {
    void* p = nullptr;
    explicit DeviceBytes(size_t n)
    {
        if (hipMalloc(&p, n ? n : 1) != hipSuccess)
            gpuFailure("no device memory for " + std::to_string(n) + " bytes");
    }
    DeviceBytes(const DeviceBytes&) = delete;
    DeviceBytes& operator=(const DeviceBytes&) = delete;
    ~DeviceBytes() { (void)hipFree(p); }
    template <typename T>
    T* as() const { return static_cast<T*>(p); }
};

void copy(void* dst, const void* src, size_t n, hipMemcpyKind kind)
{
    if (n && hipMemcpy(dst, src, n, kind) != hipSuccess)
        gpuFailure("a copy to or from the device failed");
}

} // namespace

namespace sela {

SalvageReport salvageFile(const std::string& inPath, const std::string& outPath, bool anyByte)
{
    std::ifstream probe(inPath, std::ios::binary);
    if (!probe)
        throw data::Exception("cannot open " + inPath);
    file::SelaFile sela;
    const size_t payloadBytes = sela.readHeader(probe);
    probe.close();
    const uint32_t channels = sela.selaHeader.channels;
    if (channels == 0)
        throw data::Exception("Decoder: unsupported channel count");
    if (payloadBytes / (4 + 12 * (size_t)channels) > 0xFFFFFFFFull)
        gpuFailure(inPath + " is too large");
    const uint32_t cap = (uint32_t)(payloadBytes / (4 + 12 * (size_t)channels)); // what the bytes could hold: the header's count is not believed
    SalvageReport r;
    r.announced = sela.selaHeader.numFrames;
    r.trailingBytes = payloadBytes;
    if (cap == 0)
        return r;
    if (sela_hip_device_count() <= 0)
        gpuFailure("no GPU, and no CPU fallback");
    std::vector<uint8_t> payload(payloadBytes);
    if (!sela_host::PosixFile::openForRead(inPath).readAt(payload.data(), payloadBytes, 15))
        throw data::Exception("File is too small, probably not a sela file.");

    const size_t workspaceBytes = anyByte ? sela_hip_salvage_unaligned_workspace_bytes(payloadBytes, cap) : sela_hip_salvage_workspace_bytes(payloadBytes, cap);
    const size_t outCap = payloadBytes / 4 * 4;
    DeviceBytes dPayload(payloadBytes), dOut(outCap), dOffsets(((size_t)cap + 1) * 8), dRecords((size_t)cap * sizeof(sela_hip_salvaged)), dTotals(32),
        dWorkspace(workspaceBytes);
    copy(dPayload.p, payload.data(), payloadBytes, hipMemcpyHostToDevice);
    if ((anyByte ? sela_hip_salvage_payload_unaligned_device : sela_hip_salvage_payload_device)(dPayload.as<uint8_t>(), payloadBytes, cap, channels, dOut.as<uint8_t>(), outCap, dOffsets.as<uint64_t>(),
            dRecords.as<sela_hip_salvaged>(), dTotals.as<uint64_t>(), dWorkspace.p, workspaceBytes, nullptr)
        != SELA_HIP_OK)
        gpuFailure(sela_hip_last_error());
    if (hipStreamSynchronize(nullptr) != hipSuccess)
        gpuFailure("the device reported a failure");
    uint64_t totals[4];
    copy(totals, dTotals.p, 32, hipMemcpyDeviceToHost);
    std::vector<sela_hip_salvaged> records(totals[0]);
    copy(records.data(), dRecords.p, records.size() * sizeof(sela_hip_salvaged), hipMemcpyDeviceToHost);
    r.found = totals[0];
    r.keptBytes = totals[2];
    r.trailingBytes = payloadBytes - totals[3];
    for (size_t f = 0; f < records.size(); f++)
        if (records[f].skipped_before)
            r.gaps.push_back({ 15 + records[f].offset - records[f].skipped_before, records[f].skipped_before, f });
    if (r.found == 0)
        return r;
    payload.resize(r.keptBytes); // (never more than it held)
    copy(payload.data(), dOut.p, r.keptBytes, hipMemcpyDeviceToHost);
    uint8_t header[15];
    std::memcpy(header, "SeLa", 4);
    const uint32_t rate = sela.selaHeader.sampleRate, frames = (uint32_t)r.found;
    const uint16_t bits = sela.selaHeader.bitsPerSample;
    for (int b = 0; b < 4; b++) {
        header[4 + b] = (uint8_t)(rate >> (8 * b));
        header[11 + b] = (uint8_t)(frames >> (8 * b));
    }
    header[8] = (uint8_t)bits, header[9] = (uint8_t)(bits >> 8), header[10] = (uint8_t)channels;
    const sela_host::PosixFile out = sela_host::PosixFile::create(outPath);
    out.writeAt(header, 15, 0);
    if (r.keptBytes)
        out.writeAt(payload.data(), r.keptBytes, 15);
    return r;
}

std::string formatSalvageReport(const SalvageReport& r)
{
    std::string out = "announced " + std::to_string(r.announced) + " frames, found " + std::to_string(r.found) + "\n";
    for (const SalvageGap& g : r.gaps)
        out += "gap: file offset " + std::to_string(g.fileOffset) + ", " + std::to_string(g.bytes) + " bytes, before frame " + std::to_string(g.frameBehind) + "\n";
    out += "trailing: " + std::to_string(r.trailingBytes) + " bytes\n";
    return out;
}

} // namespace sela
