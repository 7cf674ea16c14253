// decode_whole_plan.cpp -- the plan of sela_hip_decode_whole and of k_whole_plan (plan_decode_whole, sela_amd/csrc/
// sela_decode_whole_plan.h) on the CPU, for the sanitizers.  The streams are real bytes made here: every frame a sync word and one
// subframe header that says a length, or eight bytes, too short to hold one.  The model is the contract of include/sela_hip.h
// written out: a last frame that says 1 .. 4095 and not 2048 is the long one.  Prints "<cases> cases, <n> failures".
#include <cstdint>
#include <cstdio>
#include <vector>

#include "sela_decode_whole_plan.h"

namespace {

constexpr uint32_t kHeaderless = 0xFFFFFFFFu; // a frame of eight bytes

struct Table {
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> offsets;
};

Table make_table(const std::vector<uint32_t>& lengths)
{
    Table t;
    t.offsets.push_back(0);
    for (uint32_t n : lengths) {
        const uint8_t sync[4] = { 0x00, 0xFF, 0x55, 0xAA };
        t.bytes.insert(t.bytes.end(), sync, sync + 4);
        if (n == kHeaderless) {
            const uint8_t four[4] = { 0, 0, 0, 0 };
            t.bytes.insert(t.bytes.end(), four, four + 4);
        } else { // channel, type, parent, ck, cw = 0 (u16), order | rk, rw = 0 (u16), n (u16)
            const uint8_t h[12] = { 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, (uint8_t)(n & 0xFF), (uint8_t)(n >> 8) };
            t.bytes.insert(t.bytes.end(), h, h + 12);
        }
        t.offsets.push_back(t.bytes.size());
    }
    return t;
}

int failures = 0, cases = 0;

// what the contract says of a stream whose last frame says n_last (0: it holds no header), for a caller with room for `capacity`
void check(const std::vector<uint32_t>& lengths, uint64_t capacity)
{
    cases++;
    const Table t = make_table(lengths);
    const uint32_t n = (uint32_t)lengths.size();
    // (an exact copy of the bytes and no more: a read past either end is the sanitizer's to find)
    const std::vector<uint8_t> bytes(t.bytes.begin(), t.bytes.end());
    const sela::DecodeWholePlan p = sela::plan_decode_whole(bytes.data(), t.offsets.data(), n, capacity);
    uint64_t samples = 0;
    uint32_t fast = 0, route = 0, flags = 0, tail_n = 0;
    if (n) {
        const uint32_t n_last = lengths[n - 1] == kHeaderless ? 0 : lengths[n - 1];
        const bool tailed = n_last >= 1 && n_last <= 4095 && n_last != 2048;
        samples = tailed ? 2048ull * (n - 1) + n_last : 2048ull * n;
        if (samples > capacity) {
            flags = SELA_HIP_FLAG_STRIDE;
        } else {
            fast = tailed ? n - 1 : n, route = tailed ? 3 : 1, tail_n = tailed ? n_last : 0;
        }
    }
    bool ok = p.samples == samples && p.fast_frames == fast && p.route == route && p.flags == flags;
    if (tail_n)
        ok = ok && p.tail.frame == n - 1 && p.tail.n == tail_n && p.tail.lo == 0 && p.tail.hi == tail_n && p.tail.s0 == 0;
    else
        ok = ok && p.tail.lo >= p.tail.hi;
    if (!ok) {
        failures++;
        std::printf("FAIL: %u frames, the last says %u, capacity %llu: samples %llu fast %u route %u flags %u tail [%u, %u) of %u in frame %u\n", n,
            n ? lengths[n - 1] : 0u, (unsigned long long)capacity, (unsigned long long)p.samples, p.fast_frames, p.route, p.flags, p.tail.lo, p.tail.hi, p.tail.n,
            p.tail.frame);
    }
}

} // namespace

int main()
{
    const uint64_t roomy = ~0ull;
    check({}, roomy);                // n = 0
    check({}, 0);
    check({ 1500 }, roomy);          // one frame of 1500 samples: fast count 0
    check({ 1500 }, 1500);
    check({ 1500 }, 1499);           // ... that does not fit
    for (uint32_t n_last : { 2048u, 2049u, 4095u, 4096u, 0u, 1u, 2047u, 65535u, kHeaderless })
        for (uint32_t front : { 0u, 1u, 3u }) {
            std::vector<uint32_t> ls(front, 2048);
            ls.push_back(n_last);
            check(ls, roomy);
            const uint64_t s = n_last != kHeaderless && n_last >= 1 && n_last <= 4095 && n_last != 2048 ? 2048ull * front + n_last : 2048ull * (front + 1);
            check(ls, s);
            check(ls, s - 1);
            check(ls, 0);
        }
    check({ 1000, 2048, 777 }, roomy); // a front frame's length is not the plan's business
    check({ 777, 2048 }, roomy);
    std::printf("%d cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
