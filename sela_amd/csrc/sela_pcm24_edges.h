// sela_pcm24_edges.h -- which bytes of a packed 3-byte output a store round of k_window32_store (sela_window32.hip; DESIGN.md
// 5.23) writes, and how.  Plain C++ compiled for the device and for the host, so that tests/c/pcm24_edges.cpp walks exactly the
// arithmetic the kernel uses, beside sela_pcm_layout.h's.
//
// A workgroup's SHARE of the output is a run of bytes [B0, B1) at any byte phase: (hi - lo) * channels values of three bytes.
// It stores the share in ROUNDS of consecutive values, round r being the bytes [b0, b1) with b0 = B0 for the first and b1 = B1
// for the last.  A round OWNS [own0, own1): its bytes with every boundary between two rounds of a share moved down to a multiple
// of 4 -- the dword that straddles it belongs to the later round, which therefore also forms the trailing bytes of the value in
// front of its own (at most three bytes, so one value: the `lead`).  So only the two ends of a SHARE are ever stored as single
// bytes -- `head` bytes up to the first multiple of 4, `tail` bytes behind the last -- and never a byte of a neighbour's share;
// everything between goes out as aligned dwords.
#ifndef SELA_PCM24_EDGES_H_
#define SELA_PCM24_EDGES_H_

#include <cstdint>

#include "sela_pcm_layout.h" // SELA_PCM_HD

namespace sela {

struct Pcm24Span {
    uint64_t head_at; // bytes stored singly: [head_at, head_at + head)
    uint32_t head;
    uint64_t mid_at;  // whole dwords: `dwords` of them from mid_at, a multiple of 4
    uint64_t dwords;
    uint64_t tail_at; // bytes stored singly: [tail_at, tail_at + tail)
    uint32_t tail;
};

// The round [b0, b1) of a share: first / last say whether b0 / b1 is the share's own end.
SELA_PCM_HD Pcm24Span pcm24_span(uint64_t b0, uint64_t b1, bool first, bool last)
{
    const uint64_t own0 = first ? b0 : b0 & ~(uint64_t)3;
    uint64_t own1 = last ? b1 : b1 & ~(uint64_t)3;
    if (own1 < own0) // (a first round shorter than its way to a multiple of 4 that is not the last: it owns nothing)
        own1 = own0;
    const uint64_t up = (own0 + 3) & ~(uint64_t)3;
    Pcm24Span s;
    s.head_at = own0;
    s.head = (uint32_t)((up < own1 ? up : own1) - own0);
    s.mid_at = own0 + s.head;
    s.dwords = (own1 - s.mid_at) / 4;
    s.tail_at = s.mid_at + 4 * s.dwords;
    s.tail = (uint32_t)(own1 - s.tail_at);
    return s;
}

// The round's values stand in a table with the lead in front: slot 0 is the value in front of the round's first, slot 1 + v is
// the round's value v.  Byte `at` of the output (at >= b0 - 3) is byte pcm24_byte_of(at - (b0 - 3)) of slot pcm24_slot_of(same).
SELA_PCM_HD uint32_t pcm24_slot_of(uint32_t from_lead) { return from_lead / 3; }
SELA_PCM_HD uint32_t pcm24_byte_of(uint32_t from_lead) { return from_lead % 3; }

// One output byte, and the aligned dword whose first byte it is, from the table.
template <typename Table>
SELA_PCM_HD uint8_t pcm24_byte(const Table& slots, uint32_t from_lead)
{
    return (uint8_t)((uint32_t)slots[pcm24_slot_of(from_lead)] >> (8 * pcm24_byte_of(from_lead)));
}
template <typename Table>
SELA_PCM_HD uint32_t pcm24_dword(const Table& slots, uint32_t from_lead)
{
    const uint32_t q = pcm24_slot_of(from_lead); // four bytes lie in two neighbouring values; the dword's last byte is in slot q + 1
    const uint64_t both = (uint64_t)((uint32_t)slots[q] & 0xFFFFFFu) | (uint64_t)((uint32_t)slots[q + 1] & 0xFFFFFFu) << 24;
    return (uint32_t)(both >> (8 * pcm24_byte_of(from_lead)));
}

} // namespace sela
#endif // SELA_PCM24_EDGES_H_
