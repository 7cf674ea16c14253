// workspace_carve.cpp -- sela::Carve (sela_amd/csrc/sela_workspace.h) on its own, under ASan + UBSan (tests/test_workspace_cpu.py).
//
// A made-up workspace of mixed-type pieces with a nested call's range inside, the way the library's descriptions are written: one
// function over a Carve&.  It is measured, then placed into malloc'ed buffers of exactly bytes() at each of the 256 possible
// misalignments of the base; every byte of every piece is written (a piece that left the buffer, or the sanitizer's redzone around
// it, ends the program), and the pieces listed by the measuring pass are held against the pointers of the placing pass.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sela_workspace.h"

using sela::Carve;
using sela::CarvePieces;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            failures++;                                                      \
        }                                                                    \
    } while (0)

struct Record { // (12 bytes: a size that is no power of two)
    uint32_t a, b, c;
};

struct InnerWs {
    uint16_t* shorts;
    double* doubles;
};
static InnerWs carve_inner(Carve& c, uint64_t n)
{
    InnerWs w;
    w.shorts = c.take<uint16_t>(3 * n + 1);
    w.doubles = c.take<double>(n);
    return w;
}
static uint64_t inner_bytes(uint64_t n, Carve* at = nullptr)
{
    return sela::measured(at, [&](Carve& c) { carve_inner(c, n); });
}

struct OuterWs {
    uint8_t* bytes;
    Record* records;
    uint32_t* none; // a piece of no elements
    void* inner;    // a nested call's workspace, handed on whole
    uint64_t* words;
    uint8_t* last;
};
static OuterWs carve_outer(Carve& c, uint64_t n)
{
    OuterWs w;
    w.bytes = c.take<uint8_t>(n);
    w.records = c.take<Record>(n);
    w.none = c.take<uint32_t>(0);
    Carve inner = c.sub(inner_bytes(n));
    w.inner = inner.base();
    inner_bytes(n, &inner); // (its pieces, for a listing)
    w.words = c.take<uint64_t>(n / 2);
    w.last = c.take<uint8_t>(1);
    return w;
}

template <typename T>
static void fill(T* p, uint64_t count, int value)
{
    std::memset(static_cast<void*>(p), value, count * sizeof(T));
}

static void one_shape(uint64_t n)
{
    // the measuring pass, listing its pieces
    std::vector<uint64_t> pairs(2 * 16);
    CarvePieces pieces = { pairs.data(), 16, 0 };
    Carve measure(&pieces);
    carve_outer(measure, n);
    const uint64_t bytes = measure.bytes();
    CHECK(pieces.count == 7); // bytes, records, none, the inner call's two, words, last
    CHECK(bytes % 256 == 0 && bytes == sela::workspace_up(measure.end()) + 256);
    Carve plain;
    carve_outer(plain, n);
    CHECK(plain.bytes() == bytes && plain.end() == measure.end()); // (listing changes nothing)
    for (int i = 0; i < pieces.count; i++) {
        CHECK(pairs[2 * i] % 256 == 0);
        if (i)
            CHECK(pairs[2 * i] >= pairs[2 * i - 2] + pairs[2 * i - 1]); // ascending, no overlap
    }
    CHECK(pairs[2 * 2 + 1] == 0 && pairs[2 * 3] == pairs[2 * 2]); // the empty piece takes no room: the next one starts where it is
    CHECK(pairs[2 * 6] + pairs[2 * 6 + 1] + 255 <= bytes);         // the last piece ends inside, whatever the base's misalignment
    // the inner call's pieces, listed on their own, are the nested ones shifted by one constant
    std::vector<uint64_t> own(2 * 4);
    CarvePieces own_pieces = { own.data(), 4, 0 };
    Carve own_measure(&own_pieces);
    const uint64_t own_bytes = inner_bytes(n, &own_measure);
    CHECK(own_pieces.count == 2 && own_bytes == inner_bytes(n));
    for (int i = 0; i < 2; i++)
        CHECK(pairs[2 * (3 + i)] - own[2 * i] == pairs[2 * 3] - own[0] && pairs[2 * (3 + i) + 1] == own[2 * i + 1]);
    CHECK(pairs[2 * 3] + own_bytes <= pairs[2 * 5]); // the range nests: the piece behind it starts behind all of it

    // the placing pass, at every misalignment
    for (unsigned shift = 0; shift < 256; shift++) {
        // (an allocation of bytes() + shift, used from `shift` on: exactly bytes() bytes, the redzone right behind them)
        unsigned char* const block = static_cast<unsigned char*>(std::malloc(bytes + shift));
        unsigned char* const ws = block + shift;
        Carve place(ws);
        const OuterWs w = carve_outer(place, n);
        const uintptr_t base = (uintptr_t)place.base();
        CHECK(base % 256 == 0 && base >= (uintptr_t)ws && base - (uintptr_t)ws < 256);
        CHECK(place.end() == measure.end() && base + place.end() <= (uintptr_t)ws + bytes);
        const uintptr_t placed[7] = { (uintptr_t)w.bytes, (uintptr_t)w.records, (uintptr_t)w.none, 0, 0, (uintptr_t)w.words, (uintptr_t)w.last };
        for (int i = 0; i < 7; i++)
            if (i != 3 && i != 4)
                CHECK(placed[i] - base == pairs[2 * i]); // the same offsets as measured
        CHECK((uintptr_t)w.inner - base == pairs[2 * 3]);
        Carve inner(w.inner); // the nested call, given its range as a pointer, as a launch is
        const InnerWs in = carve_inner(inner, n);
        CHECK((uintptr_t)in.shorts - base == pairs[2 * 3] && (uintptr_t)in.doubles - base == pairs[2 * 4]);
        fill(w.bytes, n, 0x11);
        fill(w.records, n, 0x22);
        fill(in.shorts, 3 * n + 1, 0x33);
        fill(in.doubles, n, 0x44);
        fill(w.words, n / 2, 0x55);
        fill(w.last, 1, 0x66);
        // ... and no piece was written over by a later one
        CHECK(n == 0 || (w.bytes[0] == 0x11 && w.bytes[n - 1] == 0x11 && w.records[n - 1].c == 0x22222222u && in.doubles[n - 1] != 0.0));
        CHECK(in.shorts[3 * n] == 0x3333 && w.last[0] == 0x66 && (n < 2 || w.words[n / 2 - 1] == 0x5555555555555555ull));
        std::free(block);
    }
}

int main()
{
    // nothing taken: the base's alignment alone; a null base is measured, never offset
    Carve empty;
    CHECK(empty.end() == 0 && empty.bytes() == 256 && empty.base() == nullptr);
    CHECK(empty.take<uint32_t>(0) == nullptr && empty.end() == 0 && empty.bytes() == 256);
    CHECK(sela::workspace_up(0) == 0 && sela::workspace_up(1) == 256 && sela::workspace_up(256) == 256 && sela::workspace_up(257) == 512);
    // a listing with no room counts on
    CarvePieces none = { nullptr, 0, 0 };
    Carve counting(&none);
    carve_outer(counting, 5);
    CHECK(none.count == 7);
    for (uint64_t n : { 0ull, 1ull, 2ull, 21ull, 85ull, 256ull, 1000ull })
        one_shape(n);
    std::printf("workspace_carve: %d failures\n", failures);
    return failures ? 1 : 0;
}
