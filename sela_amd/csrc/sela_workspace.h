// sela_workspace.h -- how every device-pointer call cuts its caller-allocated workspace into pieces.
//
// A workspace is described ONCE, by a function that takes a Carve& and the call's shape and returns a struct of typed pointers
// (carve_encode, carve_decode_n, ...: beside the launch that uses them).  The *_workspace_bytes function runs it on a measuring
// Carve and asks bytes(); the launch runs it on the caller's pointer; a debug hook that reads one piece back runs it too and takes
// that member.  So a call's size and its pointers cannot disagree.
//
// Every piece starts at a multiple of 256 bytes from the base, and the base is the caller's pointer aligned up to 256: include/
// sela_hip.h promises the callers that any alignment will do.  Plain C++17, no HIP: tests/c/workspace_carve.cpp compiles it alone.
#ifndef SELA_WORKSPACE_H_
#define SELA_WORKSPACE_H_

#include <cstddef>
#include <cstdint>

namespace sela {

constexpr uint64_t kWorkspaceAlign = 256;
constexpr uint64_t workspace_up(uint64_t b) { return (b + (kWorkspaceAlign - 1)) & ~(kWorkspaceAlign - 1); }

// The (offset, bytes) of every piece taken, from the outermost Carve's aligned base: what sela_hip_debug_workspace_pieces
// returns.  count runs on beyond capacity; only the first `capacity` pairs are written.
struct CarvePieces {
    uint64_t* pairs;
    int capacity, count;
};

class Carve {
public:
    Carve() = default;                                                     // to measure: the pointers it hands out are offsets, never dereferenced
    explicit Carve(const void* base) : base_(workspace_up((uintptr_t)base)), root_(base_) {}
    explicit Carve(CarvePieces* pieces) : pieces_(pieces) {}               // to measure, and to list the pieces

    // `count` elements of T at the next multiple of 256.  (count 0: a pointer to nothing, at the place the next piece gets.)
    template <typename T>
    T* take(uint64_t count)
    {
        const uint64_t at = workspace_up(at_);
        at_ = at + count * sizeof(T);
        note(at, count * sizeof(T));
        return reinterpret_cast<T*>((uintptr_t)(base_ + at));
    }

    // The next `bytes` bytes (from a multiple of 256) as a workspace of their own, for a call that carves its own: `bytes` is that
    // call's size, base alignment included, so the range is handed on whole and nothing is subtracted or added here.
    Carve sub(uint64_t bytes)
    {
        Carve inner;
        inner.base_ = base_ + workspace_up(at_);
        inner.root_ = root_;
        inner.pieces_ = pieces_;
        at_ = workspace_up(at_) + bytes;
        return inner;
    }

    bool listing() const { return pieces_ != nullptr; }                      // someone wants the pieces: a stacked description then runs its inner calls' too
    void* base() const { return reinterpret_cast<void*>((uintptr_t)base_); } // the aligned base: what a sub() range's own call is given
    uint64_t end() const { return at_; }                                     // where the last piece ends, from the aligned base
    uint64_t bytes() const { return workspace_up(at_) + kWorkspaceAlign; }   // the size to ask of the caller: the end, and the base's alignment

private:
    void note(uint64_t at, uint64_t size)
    {
        if (!pieces_)
            return;
        if (pieces_->count < pieces_->capacity) {
            pieces_->pairs[2 * pieces_->count] = base_ - root_ + at;
            pieces_->pairs[2 * pieces_->count + 1] = size;
        }
        pieces_->count++;
    }
    uint64_t base_ = 0, root_ = 0, at_ = 0;
    CarvePieces* pieces_ = nullptr;
};

// What a *_workspace_bytes function returns: its call's description run on `at` -- a Carve that lists its pieces, or a sub() range
// of another call's workspace -- or on a fresh measuring one.
template <typename Describe>
size_t measured(Carve* at, Describe describe)
{
    Carve fresh;
    Carve& c = at ? *at : fresh;
    describe(c);
    return (size_t)c.bytes();
}

} // namespace sela
#endif
