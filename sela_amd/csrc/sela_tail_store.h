// sela_tail_store.h -- what a store kernel makes of the records of a frame whose subframes were decoded one wave each into the
// workspace: the record, the list of writes and the combine of one sample.  Device code, shared by the kernels of the long last
// frame (sela_window_whole.hip: k_tailwin_store, k_whole_store) and by the 32-bit windows (sela_window32.hip:
// k_window32_store).  Include it inside namespace sela, behind sela_window_tail.h.
#ifndef SELA_TAIL_STORE_H_
#define SELA_TAIL_STORE_H_

struct TailSub { // one per (window, subframe position), written by k_tailwin_decode
    uint8_t channel, type, parent, ok;
    uint32_t n, flags, pad;
};
static_assert(sizeof(TailSub) == 16, "workspace formula");

constexpr uint32_t kTailPlanThreads = 256, kTailStoreThreads = 256, kTailChannels = 8, kTailNoParent = 0xFFu;

// What thread 0 of a store makes of a frame's records: k_interleave16's list of writes (src/frame/frame_decoder.cpp:17-69) --
// independent subframes first, then dependent ones in subframe order -- under its rules: the channel and the parent exist, the
// parent is long enough, every channel ends at the length n_frame that the frame's first subframe says.  Returns the frame's flags;
// ok == 0: the decode declined a subframe or the rules refuse the layout, and nothing is to be stored.
struct TailStoreList {
    uint32_t sub[kTailChannels], n[kTailChannels], dst[kTailChannels], parent[kTailChannels], cnt[kTailChannels];
    uint32_t ops, ok;
};
__device__ inline uint32_t tail_store_list(const TailSub* __restrict__ inf, uint32_t channels /* <= kTailChannels */, uint32_t n_frame, TailStoreList& l)
{
    uint32_t flags = 0;
    bool declined = false;
    for (uint32_t c = 0; c < channels; c++) {
        l.cnt[c] = 0;
        declined |= !inf[c].ok;
        flags |= inf[c].flags;
    }
    bool bad = false;
    uint32_t k = 0;
    for (uint32_t type = 0; type < 2 && !declined; type++)
        for (uint32_t c = 0; c < channels; c++) {
            const TailSub si = inf[c];
            if (si.type != type)
                continue;
            if (si.channel >= channels || (type == 1 && (si.parent >= channels || l.cnt[si.parent] < si.n))) {
                bad = true;
                continue;
            }
            l.sub[k] = c, l.n[k] = si.n, l.dst[k] = si.channel, l.parent[k] = type == 1 ? si.parent : kTailNoParent;
            k++;
            l.cnt[si.channel] = si.n;
        }
    for (uint32_t c = 0; c < channels && !declined; c++)
        bad |= l.cnt[c] != n_frame;
    if (bad)
        flags |= SELA_HIP_FLAG_BAD_FRAME;
    l.ops = k, l.ok = declined || bad ? 0u : 1u;
    return flags;
}

// Sample i of every channel of the frame, by the list, into column t of the table (32-bit: narrowed where it is stored).
__device__ inline void tail_store_sample(const int32_t* __restrict__ fd, const TailStoreList& l, uint32_t i, int32_t (*tab)[kTailStoreThreads], uint32_t t)
{
    for (uint32_t k = 0; k < l.ops; k++) {
        if (i >= l.n[k])
            continue;
        int32_t v = fd[(size_t)l.sub[k] * kTailStride + i];
        const uint32_t p = l.parent[k];
        if (p != kTailNoParent)
            v = (int32_t)((uint32_t)tab[p][t] - (uint32_t)v);
        tab[l.dst[k]][t] = v;
    }
}

#endif // SELA_TAIL_STORE_H_
