// sela_group_reduce.h -- one value per lane put together over every group of consecutive lanes that hold one bucket: what the
// envelope kernels of sela_envelope.hip and sela_envelope32.hip (5.32) share.  Device code only.
#ifndef SELA_GROUP_REDUCE_H_
#define SELA_GROUP_REDUCE_H_

#include <cstdint>

#include <hip/hip_runtime.h>

namespace sela {

// One value per lane put together over every group of `lanes` consecutive lanes (8, 16, 32 or 64, wave-uniform; op: add or
// unsigned max, for both of which a 0 changes nothing).  Butterflies within a row of 16 -- quad_perm, row_half_mirror,
// row_mirror: every lane of a group of 8 or 16 ends with its group's result -- then wave_sum_small's row_bcast rungs under their
// row masks.  The LAST FOUR lanes of every group hold the group's result, whatever `lanes` is.
template <typename Op>
__device__ __forceinline__ uint32_t group_reduce(uint32_t v, uint32_t lanes, Op op)
{
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1 /* quad_perm:[1,0,3,2] */, 0xf, 0xf, false));
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E /* quad_perm:[2,3,0,1] */, 0xf, 0xf, false));
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141 /* row_half_mirror */, 0xf, 0xf, false));
    if (lanes >= 16)
        v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140 /* row_mirror */, 0xf, 0xf, false));
    if (lanes >= 32)
        v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142 /* row_bcast:15 */, 0xa, 0xf, false));
    if (lanes >= 64)
        v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143 /* row_bcast:31 */, 0xc, 0xf, false));
    return v;
}

} // namespace sela
#endif
