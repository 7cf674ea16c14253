// The layout of sela_hip_level32 as a C++ compiler sees include/sela_hip.h: size, alignment and the offset of every field, one line
// that tests/test_levels32_entry_checks.py holds against codec.LEVEL32_DTYPE.
#include <cstddef>
#include <cstdio>

#include "sela_hip.h"

int main()
{
    std::printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(sela_hip_level32), alignof(sela_hip_level32), offsetof(sela_hip_level32, peak),
        offsetof(sela_hip_level32, samples), offsetof(sela_hip_level32, sum), offsetof(sela_hip_level32, sum_squares_lo), offsetof(sela_hip_level32, sum_squares_hi));
    return 0;
}
