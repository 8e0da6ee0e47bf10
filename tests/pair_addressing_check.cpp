// The host guard of the packed pair kernels' 32-bit addressing (csrc/pair_addressing.h), as a program: one line per case on standard
// input -- atomSlots fs fixed tileCapacity maskCapacity -- and "1" (32-bit offsets) or "0" (the 64-bit kernels) per line on standard output.
// Built and run by tests/test_pair_kernel_addressing.py with the host compiler; no HIP, no GPU.
#include "pair_addressing.h"
#include <cstdio>

int main() {
    long long atoms, tiles, masks; int fs, fixed;
    while (std::scanf("%lld %d %d %lld %lld", &atoms, &fs, &fixed, &tiles, &masks) == 5) {
        const snb::PairArrayExtents e = {atoms, fs, fixed != 0, tiles, masks};
        std::printf("%d\n", snb::pairOffsetsFit32(e) ? 1 : 0);
    }
    return 0;
}
