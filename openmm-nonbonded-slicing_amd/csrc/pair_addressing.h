// pair_addressing.h -- host only: may a launch of the packed pair kernels (direct.hip) address its arrays with 32-bit byte offsets?
//
// The packed kernels form every per-tile address as `scalar base + 32-bit byte offset` (one shifted index per tile, the base as the scalar
// operand of the load or atomic).  That is right only while each array they index that way stays below 2^31 bytes; the instantiations in
// namespace `wide` keep 64-bit indices for everything larger.  The choice is made where the engine fills DirectParams (wideOffsets), from
// the capacities of the arrays -- not from the counts of one neighbour list, so that a rebuild never changes the kernel of a captured step.
// No HIP here: tests/test_pair_kernel_addressing.py compiles this header with the host compiler alone.
#pragma once
#include <cstdint>

namespace snb {

constexpr int64_t kOffset32Limit = int64_t(1) << 31;      // bytes: every offset stays a non-negative int (-1 marks a lane with nothing to scatter)
constexpr int64_t kMul24Limit = int64_t(1) << 24;         // the offset of an atom slot is one 24-bit multiply: slot index x bytes per slot

// bytes between the accumulators of two consecutive atom slots of one force component: fs elements of 4 bytes, or of 8 (fixed point)
inline int64_t forceSlotBytes(int fs, bool fixed) { return int64_t(fs) * (fixed ? 8 : 4); }

struct PairArrayExtents {
    int64_t atomSlots;       // padded atom count: the force components hold atomSlots x fs elements
    int fs; bool fixed;      // index stride of an atom in a force component; 64-bit fixed-point elements
    int64_t tileCapacity;    // tiles the list arrays are allocated for: tileJ 128 bytes, tileInfo 16 bytes a tile
    int64_t maskCapacity;    // exclusion-mask tiles allocated: 128 bytes each
};

inline bool pairOffsetsFit32(const PairArrayExtents& e) {
    if (e.atomSlots < 0 || e.fs <= 0 || e.tileCapacity < 0 || e.maskCapacity < 0) return false;
    const int64_t slot = forceSlotBytes(e.fs, e.fixed);
    if (slot >= kMul24Limit || e.atomSlots > kMul24Limit) return false;
    if (e.atomSlots * slot >= kOffset32Limit) return false;                     // the force components
    if (e.tileCapacity >= kOffset32Limit / 128) return false;                   // tileJ (tileInfo is an eighth of it)
    if (e.maskCapacity >= kOffset32Limit / 128) return false;                   // masks
    return true;
}

}  // namespace snb
