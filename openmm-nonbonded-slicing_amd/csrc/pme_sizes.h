// LDS arithmetic of the kernels whose dynamic LDS request grows with the subset count, and the guard snb_create derives from it.
// Host code without HIP: pme.hip sizes the launch of k_convolveX with it, engine.hip refuses what cannot run, tests/pme_sizes_check.cpp
// checks it on the CPU.
#pragma once
#include <cstddef>

namespace snb {

// k_convolveX (pme.hip) keeps, per (ky, kz) column, two buffers of nx points for every held subset and one line of the reciprocal-space
// kernel; beside the columns one table of nx roots of unity.  realBytes: 4 (single, mixed) or 8 (double); a complex value is two reals.
struct ConvLds {
    size_t perCol;      // bytes per column
    int NB;             // columns per work-group: 8, 4, 2 or 1
    size_t total;       // the dynamic LDS request, perCol * NB + roots of unity
};
inline size_t convLdsPerCol(int nx, int nsub, size_t realBytes) { return (size_t)2 * nx * nsub * (2 * realBytes) + (size_t)nx * realBytes; }
inline size_t convLdsTotal(int nx, int nsub, size_t realBytes, int NB) { return convLdsPerCol(nx, nsub, realBytes) * NB + (size_t)nx * (2 * realBytes); }
// columns per work-group: 8 adjacent (ky,kz) columns are one 64-byte line per (subset, kx) row -- measured on c3 (4 subsets):
// NB = 4: 68 us, 5: 64, 7: 69, 8: 48.5, 16: 60.5 -- so 8 when that fits the budget (SNB_CONV_LDS_KB, 72 KB), else 4, 2, 1
inline ConvLds convLds(int nx, int nsub, size_t realBytes, int budgetKB) {
    ConvLds c;
    c.perCol = convLdsPerCol(nx, nsub, realBytes);
    c.NB = 8;
    while (c.NB > 1 && c.perCol * c.NB > (size_t)budgetKB * 1024) c.NB >>= 1;
    c.total = convLdsTotal(nx, nsub, realBytes, c.NB);
    return c;
}
// static LDS of k_convolveX beside the request: s_red, (NT / 64) * 4 doubles at NT = 512 (pme.hip static_asserts it)
constexpr size_t kConvStaticLds = 256;
// the guard: the smallest request the launch can fall back to (one column per work-group) must fit the device beside the static part
inline size_t convLdsNeed(int nx, int nsub, size_t realBytes) { return convLdsTotal(nx, nsub, realBytes, 1) + kConvStaticLds; }
inline bool convLdsFits(int nx, int nsub, size_t realBytes, size_t deviceLimit) { return convLdsNeed(nx, nsub, realBytes) <= deviceLimit; }

// The pair-list energy bodies (direct.hip exceptionsBody / exclusionAtomsBody) reduce their slice energies in 2 S doubles of dynamic LDS,
// inside the tile kernels or in kernels of their own, none of which raises its limit: the request and the kernel's static LDS (12.1 KB in the
// largest tile kernel) share the 64 KB every kernel may use without asking.  48 KB is S = 3072 slices: 77 subsets.
constexpr size_t kPairListLdsMax = 48 * 1024;
inline size_t pairListLds(long long nSlices) { return (size_t)16 * (size_t)nSlices; }
inline bool pairListLdsFits(long long nSlices) { return pairListLds(nSlices) <= kPairListLdsMax; }

}  // namespace snb
