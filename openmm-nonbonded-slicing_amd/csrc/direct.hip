// direct.hip -- direct-space sliced pair kernel for gfx950 (MI355X), plus the per-pair list kernels
// (1-4 exceptions, Ewald exclusion corrections).
//
// What it replaces in the reference: the pair-interaction snippet platforms/common/src/kernels/coulombLennardJones.cc:1-124
// (spliced into OpenMM's 32x32 tile kernel), the exception snippet nonbondedExceptions.cc:1-25 and the exclusion
// snippet pmeExclusions.cc:1-47; arithmetic parity is with platforms/reference/src/ReferenceSlicedLJCoulombIxn.cpp:367-506,
// 571-631 and ReferenceSlicedLJCoulomb14.cpp:61-95.
//
// MI355X mapping (not the reference's): one 64-lane wavefront owns one 32-atom i-block.  Lane l holds i-atom
// (l & 31); the two 32-lane halves work on different j-atoms of the same 32-atom j-tile, so a tile is 16 steps of
// 64 pair slots.  j-atoms are staged once per tile into LDS (posq b128 + sigeps b64, stored twice so the rotated
// read index il+h+2s needs no wrap), j-forces are accumulated with LDS float atomics (ds_add_f32) and flushed with
// one global atomic per j-atom and component.  Because blocks are subset-uniform, the slice of a tile is a scalar:
// lambda scaling costs two multiplies per TILE and per-slice energies are two accumulators per tile -- there is no
// per-pair slice arithmetic at all (the reference computes the slice index and loads LAMBDA[slice] per pair).
#include "snb_internal.h"
#include "switches.h"
#include "pair_math.h"
#include <hip/hip_ext.h>
#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#ifndef SNB_DIRECT_F64_WAVES
#define SNB_DIRECT_F64_WAVES 2      // waves per SIMD the double-precision pair kernel is compiled for (256 VGPRs: no spills; measured on c5)
#endif
namespace snb {

// Force accumulation of atom slot `a`.  SNB_MIXED engines (P::fixed) keep the direct-space accumulators as 64-bit fixed point, 2^32 per
// kJ/mol/nm, the way every GPU platform of the reference does (realToFixedPoint; CommonNonbondedSlicingKernels.cpp adds into
// getLongForceBuffer, pme.cc:381-389): integer sums do not depend on the order in which waves arrive, so the force of a step is
// reproducible bit for bit.  The component arrays are then arrays of 64-bit words behind the same base pointers.
__device__ inline unsigned long long toFixedForce(float v) { return (unsigned long long)(long long)(v * 4294967296.0f); }
template <typename P> __device__ inline void fAdd(const P& p, float* comp, size_t a, float v) {
    if (p.fixed) { __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(comp) + a * p.fs, toFixedForce(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); return; }
    gAdd(comp + a * p.fs, v);
}
template <typename P> __device__ inline void fAdd(const P& p, double* comp, size_t a, double v) { gAdd(comp + a * p.fs, v); }
// (the packed tile kernel takes the choice as a template parameter: the run-time test cost the default path 2.7 % on c3)
template <bool FIXED, typename P> __device__ inline void fAddT(const P& p, float* comp, size_t a, float v) {
    if constexpr (FIXED) __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(comp) + a * p.fs, toFixedForce(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else gAdd(comp + a * p.fs, v);
}
// The same accumulation at a 32-bit byte offset from the component's base (p.fBytes per atom slot; launches whose force arrays stay below
// 2^31 bytes, pair_addressing.h): the atomic takes the base as its scalar operand and the offset as it stands, where the 64-bit index
// above costs a multiply, a shift and an add per component.  loadAt: a load addressed the same way (list entries, tile headers, masks).
template <typename T> __device__ __forceinline__ T loadAt(const void* base, unsigned byteOffset) { return *reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + byteOffset); }
template <bool FIXED> __device__ inline void fAddAt(float* comp, unsigned byteOffset, float v) {
    char* const a = reinterpret_cast<char*>(comp) + byteOffset;
    if constexpr (FIXED) __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(a), toFixedForce(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else gAdd(reinterpret_cast<float*>(a), v);
}

// Physical CU of the calling wave: XCC_ID[2:0] (hardware register 20) and the SE_ID | SH_ID | CU_ID bits 15:8 of HW_ID (register 4).
// Used only to count co-resident work-groups of one launch (SNB_CU_SLOTS entries).
__device__ inline int physicalCu() {
    const unsigned xcc = __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20);      // size-1 = 3, offset 0
    const unsigned cu = __builtin_amdgcn_s_getreg((7 << 11) | (8 << 6) | 4);        // size-1 = 7, offset 8
    return (int)(((xcc & 7u) << 8) | (cu & 255u));
}

// CU-limited launch of an overlapped step (engine.hip, overlapMode): may this work-group stay on its CU?  Called by every thread (one barrier).
// The reciprocal pipeline's work-groups need what the limit leaves free IN ONE PIECE: registers are allocated as contiguous ranges per
// wave, and two resident pair work-groups picked by order of arrival sit at random two of the four positions the dispatcher filled,
// which leaves the plane kernel's 4 x 64 registers per SIMD without room on a third of the CUs (measured: it then waits for the pair
// kernel to end).  So the rule is positional: a work-group stays when each of its four waves was allocated within the lowest
// cuBaseMax + its own size registers of its SIMD (VGPR_BASE, bits 5:0 of GPR_ALLOC, in units of 8 registers) -- on an idle CU exactly the
// first cuLimit work-groups the dispatcher placed -- and everything above them stays free and contiguous.  cuBaseMax < 0: the arrival-count rule.
// cuSlots[key]: arrivals in the low half, work-groups that stayed in the high half (statistics, SNB_OVERLAP_DEBUG).
template <typename P> __device__ inline bool cuResident(const P& p) {
    __shared__ int s_base[4];
    __shared__ int s_stay;
    if ((threadIdx.x & 63) == 0) s_base[threadIdx.x >> 6] = (int)__builtin_amdgcn_s_getreg((5 << 11) | (0 << 6) | 5);
    __syncthreads();
    if (threadIdx.x == 0) {
        const int maxBase = max(max(s_base[0], s_base[1]), max(s_base[2], s_base[3]));
        const int key = physicalCu();
        int stay, old;
        if (p.cuBaseMax >= 0) { stay = maxBase <= p.cuBaseMax ? 1 : 0; old = atomicAdd(&p.cuSlots[key], stay ? 0x10001 : 1) & 0xFFFF; }
        else { old = atomicAdd(&p.cuSlots[key], 1) & 0xFFFF; stay = old < p.cuLimit ? 1 : 0; if (stay) atomicAdd(&p.cuSlots[key], 0x10000); }
        s_stay = stay;
        if (p.cuTrace && old < 4) { p.cuTrace[(key * 4 + old) * 2] = (int)__builtin_amdgcn_s_getreg((31 << 11) | 5) ^ (stay << 31); p.cuTrace[(key * 4 + old) * 2 + 1] = (int)__builtin_amdgcn_s_getreg((31 << 11) | 6); }      // GPR_ALLOC (top bit: stayed), LDS_ALLOC
    }
    __syncthreads();
    return s_stay != 0;
}

// Work items of an overlapped step are handed out through SNB_WORK_SHARDS counters, each on a 128-byte line of its own; counter k owns items
// k, k + SNB_WORK_SHARDS, ... (the list is sorted longest first, so every counter's sequence is too).  One counter for all waves serialises
// at ~15 ns per claim (same-address device-scope atomics: 28 768 claims = 0.44 ms, measured) -- sixteen are far below that rate.
// A wave starts at a home counter and, once that one is exhausted, reads all counters in one load and moves to the next one with items left.
// FRESH: the counters' per-lane address is formed where it is used (the rare path of an exhausted counter) instead of being held in two
// registers for the whole kernel -- the derivative kernel, which has none to spare (k_directPackedSelected).
template <bool FRESH = false> struct WorkClaim {
    int* ctr; int numWork, shard, lane;
    __device__ int myLane() const { int l = lane; if constexpr (FRESH) asm volatile("" : "+v"(l)); return l; }
    __device__ int issue() const { int v = 0; if (lane == 0) v = atomicAdd(&ctr[shard * 32], 1); return v; }      // lane 0 holds the claim
    __device__ bool anyLeft() const {      // (one load of all counters: a launch that arrives when everything is claimed leaves after one round trip)
        int left = 0;
        const int l = myLane();
        if (l < SNB_WORK_SHARDS) left = (numWork - l + SNB_WORK_SHARDS - 1) / SNB_WORK_SHARDS - __hip_atomic_load(&ctr[l * 32], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return __ballot(left > 0) != 0;
    }
    __device__ int resolve(int v) {      // item index of a claim issued on `shard`, moving on to other counters when that one has run out; numWork: no items left
        int idx = shard + SNB_WORK_SHARDS * __builtin_amdgcn_readfirstlane(v);
        while (idx >= numWork) {
            int left = 0;
            const int l = myLane();
            if (l < SNB_WORK_SHARDS) left = (numWork - l + SNB_WORK_SHARDS - 1) / SNB_WORK_SHARDS - __hip_atomic_load(&ctr[l * 32], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned m = (unsigned)__ballot(left > 0);
            if (m == 0) return numWork;
            const int from = (shard + 1) & (SNB_WORK_SHARDS - 1);
            const unsigned rot = ((m | (m << SNB_WORK_SHARDS)) >> from) & ((1u << SNB_WORK_SHARDS) - 1);
            shard = (from + __builtin_ctz(rot)) & (SNB_WORK_SHARDS - 1);
            idx = shard + SNB_WORK_SHARDS * __builtin_amdgcn_readfirstlane(issue());
        }
        return idx;
    }
};


// A field of the kernel's FIRST argument, read from the kernel-argument segment behind a barrier the compiler cannot move the load across.
// Kernel arguments are scalar loads the compiler hoists to the kernel's entry and keeps in SGPRs for the whole kernel; what only a rare
// path reads (the derivative kernel's energy polynomial, 14 coefficients, and its energy partition) then pushes the tile loop over the
// scalar register file, and every trip reloads spilled SGPRs with v_readlane.  Through this the rare path loads its constants itself.
#define SNB_KERNARG __attribute__((address_space(4)))
template <typename T> __device__ __forceinline__ const SNB_KERNARG T* kernargField(size_t offset) {
    const SNB_KERNARG char* k = (const SNB_KERNARG char*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(k));
    return (const SNB_KERNARG T*)(k + offset);
}

// ---- cross-lane helpers -------------------------------------------------------------------------
// DPP row_ror:1 -- every 16-lane row rotates by one lane (lane c receives the value of lane (c-1)&15).
__device__ inline float rowRor1(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x121, 0xF, 0xF, true)); }
__device__ inline double rowRor1(double v) {
    long long b = __builtin_bit_cast(long long, v);
    int lo = (int)b, hi = (int)(b >> 32);
    lo = __builtin_amdgcn_update_dpp(0, lo, 0x121, 0xF, 0xF, false);
    hi = __builtin_amdgcn_update_dpp(0, hi, 0x121, 0xF, 0xF, false);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned)lo);
}

// The 16 pair steps of one tile for this lane's row.  MASKED: the tile carries an exclusion/padding mask;
// SWITCH: LJ switching function active.  Both are wave-uniform and resolved at compile time so that the common
// case (no mask, no switch) carries no test for them in the loop.
// FORCES == false (energy-only tile kernel, ENERGY == true): the energies alone -- no force accumulation, so the force arithmetic is dead code.
// POLYALL (double precision): every polynomial of the forces arithmetic passed the guard of ewald_fit.h, so none is tested in the loop; false: each is
// tested by a wave-uniform branch on the kernel argument (measured on c3 in double: the tests alone cost 18 % of the step, so the common case is compiled without them).
template <typename Real, int MC, bool WRAP, bool ENERGY, bool MASKED, bool SWITCH, bool FORCES = true, bool POLYALL = false>
__device__ __forceinline__ void tileSteps(const DirectParams<Real>& p, const typename Vec<Real>::T4* rdPos, const typename Vec<Real>::T2* rdSe,
                                          const typename Vec<Real>::T4 pi, const typename Vec<Real>::T2 sei, const Real qi, const Real qiS, const Real epsiS,
                                          const Real c6i, const Real lamC, const Real lamL, const unsigned maskWord, const int c,
                                          Real& fix, Real& fiy, Real& fiz, Real& fjx, Real& fjy, Real& fjz, Real& ecl, Real& elj) {
    using T4 = typename Vec<Real>::T4;
    using T2 = typename Vec<Real>::T2;
#pragma unroll 4
        for (int s = 0; s < 16; s++) {
            const T4 xj = rdPos[-s];
            const T2 sj2 = rdSe[-s];
            Real dx = pi.x - xj.x, dy = pi.y - xj.y, dz = pi.z - xj.z;
            if (WRAP) wrapDelta<Real>(dx, dy, dz, p.box, p.invBoxDiag);
            const Real r2 = dx * dx + dy * dy + dz * dz;
            const Real invR = rsq(r2);
            const Real r = r2 * invR;
            bool include = MC == MC_NOCUTOFF ? true : (r2 < p.cutoff2);
            if (MASKED) include = include && !((maskWord >> ((c - s) & 15)) & 1u);

            // Lennard-Jones (ReferenceSlicedLJCoulombIxn.cpp:390-396, 600-616)
            const Real sig = sei.x + sj2.x;
            Real s2 = sig * invR; s2 *= s2;
            const Real s6 = s2 * s2 * s2;
            Real fLJ, eLJ = 0, fC, eC = 0;
            if (ENERGY) {
                const Real es6 = sei.y * sj2.y * s6;
                fLJ = es6 * (Real(12) * s6 - Real(6));
                eLJ = es6 * (s6 - Real(1));
            } else {
                const Real es6 = epsiS * sj2.y * s6;
                fLJ = es6 * (Real(12) * s6 - Real(6));
            }
            if (MC == MC_LJPME && !ENERGY && std::is_same<Real, double>::value && (POLYALL || (p.ewUsePoly & SNB_POLY_DISPERSION))) {
                // forces only, double: 6 c6 [1 - e^{-x}(1 + x + x^2/2 + x^3/6)] / r^6 = 6 c6 r^2 Gd(r^2), x = (alpha_d r)^2, with
                // Gd(r^2) = alpha_d^8 e^{-x} sum_k x^k / (k+4)!  an entire function of r^2: a degree-17 polynomial in the same t as the
                // Ewald factor (~1e-12 of Gd(0) at alpha_d rmax = 2.94; used where the guard of ewald_fit.h keeps it) instead of a double-precision exp and its pre-factors
                const Real t = r2 * p.ewScale - Real(1);
                Real gd = p.dispPoly[SNB_DISP_DEG_F64];
#pragma unroll
                for (int k = SNB_DISP_DEG_F64 - 1; k >= 0; k--) gd = gd * t + p.dispPoly[k];
                const Real c6 = c6i * (Real(8) * sj2.x * sj2.x * sj2.x * sj2.y);
                fLJ += Real(6) * c6 * gd * r2 * lamL;
            } else if (MC == MC_LJPME) {
                // multiplicative grid term + potential shifts (:398-426)
                const Real dar2 = p.alphaD * p.alphaD * r2;
                const Real dar4 = dar2 * dar2, dar6 = dar4 * dar2;
                const Real invR2 = invR * invR;
                const Real c6 = c6i * (Real(8) * sj2.x * sj2.x * sj2.x * sj2.y);
                const Real coef = invR2 * invR2 * invR2 * c6;
                const Real expd = fexp(-dar2);
                const Real epre = Real(1) + dar2 + Real(0.5) * dar4;
                const Real dpre = epre + dar6 * Real(1.0 / 6.0);
                const Real fmul = Real(6) * coef * (Real(1) - expd * dpre);
                if (ENERGY) {
                    Real sg2 = sig * sig; const Real sg6 = sg2 * sg2 * sg2 * p.invCut6;
                    eLJ += coef * (Real(1) - expd * epre) + sei.y * sj2.y * (Real(1) - sg6) * sg6 - c6 * p.multShift6;
                    fLJ += fmul;
                } else
                    fLJ += fmul * lamL;
            } else if (MC != MC_NOCUTOFF) {
                if (SWITCH && r > p.switchDist) {        // (:380-384, 428-431)
                    const Real tt = (r - p.switchDist) * p.invSwitchWidth;
                    const Real sw = Real(1) + tt * tt * tt * (Real(-10) + tt * (Real(15) - tt * Real(6)));
                    const Real dsw = tt * tt * (Real(-30) + tt * (Real(60) - tt * Real(30))) * p.invSwitchWidth;
                    Real e0 = eLJ;
                    if (!ENERGY) { const Real es6 = epsiS * sj2.y * s6; e0 = es6 * (s6 - Real(1)); }
                    fLJ = fLJ * sw - e0 * dsw * r;
                    eLJ *= sw;
                }
            }
            // Coulomb
            const Real qq = (ENERGY ? qi : qiS) * xj.w;
            if ((MC == MC_EWALD || MC == MC_LJPME) && !ENERGY && std::is_same<Real, double>::value && (POLYALL || (p.ewUsePoly & SNB_POLY_FORCE))) {
                // forces only: [erfc(ar)/r + 2a/sqrt(pi) e^{-(ar)^2}] = 1/r - r^2 Bt(r^2), Bt a degree-16 polynomial (~6e-12 of Bt(0) at alpha rmax = 2.94; used where the guard of ewald_fit.h keeps it): no libm erfc / exp
                const Real t = r2 * p.ewScale - Real(1);
                Real bt = p.ewPoly[SNB_EW_DEG_F64];
#pragma unroll
                for (int k = SNB_EW_DEG_F64 - 1; k >= 0; k--) bt = bt * t + p.ewPoly[k];
                fC = qq * (invR - r2 * bt);
            } else if (MC == MC_EWALD || MC == MC_LJPME) {
                const Real ar = p.alpha * r;
                const Real ex = expNegAlpha2R2(p.alpha2l2e, p.alpha, r2);
                const Real erfcv = erfcFromExp(ar, ex);
                const Real pref = qq * invR;
                fC = pref * (erfcv + ar * ex * Real(1.1283791670955126));   // 2/sqrt(pi) (:387-388)
                if (ENERGY) eC = pref * erfcv;                                // (:444)
            } else if (MC == MC_RF) {
                fC = qq * (invR - Real(2) * p.krf * r2);                      // (:609)
                if (ENERGY) eC = qq * (invR + p.krf * r2 - p.crf);            // (:619)
            } else {
                fC = qq * invR;                                               // (:611)
                if (ENERGY) eC = fC;
            }
            if (ENERGY) { ecl += include ? eC : Real(0); elj += include ? eLJ : Real(0); }
            if constexpr (FORCES) {
            Real f = ENERGY ? (lamL * fLJ + lamC * fC) : (fLJ + fC);
            f *= invR * invR;
            f = include ? f : Real(0);
            const Real gx = f * dx, gy = f * dy, gz = f * dz;
            fix += gx; fiy += gy; fiz += gz;
            // the accumulator follows its j-slot along the row: rotate in (slot of lane c at step s = slot of lane c-1 at step s-1), then add
            fjx = rowRor1(fjx) - gx; fjy = rowRor1(fjy) - gy; fjz = rowRor1(fjz) - gz;
            }
        }
}

// ---- packed single-precision variant of the 16 pair steps ---------------------------------------------------------
// On gfx950 v_pk_mul_f32 / v_pk_add_f32 issue at the cost of their scalar forms (measured, tools/ubench_valu.hip), so a
// lane that works on TWO j-slots at once halves the issue cost of every plain multiply/add (FMAs and transcendentals
// cost the same either way).  8 steps; at step s lane c meets slots (c-2s) [component .x] and (c-2s-1) [component .y];
// each component's j-force accumulator follows its slot with a two-lane DPP rotation per step.
typedef float v2f __attribute__((ext_vector_type(2)));
// a * b.yy in one v_pk_mul_f32 that reads the high half of b for both results (op_sel).  Written as a * b.yy the multiply is selected with
// the broadcast operand's LOW half (op_sel_hi) wherever b is the second half of a 128-bit LDS read, behind a v_mov_b32 that copies the odd
// register into the even one: six copies per four pair steps of tileStepsPacked.  Same operation, same rounding.
// a * k.xx + k.yy with both constants in ONE scalar register pair.  A packed instruction takes a single scalar operand, so of two constants
// held apart one is copied into a vector pair in every trip (v_mov_b64); the same pair named twice is one operand.  One fused multiply-add,
// as the compiler contracts a * kx + ky.
__device__ __forceinline__ v2f pkFmaK(v2f a, v2f k) { v2f r; asm("v_pk_fma_f32 %0, %1, %2, %2 op_sel:[0,0,1] op_sel_hi:[1,0,1]" : "=v"(r) : "v"(a), "s"(k)); return r; }
__device__ __forceinline__ v2f pkMulHi(v2f a, v2f b) { v2f r; asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,1]" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ inline float rowRor8(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xF, 0xF, true)); }

// ---- the tile kernel ----------------------------------------------------------------------------
// Work item = (i-block, run of <= 8 tiles).  Lane layout: 4 DPP rows of 16 lanes; row r works on the 16x16 sub-tile
// (i-half r&1, j-half r>>1).  At step s lane c of a row meets j-slot (c-s)&15 of its j-half; the j-force accumulator
// travels WITH the j-slot by a one-lane DPP row rotation per step (v_add_f32_dpp: one VALU op per component, no LDS),
// so after 16 steps lane c holds the force on j-slot c.  j-atom data is read from LDS (staged once per tile, each
// 16-atom half stored twice so the rotated index c+16-s needs no wrap).
// (FORCES == false: the energy-only list bodies of include_forces == 0 steps -- slice energies alone, no force update)
template <typename Real, bool ENERGY, bool FORCES = true> __device__ __forceinline__ void exceptionsBody(const PairListParams<Real>& p, const int blk);
template <typename Real, bool ENERGY, bool FORCES = true> __device__ __forceinline__ void exclusionAtomsBody(const PairListParams<Real>& p, const int blk);
// (as in k_directPacked: the first nListBlocks work-groups of the launch run the O(N) pair lists -- exclusion corrections, then 1-4
// exceptions -- so that their latency-bound work overlaps the tile work instead of trailing it as a 65 us launch of its own on c5)
template <typename Real, int MC, bool WRAP, bool ENERGY, bool POLYALL>
__global__ __launch_bounds__(256, (sizeof(Real) == 8 ? SNB_DIRECT_F64_WAVES : 4)) void k_direct(const DirectParams<Real> p, const PairListParams<Real> q, const int nExclBlocks, const int nListBlocks) {
    // (a CU-limited launch takes its list blocks LAST: its tile work-groups must be the first thing the dispatcher places on the idle CUs)
    const int listBlock = p.listsLast ? (int)blockIdx.x - ((int)gridDim.x - nListBlocks) : (int)blockIdx.x;
    if (listBlock >= 0 && listBlock < nListBlocks) {      // (energy steps: the list bodies reduce their slice energies in 2 S doubles of dynamic LDS)
        if (listBlock < nExclBlocks) { PairListParams<Real> qe = q; qe.n = q.nExclAtoms; exclusionAtomsBody<Real, ENERGY>(qe, listBlock); }
        else exceptionsBody<Real, ENERGY>(q, listBlock - nExclBlocks);
        return;
    }
    const int tileBlock = p.listsLast ? (int)blockIdx.x : (int)blockIdx.x - nListBlocks, nTileBlocks = gridDim.x - nListBlocks;
    if (p.stepTrace && tileBlock == 0 && threadIdx.x == 0) p.stepTrace[p.traceSlot] = (long long)wall_clock64();
    double* const sliceE = SNB_SLICE_E_PARTITION(p.sliceE, p.nsub * (p.nsub + 1));
    using T4 = typename Vec<Real>::T4;
    using T2 = typename Vec<Real>::T2;
    __shared__ T4 s_pos[4][64];
    __shared__ T2 s_se[4][64];
    // (overlapped steps: CU-limited first launch and items through the device counters, as in k_directPacked)
    if (p.cuSlots != nullptr && p.cuLimit > 0 && !cuResident(p)) return;
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool dyn = p.workCounter != nullptr;
    WorkClaim<> wc{p.workCounter, p.numWork, (tileBlock * 4 + wid) & (SNB_WORK_SHARDS - 1), lane};
    int item = tileBlock * 4 + wid;
    if (dyn) item = wc.anyLeft() ? wc.resolve(wc.issue()) : p.numWork;
    for (; item < p.numWork; ) {   // no block-level barrier inside the loop
    int claimed = 0;
    if (dyn) claimed = wc.issue();
    const int4 wi = p.workItems[p.workStart + item * p.workStride];
    const int I = __builtin_amdgcn_readfirstlane(wi.x);
    const int tBegin = __builtin_amdgcn_readfirstlane(wi.y), tEnd = tBegin + __builtin_amdgcn_readfirstlane(wi.z);
    const int c = lane & 15, row = lane >> 4;
    const int il = 16 * (row & 1) + c;                   // my i-atom within the block
    const int jh = row >> 1;                             // my j-half
    const int stageJ = 16 * (lane >> 5) + c;             // j-atom this lane stages (entry `lane` of the doubled image)

    const T4 pi = p.posq[I * 32 + il];
    const T2 sei = p.sigeps[I * 32 + il];
    const Real qi = pi.w * p.k4pe;
    Real c6i = 0;
    if (MC == MC_LJPME) c6i = Real(8) * sei.x * sei.x * sei.x * sei.y;
    Real fix = 0, fiy = 0, fiz = 0;
    Real ecl = 0, elj = 0;
    int curSlice = -1;

    T4* myPos = s_pos[wid];
    T2* mySe = s_se[wid];
    const T4* rdPos = myPos + 32 * jh + c + 16;          // entry for step s is rdPos[-s]
    const T2* rdSe = mySe + 32 * jh + c + 16;

    // software pipeline, two tiles deep: while tile t is computed the j-atoms, mask word and lambdas of tile t+1 are in flight
    // (their addresses come from tileJ/tileInfo words loaded one tile earlier) and the tileJ/tileInfo words of tile t+2 are
    // requested, so no load at the head of a tile waits on another load
    T4 pj; T2 sej;
    auto fetch = [&](int code, T4& x, T2& se) {
        if (code != -1) {   // -1 = padding slot (image codes use bits 27..31, so the sign bit is NOT a validity flag)
            const int idx = code & SNB_JIDX_MASK;
            x = p.posq[idx]; se = p.sigeps[idx];
            if (!WRAP) {
                const int sc = (code >> SNB_JSHIFT_BITS) & 127;
                const int kx = sc / 25, ky = (sc - 25 * kx) / 5, kz = sc - 25 * kx - 5 * ky;
                const Real ka = Real(kx - 2), kb = Real(ky - 2), kc = Real(kz - 2);      // lattice image: + ka a + kb b + kc c (rows of p.box)
                x.x += ka * p.box[0] + kb * p.box[3] + kc * p.box[6]; x.y += kb * p.box[4] + kc * p.box[7]; x.z += kc * p.box[8];
            }
        } else { x.x = Real(3e9) + Real(1e6) * c; x.y = Real(-5e9); x.z = Real(7e9); x.w = 0; se.x = 0; se.y = 0; }
    };
    struct TileHead { int slice, maskIdx; };
    // energy steps: a tile whose slice is not wanted (p.sliceNeed) runs the forces-only arithmetic
    auto loadHead = [&](int t) { const int4 v = p.tileInfo[t]; return TileHead{v.x & 0xFFFF, v.y}; };      // (slice of the tile, mask index)
    auto loadMask = [&](const TileHead& h) { return (h.maskIdx >= 0) ? p.masks[h.maskIdx * 32 + il] : 0u; };
    int jcode = p.tileJ[tBegin * 32 + stageJ];
    TileHead head = loadHead(tBegin);
    int jcodeNext = -1; TileHead headNext = head;
    if (tBegin + 1 < tEnd) { jcodeNext = p.tileJ[(tBegin + 1) * 32 + stageJ]; headNext = loadHead(tBegin + 1); }
    fetch(jcode, pj, sej);
    unsigned maskPre = loadMask(head);
    int slicePre = head.slice;
    Real lamCPre = p.lambdas[2 * slicePre], lamLPre = p.lambdas[2 * slicePre + 1];

    for (int t = tBegin; t < tEnd; t++) {
        __builtin_amdgcn_wave_barrier();
        myPos[lane] = pj; mySe[lane] = sej;
        const int curCode = jcode;
        const bool hasMask = head.maskIdx >= 0;
        unsigned maskWord = maskPre;
        const int slice = slicePre;
        const Real lamC = lamCPre, lamL = lamLPre;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        jcode = jcodeNext; head = headNext;
        if (t + 1 < tEnd) {
            fetch(jcode, pj, sej);
            maskPre = loadMask(head);
            slicePre = head.slice;
            lamCPre = p.lambdas[2 * slicePre]; lamLPre = p.lambdas[2 * slicePre + 1];
        }
        if (t + 2 < tEnd) { jcodeNext = p.tileJ[(t + 2) * 32 + stageJ]; headNext = loadHead(t + 2); }

        if (ENERGY && slice != curSlice) {
            if (curSlice >= 0) {
                double a = waveSum((double)ecl), b = waveSum((double)elj);
                if (lane == 0) { atomicAdd(&sliceE[2 * curSlice], a); atomicAdd(&sliceE[2 * curSlice + 1], b); }
            }
            ecl = 0; elj = 0; curSlice = slice;
        }
        maskWord >>= 16 * jh;                            // my j-half's 16 bits
        // lambda folded into the i-side parameters once per tile (forces only need the scaled values)
        const Real qiS = qi * lamC;
        const Real epsiS = sei.y * lamL;
        Real fjx = 0, fjy = 0, fjz = 0;

        const bool tileE = ENERGY && p.sliceNeed[slice] != 0;      // (uniform)
#define SNB_TILE_STEPS(E, M, SW) tileSteps<Real, MC, WRAP, E, M, SW, true, POLYALL>(p, rdPos, rdSe, pi, sei, qi, qiS, epsiS, c6i, lamC, lamL, maskWord, c, fix, fiy, fiz, fjx, fjy, fjz, ecl, elj)
        if (p.useSwitch && MC != MC_LJPME && MC != MC_NOCUTOFF) {
            if (tileE) { if (hasMask) SNB_TILE_STEPS(ENERGY, true, true); else SNB_TILE_STEPS(ENERGY, false, true); }
            else { if (hasMask) SNB_TILE_STEPS(false, true, true); else SNB_TILE_STEPS(false, false, true); }
        } else {
            if (tileE) { if (hasMask) SNB_TILE_STEPS(ENERGY, true, false); else SNB_TILE_STEPS(ENERGY, false, false); }
            else { if (hasMask) SNB_TILE_STEPS(false, true, false); else SNB_TILE_STEPS(false, false, false); }
        }
#undef SNB_TILE_STEPS
            // rotate-then-add leaves lane c holding slot c+1: one more rotation brings every slot home
        fjx = rowRor1(fjx); fjy = rowRor1(fjy); fjz = rowRor1(fjz);
        // add the two i-halves (rows r and r^1) and flush
        fjx += __shfl_xor(fjx, 16, 64); fjy += __shfl_xor(fjy, 16, 64); fjz += __shfl_xor(fjz, 16, 64);
        if ((row & 1) == 0 && curCode != -1) {            // lanes 0-15 (j-half 0) and 32-47 (j-half 1): entry `lane` == j-slot
            const int jidx = curCode & SNB_JIDX_MASK;
            fAdd(p, p.fx, jidx, fjx); fAdd(p, p.fy, jidx, fjy); fAdd(p, p.fz, jidx, fjz);
        }
    }
    // rows r and r^2 hold the same i-atoms (different j-halves)
    fix += __shfl_xor(fix, 32, 64); fiy += __shfl_xor(fiy, 32, 64); fiz += __shfl_xor(fiz, 32, 64);
    if (row < 2) { fAdd(p, p.fx, (I * 32 + il), fix); fAdd(p, p.fy, (I * 32 + il), fiy); fAdd(p, p.fz, (I * 32 + il), fiz); }
    if (ENERGY && curSlice >= 0) {
        double a = waveSum((double)ecl), b = waveSum((double)elj);
        if (lane == 0) { atomicAdd(&sliceE[2 * curSlice], a); atomicAdd(&sliceE[2 * curSlice + 1], b); }
    }
    __builtin_amdgcn_wave_barrier();
    item = dyn ? wc.resolve(claimed) : item + nTileBlocks * 4;
    }   // work-item loop
    if (p.stepTrace && threadIdx.x == 0) p.stepTrace[p.traceSlot + 1] = (long long)wall_clock64();
}

// ---- single-precision forces-only tile kernel with packed math ---------------------------------------
// Same work items, tiles and masks as k_direct, different lane layout: lane (row r, column c) holds TWO i-atoms (c and c+16)
// as the halves of float2 registers and meets ONE j-slot per step, slot 8r + ((c - s) & 7) of j-quarter r, for 8 steps.
// All pair arithmetic issues as v_pk_*_f32 on (i_c, j) and (i_c+16, j): the j-side operands are broadcast by op_sel (no register
// shuffling), the i-side operands are packed once per work item, and one LDS read (b128 + b64) feeds two pair slots.  The
// j-force accumulator travels with its slot by a one-lane row rotation fused into the subtract (v_sub_f32_dpp); lanes c and
// c+8 carry two partial sums of the same slot and are merged by an 8-lane rotation at the end of the tile.
// Staging: entry e (0..15) of quarter r holds atom 8r + (e & 7), so the rotated read index (c & 7) + 8 - s needs no wrap.
// ENERGY: the raw (unscaled) pair energies of the tile's slice are accumulated as well -- eLJ = eps_ij s6 (s6 - 1) and the Coulomb
// energy of the method (Ewald: qq erfc(ar)/r with the A&S erfc) -- from the
// RAW i-parameters qiRaw / epsiRaw, while the forces keep using the lambda-scaled ones.  A force that asks for energy-parameter
// derivatives needs them on every step (the reference accumulates them whether or not the energy is requested, Q4): those steps run
// the energy body on the tiles of the wanted slices alone (directPackedBody, E_TILES).
// EPOLY: p.ewPolyE, or the same coefficients through kernargField (below) where only a few tiles of a launch want energies.
template <int MC, bool MASKED, bool POLY, bool ENERGY, bool SWITCH, bool FORCES = true, typename EPOLY = const float*, int UNROLL = 4>      // FORCES == false: energies alone, as tileSteps
__device__ __forceinline__ void tileStepsPacked(const DirectParams<float>& p, const EPOLY ewPolyE, const float4* rdPos, const float2* rdSe, const v2f pix, const v2f piy, const v2f piz,
                                                const v2f sigi, const v2f qiS, const v2f epsiS, const v2f qiRaw, const v2f epsiRaw, const v2f c6iRaw, const float lamL, const unsigned maskA, const unsigned maskB, const int c,
                                                v2f& fix, v2f& fiy, v2f& fiz, float& fjx, float& fjy, float& fjz, v2f& ecl, v2f& elj) {
#pragma unroll UNROLL
    for (int s = 0; s < 8; s++) {
        // (the j-slot as two-element vectors, for pkMulHi)
        const v2f* const rp = reinterpret_cast<const v2f*>(rdPos - s);
        const v2f xy = rp[0], zw = rp[1];
        const v2f sj = *reinterpret_cast<const v2f*>(rdSe - s);
        const v2f dx = pix - xy.xx, dy = piy - xy.yy, dz = piz - zw.xx;
        const v2f r2 = dx * dx + dy * dy + dz * dz;
        const v2f invR = {__builtin_amdgcn_rsqf(r2.x), __builtin_amdgcn_rsqf(r2.y)};
        // Lennard-Jones (sigeps holds sigma/2 and 2 sqrt(eps))
        v2f s2 = (sigi + sj.xx) * invR; s2 = s2 * s2;
        const v2f s6 = s2 * s2 * s2;
        const v2f es6 = pkMulHi(epsiS, sj) * s6;
        v2f f = es6 * pkFmaK(s6, v2f{12.0f, -6.0f});
        v2f eLJ = {0.f, 0.f}, eC = {0.f, 0.f};
        if (ENERGY) eLJ = (pkMulHi(epsiRaw, sj) * s6) * (s6 - 1.0f);
        if (SWITCH) {
            // LJ switching function (ReferenceSlicedLJCoulombIxn.cpp:380-384, 428-431): branch-free, tt clamps to 0 below the switching distance
            const v2f r = r2 * invR;
            v2f tt = (r - p.switchDist) * p.invSwitchWidth;
            tt.x = tt.x > 0.0f ? tt.x : 0.0f; tt.y = tt.y > 0.0f ? tt.y : 0.0f;
            const v2f t2 = tt * tt;
            const v2f sw = (t2 * tt) * ((tt * -6.0f + 15.0f) * tt + -10.0f) + 1.0f;
            const v2f dsw = t2 * ((tt * -30.0f + 60.0f) * tt + -30.0f) * p.invSwitchWidth;
            f = f * sw - (es6 * (s6 - 1.0f)) * (dsw * r);          // the lambda-scaled pair energy drives the force term
            if (ENERGY) eLJ = eLJ * sw;
        }
        const v2f invR2 = invR * invR;
        if (MC == MC_LJPME) {
            // LJPME: the mesh carries the geometric-mean dispersion; inside the cutoff the real-space term corrects to Lorentz-Berthelot
            // (multiplicative grid term + potential shifts, ReferenceSlicedLJCoulombIxn.cpp:398-426)
            const v2f dar2 = r2 * (p.alphaD * p.alphaD), dar4 = dar2 * dar2;
            const float sj3 = sj.x * sj.x * sj.x;
            const v2f c6 = c6iRaw * (8.0f * sj3 * sj.y);
            const v2f coef = (invR2 * invR2 * invR2) * c6;
            const v2f ed = dar2 * -1.4426950408889634f;
            const v2f expd = {__builtin_amdgcn_exp2f(ed.x), __builtin_amdgcn_exp2f(ed.y)};
            const v2f epre = dar4 * 0.5f + dar2 + 1.0f;
            const v2f dpre = (dar4 * dar2) * (1.0f / 6.0f) + epre;
            const v2f fmul = (coef * 6.0f) * (1.0f - expd * dpre);
            f = f + fmul * lamL;
            if (ENERGY) {
                const v2f sg = sigi + sj.xx;
                v2f sg2 = sg * sg; const v2f sg6 = (sg2 * sg2 * sg2) * p.invCut6;
                eLJ = eLJ + coef * (1.0f - expd * epre) + pkMulHi(epsiRaw, sj) * ((1.0f - sg6) * sg6) - c6 * p.multShift6;
            }
        }
        // Coulomb
        const v2f qq = pkMulHi(qiS, zw);
        v2f qqRaw = {0.f, 0.f};
        if (ENERGY) qqRaw = pkMulHi(qiRaw, zw);
        if ((MC == MC_EWALD || MC == MC_LJPME) && POLY) {
            // [erfc(ar)/r + 2a/sqrt(pi) e^{-(ar)^2}] / r^2 = 1/r^3 - Bt(r^2), Bt a degree-11 polynomial in t = r^2 * ewScale - 1: no exp, no rcp (POLY: where the guard of ewald_fit.h keeps it)
            const v2f t = r2 * p.ewScale - 1.0f;
            v2f bt = pkFmaK(t, v2f{p.ewPoly[11], p.ewPoly[10]});
#pragma unroll
            for (int k = 9; k >= 0; k--) bt = bt * t + p.ewPoly[k];
            f = f * invR2 + qq * (invR2 * invR - bt);
            if (ENERGY) {
                // pair ENERGY: qq (1/r - Et(r^2)), Et = erf(ar)/r a degree-13 polynomial in the same t.  The A&S erfc used before is good to
                // 1.5e-7 absolute, but its error is one-signed over most of the range and qq erfc(ar)/r is summed over 6e7 pairs: +1.0 kJ/mol
                // on the water-water slice of the 96k-atom box, whose direct (6.5e6) and reciprocal (-6.5e6) parts cancel to 788 -- 1.3e-3.
                // Degree 13 leaves a tenth of that (tools/erfc_energy_check.py; degree 11 is worse than A&S, beyond 13 float coefficients limit it).
                v2f et = t * ewPolyE[13] + ewPolyE[12];
#pragma unroll
                for (int k = 11; k >= 0; k--) et = et * t + ewPolyE[k];
                eC = qqRaw * (invR - et);
            }
        } else if (MC == MC_EWALD || MC == MC_LJPME) {
            const v2f r = r2 * invR;
            const v2f ar = r * p.alpha;
            const v2f e2 = r2 * (-p.alpha2l2e);
            const v2f ex = {__builtin_amdgcn_exp2f(e2.x), __builtin_amdgcn_exp2f(e2.y)};
            const v2f den = ar * 0.3275911f + 1.0f;
            const v2f tt = {__builtin_amdgcn_rcpf(den.x), __builtin_amdgcn_rcpf(den.y)};
            v2f poly = tt * 1.061405429f + (-1.453152027f);
            poly = poly * tt + 1.421413741f;
            poly = poly * tt + (-0.284496736f);
            poly = poly * tt + 0.254829592f;
            const v2f erfcv = poly * tt * ex;
            f = (f + (qq * invR) * (erfcv + (ar * ex) * 1.1283791670955126f)) * invR2;
            if (ENERGY) eC = (qqRaw * invR) * erfcv;
        } else if (MC == MC_RF) {
            f = (f + qq * (invR - r2 * (2.0f * p.krf))) * invR2;
            if (ENERGY) eC = qqRaw * (invR + r2 * p.krf - p.crf);
        } else {
            f = (f + qq * invR) * invR2;
            if (ENERGY) eC = qqRaw * invR;
        }
        bool inA = MC == MC_NOCUTOFF ? true : (r2.x < p.cutoff2), inB = MC == MC_NOCUTOFF ? true : (r2.y < p.cutoff2);
        if (MASKED) { const int k = (c - s) & 7; inA = inA && !((maskA >> k) & 1u); inB = inB && !((maskB >> k) & 1u); }
        f.x = inA ? f.x : 0.0f; f.y = inB ? f.y : 0.0f;
        if (ENERGY) {
            eC.x = inA ? eC.x : 0.0f; eC.y = inB ? eC.y : 0.0f; eLJ.x = inA ? eLJ.x : 0.0f; eLJ.y = inB ? eLJ.y : 0.0f;
            ecl = ecl + eC; elj = elj + eLJ;
        }
        if constexpr (FORCES) {
        const v2f gx = f * dx, gy = f * dy, gz = f * dz;
        fix = fix + gx; fiy = fiy + gy; fiz = fiz + gz;
        fjx = rowRor1(fjx) - (gx.x + gx.y); fjy = rowRor1(fjy) - (gy.x + gy.y); fjz = rowRor1(fjz) - (gz.x + gz.y);
        }
    }
}

// The first nListBlocks work-groups of the launch run the O(N) pair lists (exclusion corrections, then 1-4 exceptions: latency-bound
// work that overlaps the VALU-bound tile work instead of trailing it as a launch of its own); the others loop over tile work items.
//
// Energy bookkeeping of the tile loop (EMODE):
//   E_RUNS  (include_energy == 1, every slice wanted): ecl/elj live across the tiles of a work item and are reduced when the slice changes
//           -- one wave reduction per RUN of tiles; a reduction per tile would cost these steps about 15 %.
//   E_TILES (include_energy == 2, derivative steps: the slices of snb_set_energy_slices, a few per cent of the tiles): nothing of the
//           bookkeeping is live across a tile.  A wanted tile starts its own ecl/elj at zero and reduces them at its end (the same
//           reduction: wave sum in double, lane 0, two atomics into the slice's partition); every other tile takes the forces kernel's
//           path plus the wanted-or-not decision -- one dword of p.sliceNeed requested with the tile's atoms and moved to an SGPR,
//           together with the slice, when the tile is staged.  With the run state (curSlice, curNeeded, two accumulators, the vector
//           compare of the slices) the E_RUNS form carries across the forces path, the kernel exceeds the scalar register file and
//           reloads spilled SGPRs with v_readlane on every trip: 27 of the 59 VALU instructions a pair of unwanted tiles cost it over
//           the forces kernel (docs/MEASUREMENT_LOG.md, "derivative tiles").
enum { E_NONE = 0, E_RUNS = 1, E_TILES = 2 };
template <int MC, bool POLY, int EMODE, bool SWITCH, bool FIXED, bool WIDE>      // WIDE: 64-bit indices (fAddT), else 32-bit byte offsets (fAddAt, loadAt)
__device__ __forceinline__ void directPackedBody(const DirectParams<float>& p, const PairListParams<float>& q, const int nExclBlocks, const int nListBlocks) {
    constexpr bool ENERGY = EMODE != E_NONE, RUNS = EMODE == E_RUNS, TILES = EMODE == E_TILES;
    const int listBlock = p.listsLast ? (int)blockIdx.x - ((int)gridDim.x - nListBlocks) : (int)blockIdx.x;      // (CU-limited launch: list blocks last, see k_direct)
    if (listBlock >= 0 && listBlock < nListBlocks) {      // (energy steps: the list bodies reduce their slice energies in 2 S doubles of dynamic LDS)
        if (listBlock < nExclBlocks) { PairListParams<float> qe = q; qe.n = q.nExclAtoms; exclusionAtomsBody<float, ENERGY>(qe, listBlock); }
        else exceptionsBody<float, ENERGY>(q, listBlock - nExclBlocks);
        return;
    }
    const int tileBlock = p.listsLast ? (int)blockIdx.x : (int)blockIdx.x - nListBlocks, nTileBlocks = gridDim.x - nListBlocks;
    if (p.stepTrace && tileBlock == 0 && threadIdx.x == 0) p.stepTrace[p.traceSlot] = (long long)wall_clock64();
    double* const sliceE = SNB_SLICE_E_PARTITION(p.sliceE, p.nsub * (p.nsub + 1));
    __shared__ float4 s_pos[4][64];
    __shared__ float2 s_se[4][64];
    __shared__ float4 s_shift[128];      // lattice-image shift of every 7-bit image code (125 in use): + ka a + kb b + kc c (rows of p.box)
    if (threadIdx.x < 128) {
        const int sc = threadIdx.x;
        const int kx = sc / 25, ky = (sc - 25 * kx) / 5, kz = sc - 25 * kx - 5 * ky;
        const float ka = float(kx - 2), kb = float(ky - 2), kc = float(kz - 2);
        s_shift[sc] = sc < 125 ? make_float4(ka * p.box[0] + kb * p.box[3] + kc * p.box[6], kb * p.box[4] + kc * p.box[7], kc * p.box[8], 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // CU-limited first launch of an overlapped step: work-groups beyond the limit leave at once (the items are handed out through the
    // counters, so nothing is lost) and the reciprocal pipeline's work-groups always find the registers and LDS the limit leaves free
    if (p.cuSlots != nullptr && p.cuLimit > 0) { if (!cuResident(p)) return; }
    else __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool dyn = p.workCounter != nullptr;      // (uniform) items through the device counters: every wave of either launch claims one at a time
    WorkClaim<TILES> wc{p.workCounter, p.numWork, (tileBlock * 4 + wid) & (SNB_WORK_SHARDS - 1), lane};
    int item = tileBlock * 4 + wid;
    if (dyn) item = wc.anyLeft() ? wc.resolve(wc.issue()) : p.numWork;
    for (; item < p.numWork; ) {   // no block-level barrier inside the loop
    int claimed = 0;
    if (dyn) claimed = wc.issue();      // the next item, requested a whole item ahead (claims past the end are harmless)
    const int4 wi = p.workItems[p.workStart + item * p.workStride];
    const int I = __builtin_amdgcn_readfirstlane(wi.x);
    const int tBegin = __builtin_amdgcn_readfirstlane(wi.y), tEnd = tBegin + __builtin_amdgcn_readfirstlane(wi.z);
    const int c = lane & 15, row = lane >> 4;
    const int stageJ = 8 * row + (c & 7);                // j-atom this lane stages (entry c of quarter `row`)

    const float4 pa = p.posq[I * 32 + c], pb = p.posq[I * 32 + 16 + c];
    const float2 sa = p.sigeps[I * 32 + c], sb = p.sigeps[I * 32 + 16 + c];
    const v2f pix = {pa.x, pb.x}, piy = {pa.y, pb.y}, piz = {pa.z, pb.z};
    const v2f qi = {pa.w * p.k4pe, pb.w * p.k4pe}, sigi = {sa.x, sb.x}, epsi = {sa.y, sb.y};
    v2f fix = {0.f, 0.f}, fiy = {0.f, 0.f}, fiz = {0.f, 0.f};
    const v2f c6i = {8.0f * sa.x * sa.x * sa.x * sa.y, 8.0f * sb.x * sb.x * sb.x * sb.y};      // LJPME: c6 of the two i-atoms
    v2f ecl = {0.f, 0.f}, elj = {0.f, 0.f};
    int curSlice = -1; bool curNeeded = false;
    auto flushEnergy = [&]() {   // raw energies of the slice just finished: wave sum in double, one atomic per term
        if (curSlice >= 0) {
            const double a = waveSum((double)ecl.x + (double)ecl.y), b = waveSum((double)elj.x + (double)elj.y);
            if (lane == 0) { atomicAdd(&sliceE[2 * curSlice], a); atomicAdd(&sliceE[2 * curSlice + 1], b); }
        }
        ecl = {0.f, 0.f}; elj = {0.f, 0.f};
    };
    auto flushTile = [&](int slice, v2f e, v2f l) {   // E_TILES: the raw energies of one wanted tile, reduced as flushEnergy does
        const double a = waveSum((double)e.x + (double)e.y), b = waveSum((double)l.x + (double)l.y);
        const int ns = *kernargField<int>(offsetof(DirectParams<float>, nsub));
        double* const part = SNB_SLICE_E_PARTITION(*kernargField<double*>(offsetof(DirectParams<float>, sliceE)), ns * (ns + 1));
        if (lane == 0) { atomicAdd(&part[2 * slice], a); atomicAdd(&part[2 * slice + 1], b); }
    };

    float4* myPos = s_pos[wid];
    float2* mySe = s_se[wid];
    const float4* rdPos = myPos + 16 * row + (c & 7) + 8;   // entry for step s is rdPos[-s]
    const float2* rdSe = mySe + 16 * row + (c & 7) + 8;

    // two-tile-deep software pipeline, as in k_direct
    // Software pipeline over the item's tiles with TWO register sets used alternately (the tile loop is unrolled by two).  While tile t
    // (set X) is evaluated, the atoms, masks and lambdas of tile t+1 are requested into set Y, and the list entry + header of tile t+2
    // into the jcode/head fields of X (X's own entry has been copied to `curCode` by then).  No requested register is copied, shifted
    // or converted before the trip in which it is consumed -- a copy (a loop-carried "next = loaded" move), the image shift added at
    // the load, or a uniform header moved to SGPRs behind its load each cost a full memory round trip per tile, atomics included,
    // because the wait counter is in-order.
    struct TileRegs { int jcode, slice, maskIdx; float4 pj; float2 sej; float shx, shy, shz; unsigned mA, mB; float2 lam; int need; };
    TileRegs A, B;
    int vzero; asm volatile("v_mov_b32 %0, 0" : "=v"(vzero));      // a zero the compiler cannot see through (keeps the header load in VGPRs)
    // (the j-force atomics of a tile are issued at the start of the NEXT trip: an atomic sits behind a conditional skip the wait-count
    // pass cannot count, so any wait after it degrades to "everything"; issued first, they are a whole tile old when that wait comes)
    float pendX = 0.f, pendY = 0.f, pendZ = 0.f; int pendIdx = -1;
#ifdef SNB_EXP_NO_JATOMICS      // experiment builds only (wrong forces): the kernel without its j-force scatter
    auto flushPending = [&]() { asm volatile("" :: "v"(pendX), "v"(pendY), "v"(pendZ), "v"(pendIdx)); };
#else
    // (pendIdx: the atom slot, or without WIDE its byte offset in the force arrays, formed once per tile)
    auto flushPending = [&]() {
        if (pendIdx >= 0) {
            if constexpr (WIDE) { fAddT<FIXED>(p, p.fx, pendIdx, pendX); fAddT<FIXED>(p, p.fy, pendIdx, pendY); fAddT<FIXED>(p, p.fz, pendIdx, pendZ); }
            else { fAddAt<FIXED>(p.fx, pendIdx, pendX); fAddAt<FIXED>(p.fy, pendIdx, pendY); fAddAt<FIXED>(p.fz, pendIdx, pendZ); }
        }
    };
#endif
    auto requestList = [&](TileRegs& r, int t) {                    // list entry + header of tile t
        int2 v;
        if constexpr (WIDE) { r.jcode = p.tileJ[t * 32 + stageJ]; v = *reinterpret_cast<const int2*>(&p.tileInfo[t + vzero]); }
        else { r.jcode = loadAt<int>(p.tileJ, (unsigned)t * 128u + 4u * stageJ); v = loadAt<int2>(p.tileInfo, (unsigned)t * 16u + (unsigned)vzero); }
        r.slice = v.x; r.maskIdx = v.y;
    };
    auto requestAtoms = [&](TileRegs& r) {                          // needs r.jcode / r.slice / r.maskIdx (requested a tile earlier)
        const int code = r.jcode;
        asm volatile("" :: "v"(code), "v"(r.slice), "v"(r.maskIdx));   // the wait for the list entry belongs HERE, before anything younger is issued
        flushPending();
        const int idx = code == -1 ? 0 : (code & SNB_JIDX_MASK);
        r.pj = p.posq[idx]; r.sej = p.sigeps[idx];
        const float4 sh = s_shift[(code >> SNB_JSHIFT_BITS) & 127];      // lattice image of the entry (table filled at kernel start)
        r.shx = sh.x; r.shy = sh.y; r.shz = sh.z;
        const int mi = r.maskIdx < 0 ? 0 : r.maskIdx;              // unconditional loads: a conditionally loaded register is a phi with a copy
        if constexpr (WIDE) { r.mA = p.masks[mi * 32 + c]; r.mB = p.masks[mi * 32 + 16 + c]; }
        else { const unsigned mo = 4u * (unsigned)(mi * 32 + c); r.mA = loadAt<unsigned>(p.masks, mo); r.mB = loadAt<unsigned>(p.masks, mo + 64u); }
        r.lam = *reinterpret_cast<const float2*>(&p.lambdas[2 * (r.slice & 0xFFFF)]);      // (the slice index comes with the tile header, written by the builder)
        if (ENERGY) r.need = p.sliceNeed[r.slice & 0xFFFF];      // energy steps: is this slice's energy wanted?
    };
    // what the staging of a tile leaves behind for its evaluation
    struct Staged { int code; bool hasMask; unsigned maskA, maskB; float lamC, lamL; int slice; bool needE; };
    auto stage = [&](TileRegs& R) {                                 // tile R -> LDS (the wait for its atoms sits here, in straight-line code)
        Staged st;
        __builtin_amdgcn_wave_barrier();
        st.code = R.jcode;
        if (st.code != -1) { myPos[lane] = make_float4(R.pj.x + R.shx, R.pj.y + R.shy, R.pj.z + R.shz, R.pj.w); mySe[lane] = R.sej; }
        else { myPos[lane] = make_float4(3e9f + 1e6f * c, -5e9f, 7e9f, 0.f); mySe[lane] = make_float2(0.f, 0.f); }      // padding slot: parked far away
        st.hasMask = R.maskIdx >= 0;
        st.maskA = st.hasMask ? R.mA >> (8 * row) : 0u; st.maskB = st.hasMask ? R.mB >> (8 * row) : 0u;   // my j-quarter's 8 bits
        st.lamC = R.lam.x; st.lamL = R.lam.y;
        if constexpr (TILES) st.slice = __builtin_amdgcn_readfirstlane(R.slice) & 0xFFFF;      // (scalar: only a wanted tile's reduction reads it)
        else st.slice = R.slice & 0xFFFF;
        st.needE = ENERGY && __builtin_amdgcn_readfirstlane(R.need) != 0;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        return st;
    };
    // One trip: request (unconditionally -- past the item's end the indices are clamped and the data unused, so that the number of
    // memory operations in flight is a compile-time constant and every wait can be exact), evaluate the staged tile X, scatter its
    // j-forces, then stage Y.  The wait for Y's atoms thus comes after a whole tile of arithmetic and leaves the younger requests and
    // the atomics in flight.
    auto tile = [&](TileRegs& X, TileRegs& Y, const int t, Staged& st) {
        requestAtoms(Y);      // (issues the previous tile's j-force atomics first)
        requestList(X, t + 2 < tEnd ? t + 2 : tEnd - 1);
        // (E_RUNS; the sums of a slice nobody asked for are zero: no wave reduction, no atomics)
        if (RUNS && st.slice != curSlice) { if (curNeeded) flushEnergy(); curSlice = st.slice; curNeeded = st.needE; }
        const v2f qiS = qi * st.lamC, epsiS = epsi * st.lamL;      // lambda folded into the i-side parameters once per tile
        float fjx = 0, fjy = 0, fjz = 0;
#define SNB_TILE_PACKED(M, E, EP, ECL, ELJ) tileStepsPacked<MC, M, POLY, E, SWITCH>(p, EP, rdPos, rdSe, pix, piy, piz, sigi, qiS, epsiS, qi, epsi, c6i, st.lamL, st.maskA, st.maskB, c, fix, fiy, fiz, fjx, fjy, fjz, ECL, ELJ)
        if (TILES && st.needE) {      // a wanted tile of a derivative step: its own sums, reduced here
            v2f te = {0.f, 0.f}, tl = {0.f, 0.f};
            const auto ep = kernargField<float>(offsetof(DirectParams<float>, ewPolyE));
#define SNB_TILE_WANTED(M) tileStepsPacked<MC, M, POLY, true, SWITCH, true, decltype(ep), 2>(p, ep, rdPos, rdSe, pix, piy, piz, sigi, qiS, epsiS, qi, epsi, c6i, st.lamL, st.maskA, st.maskB, c, fix, fiy, fiz, fjx, fjy, fjz, te, tl)
            if (st.hasMask) SNB_TILE_WANTED(true); else SNB_TILE_WANTED(false);      // (two steps unrolled, not four: the kernel keeps the forces kernel's register allocation)
#undef SNB_TILE_WANTED
            flushTile(st.slice, te, tl);
        }
        else if (RUNS && st.needE) { if (st.hasMask) SNB_TILE_PACKED(true, ENERGY, p.ewPolyE, ecl, elj); else SNB_TILE_PACKED(false, ENERGY, p.ewPolyE, ecl, elj); }
        else { if (st.hasMask) SNB_TILE_PACKED(true, false, p.ewPolyE, ecl, elj); else SNB_TILE_PACKED(false, false, p.ewPolyE, ecl, elj); }      // forces only (also: energy steps, slice not wanted)
#undef SNB_TILE_PACKED
        // rotate-then-subtract leaves lane c holding slot (c+1)&7, and lanes c and c+8 carry the two partial sums of a slot: these are
        // merged where they lie (the add takes the rotated operand itself, v_add_f32_dpp), then one more rotation brings every slot
        // home -- the same two terms in one add as rotating first, so the sum is the same in every bit
        fjx = fjx + rowRor8(fjx); fjy = fjy + rowRor8(fjy); fjz = fjz + rowRor8(fjz);
        pendX = rowRor1(fjx); pendY = rowRor1(fjy); pendZ = rowRor1(fjz);
        const int curCode = st.code;
        const int curJ = curCode & SNB_JIDX_MASK;
        pendIdx = (c < 8 && curCode != -1) ? (WIDE ? curJ : (int)__umul24(curJ, p.fBytes)) : -1;      // entry c < 8 of quarter `row` == j-slot 8*row + c == the atom this lane staged
        st = stage(Y);
    };
    requestList(A, tBegin);
    B = A;
    requestList(B, tBegin + 1 < tEnd ? tBegin + 1 : tBegin);
    requestAtoms(A);
    Staged st = stage(A);
    for (int t = tBegin; t < tEnd; t += 2) {
        tile(A, B, t, st);
        if (t + 1 < tEnd) tile(B, A, t + 1, st);
    }
    flushPending();
    // the four rows hold partial sums for the same i-atoms (different j-quarters)
    float ox = fix.x, oy = fiy.x, oz = fiz.x, ux = fix.y, uy = fiy.y, uz = fiz.y;
    ox += __shfl_xor(ox, 16, 64); oy += __shfl_xor(oy, 16, 64); oz += __shfl_xor(oz, 16, 64);
    ux += __shfl_xor(ux, 16, 64); uy += __shfl_xor(uy, 16, 64); uz += __shfl_xor(uz, 16, 64);
    ox += __shfl_xor(ox, 32, 64); oy += __shfl_xor(oy, 32, 64); oz += __shfl_xor(oz, 32, 64);
    ux += __shfl_xor(ux, 32, 64); uy += __shfl_xor(uy, 32, 64); uz += __shfl_xor(uz, 32, 64);
    int Iout = I;
    if constexpr (TILES) asm volatile("" : "+s"(Iout));      // (the i-atoms' 64-bit index is formed here, not held in two registers across the item's tiles)
    if constexpr (WIDE) {
    if (row == 0) { fAddT<FIXED>(p, p.fx, (Iout * 32 + c), ox); fAddT<FIXED>(p, p.fy, (Iout * 32 + c), oy); fAddT<FIXED>(p, p.fz, (Iout * 32 + c), oz); }
    if (row == 1) { fAddT<FIXED>(p, p.fx, (Iout * 32 + 16 + c), ux); fAddT<FIXED>(p, p.fy, (Iout * 32 + 16 + c), uy); fAddT<FIXED>(p, p.fz, (Iout * 32 + 16 + c), uz); }
    } else {
    const unsigned oa = __umul24(Iout * 32 + c, p.fBytes), ob = __umul24(Iout * 32 + 16 + c, p.fBytes);
    if (row == 0) { fAddAt<FIXED>(p.fx, oa, ox); fAddAt<FIXED>(p.fy, oa, oy); fAddAt<FIXED>(p.fz, oa, oz); }
    if (row == 1) { fAddAt<FIXED>(p.fx, ob, ux); fAddAt<FIXED>(p.fy, ob, uy); fAddAt<FIXED>(p.fz, ob, uz); }
    }
    if (RUNS) { if (curNeeded) flushEnergy(); curSlice = -1; curNeeded = false; }
    __builtin_amdgcn_wave_barrier();
    item = dyn ? wc.resolve(claimed) : item + nTileBlocks * 4;
    }   // work-item loop
    if (p.stepTrace && threadIdx.x == 0) p.stepTrace[p.traceSlot + 1] = (long long)wall_clock64();      // (plain store: the last work-group to leave writes last)
}
template <int MC, bool POLY, bool ENERGY, bool SWITCH, bool FIXED>
__global__ __launch_bounds__(256, 4) void k_directPacked(const DirectParams<float> p, const PairListParams<float> q, const int nExclBlocks, const int nListBlocks) {
    directPackedBody<MC, POLY, ENERGY ? E_RUNS : E_NONE, SWITCH, FIXED, false>(p, q, nExclBlocks, nListBlocks);
}
// derivative steps (include_energy == 2): the same launch with the per-tile bookkeeping (no switching function: directKernel)
template <int MC, bool POLY, bool FIXED>
__global__ __launch_bounds__(256, 4) void k_directPackedSelected(const DirectParams<float> p, const PairListParams<float> q, const int nExclBlocks, const int nListBlocks) {
    directPackedBody<MC, POLY, E_TILES, false, FIXED, false>(p, q, nExclBlocks, nListBlocks);
}
// The same two kernels with 64-bit indices, for launches with a force or list array of 2^31 bytes or more (p.wideOffsets, set where the
// engine fills DirectParams)
namespace wide {
template <int MC, bool POLY, bool ENERGY, bool SWITCH, bool FIXED>
__global__ __launch_bounds__(256, 4) void k_directPacked(const DirectParams<float> p, const PairListParams<float> q, const int nExclBlocks, const int nListBlocks) {
    directPackedBody<MC, POLY, ENERGY ? E_RUNS : E_NONE, SWITCH, FIXED, true>(p, q, nExclBlocks, nListBlocks);
}
template <int MC, bool POLY, bool FIXED>
__global__ __launch_bounds__(256, 4) void k_directPackedSelected(const DirectParams<float> p, const PairListParams<float> q, const int nExclBlocks, const int nListBlocks) {
    directPackedBody<MC, POLY, E_TILES, false, FIXED, true>(p, q, nExclBlocks, nListBlocks);
}
}  // namespace wide

// ---- energy-only tile kernels (steps with include_forces == 0) ------------------------------------
// The raw slice energies of the same work items and tiles, from the same lane layout and the same per-lane accumulation order as the
// energy instantiations of k_direct / k_directPacked (so the sums agree with those of an energy step to rounding), with no force arithmetic,
// no force accumulators and no force stores.  A tile whose slice is not wanted (p.sliceNeed; include_energy == 2) is skipped whole --
// the decision is uniform per tile, so the wave never loads its atoms.  The first nListBlocks work-groups run the energy-only pair lists.
// No software pipeline: these steps are few (reporters, barostat trials, re-analysis), the forces-step kernels stay as they are.
template <typename Real, int MC, bool WRAP>
__global__ __launch_bounds__(256, (sizeof(Real) == 8 ? SNB_DIRECT_F64_WAVES : 4)) void k_directEnergy(const DirectParams<Real> p, const PairListParams<Real> q, const int nExclBlocks, const int nListBlocks) {
    if ((int)blockIdx.x < nListBlocks) {
        if ((int)blockIdx.x < nExclBlocks) { PairListParams<Real> qe = q; qe.n = q.nExclAtoms; exclusionAtomsBody<Real, true, false>(qe, blockIdx.x); }
        else exceptionsBody<Real, true, false>(q, blockIdx.x - nExclBlocks);
        return;
    }
    const int tileBlock = (int)blockIdx.x - nListBlocks, nTileBlocks = gridDim.x - nListBlocks;
    double* const sliceE = SNB_SLICE_E_PARTITION(p.sliceE, p.nsub * (p.nsub + 1));
    using T4 = typename Vec<Real>::T4;
    using T2 = typename Vec<Real>::T2;
    __shared__ T4 s_pos[4][64];
    __shared__ T2 s_se[4][64];
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 15, row = lane >> 4;
    const int il = 16 * (row & 1) + c, jh = row >> 1, stageJ = 16 * (lane >> 5) + c;      // (lane layout of k_direct)
    T4* myPos = s_pos[wid];
    T2* mySe = s_se[wid];
    const T4* rdPos = myPos + 32 * jh + c + 16;
    const T2* rdSe = mySe + 32 * jh + c + 16;
    for (int item = tileBlock * 4 + wid; item < p.numWork; item += nTileBlocks * 4) {
        const int4 wi = p.workItems[p.workStart + item * p.workStride];
        const int I = __builtin_amdgcn_readfirstlane(wi.x);
        const int tBegin = __builtin_amdgcn_readfirstlane(wi.y), tEnd = tBegin + __builtin_amdgcn_readfirstlane(wi.z);
        const T4 pi = p.posq[I * 32 + il];
        const T2 sei = p.sigeps[I * 32 + il];
        const Real qi = pi.w * p.k4pe;
        Real c6i = 0;
        if (MC == MC_LJPME) c6i = Real(8) * sei.x * sei.x * sei.x * sei.y;
        Real ecl = 0, elj = 0;
        int curSlice = -1;
        for (int t = tBegin; t < tEnd; t++) {
            const int4 head = p.tileInfo[t];
            const int slice = __builtin_amdgcn_readfirstlane(head.x & 0xFFFF), maskIdx = __builtin_amdgcn_readfirstlane(head.y);
            if (slice != curSlice) {
                if (curSlice >= 0) {
                    const double a = waveSum((double)ecl), b = waveSum((double)elj);
                    if (lane == 0) { atomicAdd(&sliceE[2 * curSlice], a); atomicAdd(&sliceE[2 * curSlice + 1], b); }
                }
                ecl = 0; elj = 0; curSlice = slice;
            }
            if (__builtin_amdgcn_readfirstlane(p.sliceNeed[slice]) == 0) continue;      // (uniform) slice not wanted: the whole tile is skipped
            const int code = p.tileJ[t * 32 + stageJ];
            T4 pj; T2 sej;
            if (code != -1) {
                const int idx = code & SNB_JIDX_MASK;
                pj = p.posq[idx]; sej = p.sigeps[idx];
                if (!WRAP) {
                    const int sc = (code >> SNB_JSHIFT_BITS) & 127;
                    const int kx = sc / 25, ky = (sc - 25 * kx) / 5, kz = sc - 25 * kx - 5 * ky;
                    const Real ka = Real(kx - 2), kb = Real(ky - 2), kc = Real(kz - 2);
                    pj.x += ka * p.box[0] + kb * p.box[3] + kc * p.box[6]; pj.y += kb * p.box[4] + kc * p.box[7]; pj.z += kc * p.box[8];
                }
            } else { pj.x = Real(3e9) + Real(1e6) * c; pj.y = Real(-5e9); pj.z = Real(7e9); pj.w = 0; sej.x = 0; sej.y = 0; }
            const unsigned maskWord = (maskIdx >= 0 ? p.masks[maskIdx * 32 + il] : 0u) >> (16 * jh);
            const Real lamC = p.lambdas[2 * slice], lamL = p.lambdas[2 * slice + 1];
            __builtin_amdgcn_wave_barrier();
            myPos[lane] = pj; mySe[lane] = sej;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            Real fix = 0, fiy = 0, fiz = 0, fjx = 0, fjy = 0, fjz = 0;      // (not touched: FORCES == false)
#define SNB_TILE_E(M, SW) tileSteps<Real, MC, WRAP, true, M, SW, false>(p, rdPos, rdSe, pi, sei, qi, qi, sei.y, c6i, lamC, lamL, maskWord, c, fix, fiy, fiz, fjx, fjy, fjz, ecl, elj)
            if (p.useSwitch && MC != MC_LJPME && MC != MC_NOCUTOFF) { if (maskIdx >= 0) SNB_TILE_E(true, true); else SNB_TILE_E(false, true); }
            else { if (maskIdx >= 0) SNB_TILE_E(true, false); else SNB_TILE_E(false, false); }
#undef SNB_TILE_E
            __builtin_amdgcn_wave_barrier();
        }
        if (curSlice >= 0) {
            const double a = waveSum((double)ecl), b = waveSum((double)elj);
            if (lane == 0) { atomicAdd(&sliceE[2 * curSlice], a); atomicAdd(&sliceE[2 * curSlice + 1], b); }
        }
    }
}

// Packed single-precision form (the energy instantiation of k_directPacked without its forces): lane (row r, column c) holds i-atoms c and
// c+16 and meets one j-slot of j-quarter r per step, 8 steps per tile, tileStepsPacked with FORCES == false.
template <int MC, bool POLY, bool SWITCH>
__global__ __launch_bounds__(256, 4) void k_directPackedEnergy(const DirectParams<float> p, const PairListParams<float> q, const int nExclBlocks, const int nListBlocks) {
    if ((int)blockIdx.x < nListBlocks) {
        if ((int)blockIdx.x < nExclBlocks) { PairListParams<float> qe = q; qe.n = q.nExclAtoms; exclusionAtomsBody<float, true, false>(qe, blockIdx.x); }
        else exceptionsBody<float, true, false>(q, blockIdx.x - nExclBlocks);
        return;
    }
    const int tileBlock = (int)blockIdx.x - nListBlocks, nTileBlocks = gridDim.x - nListBlocks;
    double* const sliceE = SNB_SLICE_E_PARTITION(p.sliceE, p.nsub * (p.nsub + 1));
    __shared__ float4 s_pos[4][64];
    __shared__ float2 s_se[4][64];
    __shared__ float4 s_shift[128];      // lattice-image shift of every 7-bit image code, as in k_directPacked
    if (threadIdx.x < 128) {
        const int sc = threadIdx.x;
        const int kx = sc / 25, ky = (sc - 25 * kx) / 5, kz = sc - 25 * kx - 5 * ky;
        const float ka = float(kx - 2), kb = float(ky - 2), kc = float(kz - 2);
        s_shift[sc] = sc < 125 ? make_float4(ka * p.box[0] + kb * p.box[3] + kc * p.box[6], kb * p.box[4] + kc * p.box[7], kc * p.box[8], 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 15, row = lane >> 4;
    const int stageJ = 8 * row + (c & 7);
    float4* myPos = s_pos[wid];
    float2* mySe = s_se[wid];
    const float4* rdPos = myPos + 16 * row + (c & 7) + 8;
    const float2* rdSe = mySe + 16 * row + (c & 7) + 8;
    for (int item = tileBlock * 4 + wid; item < p.numWork; item += nTileBlocks * 4) {
        const int4 wi = p.workItems[p.workStart + item * p.workStride];
        const int I = __builtin_amdgcn_readfirstlane(wi.x);
        const int tBegin = __builtin_amdgcn_readfirstlane(wi.y), tEnd = tBegin + __builtin_amdgcn_readfirstlane(wi.z);
        const float4 pa = p.posq[I * 32 + c], pb = p.posq[I * 32 + 16 + c];
        const float2 sa = p.sigeps[I * 32 + c], sb = p.sigeps[I * 32 + 16 + c];
        const v2f pix = {pa.x, pb.x}, piy = {pa.y, pb.y}, piz = {pa.z, pb.z};
        const v2f qi = {pa.w * p.k4pe, pb.w * p.k4pe}, sigi = {sa.x, sb.x}, epsi = {sa.y, sb.y};
        const v2f c6i = {8.0f * sa.x * sa.x * sa.x * sa.y, 8.0f * sb.x * sb.x * sb.x * sb.y};
        v2f ecl = {0.f, 0.f}, elj = {0.f, 0.f};
        int curSlice = -1; bool curNeeded = false;
        auto flushEnergy = [&]() {      // (as k_directPacked's: wave sum in double, one atomic per term)
            if (curSlice >= 0) {
                const double a = waveSum((double)ecl.x + (double)ecl.y), b = waveSum((double)elj.x + (double)elj.y);
                if (lane == 0) { atomicAdd(&sliceE[2 * curSlice], a); atomicAdd(&sliceE[2 * curSlice + 1], b); }
            }
            ecl = {0.f, 0.f}; elj = {0.f, 0.f};
        };
        for (int t = tBegin; t < tEnd; t++) {
            const int2 head = *reinterpret_cast<const int2*>(&p.tileInfo[t]);
            const int slice = __builtin_amdgcn_readfirstlane(head.x & 0xFFFF), maskIdx = __builtin_amdgcn_readfirstlane(head.y);
            const bool need = __builtin_amdgcn_readfirstlane(p.sliceNeed[slice]) != 0;
            if (slice != curSlice) { if (curNeeded) flushEnergy(); curSlice = slice; curNeeded = need; }
            if (!need) continue;      // (uniform) slice not wanted: the whole tile is skipped
            const int code = p.tileJ[t * 32 + stageJ];
            float4 pj = make_float4(3e9f + 1e6f * c, -5e9f, 7e9f, 0.f);      // padding slot: parked far away
            float2 sej = make_float2(0.f, 0.f);
            if (code != -1) {
                const int idx = code & SNB_JIDX_MASK;
                const float4 x = p.posq[idx];
                const float4 sh = s_shift[(code >> SNB_JSHIFT_BITS) & 127];
                pj = make_float4(x.x + sh.x, x.y + sh.y, x.z + sh.z, x.w); sej = p.sigeps[idx];
            }
            unsigned maskA = 0u, maskB = 0u;
            if (maskIdx >= 0) { maskA = p.masks[maskIdx * 32 + c] >> (8 * row); maskB = p.masks[maskIdx * 32 + 16 + c] >> (8 * row); }
            const float lamL = p.lambdas[2 * slice + 1];
            __builtin_amdgcn_wave_barrier();
            myPos[lane] = pj; mySe[lane] = sej;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            v2f fix = {0.f, 0.f}, fiy = {0.f, 0.f}, fiz = {0.f, 0.f};      // (not touched: FORCES == false)
            float fjx = 0.f, fjy = 0.f, fjz = 0.f;
            if (maskIdx >= 0) tileStepsPacked<MC, true, POLY, true, SWITCH, false>(p, p.ewPolyE, rdPos, rdSe, pix, piy, piz, sigi, qi, epsi, qi, epsi, c6i, lamL, maskA, maskB, c, fix, fiy, fiz, fjx, fjy, fjz, ecl, elj);
            else tileStepsPacked<MC, false, POLY, true, SWITCH, false>(p, p.ewPolyE, rdPos, rdSe, pix, piy, piz, sigi, qi, epsi, qi, epsi, c6i, lamL, maskA, maskB, c, fix, fiy, fiz, fjx, fjy, fjz, ecl, elj);
            __builtin_amdgcn_wave_barrier();
        }
        if (curNeeded) flushEnergy();
    }
}


// evStart/evStop (both or neither): hipExtLaunchKernelGGL stamps them with the kernel's own begin and end -- the duration rocprofv3 reports,
// without the marker-packet overhead of hipEventRecord pairs around the launch.  *timed tells the caller whether a kernel took them.
#define SNB_LAUNCH_LDS(KERNEL, GRID, LDS, ...) do { if (evStart) { hipExtLaunchKernelGGL(KERNEL, GRID, block, LDS, s, evStart, evStop, 0, __VA_ARGS__); *timed = true; } \
                                                 else hipLaunchKernelGGL(KERNEL, GRID, block, LDS, s, __VA_ARGS__); } while (0)
template <typename Real> using TileKernel = void (*)(DirectParams<Real>, PairListParams<Real>, int, int);
// The tile kernel of a forces step.  *packed: the single-precision packed kernel, which carries the pair lists whatever SNB_NO_FUSED_LISTS says.
template <typename Real, int MC> static TileKernel<Real> directKernel(const DirectParams<Real>& p, bool wrap, int energyMode, bool* packed) {
    const bool energy = energyMode != E_NONE;      // (E_TILES: the packed kernel alone has the per-tile form; the scalar kernel keeps its runs)
    *packed = false;
    if constexpr (std::is_same<Real, float>::value) {
        if (!wrap && !(energy && switches().scalarEnergyKernel) && !(p.useSwitch && MC == MC_NOCUTOFF)) {
            *packed = true;
            // (one template switch for both polynomials: an energy step keeps them only where both passed the guard, engine.hip buildEwaldPoly)
            const int polyNeed = energy ? (SNB_POLY_FORCE | SNB_POLY_ENERGY) : SNB_POLY_FORCE;
            const bool poly = (MC == MC_EWALD || MC == MC_LJPME) && (p.ewUsePoly & polyNeed) == polyNeed;
#define SNB_PACKED(P, E, S) do { if (p.wideOffsets) return p.fixed ? wide::k_directPacked<MC, P, E, S, true> : wide::k_directPacked<MC, P, E, S, false>; \
                                 return p.fixed ? k_directPacked<MC, P, E, S, true> : k_directPacked<MC, P, E, S, false>; } while (0)
            // derivative steps: the per-tile form where it is free of scratch -- not with the switching function and not under LJPME, whose energy
            // bodies spill in either form (tests/test_host_cpu.py keeps the list of kernels that may); those keep the run-based kernel
#define SNB_SELECTED(P) do { if (p.wideOffsets) return p.fixed ? wide::k_directPackedSelected<MC, P, true> : wide::k_directPackedSelected<MC, P, false>; \
                             return p.fixed ? k_directPackedSelected<MC, P, true> : k_directPackedSelected<MC, P, false>; } while (0)
            if constexpr (MC != MC_LJPME) {
                if (energyMode == E_TILES && !p.useSwitch) {
                    if constexpr (MC == MC_NOCUTOFF) SNB_SELECTED(false);
                    else { if (poly) SNB_SELECTED(true); else SNB_SELECTED(false); }
                }
            }
#undef SNB_SELECTED
            if constexpr (MC == MC_NOCUTOFF) { if (energy) SNB_PACKED(false, true, false); else SNB_PACKED(false, false, false); }
            else if (p.useSwitch && MC != MC_LJPME) {      // (no switching function under LJPME, Q2)
                if (energy) { if (poly) SNB_PACKED(true, true, true); else SNB_PACKED(false, true, true); }
                else { if (poly) SNB_PACKED(true, false, true); else SNB_PACKED(false, false, true); }
            } else {
                if (energy) { if (poly) SNB_PACKED(true, true, false); else SNB_PACKED(false, true, false); }
                else { if (poly) SNB_PACKED(true, false, false); else SNB_PACKED(false, false, false); }
            }
#undef SNB_PACKED
        }
    }
    // the scalar tile kernel: double precision, per-pair wrapping, the switches above
    // double precision with every polynomial of the method in use (the benchmark point): the instantiation without tests in the loop
    if constexpr (std::is_same<Real, double>::value && (MC == MC_EWALD || MC == MC_LJPME)) {
        const int all = SNB_POLY_FORCE | (MC == MC_LJPME ? SNB_POLY_DISPERSION : 0);
        if ((p.ewUsePoly & all) == all) {
            if (wrap) return energy ? k_direct<Real, MC, true, true, true> : k_direct<Real, MC, true, false, true>;
            return energy ? k_direct<Real, MC, false, true, true> : k_direct<Real, MC, false, false, true>;
        }
    }
    if (wrap) return energy ? k_direct<Real, MC, true, true, false> : k_direct<Real, MC, true, false, false>;
    return energy ? k_direct<Real, MC, false, true, false> : k_direct<Real, MC, false, false, false>;
}
template <typename Real, int MC> static bool launchDirectMC(const DirectParams<Real>& p, bool wrap, int energy, const PairListParams<Real>* lists, hipStream_t s, hipEvent_t evStart, hipEvent_t evStop, bool* timed) {
    const int myItems = p.numWork;
    if (myItems <= 0) return false;
    int nwg = (myItems + 3) / 4;
    { const int cap = switches().directWgs; if (cap > 0 && nwg > cap) nwg = cap; }
    if (p.workCounter && p.gridCap > 0) nwg = p.cuLimit > 0 ? p.gridCap : std::min(nwg, p.gridCap);      // overlapped step: resident waves claim their items
    bool packed;
    const TileKernel<Real> kernel = directKernel<Real, MC>(p, wrap, energy, &packed);
    PairListParams<Real> q;
    std::memset(&q, 0, sizeof(q));
    int nExclBlocks = 0, nListBlocks = 0;
    const bool fuseLists = lists != nullptr && (packed || !switches().noFusedLists);
    if (fuseLists) { q = *lists; nExclBlocks = (q.nExclAtoms + 255) / 256; nListBlocks = nExclBlocks + (q.n + 255) / 256; }
    const size_t listLds = (fuseLists && energy != E_NONE) ? sizeof(double) * 2 * q.nSlices : 0;      // the energy list bodies reduce per slice in LDS
    const dim3 gridAll(nwg + nListBlocks), block(256);
    SNB_LAUNCH_LDS(kernel, gridAll, listLds, p, q, nExclBlocks, nListBlocks);
    return fuseLists;
}
// register allocation, in the hardware's units of 8 VGPRs (accumulation registers included), of the tile kernel launchDirect runs for
// these arguments (of p: useSwitch, ewUsePoly, fixed; energy: 0 / 1 / 2 as include_energy); 16 when the runtime cannot tell
template <typename Real> int directVgprUnits(const DirectParams<Real>& p, int mc, bool wrap, int energy) {
    bool packed;
    TileKernel<Real> kernel;
    switch (mc) {
        case MC_NOCUTOFF: kernel = directKernel<Real, MC_NOCUTOFF>(p, wrap, energy, &packed); break;
        case MC_RF: kernel = directKernel<Real, MC_RF>(p, wrap, energy, &packed); break;
        case MC_EWALD: kernel = directKernel<Real, MC_EWALD>(p, wrap, energy, &packed); break;
        default: kernel = directKernel<Real, MC_LJPME>(p, wrap, energy, &packed); break;
    }
    hipFuncAttributes attr;
    return (hipFuncGetAttributes(&attr, (const void*)kernel) == hipSuccess && attr.numRegs > 0) ? (attr.numRegs + 7) / 8 : 16;
}
template int directVgprUnits<float>(const DirectParams<float>&, int, bool, int);
template int directVgprUnits<double>(const DirectParams<double>&, int, bool, int);

// Returns true when the launch also ran the pair lists passed in `lists` (single-precision forces-only tile kernel); otherwise the
// caller launches them itself.
template <typename Real> bool launchDirect(const DirectParams<Real>& p0, int mc, bool wrap, int energy, const PairListParams<Real>* lists, hipStream_t s, hipEvent_t evStart, hipEvent_t evStop, bool* timed) {
    const DirectParams<Real>& p = p0;
    switch (mc) {
        case MC_NOCUTOFF: return launchDirectMC<Real, MC_NOCUTOFF>(p, wrap, energy, lists, s, evStart, evStop, timed);
        case MC_RF: return launchDirectMC<Real, MC_RF>(p, wrap, energy, lists, s, evStart, evStop, timed);
        case MC_EWALD: return launchDirectMC<Real, MC_EWALD>(p, wrap, energy, lists, s, evStart, evStop, timed);
        default: return launchDirectMC<Real, MC_LJPME>(p, wrap, energy, lists, s, evStart, evStop, timed);
    }
}
template bool launchDirect<float>(const DirectParams<float>&, int, bool, int, const PairListParams<float>*, hipStream_t, hipEvent_t, hipEvent_t, bool*);
template bool launchDirect<double>(const DirectParams<double>&, int, bool, int, const PairListParams<double>*, hipStream_t, hipEvent_t, hipEvent_t, bool*);

// Energy-only step (include_forces == 0): k_directPackedEnergy wherever the forces step runs k_directPacked, k_directEnergy elsewhere (double
// precision, per-pair wrapping; the guard on a NoCutoff switch only mirrors launchDirectMC -- the engine never sets useSwitch for NoCutoff).
// The pair lists passed in `lists` always ride along; returns whether there were any.
template <typename Real, int MC> static bool launchDirectEnergyMC(const DirectParams<Real>& p, bool wrap, const PairListParams<Real>* lists, hipStream_t s, hipEvent_t evStart, hipEvent_t evStop, bool* timed) {
    if (p.numWork <= 0) return false;
    dim3 block(256);
    PairListParams<Real> q;
    std::memset(&q, 0, sizeof(q));
    int nExclBlocks = 0, nListBlocks = 0;
    if (lists) { q = *lists; nExclBlocks = (q.nExclAtoms + 255) / 256; nListBlocks = nExclBlocks + (q.n + 255) / 256; }
    const size_t listLds = lists ? sizeof(double) * 2 * q.nSlices : 0;
    const dim3 gridAll((p.numWork + 3) / 4 + nListBlocks);
    if constexpr (std::is_same<Real, float>::value) {
        if (!wrap && !(p.useSwitch && MC == MC_NOCUTOFF)) {
            const bool poly = (MC == MC_EWALD || MC == MC_LJPME) && (p.ewUsePoly & SNB_POLY_ENERGY);      // (no forces: the energy polynomial alone)
#define SNB_PACKED_E(P, S) SNB_LAUNCH_LDS((k_directPackedEnergy<MC, P, S>), gridAll, listLds, p, q, nExclBlocks, nListBlocks)
            if constexpr (MC == MC_NOCUTOFF) SNB_PACKED_E(false, false);
            else if (p.useSwitch && MC != MC_LJPME) { if (poly) SNB_PACKED_E(true, true); else SNB_PACKED_E(false, true); }
            else { if (poly) SNB_PACKED_E(true, false); else SNB_PACKED_E(false, false); }
#undef SNB_PACKED_E
            return lists != nullptr;
        }
    }
    if (wrap) SNB_LAUNCH_LDS((k_directEnergy<Real, MC, true>), gridAll, listLds, p, q, nExclBlocks, nListBlocks);
    else SNB_LAUNCH_LDS((k_directEnergy<Real, MC, false>), gridAll, listLds, p, q, nExclBlocks, nListBlocks);
    return lists != nullptr;
}
template <typename Real> bool launchDirectEnergy(const DirectParams<Real>& p, int mc, bool wrap, const PairListParams<Real>* lists, hipStream_t s, hipEvent_t evStart, hipEvent_t evStop, bool* timed) {
    switch (mc) {
        case MC_NOCUTOFF: return launchDirectEnergyMC<Real, MC_NOCUTOFF>(p, wrap, lists, s, evStart, evStop, timed);
        case MC_RF: return launchDirectEnergyMC<Real, MC_RF>(p, wrap, lists, s, evStart, evStop, timed);
        case MC_EWALD: return launchDirectEnergyMC<Real, MC_EWALD>(p, wrap, lists, s, evStart, evStop, timed);
        default: return launchDirectEnergyMC<Real, MC_LJPME>(p, wrap, lists, s, evStart, evStop, timed);
    }
}
template bool launchDirectEnergy<float>(const DirectParams<float>&, int, bool, const PairListParams<float>*, hipStream_t, hipEvent_t, hipEvent_t, bool*);
template bool launchDirectEnergy<double>(const DirectParams<double>&, int, bool, const PairListParams<double>*, hipStream_t, hipEvent_t, hipEvent_t, bool*);

// ---- 1-4 exceptions: ReferenceSlicedLJCoulomb14.cpp:61-95 ----------------------------------------
template <typename Real, bool ENERGY, bool FORCES> __device__ __forceinline__ void exceptionsBody(const PairListParams<Real>& p, const int blk) {
    extern __shared__ double s_sliceE[];   // [2*S]
    const int nS2 = 2 * p.nSlices;
    if (ENERGY) { for (int i = threadIdx.x; i < nS2; i += 256) s_sliceE[i] = 0.0; __syncthreads(); }
    const int k = blk * 256 + threadIdx.x;
    double e0 = 0, e1 = 0; int slice = 0;
    if (k < p.n) {
        int2 ij = p.pairs[k];
        ij.x = p.userToSorted[ij.x]; ij.y = p.userToSorted[ij.y];
        const auto par = p.params[k];
        const auto xi = p.posq[ij.x]; const auto xj = p.posq[ij.y];
        Real dx = xi.x - xj.x, dy = xi.y - xj.y, dz = xi.z - xj.z;
        if (p.periodic) { Real inv[3] = {Real(1) / p.box[0], Real(1) / p.box[4], Real(1) / p.box[8]}; wrapDelta<Real>(dx, dy, dz, p.box, inv); }
        else unwrapDelta<Real>(dx, dy, dz, p.imageOffset, ij.x, ij.y);
        const Real invR = rsq(dx * dx + dy * dy + dz * dz);
        Real s2 = invR * par.x; s2 *= s2;
        const Real s6 = s2 * s2 * s2;
        slice = (int)par.w;
        const Real lamC = p.lambdas[2 * slice], lamL = p.lambdas[2 * slice + 1];
        Real dEdR = lamL * par.y * (Real(12) * s6 - Real(6)) * s6 + lamC * par.z * invR;
        dEdR *= invR * invR;
        if constexpr (FORCES) {
        fAdd(p, p.fx, ij.x, dEdR * dx); fAdd(p, p.fy, ij.x, dEdR * dy); fAdd(p, p.fz, ij.x, dEdR * dz);
        fAdd(p, p.fx, ij.y, -dEdR * dx); fAdd(p, p.fy, ij.y, -dEdR * dy); fAdd(p, p.fz, ij.y, -dEdR * dz);
        }
        if (ENERGY && p.sliceNeed[slice]) { e0 = par.z * invR; e1 = par.y * (s6 - Real(1)) * s6; }
    }
    if (ENERGY) {
        if (k < p.n) {
            __hip_atomic_fetch_add(&s_sliceE[2 * slice], e0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_add(&s_sliceE[2 * slice + 1], e1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        __syncthreads();
        for (int i = threadIdx.x; i < nS2; i += 256) { const double v = s_sliceE[i]; if (v != 0.0) atomicAdd(&SNB_SLICE_E_PARTITION(p.sliceE, 2 * p.nSlices)[i], v); }
    }
}

// ---- Ewald exclusion corrections: ReferenceSlicedLJCoulombIxn.cpp:449-506 -------------------------
// One thread per ATOM walking its own exclusion list (CSR over sorted indices): every excluded pair is evaluated
// from both ends, so the force update is a plain read-modify-write of the atom's own accumulator -- no atomics
// (2 M scattered float atomics cost 70 us on MI355X; this costs a few us).  Energies: half a pair from each end,
// reduced per slice in LDS (ds_add_f64) and flushed with one global atomic per slice and work-group.
template <typename Real, bool ENERGY, bool FORCES> __device__ __forceinline__ void exclusionAtomsBody(const PairListParams<Real>& p, const int blk) {
    extern __shared__ double s_sliceE[];   // [2*S]
    const int nS2 = 2 * p.nSlices;
    if (ENERGY) { for (int i = threadIdx.x; i < nS2; i += 256) s_sliceE[i] = 0.0; __syncthreads(); }
    const int a = blk * 256 + threadIdx.x;
    const int ua = a < p.n ? p.sortedToUser[a] : -1;
    if (ua >= 0) {
        const int e0 = p.exclStart[ua], e1 = p.exclStart[ua + 1];
        if (e1 > e0) {
            const auto xi = p.posq[a];
            const auto sei = p.sigeps[a];
            const int si = p.blockSubset[a >> 5];
            const Real qi = xi.w * Real(SNB_ONE_4PI_EPS0);
            const Real c6i = Real(8) * sei.x * sei.x * sei.x * sei.y;
            Real inv[3] = {Real(1) / p.box[0], Real(1) / p.box[4], Real(1) / p.box[8]};
            Real fx = 0, fy = 0, fz = 0;
            for (int e = e0; e < e1; e++) {
                const int b = p.userToSorted[p.exclList[e]];
                const auto xj = p.posq[b];
                Real dx = xi.x - xj.x, dy = xi.y - xj.y, dz = xi.z - xj.z;
                if (p.periodic) wrapDelta<Real>(dx, dy, dz, p.box, inv); else unwrapDelta<Real>(dx, dy, dz, p.imageOffset, a, b);
                const Real r2 = dx * dx + dy * dy + dz * dz;
                const Real r = sqrt(r2);
                const Real invR = Real(1) / r;
                const Real ar = p.alpha * r;
                const int slice = sliceOf(si, p.blockSubset[b >> 5]);
                const Real lamC = p.lambdas[2 * slice], lamL = p.lambdas[2 * slice + 1];
                const Real qq = qi * xj.w;
                const Real ex = fexp(-ar * ar);
                // energy evaluations use libm erf in double even in the single-precision engine: the raw slice energy is a
                // small difference of large direct/reciprocal/exclusion sums and a 1e-7 bias in erf would show up in it.
                // The exclusion-correction ENERGY of a solvated box is a huge sum (2e7 kJ/mol for 300k atoms of water: every O-H and H-H pair of
                // every molecule) that the reciprocal-space energy cancels to a few thousand: it is formed in double from the stored
                // coordinates, charges and the double alpha -- products like k*qO*qH rounded to float are off by the SAME 1e-7 for all
                // 2e5 identical pairs, which alone was 0.8 kJ/mol (1.1e-3 of the water-water slice of the 96k-atom box).
                double erfv, rd = 0, qqd = 0;
                const bool wantE = ENERGY && p.sliceNeed[slice] != 0;
                if constexpr (!FORCES) { if (!wantE) continue; }
                if (wantE) {
                    rd = sqrt((double)dx * (double)dx + (double)dy * (double)dy + (double)dz * (double)dz);
                    qqd = (double)xi.w * (double)xj.w * SNB_ONE_4PI_EPS0;
                    erfv = erf(p.alpha64 * rd);
                } else erfv = erfOf(ar, ex);
                Real f = 0;
                if (erfv > 1e-6) {
                    f = -lamC * qq * invR * invR * invR * Real(exclusionG(ar, ex, erfv));
                    if (wantE) __hip_atomic_fetch_add(&s_sliceE[2 * slice], -0.5 * qqd * erfv / rd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                } else if (wantE)
                    __hip_atomic_fetch_add(&s_sliceE[2 * slice], -0.5 * p.alpha64 * 1.1283791670955126 * qqd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (p.ljpme) {
                    const auto sej = p.sigeps[b];
                    const Real c6 = c6i * (Real(8) * sej.x * sej.x * sej.x * sej.y);
                    const Real dar2 = p.alphaD * p.alphaD * r2;
                    const Real invR2 = invR * invR;
                    const Real coef = c6 * invR2 * invR2 * invR2;
                    Real h3, h4;      // 1 - exp(-dar2) (1 + dar2 + dar2^2/2 [+ dar2^3/6]), by series where they cancel (pair_math.h)
                    dispersionExclusion(dar2, fexp(-dar2), h3, h4);
                    if (wantE) __hip_atomic_fetch_add(&s_sliceE[2 * slice + 1], 0.5 * (double)(coef * h3), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    // reference: dEdR = -6 c6 r^-8 (...), forces[ii] -= lam*dEdR*delta  =>  +6 lam c6 r^-8 (...) * delta on ii
                    f += lamL * Real(6) * coef * invR2 * h4;
                }
                fx += f * dx; fy += f * dy; fz += f * dz;
            }
            if constexpr (FORCES) { fAdd(p, p.fx, a, fx); fAdd(p, p.fy, a, fy); fAdd(p, p.fz, a, fz); }   // atomics: the 1-4 blocks of the same launch add to the same atoms
        }
    }
    if (ENERGY) {
        __syncthreads();
        for (int i = threadIdx.x; i < nS2; i += 256) { const double v = s_sliceE[i]; if (v != 0.0) atomicAdd(&SNB_SLICE_E_PARTITION(p.sliceE, 2 * p.nSlices)[i], v); }
    }
}

// One launch for both O(N) pair lists: blocks [0, nExclBlocks) run the per-atom Ewald exclusion corrections (p.nExclAtoms atoms),
// the remaining blocks the 1-4 exceptions (p.n pairs).
template <typename Real, bool ENERGY> __global__ __launch_bounds__(256) void k_pairLists(const PairListParams<Real> p, const int nExclBlocks) {
    if ((int)blockIdx.x < nExclBlocks) { PairListParams<Real> q = p; q.n = p.nExclAtoms; exclusionAtomsBody<Real, ENERGY>(q, blockIdx.x); }
    else exceptionsBody<Real, ENERGY>(p, blockIdx.x - nExclBlocks);
}
template <typename Real> void launchPairLists(const PairListParams<Real>& p, bool energy, hipStream_t s) {
    const int nExclBlocks = (p.nExclAtoms + 255) / 256, nExcBlocks = (p.n + 255) / 256;
    if (nExclBlocks + nExcBlocks <= 0) return;
    dim3 grid(nExclBlocks + nExcBlocks), block(256);
    const size_t lds = sizeof(double) * 2 * p.nSlices;
    if (energy) hipLaunchKernelGGL((k_pairLists<Real, true>), grid, block, lds, s, p, nExclBlocks);
    else hipLaunchKernelGGL((k_pairLists<Real, false>), grid, block, 0, s, p, nExclBlocks);
}
template void launchPairLists<float>(const PairListParams<float>&, bool, hipStream_t);
template void launchPairLists<double>(const PairListParams<double>&, bool, hipStream_t);
// the same two lists with energies alone (steps with include_forces == 0 whose tile kernel did not take them)
template <typename Real> __global__ __launch_bounds__(256) void k_pairListsEnergy(const PairListParams<Real> p, const int nExclBlocks) {
    if ((int)blockIdx.x < nExclBlocks) { PairListParams<Real> q = p; q.n = p.nExclAtoms; exclusionAtomsBody<Real, true, false>(q, blockIdx.x); }
    else exceptionsBody<Real, true, false>(p, blockIdx.x - nExclBlocks);
}
template <typename Real> void launchPairListsEnergy(const PairListParams<Real>& p, hipStream_t s) {
    const int nExclBlocks = (p.nExclAtoms + 255) / 256, nExcBlocks = (p.n + 255) / 256;
    if (nExclBlocks + nExcBlocks <= 0) return;
    hipLaunchKernelGGL((k_pairListsEnergy<Real>), dim3(nExclBlocks + nExcBlocks), dim3(256), sizeof(double) * 2 * p.nSlices, s, p, nExclBlocks);
}
template void launchPairListsEnergy<float>(const PairListParams<float>&, hipStream_t);
template void launchPairListsEnergy<double>(const PairListParams<double>&, hipStream_t);

}  // namespace snb
