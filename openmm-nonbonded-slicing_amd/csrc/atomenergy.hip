// atomenergy.hip -- per-atom interaction energies with every subset (snb_evaluate_atom_energies).
//
// A[i][J][t] = raw energy (t = 0 Coulomb, 1 vdW) of atom i with all atoms of subset J.  The kernels here fill a table
// double [Npad][nsub][2] over the SORTED atom index; the finish kernel adds the closed-form terms and writes the caller's
// table in user order.  Analysis kernels beside the step kernels: they share the lists, the tiles and the parameter structs of
// direct.hip / pme.hip and the energy expressions of the energy-only kernels, and write nothing a step reads.
//
//   k_atomTiles      the tiles of the pair kernel.  A tile lies in one slice (32 i-atoms of one block x 32 j-atoms of one subset), so
//                    inside a tile every i-atom's pair energy belongs to column s_J and every j-atom's to column s_I: the i-side is the
//                    lane's own running sum (flushed per run of tiles of one j subset), the j-side a per-wave LDS region [32][2] the
//                    steps add into, flushed per tile.  Every pair is visited once (diagonal tiles included) and credits both ends.
//   list blocks      Ewald exclusion corrections (one thread per atom, the whole pair energy into its own row -- the partner's thread
//                    credits the other end) and 1-4 exceptions (one thread per pair, both ends), in the same launch.
//   k_atomPotential  q_i psi_J(r_i) for every held mesh J from the UNMIXED potentials (the pipeline of a rank that owns every mesh):
//                    the value part of the interpolation, no force arithmetic.
//   k_atomFinish     twice the Ewald self terms into column s_i, the neutralising background -2 c q_i Q_J, sorted -> user order.
//   k_groupSums      the same completed rows summed over lists of user atoms (snb_evaluate_group_energies): short
//   k_groupCombine   lists one thread per (group, subset), long lists one wave per chunk and a second launch that adds a group's chunks
//                    in list order -- no atomics, so a group's row is a function of the working table alone.
#include "snb_internal.h"
#include "pair_math.h"
#include <algorithm>
#include <cstring>
#include <vector>

namespace snb {

// raw pair energies of (i, j) as the energy instantiation of tileSteps (direct.hip) forms them; returns whether the pair is inside the cutoff
template <typename Real, int MC, bool WRAP>
__device__ __forceinline__ bool pairEnergies(const DirectParams<Real>& p, const typename Vec<Real>::T4 pi, const typename Vec<Real>::T2 sei, const Real qi, const Real c6i,
                                             const typename Vec<Real>::T4 xj, const typename Vec<Real>::T2 sj2, Real& eC, Real& eLJ) {
    Real dx = pi.x - xj.x, dy = pi.y - xj.y, dz = pi.z - xj.z;
    if (WRAP) wrapDelta<Real>(dx, dy, dz, p.box, p.invBoxDiag);
    const Real r2 = dx * dx + dy * dy + dz * dz;
    const Real invR = rsq(r2);
    const Real r = r2 * invR;
    const bool include = MC == MC_NOCUTOFF ? true : (r2 < p.cutoff2);
    // Lennard-Jones (sigeps holds sigma/2 and 2 sqrt(eps))
    const Real sig = sei.x + sj2.x;
    Real s2 = sig * invR; s2 *= s2;
    const Real s6 = s2 * s2 * s2;
    eLJ = sei.y * sj2.y * s6 * (s6 - Real(1));
    if (MC == MC_LJPME) {      // multiplicative grid term + potential shifts
        const Real dar2 = p.alphaD * p.alphaD * r2, dar4 = dar2 * dar2;
        const Real invR2 = invR * invR;
        const Real c6 = c6i * (Real(8) * sj2.x * sj2.x * sj2.x * sj2.y);
        const Real coef = invR2 * invR2 * invR2 * c6;
        const Real expd = fexp(-dar2);
        const Real epre = Real(1) + dar2 + Real(0.5) * dar4;
        Real sg2 = sig * sig; const Real sg6 = sg2 * sg2 * sg2 * p.invCut6;
        eLJ += coef * (Real(1) - expd * epre) + sei.y * sj2.y * (Real(1) - sg6) * sg6 - c6 * p.multShift6;
    } else if (MC != MC_NOCUTOFF) {
        if (p.useSwitch && r > p.switchDist) {
            const Real tt = (r - p.switchDist) * p.invSwitchWidth;
            eLJ *= Real(1) + tt * tt * tt * (Real(-10) + tt * (Real(15) - tt * Real(6)));
        }
    }
    const Real qq = qi * xj.w;
    if ((MC == MC_EWALD || MC == MC_LJPME) && sizeof(Real) == 4 && (p.ewUsePoly & SNB_POLY_ENERGY)) {
        // single precision: qq (1/r - Et(r^2)), Et = erf(ar)/r as the degree-13 polynomial of the packed energy kernels -- the error of the
        // Abramowitz & Stegun erfc is one-signed and an atom's column sums thousands of pairs whose direct and reciprocal parts cancel
        const Real t = r2 * p.ewScale - Real(1);
        Real et = p.ewPolyE[13];
#pragma unroll
        for (int k = 12; k >= 0; k--) et = et * t + p.ewPolyE[k];
        eC = qq * (invR - et);
    } else if (MC == MC_EWALD || MC == MC_LJPME) {
        const Real ar = p.alpha * r;
        eC = qq * invR * erfcFromExp(ar, expNegAlpha2R2(p.alpha2l2e, p.alpha, r2));
    } else if (MC == MC_RF) eC = qq * (invR + p.krf * r2 - p.crf);
    else eC = qq * invR;
    return include;
}

__device__ inline void tabAdd(double* tab, int nsub, int atom, int col, double e0, double e1) {
    double* const e = tab + ((size_t)atom * nsub + col) * 2;
    if (e0 != 0.0) gAdd(e, e0);
    if (e1 != 0.0) gAdd(e + 1, e1);
}

// 1-4 exceptions: the energies of exceptionsBody (direct.hip), credited to both ends
template <typename Real> __device__ __forceinline__ void atomExceptionsBody(const PairListParams<Real>& p, const int blk, double* tab, const int nsub) {
    const int k = blk * 256 + threadIdx.x;
    if (k >= p.n) return;
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
    const double e0 = par.z * invR, e1 = par.y * (s6 - Real(1)) * s6;
    tabAdd(tab, nsub, ij.x, p.blockSubset[ij.y >> 5], e0, e1);
    tabAdd(tab, nsub, ij.y, p.blockSubset[ij.x >> 5], e0, e1);
}

// Ewald exclusion corrections: the energies of exclusionAtomsBody (direct.hip; formed in double as there).  The atom's thread walks its own
// exclusion list and takes the WHOLE pair energy into its own row, column of the partner's subset; the partner's thread does the same.
template <typename Real> __device__ __forceinline__ void atomExclusionsBody(const PairListParams<Real>& p, const int blk, double* tab, const int nsub) {
    const int a = blk * 256 + threadIdx.x;
    const int ua = a < p.nExclAtoms ? p.sortedToUser[a] : -1;
    if (ua < 0) return;
    const int e0 = p.exclStart[ua], e1 = p.exclStart[ua + 1];
    if (e1 <= e0) return;
    const auto xi = p.posq[a];
    const auto sei = p.sigeps[a];
    const Real c6i = Real(8) * sei.x * sei.x * sei.x * sei.y;
    Real inv[3] = {Real(1) / p.box[0], Real(1) / p.box[4], Real(1) / p.box[8]};
    for (int e = e0; e < e1; e++) {
        const int b = p.userToSorted[p.exclList[e]];
        const auto xj = p.posq[b];
        Real dx = xi.x - xj.x, dy = xi.y - xj.y, dz = xi.z - xj.z;
        if (p.periodic) wrapDelta<Real>(dx, dy, dz, p.box, inv); else unwrapDelta<Real>(dx, dy, dz, p.imageOffset, a, b);
        const double rd = sqrt((double)dx * (double)dx + (double)dy * (double)dy + (double)dz * (double)dz);
        const double qqd = (double)xi.w * (double)xj.w * SNB_ONE_4PI_EPS0;
        const double erfv = erf(p.alpha64 * rd);
        const double ec = erfv > 1e-6 ? -qqd * erfv / rd : -p.alpha64 * 1.1283791670955126 * qqd;
        double el = 0;
        if (p.ljpme) {
            const Real r2 = dx * dx + dy * dy + dz * dz;
            const Real invR = Real(1) / sqrt(r2);
            const auto sej = p.sigeps[b];
            const Real c6 = c6i * (Real(8) * sej.x * sej.x * sej.x * sej.y);
            const Real dar2 = p.alphaD * p.alphaD * r2, dar4 = dar2 * dar2;
            const Real invR2 = invR * invR;
            el = (double)(c6 * invR2 * invR2 * invR2 * (Real(1) - fexp(-dar2) * (Real(1) + dar2 + Real(0.5) * dar4)));
        }
        tabAdd(tab, nsub, a, p.blockSubset[b >> 5], ec, el);
    }
}

// Tile kernel.  One wave per work item (an i-block and a run of its tiles), as the pair kernels; lane l holds i-atom l & 31 and meets the
// j-slots of half l >> 5, 16 steps per tile: at step s slot 16 (l >> 5) + ((l + s) & 15), so the 32 lanes of a half read 16 LDS entries
// (each by two lanes) and the j-side LDS adds of a step collide at most two ways.  The first nListBlocks work-groups run the pair lists.
// sliceNeed is not consulted: the table covers every slice.
template <typename Real, int MC, bool WRAP>
__global__ __launch_bounds__(256) void k_atomTiles(const DirectParams<Real> p, const PairListParams<Real> q, const int nExclBlocks, const int nListBlocks, double* const tab) {
    if ((int)blockIdx.x < nListBlocks) {
        if ((int)blockIdx.x < nExclBlocks) atomExclusionsBody<Real>(q, blockIdx.x, tab, p.nsub);
        else atomExceptionsBody<Real>(q, blockIdx.x - nExclBlocks, tab, p.nsub);
        return;
    }
    const int tileBlock = (int)blockIdx.x - nListBlocks, nTileBlocks = gridDim.x - nListBlocks;
    using T4 = typename Vec<Real>::T4;
    using T2 = typename Vec<Real>::T2;
    __shared__ T4 s_pos[4][32];
    __shared__ T2 s_se[4][32];
    __shared__ Real s_ej[4][32][2];
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int il = lane & 31, jh = lane >> 5;
    T4* const myPos = s_pos[wid];
    T2* const mySe = s_se[wid];
    Real (*const myEj)[2] = s_ej[wid];
    const int nsub = p.nsub;
    for (int item = tileBlock * 4 + wid; item < p.numWork; item += nTileBlocks * 4) {
        const int4 wi = p.workItems[p.workStart + item * p.workStride];
        const int I = __builtin_amdgcn_readfirstlane(wi.x);
        const int tBegin = __builtin_amdgcn_readfirstlane(wi.y), tEnd = tBegin + __builtin_amdgcn_readfirstlane(wi.z);
        const int sI = __builtin_amdgcn_readfirstlane(p.blockSubset[I]);
        const T4 pi = p.posq[I * 32 + il];
        const T2 sei = p.sigeps[I * 32 + il];
        const Real qi = pi.w * p.k4pe;
        Real c6i = 0;
        if (MC == MC_LJPME) c6i = Real(8) * sei.x * sei.x * sei.x * sei.y;
        Real ecl = 0, elj = 0;
        int curJ = -1;
        // i-side: the two lanes of an i-atom (one per j-half) merged, then one add per term into column curJ
        auto flushI = [&]() {
            const double a = (double)ecl + (double)__shfl_xor(ecl, 32, 64), b = (double)elj + (double)__shfl_xor(elj, 32, 64);
            if (curJ >= 0 && jh == 0) tabAdd(tab, nsub, I * 32 + il, curJ, a, b);
            ecl = 0; elj = 0;
        };
        for (int t = tBegin; t < tEnd; t++) {
            const int4 head = p.tileInfo[t];
            const int maskIdx = __builtin_amdgcn_readfirstlane(head.y), sJ = __builtin_amdgcn_readfirstlane(head.z);
            if (sJ != curJ) { flushI(); curJ = sJ; }
            const int code = p.tileJ[t * 32 + il];      // (both halves load it: lanes l and l + 32 hold the same j-slot here)
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
            } else { pj.x = Real(3e9) + Real(1e6) * il; pj.y = Real(-5e9); pj.z = Real(7e9); pj.w = 0; sej.x = 0; sej.y = 0; }      // padding slot: parked far away
            const unsigned maskWord = maskIdx >= 0 ? p.masks[maskIdx * 32 + il] : 0u;
            __builtin_amdgcn_wave_barrier();
            if (jh == 0) { myPos[il] = pj; mySe[il] = sej; myEj[il][0] = 0; myEj[il][1] = 0; }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
#pragma unroll 4
            for (int s = 0; s < 16; s++) {
                const int jj = 16 * jh + ((il + s) & 15);
                Real eC, eLJ;
                bool include = pairEnergies<Real, MC, WRAP>(p, pi, sei, qi, c6i, myPos[jj], mySe[jj], eC, eLJ);
                include = include && !((maskWord >> jj) & 1u);
                if (include) {
                    ecl += eC; elj += eLJ;
                    ldsAdd(&myEj[jj][0], eC); ldsAdd(&myEj[jj][1], eLJ);
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            // j-side: lanes 0-31 flush slot l into column s_I of their j-atom
            if (jh == 0 && code != -1) tabAdd(tab, nsub, code & SNB_JIDX_MASK, sI, (double)myEj[il][0], (double)myEj[il][1]);
        }
        flushI();
        __builtin_amdgcn_wave_barrier();
    }
}

template <typename Real, int MC> static void launchAtomPairsMC(const DirectParams<Real>& p, bool wrap, const PairListParams<Real>* lists, double* tab, hipStream_t s) {
    PairListParams<Real> q;
    std::memset(&q, 0, sizeof(q));
    int nExclBlocks = 0, nListBlocks = 0;
    if (lists) { q = *lists; nExclBlocks = (q.nExclAtoms + 255) / 256; nListBlocks = nExclBlocks + (q.n + 255) / 256; }
    const int nTileBlocks = p.numWork > 0 ? (p.numWork + 3) / 4 : 0;
    if (nTileBlocks + nListBlocks <= 0) return;
    const dim3 grid(nTileBlocks + nListBlocks), block(256);
    if (wrap) hipLaunchKernelGGL((k_atomTiles<Real, MC, true>), grid, block, 0, s, p, q, nExclBlocks, nListBlocks, tab);
    else hipLaunchKernelGGL((k_atomTiles<Real, MC, false>), grid, block, 0, s, p, q, nExclBlocks, nListBlocks, tab);
}
template <typename Real> void launchAtomPairs(const DirectParams<Real>& p, int mc, bool wrap, const PairListParams<Real>* lists, double* tab, hipStream_t s) {
    switch (mc) {
        case MC_NOCUTOFF: launchAtomPairsMC<Real, MC_NOCUTOFF>(p, wrap, lists, tab, s); break;
        case MC_RF: launchAtomPairsMC<Real, MC_RF>(p, wrap, lists, tab, s); break;
        case MC_EWALD: launchAtomPairsMC<Real, MC_EWALD>(p, wrap, lists, tab, s); break;
        default: launchAtomPairsMC<Real, MC_LJPME>(p, wrap, lists, tab, s); break;
    }
}
template void launchAtomPairs<float>(const DirectParams<float>&, int, bool, const PairListParams<float>*, double*, hipStream_t);
template void launchAtomPairs<double>(const DirectParams<double>&, int, bool, const PairListParams<double>*, double*, hipStream_t);

// ---- reciprocal potentials per atom ------------------------------------------------------------------------------------------------
// B-spline weights of order 5 (the values of pme.hip's bspline5, without the derivatives)
template <typename Real> __device__ inline void bsplineWeights5(Real dr, Real* d) {
    d[4] = 0; d[1] = dr; d[0] = 1 - dr; d[2] = 0; d[3] = 0;
    d[2] = Real(0.5) * dr * d[1];
    d[1] = Real(0.5) * ((dr + 1) * d[0] + (2 - dr) * d[1]);
    d[0] = Real(0.5) * (1 - dr) * d[0];
    d[3] = Real(1.0 / 3.0) * dr * d[2];
    d[2] = Real(1.0 / 3.0) * ((dr + 1) * d[1] + (3 - dr) * d[2]);
    d[1] = Real(1.0 / 3.0) * ((dr + 2) * d[0] + (2 - dr) * d[1]);
    d[0] = Real(1.0 / 3.0) * (1 - dr) * d[0];
    d[4] = Real(0.25) * dr * d[3];
    d[3] = Real(0.25) * ((dr + 1) * d[2] + (4 - dr) * d[3]);
    d[2] = Real(0.25) * ((dr + 2) * d[1] + (3 - dr) * d[2]);
    d[1] = Real(0.25) * ((dr + 3) * d[0] + (2 - dr) * d[1]);
    d[0] = Real(0.25) * (1 - dr) * d[0];
}
// 32 lanes per atom, lane = one (x, y) row of the 5 x 5 x 5 stencil, as the gather interpolation k_interpolate (pme.hip); the atom loops over
// the held meshes (unmixed: mesh g is the potential of subset gridSubset[g]) and adds q_i psi_J(r_i) -- c6_i psi_J for the dispersion mesh --
// into its row of the table.  Plain read-modify-write: the launch is ordered behind the pair kernels and an entry has one writer here.
template <typename Real> __global__ __launch_bounds__(256) void k_atomPotential(const PmeParams<Real> p, double* const tab) {
    const int gid = blockIdx.x * 8 + (threadIdx.x >> 5);
    const int r = threadIdx.x & 31;
    if (gid >= p.natoms) return;
    const int si = p.atomSubset[gid];
    if (si < 0) return;      // padding slot (uniform over the atom's 32 lanes)
    const auto pos = p.posq[gid];
    Real q = pos.w;
    if (p.dispersion) { const auto se = p.sigeps[gid]; q = Real(8) * se.x * se.x * se.x * se.y; }
    if (q == Real(0)) return;
    int idx[3]; Real fr[3];
    gridCoord<Real>(p.recip, p.recipLo, pos.x, pos.y, pos.z, p.d.nx, p.d.ny, p.d.nz, idx, fr);
    Real tx[5], ty[5], tz[5];
    bsplineWeights5<Real>(fr[0], tx); bsplineWeights5<Real>(fr[1], ty); bsplineWeights5<Real>(fr[2], tz);
    const int ix = r < 25 ? r / 5 : 0, iy = r < 25 ? r - ix * 5 : 0;
    int xi = idx[0] + ix; if (xi >= p.d.nx) xi -= p.d.nx;
    int yi = idx[1] + iy; if (yi >= p.d.ny) yi -= p.d.ny;
    Real w = 0;
#pragma unroll
    for (int k = 0; k < 5; k++) { if (k == ix) w = tx[k]; }
#pragma unroll
    for (int k = 0; k < 5; k++) { if (k == iy) w *= ty[k]; }
    if (r >= 25) w = 0;
    const int term = p.dispersion ? 1 : 0;
    for (int g = 0; g < p.nsub; g++) {
        const Real* row = p.gridReal + (((size_t)g * p.d.nx + xi) * p.d.ny + yi) * p.d.nz;
        Real sz = 0;
#pragma unroll
        for (int iz = 0; iz < 5; iz++) {
            int zi = idx[2] + iz; if (zi >= p.d.nz) zi -= p.d.nz;
            sz += tz[iz] * row[zi];
        }
        double v = (double)(w * sz);
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (r == 0) tab[((size_t)gid * p.nsubTotal + p.gridSubset[g]) * 2 + term] += (double)q * v;
    }
}
template <typename Real> void launchAtomPotential(const PmeParams<Real>& p, double* tab, hipStream_t s) {
    if (p.natoms <= 0 || p.nsub <= 0) return;
    hipLaunchKernelGGL((k_atomPotential<Real>), dim3((p.natoms + 7) / 8), dim3(256), 0, s, p, tab);
}
template void launchAtomPotential<float>(const PmeParams<float>&, double*, hipStream_t);
template void launchAtomPotential<double>(const PmeParams<double>&, double*, hipStream_t);

// ---- finish ------------------------------------------------------------------------------------------------------------------------
// Entry (a, J) of the sorted-order working table, completed: the sum rule halves the diagonal column, so the self terms enter twice; the
// background -2 c q_i Q_J sums to the slice's c Q_I Q_J (x 2 off the diagonal) of sliceFinishClosedForm.
template <typename Real>
__device__ __forceinline__ void atomRowEntry(const double* __restrict__ tab, const int a, const int J, const int nsub, const int* __restrict__ blockSubset,
                                             const typename Vec<Real>::T4* __restrict__ posq, const typename Vec<Real>::T2* __restrict__ sigeps, const SliceFinish& f,
                                             double& e0, double& e1) {
    const double* e = tab + ((size_t)a * nsub + J) * 2;
    e0 = e[0]; e1 = e[1];
    if (f.sums) {
        const double q = (double)posq[a].w;
        e0 += 2.0 * f.background * q * f.sums[3 * J];
        if (blockSubset[a >> 5] == J) {
            const auto se = sigeps[a];
            const double hs = (double)se.x, c6 = 8.0 * hs * hs * hs * (double)se.y;
            e0 += 2.0 * f.selfCoulomb * q * q;
            e1 += 2.0 * f.selfDispersion * c6 * c6;
        }
    }
}
// One thread per (user atom, subset): closed-form terms, sorted -> user order.
template <typename Real>
__global__ __launch_bounds__(256) void k_atomFinish(const double* __restrict__ tab, const int* __restrict__ userToSorted, const int* __restrict__ blockSubset,
                                                    const typename Vec<Real>::T4* __restrict__ posq, const typename Vec<Real>::T2* __restrict__ sigeps,
                                                    const int nAtoms, const int nsub, const SliceFinish f, double* __restrict__ out) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)nAtoms * nsub) return;
    const int u = (int)(t / nsub), J = (int)(t - (long long)u * nsub);
    double e0, e1;
    atomRowEntry<Real>(tab, userToSorted[u], J, nsub, blockSubset, posq, sigeps, f, e0, e1);
    out[2 * t] = e0; out[2 * t + 1] = e1;
}
template <typename Real>
void launchAtomFinish(const double* tab, const int* userToSorted, const int* blockSubset, const typename Vec<Real>::T4* posq, const typename Vec<Real>::T2* sigeps,
                      int nAtoms, int nsub, const SliceFinish& f, double* out, hipStream_t s) {
    const long long n = (long long)nAtoms * nsub;
    if (n <= 0) return;
    hipLaunchKernelGGL((k_atomFinish<Real>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, tab, userToSorted, blockSubset, posq, sigeps, nAtoms, nsub, f, out);
}
template void launchAtomFinish<float>(const double*, const int*, const int*, const Vec<float>::T4*, const Vec<float>::T2*, int, int, const SliceFinish&, double*, hipStream_t);
template void launchAtomFinish<double>(const double*, const int*, const int*, const Vec<double>::T4*, const Vec<double>::T2*, int, int, const SliceFinish&, double*, hipStream_t);

// ---- groups ------------------------------------------------------------------------------------------------------------------------
// Rows of the completed table summed over lists of USER atom indices (CSR: start[G + 1], atoms[start[G]]; lists may overlap, repeat an index,
// be empty).  The mapping follows the list's length (planGroups):
//   up to SNB_GROUP_SERIAL atoms   one THREAD per (group, subset) walks the list -- a three-atom water costs nsub lanes, not a wave;
//   longer                         chunks of max(256, length / 256 rounded up to 64) atoms, one WAVE per chunk: lanes stride the chunk, a fixed
//                                  butterfly adds the 64 partial sums, lane 0 stores the chunk's row; k_groupCombine then adds a group's
//                                  chunks (256 at the most) in list order.  "The protein" spreads over as many waves as it has chunks.
// Both kinds run in one launch (the first nSmallBlocks work-groups take the short lists).  Every entry of out[G][nsub][2] is written once.
void planGroups(int nGroups, const int32_t* start, GroupPlan& plan) {
    plan.nGroups = nGroups; plan.nSmall = plan.nChunks = plan.nLarge = 0;
    const int nIdx = start[nGroups];
    std::vector<int> small, chunks, large;
    for (int g = 0; g < nGroups; g++) {
        const int b = start[g], len = start[g + 1] - b;
        if (len <= SNB_GROUP_SERIAL) { small.push_back(g); continue; }
        const int clen = std::max(256, ((len + 255) / 256 + 63) / 64 * 64);
        const int first = (int)chunks.size() / 4;
        for (int c = b; c < b + len; c += clen) { chunks.push_back(g); chunks.push_back(c); chunks.push_back(std::min(c + clen, b + len)); chunks.push_back(0); }
        large.push_back(g); large.push_back(first); large.push_back((int)chunks.size() / 4 - first); large.push_back(0);
    }
    plan.nSmall = (int)small.size(); plan.nChunks = (int)chunks.size() / 4; plan.nLarge = (int)large.size() / 4;
    auto align4 = [](size_t n) { return (n + 3) / 4 * 4; };
    plan.offStart = 0; plan.offAtoms = (int)align4(nGroups + 1); plan.offSmall = (int)align4(plan.offAtoms + (size_t)nIdx);
    plan.offChunks = (int)align4(plan.offSmall + small.size()); plan.offLarge = plan.offChunks + (int)chunks.size();
    plan.packed.assign(plan.offLarge + large.size(), 0);
    std::copy(start, start + nGroups + 1, plan.packed.begin());
    std::copy(small.begin(), small.end(), plan.packed.begin() + plan.offSmall);
    std::copy(chunks.begin(), chunks.end(), plan.packed.begin() + plan.offChunks);
    std::copy(large.begin(), large.end(), plan.packed.begin() + plan.offLarge);
}

template <typename Real>
__global__ __launch_bounds__(256) void k_groupSums(const double* __restrict__ tab, const int* __restrict__ userToSorted, const int* __restrict__ blockSubset,
                                                   const typename Vec<Real>::T4* __restrict__ posq, const typename Vec<Real>::T2* __restrict__ sigeps, const int nsub, const SliceFinish f,
                                                   const int* __restrict__ start, const int* __restrict__ atoms, const int* __restrict__ small, const int nSmall, const int nSmallBlocks,
                                                   const int4* __restrict__ chunks, const int nChunks, double* __restrict__ partial, double* __restrict__ out) {
    if ((int)blockIdx.x < nSmallBlocks) {
        const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
        if (t >= (long long)nSmall * nsub) return;
        const int k = (int)(t / nsub), J = (int)(t - (long long)k * nsub);
        const int g = small[k];
        double s0 = 0, s1 = 0;
        for (int e = start[g], eEnd = start[g + 1]; e < eEnd; e++) {
            double e0, e1;
            atomRowEntry<Real>(tab, userToSorted[atoms[e]], J, nsub, blockSubset, posq, sigeps, f, e0, e1);
            s0 += e0; s1 += e1;
        }
        double* const o = out + ((size_t)g * nsub + J) * 2;
        o[0] = s0; o[1] = s1;
        return;
    }
    const int c = ((int)blockIdx.x - nSmallBlocks) * 4 + (int)(threadIdx.x >> 6);      // (uniform over the wave)
    if (c >= nChunks) return;
    const int lane = threadIdx.x & 63;
    const int4 ch = chunks[c];
    for (int J = 0; J < nsub; J++) {
        double s0 = 0, s1 = 0;
        for (int e = ch.y + lane; e < ch.z; e += 64) {
            double e0, e1;
            atomRowEntry<Real>(tab, userToSorted[atoms[e]], J, nsub, blockSubset, posq, sigeps, f, e0, e1);
            s0 += e0; s1 += e1;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { s0 += __shfl_xor(s0, o, 64); s1 += __shfl_xor(s1, o, 64); }
        if (lane == 0) { double* const o = partial + ((size_t)c * nsub + J) * 2; o[0] = s0; o[1] = s1; }
    }
}
// one thread per (long group, subset, term): its chunks' rows in list order
__global__ __launch_bounds__(256) void k_groupCombine(const int4* __restrict__ large, const int nLarge, const int nsub, const double* __restrict__ partial, double* __restrict__ out) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int row = 2 * nsub;
    if (t >= (long long)nLarge * row) return;
    const int k = (int)(t / row), i = (int)(t - (long long)k * row);
    const int4 lg = large[k];
    double s = 0;
    for (int c = lg.y; c < lg.y + lg.z; c++) s += partial[(size_t)c * row + i];
    out[(size_t)lg.x * row + i] = s;
}
template <typename Real>
void launchGroupFinish(const double* tab, const int* userToSorted, const int* blockSubset, const typename Vec<Real>::T4* posq, const typename Vec<Real>::T2* sigeps, int nsub,
                       const SliceFinish& f, const GroupPlan& plan, const int* packed, double* partial, double* out, hipStream_t s) {
    const int nSmallBlocks = (int)(((long long)plan.nSmall * nsub + 255) / 256), nChunkBlocks = (plan.nChunks + 3) / 4;
    if (nSmallBlocks + nChunkBlocks <= 0) return;
    const int4* const chunks = reinterpret_cast<const int4*>(packed + plan.offChunks);
    const int4* const large = reinterpret_cast<const int4*>(packed + plan.offLarge);
    hipLaunchKernelGGL((k_groupSums<Real>), dim3(nSmallBlocks + nChunkBlocks), dim3(256), 0, s, tab, userToSorted, blockSubset, posq, sigeps, nsub, f, packed + plan.offStart,
                       packed + plan.offAtoms, packed + plan.offSmall, plan.nSmall, nSmallBlocks, chunks, plan.nChunks, partial, out);
    if (plan.nLarge > 0) hipLaunchKernelGGL(k_groupCombine, dim3((unsigned)(((long long)plan.nLarge * 2 * nsub + 255) / 256)), dim3(256), 0, s, large, plan.nLarge, nsub, partial, out);
}
template void launchGroupFinish<float>(const double*, const int*, const int*, const Vec<float>::T4*, const Vec<float>::T2*, int, const SliceFinish&, const GroupPlan&, const int*, double*, double*, hipStream_t);
template void launchGroupFinish<double>(const double*, const int*, const int*, const Vec<double>::T4*, const Vec<double>::T2*, int, const SliceFinish&, const GroupPlan&, const int*, double*, double*, hipStream_t);

}  // namespace snb
