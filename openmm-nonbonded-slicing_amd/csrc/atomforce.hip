// atomforce.hip -- per-atom forces by partner subset and term (snb_evaluate_atom_forces).
//
// G[i][J][t] = - d E_raw[slice(s_i, J)][t] / d r_i  (t = 0 Coulomb, 1 vdW; a 3-vector): the force all atoms of subset J put on atom i, every
// lambda 1.  The kernels here fill a table double [Npad][nsub][2][3] over the SORTED atom index; the finish kernel writes the caller's table
// in user order.  The force twins of the kernels of atomenergy.hip: the same lists, tiles and parameter structs, 3-vectors where those carry
// scalars, and nothing a step reads is written.
//
//   k_atomForceTiles  the tiles of the pair kernel.  A tile lies in one slice, so inside a tile every i-atom's pair force belongs to column
//                     s_J and every j-atom's (the opposite force) to column s_I: the i-side is the lane's six running sums (flushed per run of
//                     tiles of one j subset), the j-side a per-wave LDS region [32][6] the steps add into, flushed per tile with the sign turned.
//   list blocks       Ewald exclusion corrections (one thread per atom, the whole pair force into its own row -- the partner's thread
//                     credits the other end) and 1-4 exceptions (one thread per pair, both ends), in the same launch.
//   k_atomField       -q_i grad psi_J(r_i) for every held mesh J from the UNMIXED potentials: the derivative part of the interpolation.
//   k_atomForceFinish sorted -> user order.  (Self term, neutralising background and dispersion correction carry no force.)
#include "snb_internal.h"
#include "pair_math.h"
#include <cstring>
#include <type_traits>

namespace snb {

// Force factors of the pair (i, j), every lambda 1, as the forces instantiation of tileSteps (direct.hip) forms them: the force on i is
// fC * delta (Coulomb) + fLJ * delta (vdW), delta = r_i - r_j (returned in dx, dy, dz).  Double precision takes the Ewald and dispersion
// factors from the polynomials of the forces kernels where the guard keeps them (p.ewUsePoly), else and in single precision from erfcFromExp / fexp.  Returns whether the pair is inside the cutoff.
template <typename Real, int MC, bool WRAP>
__device__ __forceinline__ bool pairForces(const DirectParams<Real>& p, const typename Vec<Real>::T4 pi, const typename Vec<Real>::T2 sei, const Real qi, const Real c6i,
                                           const typename Vec<Real>::T4 xj, const typename Vec<Real>::T2 sj2, Real& dx, Real& dy, Real& dz, Real& fC, Real& fLJ) {
    dx = pi.x - xj.x; dy = pi.y - xj.y; dz = pi.z - xj.z;
    if (WRAP) wrapDelta<Real>(dx, dy, dz, p.box, p.invBoxDiag);
    const Real r2 = dx * dx + dy * dy + dz * dz;
    const Real invR = rsq(r2);
    const Real r = r2 * invR;
    const bool include = MC == MC_NOCUTOFF ? true : (r2 < p.cutoff2);
    // Lennard-Jones (sigeps holds sigma/2 and 2 sqrt(eps))
    const Real sig = sei.x + sj2.x;
    Real s2 = sig * invR; s2 *= s2;
    const Real s6 = s2 * s2 * s2;
    const Real es6 = sei.y * sj2.y * s6;
    fLJ = es6 * (Real(12) * s6 - Real(6));
    if (MC == MC_LJPME && std::is_same<Real, double>::value && (p.ewUsePoly & SNB_POLY_DISPERSION)) {
        const Real t = r2 * p.ewScale - Real(1);
        Real gd = p.dispPoly[SNB_DISP_DEG_F64];
#pragma unroll
        for (int k = SNB_DISP_DEG_F64 - 1; k >= 0; k--) gd = gd * t + p.dispPoly[k];
        const Real c6 = c6i * (Real(8) * sj2.x * sj2.x * sj2.x * sj2.y);
        fLJ += Real(6) * c6 * gd * r2;
    } else if (MC == MC_LJPME) {
        const Real dar2 = p.alphaD * p.alphaD * r2;
        const Real dar4 = dar2 * dar2, dar6 = dar4 * dar2;
        const Real invR2 = invR * invR;
        const Real c6 = c6i * (Real(8) * sj2.x * sj2.x * sj2.x * sj2.y);
        const Real coef = invR2 * invR2 * invR2 * c6;
        const Real expd = fexp(-dar2);
        const Real dpre = Real(1) + dar2 + Real(0.5) * dar4 + dar6 * Real(1.0 / 6.0);
        fLJ += Real(6) * coef * (Real(1) - expd * dpre);
    } else if (MC != MC_NOCUTOFF) {
        if (p.useSwitch && r > p.switchDist) {
            const Real tt = (r - p.switchDist) * p.invSwitchWidth;
            const Real sw = Real(1) + tt * tt * tt * (Real(-10) + tt * (Real(15) - tt * Real(6)));
            const Real dsw = tt * tt * (Real(-30) + tt * (Real(60) - tt * Real(30))) * p.invSwitchWidth;
            fLJ = fLJ * sw - es6 * (s6 - Real(1)) * dsw * r;
        }
    }
    const Real qq = qi * xj.w;
    if ((MC == MC_EWALD || MC == MC_LJPME) && std::is_same<Real, double>::value && (p.ewUsePoly & SNB_POLY_FORCE)) {
        const Real t = r2 * p.ewScale - Real(1);
        Real bt = p.ewPoly[SNB_EW_DEG_F64];
#pragma unroll
        for (int k = SNB_EW_DEG_F64 - 1; k >= 0; k--) bt = bt * t + p.ewPoly[k];
        fC = qq * (invR - r2 * bt);
    } else if (MC == MC_EWALD || MC == MC_LJPME) {
        const Real ar = p.alpha * r;
        const Real ex = expNegAlpha2R2(p.alpha2l2e, p.alpha, r2);
        fC = qq * invR * (erfcFromExp(ar, ex) + ar * ex * Real(1.1283791670955126));
    } else if (MC == MC_RF) fC = qq * (invR - Real(2) * p.krf * r2);
    else fC = qq * invR;
    const Real invR2 = invR * invR;
    fC *= invR2; fLJ *= invR2;
    return include;
}

// one column entry of the table: tab[atom][col][term][0..2] += sign * v; adds of exactly zero are skipped
__device__ inline void tabAdd3(double* tab, int nsub, int atom, int col, int term, double x, double y, double z) {
    double* const e = tab + (((size_t)atom * nsub + col) * 2 + term) * 3;
    if (x != 0.0) gAdd(e, x);
    if (y != 0.0) gAdd(e + 1, y);
    if (z != 0.0) gAdd(e + 2, z);
}

// 1-4 exceptions: the forces of exceptionsBody (direct.hip) with every lambda 1, credited to both ends
template <typename Real> __device__ __forceinline__ void atomForceExceptionsBody(const PairListParams<Real>& p, const int blk, double* tab, const int nsub) {
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
    const Real invR2 = invR * invR;
    const double fC = par.z * invR * invR2, fL = par.y * (Real(12) * s6 - Real(6)) * s6 * invR2;
    const int sI = p.blockSubset[ij.x >> 5], sJ = p.blockSubset[ij.y >> 5];
    tabAdd3(tab, nsub, ij.x, sJ, 0, fC * dx, fC * dy, fC * dz);
    tabAdd3(tab, nsub, ij.x, sJ, 1, fL * dx, fL * dy, fL * dz);
    tabAdd3(tab, nsub, ij.y, sI, 0, -fC * dx, -fC * dy, -fC * dz);
    tabAdd3(tab, nsub, ij.y, sI, 1, -fL * dx, -fL * dy, -fL * dz);
}

// Ewald exclusion corrections: the forces of exclusionAtomsBody (direct.hip) with every lambda 1, formed in double from the stored
// coordinates and charges.  The atom's thread walks its own exclusion list and takes the pair force into its own row, column of the
// partner's subset; the partner's thread does the other end.
template <typename Real> __device__ __forceinline__ void atomForceExclusionsBody(const PairListParams<Real>& p, const int blk, double* tab, const int nsub) {
    const int a = blk * 256 + threadIdx.x;
    const int ua = a < p.nExclAtoms ? p.sortedToUser[a] : -1;
    if (ua < 0) return;
    const int e0 = p.exclStart[ua], e1 = p.exclStart[ua + 1];
    if (e1 <= e0) return;
    const auto xi = p.posq[a];
    const auto sei = p.sigeps[a];
    const double c6i = 8.0 * (double)sei.x * (double)sei.x * (double)sei.x * (double)sei.y;
    Real inv[3] = {Real(1) / p.box[0], Real(1) / p.box[4], Real(1) / p.box[8]};
    for (int e = e0; e < e1; e++) {
        const int b = p.userToSorted[p.exclList[e]];
        const auto xj = p.posq[b];
        Real dx = xi.x - xj.x, dy = xi.y - xj.y, dz = xi.z - xj.z;
        if (p.periodic) wrapDelta<Real>(dx, dy, dz, p.box, inv); else unwrapDelta<Real>(dx, dy, dz, p.imageOffset, a, b);
        const double ddx = dx, ddy = dy, ddz = dz;
        const double r2 = ddx * ddx + ddy * ddy + ddz * ddz;
        const double rd = sqrt(r2), invR = 1.0 / rd;
        const double x = p.alpha64 * rd;
        const double qqd = (double)xi.w * (double)xj.w * SNB_ONE_4PI_EPS0;
        const double erfv = erf(x);
        const int col = p.blockSubset[b >> 5];
        if (erfv > 1e-6) {
            const double f = -qqd * invR * invR * invR * exclusionG(x, exp(-x * x), erfv);
            tabAdd3(tab, nsub, a, col, 0, f * ddx, f * ddy, f * ddz);
        }
        if (p.ljpme) {
            const auto sej = p.sigeps[b];
            const double c6 = c6i * (8.0 * (double)sej.x * (double)sej.x * (double)sej.x * (double)sej.y);
            const double ad = (double)p.alphaD;
            const double dar2 = ad * ad * r2, dar4 = dar2 * dar2, dar6 = dar4 * dar2;
            const double invR2 = invR * invR;
            const double f = 6.0 * c6 * invR2 * invR2 * invR2 * invR2 * (1.0 - exp(-dar2) * (1.0 + dar2 + 0.5 * dar4 + dar6 * (1.0 / 6.0)));
            tabAdd3(tab, nsub, a, col, 1, f * ddx, f * ddy, f * ddz);
        }
    }
}

// Tile kernel, the shape of k_atomTiles (atomenergy.hip).  One wave per work item (an i-block and a run of its tiles); lane l holds i-atom
// l & 31 and meets the j-slots of half l >> 5, 16 steps per tile: at step s slot 16 (l >> 5) + ((l + s) & 15), so the j-side LDS adds of a
// step collide at most two ways.  The first nListBlocks work-groups run the pair lists.  sliceNeed is not consulted: the table covers every slice.
template <typename Real, int MC, bool WRAP>
__global__ __launch_bounds__(256) void k_atomForceTiles(const DirectParams<Real> p, const PairListParams<Real> q, const int nExclBlocks, const int nListBlocks, double* const tab) {
    if ((int)blockIdx.x < nListBlocks) {
        if ((int)blockIdx.x < nExclBlocks) atomForceExclusionsBody<Real>(q, blockIdx.x, tab, p.nsub);
        else atomForceExceptionsBody<Real>(q, blockIdx.x - nExclBlocks, tab, p.nsub);
        return;
    }
    const int tileBlock = (int)blockIdx.x - nListBlocks, nTileBlocks = gridDim.x - nListBlocks;
    using T4 = typename Vec<Real>::T4;
    using T2 = typename Vec<Real>::T2;
    __shared__ T4 s_pos[4][32];
    __shared__ T2 s_se[4][32];
    __shared__ Real s_fj[4][32][6];
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int il = lane & 31, jh = lane >> 5;
    T4* const myPos = s_pos[wid];
    T2* const mySe = s_se[wid];
    Real (*const myFj)[6] = s_fj[wid];
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
        Real fi[6] = {0, 0, 0, 0, 0, 0};      // Coulomb x y z, vdW x y z
        int curJ = -1;
        // i-side: the two lanes of an i-atom (one per j-half) merged, then one add per component into column curJ
        auto flushI = [&]() {
            double m[6];
#pragma unroll
            for (int c = 0; c < 6; c++) { m[c] = (double)fi[c] + (double)__shfl_xor(fi[c], 32, 64); fi[c] = 0; }
            if (curJ >= 0 && jh == 0) {
                tabAdd3(tab, nsub, I * 32 + il, curJ, 0, m[0], m[1], m[2]);
                tabAdd3(tab, nsub, I * 32 + il, curJ, 1, m[3], m[4], m[5]);
            }
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
            if (jh == 0) {
                myPos[il] = pj; mySe[il] = sej;
#pragma unroll
                for (int c = 0; c < 6; c++) myFj[il][c] = 0;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
#pragma unroll 2
            for (int s = 0; s < 16; s++) {
                const int jj = 16 * jh + ((il + s) & 15);
                Real dx, dy, dz, fC, fLJ;
                bool include = pairForces<Real, MC, WRAP>(p, pi, sei, qi, c6i, myPos[jj], mySe[jj], dx, dy, dz, fC, fLJ);
                include = include && !((maskWord >> jj) & 1u);
                if (include) {
                    const Real g[6] = {fC * dx, fC * dy, fC * dz, fLJ * dx, fLJ * dy, fLJ * dz};
#pragma unroll
                    for (int c = 0; c < 6; c++) { fi[c] += g[c]; ldsAdd(&myFj[jj][c], g[c]); }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            // j-side: lanes 0-31 flush slot l into column s_I of their j-atom, with the opposite sign
            if (jh == 0 && code != -1) {
                const int ja = code & SNB_JIDX_MASK;
                tabAdd3(tab, nsub, ja, sI, 0, -(double)myFj[il][0], -(double)myFj[il][1], -(double)myFj[il][2]);
                tabAdd3(tab, nsub, ja, sI, 1, -(double)myFj[il][3], -(double)myFj[il][4], -(double)myFj[il][5]);
            }
        }
        flushI();
        __builtin_amdgcn_wave_barrier();
    }
}

template <typename Real, int MC> static void launchAtomForcePairsMC(const DirectParams<Real>& p, bool wrap, const PairListParams<Real>* lists, double* tab, hipStream_t s) {
    PairListParams<Real> q;
    std::memset(&q, 0, sizeof(q));
    int nExclBlocks = 0, nListBlocks = 0;
    if (lists) { q = *lists; nExclBlocks = (q.nExclAtoms + 255) / 256; nListBlocks = nExclBlocks + (q.n + 255) / 256; }
    const int nTileBlocks = p.numWork > 0 ? (p.numWork + 3) / 4 : 0;
    if (nTileBlocks + nListBlocks <= 0) return;
    const dim3 grid(nTileBlocks + nListBlocks), block(256);
    if (wrap) hipLaunchKernelGGL((k_atomForceTiles<Real, MC, true>), grid, block, 0, s, p, q, nExclBlocks, nListBlocks, tab);
    else hipLaunchKernelGGL((k_atomForceTiles<Real, MC, false>), grid, block, 0, s, p, q, nExclBlocks, nListBlocks, tab);
}
template <typename Real> void launchAtomForcePairs(const DirectParams<Real>& p, int mc, bool wrap, const PairListParams<Real>* lists, double* tab, hipStream_t s) {
    switch (mc) {
        case MC_NOCUTOFF: launchAtomForcePairsMC<Real, MC_NOCUTOFF>(p, wrap, lists, tab, s); break;
        case MC_RF: launchAtomForcePairsMC<Real, MC_RF>(p, wrap, lists, tab, s); break;
        case MC_EWALD: launchAtomForcePairsMC<Real, MC_EWALD>(p, wrap, lists, tab, s); break;
        default: launchAtomForcePairsMC<Real, MC_LJPME>(p, wrap, lists, tab, s); break;
    }
}
template void launchAtomForcePairs<float>(const DirectParams<float>&, int, bool, const PairListParams<float>*, double*, hipStream_t);
template void launchAtomForcePairs<double>(const DirectParams<double>&, int, bool, const PairListParams<double>*, double*, hipStream_t);

// ---- reciprocal field per atom -----------------------------------------------------------------------------------------------------
// The derivative part of k_interpolate (pme.hip), unmixed and without lambdas: 32 lanes per atom, lane = one (x, y) row of the 5 x 5 x 5
// stencil; the atom loops over the held meshes (mesh g is the potential of subset gridSubset[g]) and adds -q_i grad psi_J(r_i) -- c6_i for
// the dispersion mesh -- into its row of the table, through the same triclinic back-transformation.  Plain read-modify-write: the launch is
// ordered behind the pair kernel and an entry has one writer here.
template <typename Real> __global__ __launch_bounds__(256) void k_atomField(const PmeParams<Real> p, double* const tab) {
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
    Real tx[5], ty[5], tz[5], dx[5], dy[5], dz[5];
    bspline5<Real>(fr[0], tx, dx); bspline5<Real>(fr[1], ty, dy); bspline5<Real>(fr[2], tz, dz);
    const int ix = r < 25 ? r / 5 : 0, iy = r < 25 ? r - ix * 5 : 0;
    int xi = idx[0] + ix; if (xi >= p.d.nx) xi -= p.d.nx;
    int yi = idx[1] + iy; if (yi >= p.d.ny) yi -= p.d.ny;
    Real txv = 0, dxv = 0, tyv = 0, dyv = 0;
#pragma unroll
    for (int k = 0; k < 5; k++) { if (k == ix) { txv = tx[k]; dxv = dx[k]; } if (k == iy) { tyv = ty[k]; dyv = dy[k]; } }
    if (r >= 25) { txv = 0; dxv = 0; }
    const int term = p.dispersion ? 1 : 0;
    const double nx = p.d.nx, ny = p.d.ny, nz = p.d.nz;
    for (int g = 0; g < p.nsub; g++) {
        const Real* row = p.gridReal + (((size_t)g * p.d.nx + xi) * p.d.ny + yi) * p.d.nz;
        Real sz = 0, sdz = 0;
#pragma unroll
        for (int iz = 0; iz < 5; iz++) {
            int zi = idx[2] + iz; if (zi >= p.d.nz) zi -= p.d.nz;
            const Real gv = row[zi];
            sz += tz[iz] * gv; sdz += dz[iz] * gv;
        }
        double fx = (double)(dxv * tyv * sz), fy = (double)(txv * dyv * sz), fz = (double)(txv * tyv * sdz);
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) { fx += __shfl_xor(fx, o, 64); fy += __shfl_xor(fy, o, 64); fz += __shfl_xor(fz, o, 64); }
        if (r == 0) {
            const double mq = -(double)q;
            double* const e = tab + (((size_t)gid * p.nsubTotal + p.gridSubset[g]) * 2 + term) * 3;
            e[0] += mq * (fx * nx * (double)p.recip[0]);
            e[1] += mq * (fx * nx * (double)p.recip[3] + fy * ny * (double)p.recip[4]);
            e[2] += mq * (fx * nx * (double)p.recip[6] + fy * ny * (double)p.recip[7] + fz * nz * (double)p.recip[8]);
        }
    }
}
template <typename Real> void launchAtomField(const PmeParams<Real>& p, double* tab, hipStream_t s) {
    if (p.natoms <= 0 || p.nsub <= 0) return;
    hipLaunchKernelGGL((k_atomField<Real>), dim3((p.natoms + 7) / 8), dim3(256), 0, s, p, tab);
}
template void launchAtomField<float>(const PmeParams<float>&, double*, hipStream_t);
template void launchAtomField<double>(const PmeParams<double>&, double*, hipStream_t);

// ---- finish ------------------------------------------------------------------------------------------------------------------------
// One thread per table value: sorted -> user order.  row = nsub * 6 values per atom.
__global__ __launch_bounds__(256) void k_atomForceFinish(const double* __restrict__ tab, const int* __restrict__ userToSorted, const int nAtoms, const int row, double* __restrict__ out) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)nAtoms * row) return;
    const int u = (int)(t / row), c = (int)(t - (long long)u * row);
    out[t] = tab[(size_t)userToSorted[u] * row + c];
}
void launchAtomForceFinish(const double* tab, const int* userToSorted, int nAtoms, int nsub, double* out, hipStream_t s) {
    const long long n = (long long)nAtoms * nsub * 6;
    if (n <= 0) return;
    hipLaunchKernelGGL(k_atomForceFinish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, tab, userToSorted, nAtoms, nsub * 6, out);
}

}  // namespace snb
